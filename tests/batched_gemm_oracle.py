"""Plain numpy fp64 reference of the batched (B, C, P) GEMM entry points of csrc/mlp.hip -- o3d_mlp_conv_fwd,
o3d_mlp_conv_dgrad / _dgrad_wt / _dgrad_plain, o3d_mlp_conv_wgrad, o3d_bn_relu_maxpool_fwd -- and of o3d_row_sum, written from
the formulas of include/o3dsot.h.  It imports nothing of the package under test and holds no GEMM arithmetic of its own: the
batched tensor (B, C, P) IS the flat (C, B*P) matrix with its columns in (b, p) order, and statistics row b*P/128 + t is
flat tile b*P/128 + t, so every GEMM is tests/gemm_oracle.py on the rearranged operands.  Two additions:
  pooled_dense  the dense gradient the pooled source (dOut, out, arg, ns) stands for
  pool_fwd      out = max_k relu(Y*scale + shift), arg = the first maximum of fmaf(y, scale, shift) as fp32, yarg = Y there
Shared by tests/test_batched_gemm_oracle_cpu.py (which ties it to Conv2d / BatchNorm2d / ReLU / max under autograd) and
tests/test_batched_gemm_kernels_gpu.py (which pins every export to it).  Ref / *_abs / n as in tests/gemm_oracle.py.
"""
from types import SimpleNamespace as Ref

import numpy as np

import gemm_oracle as G
from gemm_oracle import Dyadic, TWO24, assert_exact, f64, sparse_rows  # noqa: F401  (re-exported for the tests)

TILE = 128                 # columns per statistics row of every batched entry

# grid spacing of the terms of the exactly compared outputs that gemm_oracle.SPACING does not already name
SPACING = {"bg.pool": 0.125}
G.CO.SPACING.update(SPACING)


# ---- the rearrangement ---------------------------------------------------------------------------------------------------
def flat(A):
    """(B, C, P) -> (C, B*P), column = b*P + p"""
    A = f64(A)
    B, C, P = A.shape
    return A.transpose(1, 0, 2).reshape(C, B * P)


def unflat(M, B):
    """(C, B*P) -> (B, C, P)"""
    C, BP = M.shape
    return M.reshape(C, B, BP // B).transpose(1, 0, 2)


# ---- forward ---------------------------------------------------------------------------------------------------------------
def fwd(X, W, in_scale=None, in_shift=None, part=False, stat_c=None):
    """Y (B, Cout, P) = W . f(X (B, Cin, P)); part: rows [B*P/128][2][Cout] -> Ref(Y, Y_abs, n [, part, part_abs])"""
    B = np.shape(X)[0]
    r = G.pw_fwd(flat(X), W, in_scale, in_shift, tile=TILE if part else None, stat_c=stat_c)
    r.Y, r.Y_abs = unflat(r.Y, B), unflat(r.Y_abs, B)
    return r


def stats_fwd(Y, stat_c=None):
    """the statistics rows of a stored batched output -> part, part_abs [B*P/128][2][C]"""
    Y = f64(Y)
    return G.stats_fwd(flat(Y), np.abs(flat(Y)), TILE, stat_c)


# ---- the pooled gradient source ------------------------------------------------------------------------------------------
def pooled_dense(dOut, out, arg, ns):
    """dN[b, co, j*ns + k] = dOut[b, co, j] * [out[b, co, j] > 0] * [k == arg[b, co, j]]  (B, Cout, npoint*ns)"""
    dOut, out, arg = f64(dOut), f64(out), np.asarray(arg, np.int64)
    B, C, npoint = dOut.shape
    assert out.shape == dOut.shape == arg.shape
    k = np.arange(ns)[None, None, None, :]
    dN = np.where((k == arg[..., None]) & (out[..., None] > 0), dOut[..., None], 0.0)
    return dN.reshape(B, C, npoint * ns)


# ---- data gradients --------------------------------------------------------------------------------------------------------
def dgrad(dN, W, Y, A1, A2, A3, Yprev, scale_p, shift_p, mean_p):
    """dNprev (B, Cin, P) = (W^T dY) kept where Yprev*scale_p + shift_p > 0, dY = A1*dN + A2*Y + A3; part [B*P/128][2][Cin]
    = {sum dNprev, sum dNprev * (Yprev - mean_p)} -> Ref(G, G_abs, n = Cout, mask, part, part_abs)"""
    B = np.shape(dN)[0]
    r = G.pw_dgrad(flat(dN), f64(W).T, flat(Y), A1, A2, A3, Yprev=flat(Yprev), scale_p=scale_p, shift_p=shift_p, mean_p=mean_p,
                   tile=TILE)
    r.G, r.G_abs, r.mask = unflat(r.G, B), unflat(r.G_abs, B), unflat(r.mask, B)
    return r


def mask_fp32(Yprev, scale_p, shift_p):
    """fmaf(Yprev, scale_p, shift_p) > 0 evaluated in fp32: the product of two fp32 numbers is exact in fp64, and neither
    the fp64 addition nor the final rounding to fp32 can change the sign of a non-zero sum (no underflow at these sizes)"""
    y = np.asarray(Yprev, np.float32).astype(np.float64)
    sc = np.asarray(scale_p, np.float32).astype(np.float64)[None, :, None]
    sh = np.asarray(shift_p, np.float32).astype(np.float64)[None, :, None]
    return (y * sc + sh).astype(np.float32) > 0


def stats_bwd(Gs, Yprev, mean_p):
    Gs = f64(Gs)
    return G.stats_bwd(flat(Gs), np.abs(flat(Gs)), flat(Yprev), mean_p, TILE)


def dgrad_plain(dN, W, Y, A1, A2, A3):
    """dX (B, Cin, P) = W^T (A1*dN + A2*Y + A3) -> Ref(G, G_abs, n = Cout)"""
    B = np.shape(dN)[0]
    r = G.pw_dgrad(flat(dN), f64(W).T, flat(Y), A1, A2, A3)
    r.G, r.G_abs = unflat(r.G, B), unflat(r.G_abs, B)
    return r


# ---- weight gradient -------------------------------------------------------------------------------------------------------
def wgrad(dN, X, Y, A1, A2, A3, in_scale=None, in_shift=None):
    """dW (Cout, Cin) = sum_{b,p} dY[b, :, p] f(X)[b, :, p]^T -> Ref(dW, dW_abs, n = B*P)"""
    return G.wgrad(flat(dN), flat(X), flat(Y), A1, A2, A3, in_scale=in_scale, in_shift=in_shift)


def row_sum(Gm):
    """o3d_row_sum: out (C) = sum_p G (C, P) -> Ref(dW, dW_abs, n = P)"""
    return G.row_sum(Gm)


# ---- BN + ReLU + max over the ns neighbours -------------------------------------------------------------------------------
def pool_fwd(Y, scale, shift, ns):
    """Y (B, C, npoint*ns) -> Ref(out (B, C, npoint) = max_k relu(y*scale + shift) with out_abs and n = 2, arg = the FIRST k
    at which fmaf(y, scale, shift), rounded to fp32, is largest, yarg = Y there, n32 = those fp32 values (B, C, npoint, ns)).
    The fp32 value is the fp64 one rounded once more: the product is exact in fp64, so the two roundings differ from the
    single one of fmaf only when the fp64 sum lands on an fp32 midpoint -- never on the dyadic grids of the exact leg."""
    Y = f64(Y)
    B, C, P = Y.shape
    assert P % ns == 0
    y = Y.reshape(B, C, P // ns, ns)
    sc, sh = f64(scale)[None, :, None, None], f64(shift)[None, :, None, None]
    n = y * sc + sh
    na = np.abs(y * sc) + np.abs(sh)
    n32 = n.astype(np.float32)
    arg = n32.argmax(-1)                                   # numpy: the first occurrence of the maximum
    take = lambda a: np.take_along_axis(a, arg[..., None], -1)[..., 0]
    best, on = take(n), take(n) > 0
    return Ref(out=np.where(on, best, 0.0), out_abs=np.where(on, take(na), 0.0), n=2, arg=arg, yarg=take(y), n32=n32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
class Inputs:
    """operands of one batched problem (B, Cin, Cout, P) on the grids gemm_oracle.SPACING assumes (exact draw) or randn:
    W (Cout, Cin) with `nnz` non-zeros per row,
    X (B, Cin, P) the forward input, dN / Y (B, Cout, P), Yprev (B, Cin, P), per-channel constants of both widths"""

    def __init__(self, draw, B, Cin, Cout, P, nnz=16):
        d = draw
        self.B, self.Cin, self.Cout, self.P = B, Cin, Cout, P
        self.W = sparse_rows(d, Cout, Cin, nnz)
        self.X = d.val((B, Cin, P), 0.5, 1.0)
        self.dN, self.Y = d.val((B, Cout, P), 0.5, 1.0), d.val((B, Cout, P), 0.5, 1.0)
        self.in_scale, self.in_shift = d.coef((Cin,), zero=False), d.val((Cin,), 0.25, 0.5)
        self.A1, self.A2, self.A3 = d.coef((Cout,)), d.coef((Cout,)), d.coef((Cout,))
        self.stat_c = d.val((Cout,), 0.125, 0.5)
        self.Yprev = d.val((B, Cin, P), 0.25, 1.0)
        self.scale_p, self.shift_p, self.mean_p = d.coef((Cin,), zero=False), d.val((Cin,), 0.25, 0.5), d.val((Cin,), 0.25, 0.5)
        if Cin > 2:                                        # a negative and a zero scale_p: the mask follows the sign / the shift
            self.scale_p[1], self.scale_p[2] = -1.0 if d.exact else -abs(self.scale_p[1]), 0.0

    def pooled(self, draw, ns):
        """the pooled source of this problem's dN: dOut, out, arg (B, Cout, P / ns); arg walks every slot (so each of the four
        positions of a float4 is hit), out holds positive values, zeros, -0.0 and negative values"""
        B, C, npoint = self.B, self.Cout, self.P // ns
        dOut = draw.val((B, C, npoint), 0.5, 1.0)
        out = np.abs(draw.val((B, C, npoint), 0.5, 1.0)) + 0.5
        j = np.arange(B * C * npoint).reshape(B, C, npoint)
        arg = (j + j // npoint) % ns
        out[j % 5 == 1] = 0.0
        out[j % 5 == 2] = -0.0
        out[j % 5 == 3] *= -1.0
        return dOut, out, arg.astype(np.int32)
