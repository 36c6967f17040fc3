"""Plain numpy fp64 reference of the flat-layout (C, P) GEMM entry points (csrc/mlp_direct.hip: o3d_pw_fwd, o3d_pw_fwd_cloud,
o3d_pw_dgrad and their pairs; csrc/mlp_wgrad.hip: o3d_mlp_conv_wgrad2 with B = 1 and a dense dN, o3d_mlp_conv_wgrad2_group),
written from the formulas of include/o3dsot.h.  It imports nothing of the package under test.  Shared by
tests/test_gemm_oracle_cpu.py (which ties it to Conv1d / BatchNorm1d / ReLU under torch.autograd) and
tests/test_gemm_kernels_gpu.py (which pins every export to it).

Every function takes the fp32 inputs as the fp64 numbers they are and returns a Ref: for every output the value, the number
of terms n of its sum and *_abs, the same sum over the absolute values of every product that enters a term -- the yardstick
of the exactness condition (sum|terms| / spacing < 2^24) and of the rounding bound (n + 8) * 2^-24 * sum|terms|, both as
defined in tests/compact_oracle.py.
"""
from types import SimpleNamespace as Ref

import numpy as np

import compact_oracle as CO
from compact_oracle import Dyadic, TWO24  # noqa: F401  (re-exported for the tests)

# grid spacing of the terms of every exactly compared output, for the input steps of `Inputs` below
SPACING = {"gemm.Y": 0.125, "gemm.part0": 0.125, "gemm.part1": 1.0 / 64, "gemm.G": 0.125, "gemm.gpart0": 0.125,
           "gemm.gpart1": 1.0 / 32, "gemm.dW": 1.0 / 16, "gemm.rowsum": 0.5}
CO.SPACING.update(SPACING)
assert_exact = CO.assert_exact


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def col(v):
    return f64(v)[:, None]


# ---- operands ------------------------------------------------------------------------------------------------------------
def act(X, in_scale=None, in_shift=None):
    """f(X) = relu(x * in_scale + in_shift) per row, or X (both None) -> f, f_abs"""
    X = f64(X)
    if in_scale is None:
        return X, np.abs(X)
    n = X * col(in_scale) + col(in_shift)
    on = n > 0
    return np.where(on, n, 0.0), np.where(on, np.abs(X * col(in_scale)) + np.abs(col(in_shift)), 0.0)


def dy_of(dN, Y=None, A1=None, A2=None, A3=None):
    """dY = dN (Y None) or A1*dN + A2*Y + A3 per row -> dY, dY_abs"""
    dN = f64(dN)
    if Y is None:
        return dN, np.abs(dN)
    Y = f64(Y)
    return (col(A1) * dN + col(A2) * Y + col(A3),
            np.abs(col(A1) * dN) + np.abs(col(A2) * Y) + np.abs(col(A3)) + 0.0 * dN)


# ---- statistics partials -----------------------------------------------------------------------------------------------
def tiles(A, tile):
    C, P = A.shape
    assert P % tile == 0
    return A.reshape(C, P // tile, tile)


def stats_fwd(Y, Y_abs, tile, stat_c=None):
    """part [P/tile][2][C] = {sum y, sum (y - stat_c)^2} over each tile's columns -> part, part_abs; n = tile"""
    c = col(stat_c)[:, :, None] if stat_c is not None else 0.0
    y, ya = tiles(f64(Y), tile), tiles(f64(Y_abs), tile)
    part = np.stack([y.sum(2).T, ((y - c) ** 2).sum(2).T], axis=1)
    pabs = np.stack([ya.sum(2).T, ((ya + np.abs(c)) ** 2).sum(2).T], axis=1)
    return part, pabs


def stats_bwd(G, G_abs, Yprev, mean_p, tile):
    """part [P/tile][2][C] = {sum g, sum g * (Yprev - mean_p)} -> part, part_abs; n = tile"""
    g, ga, yp = tiles(f64(G), tile), tiles(f64(G_abs), tile), tiles(f64(Yprev), tile)
    mu = col(mean_p)[:, :, None]
    part = np.stack([g.sum(2).T, (g * (yp - mu)).sum(2).T], axis=1)
    pabs = np.stack([ga.sum(2).T, (ga * (np.abs(yp) + np.abs(mu))).sum(2).T], axis=1)
    return part, pabs


# ---- forward ---------------------------------------------------------------------------------------------------------------
def pw_fwd(X, W, in_scale=None, in_shift=None, bias=None, resid=None, tile=None, stat_c=None):
    """Y (Cout, P) = W (Cout, Cin) . f(X) [+ bias[row]] [+ resid]; tile: statistics partials of Y per `tile` columns.
    -> Ref(Y, Y_abs, n [, part, part_abs, part_n])"""
    W = f64(W)
    f, fa = act(X, in_scale, in_shift)
    Y, Ya, n = W @ f, np.abs(W) @ fa, W.shape[1]
    if bias is not None:
        Y, Ya, n = Y + col(bias), Ya + np.abs(col(bias)), n + 1
    if resid is not None:
        Y, Ya, n = Y + f64(resid), Ya + np.abs(f64(resid)), n + 1
    r = Ref(Y=Y, Y_abs=Ya, n=n)
    if tile:
        r.part, r.part_abs = stats_fwd(Y, Ya, tile, stat_c)
        r.part_n = tile
    return r


def pw_fwd_cloud(X, W, cbias, N, stat_c=None, tile=128):
    """Y (Cout, B*N) = W . X + cbias[:, column // N], cbias (Cout, B); partials of the biased output per `tile` columns"""
    W, cb = f64(W), f64(cbias)
    cloud = np.arange(f64(X).shape[1]) // N
    Y = W @ f64(X) + cb[:, cloud]
    Ya = np.abs(W) @ np.abs(f64(X)) + np.abs(cb[:, cloud])
    r = Ref(Y=Y, Y_abs=Ya, n=W.shape[1] + 1)
    r.part, r.part_abs = stats_fwd(Y, Ya, tile, stat_c)
    r.part_n = tile
    return r


# ---- data gradient ---------------------------------------------------------------------------------------------------------
def pw_dgrad(dN, Wt, Y=None, A1=None, A2=None, A3=None, Yprev=None, scale_p=None, shift_p=None, mean_p=None, resid=None,
             tile=None):
    """G (Cin, P) = Wt (Cin, Cout) . dY, dY = dN or A1*dN + A2*Y + A3 per contraction row.  Yprev given: G is kept where
    Yprev * scale_p + shift_p > 0 (else 0) and part [P/tile][2][Cin] = {sum g, sum g * (Yprev - mean_p)}; Yprev None:
    plain store [+ resid].  -> Ref(G, G_abs, n [, mask, part, part_abs, part_n])"""
    Wt = f64(Wt)
    dY, dYa = dy_of(dN, Y, A1, A2, A3)
    G, Ga, n = Wt @ dY, np.abs(Wt) @ dYa, Wt.shape[1]
    r = Ref(n=n)
    if Yprev is not None:
        assert resid is None
        r.mask = f64(Yprev) * col(scale_p) + col(shift_p) > 0
        G, Ga = np.where(r.mask, G, 0.0), np.where(r.mask, Ga, 0.0)
        if tile:
            r.part, r.part_abs = stats_bwd(G, Ga, Yprev, mean_p, tile)
            r.part_n = tile
    elif resid is not None:
        G, Ga, r.n = G + f64(resid), Ga + np.abs(f64(resid)), n + 1
    r.G, r.G_abs = G, Ga
    return r


# ---- weight gradient -------------------------------------------------------------------------------------------------------
def wgrad(dN, X, Y=None, A1=None, A2=None, A3=None, in_scale=None, in_shift=None):
    """dW (Cout, Cin) = sum_p dY[:, p] f(X)[:, p]^T -> Ref(dW, dW_abs, n = P)"""
    dY, dYa = dy_of(dN, Y, A1, A2, A3)
    f, fa = act(X, in_scale, in_shift)
    return Ref(dW=dY @ f.T, dW_abs=dYa @ fa.T, n=dY.shape[1])


def row_sum(dN):
    """the row-sum job of a group: dW (Cout) = sum_p dN -> Ref(dW, dW_abs, n = P)"""
    dN = f64(dN)
    return Ref(dW=dN.sum(1), dW_abs=np.abs(dN).sum(1), n=dN.shape[1])


# ---- BatchNorm constants from the partials (fp64), as the finalize kernels derive them ------------------------------------
def bn_consts(part, count, gamma, beta, eps, stat_c=None):
    """part [rows][2][C] = {sum y, sum (y - c)^2} -> mean, invstd, scale = gamma * invstd, shift = beta - mean * scale"""
    s = f64(part).sum(0)
    c = f64(stat_c) if stat_c is not None else 0.0
    mean = s[0] / count
    var = s[1] / count - (mean - c) ** 2
    invstd = 1.0 / np.sqrt(var + eps)
    scale = f64(gamma) * invstd
    return mean, invstd, scale, f64(beta) - mean * scale


def bn_bwd_coef(part, count, gamma, mean, invstd):
    """part [rows][2][C] = {sum g, sum g * (y - mean)} of the gradient g w.r.t. the BatchNorm output -> A1, A2, A3 with
    dY = A1 * g + A2 * y + A3 the gradient w.r.t. the BatchNorm input y"""
    s = f64(part).sum(0)
    A1 = f64(gamma) * invstd
    A2 = -A1 * invstd ** 2 * s[1] / count
    A3 = -A1 * s[0] / count - A2 * mean
    return A1, A2, A3


# ---- inputs ------------------------------------------------------------------------------------------------------------
def sparse_rows(draw, M, K, nnz, values=(1.0, -1.0, 0.5, -0.5)):
    """(M, K) matrix with nnz non-zeros per row drawn from `values`; the rows walk a permutation of the K columns, so every
    column holds a non-zero once M * nnz >= K (a dropped k then shows in some row).  A Randn draw: dense randn."""
    if not draw.exact:
        return draw.val((M, K))
    nnz = min(nnz, K)
    perm = draw.rng.permutation(K)
    W = np.zeros((M, K))
    v = draw.rng.choice(np.array(values), size=(M, nnz))
    for m in range(M):
        W[m, perm[(m * nnz + np.arange(nnz)) % K]] = v[m]
    assert M * nnz < K or (W != 0).any(0).all()
    return W


class Inputs:
    """operands of one (M, K, P) problem on the grids SPACING assumes (exact draw) or randn (rounded draw); `nnz` non-zero
    weights per row keep sum|terms| of the second-moment partials below 2^24 grid steps for every K the tests use"""

    def __init__(self, draw, M, K, P, nnz=16):
        d = draw
        self.M, self.K, self.P = M, K, P
        self.W = sparse_rows(d, M, K, nnz)                    # forward: (Cout, Cin); data gradient: Wt (Cin, Cout)
        self.X = d.val((K, P), 0.5, 1.0)                      # forward input / dN of the data gradient
        self.Y = d.val((K, P), 0.5, 1.0)                      # data gradient: this layer's raw output
        self.in_scale, self.in_shift = d.coef((K,), zero=False), d.val((K,), 0.25, 0.5)
        self.A1, self.A2, self.A3 = d.coef((K,)), d.coef((K,)), d.coef((K,))
        self.bias, self.resid = d.val((M,), 0.125, 1.0), d.val((M, P), 0.125, 1.0)
        self.stat_c = d.val((M,), 0.125, 0.5)
        self.Yprev = d.val((M, P), 0.25, 1.0)
        self.scale_p, self.shift_p, self.mean_p = d.coef((M,), zero=False), d.val((M,), 0.25, 0.5), d.val((M,), 0.25, 0.5)
