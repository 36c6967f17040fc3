"""Plain numpy fp64 reference of the kernels around the GEMMs of a per-point stack, written from the formulas of
include/o3dsot.h and the file headers of csrc/pointwise.hip / csrc/xcorr.hip / csrc/mlp.hip:
  * the chain ends on the flat (C, P = B*N) layout: o3d_bn_relu_apply, o3d_act_bwd_partials, o3d_gmax_fwd, o3d_gmax_bwd_pk,
    o3d_cloud_sum_dy, o3d_thin_bwd;
  * the packed max-gradient source pk (C, balls, 2) = {masked gradient, bits(arg-max slot)} with ns columns per ball: its
    producers o3d_gmax_bwd_pk and o3d_pool_bwd_partials_split, and expand_pk, which turns it into the dense one-hot dN the
    GEMM oracles (gemm_oracle.wgrad / pw_dgrad) take -- the reference of o3d_mlp_conv_wgrad2 / o3d_mlp_conv_dgrad_wt on pk;
  * layer 0 of the P2B fusion: o3d_xcorr_expand / o3d_xcorr_reduce.
It imports nothing of the package under test.  Shared by tests/test_pointwise_oracle_cpu.py (which ties it to Conv1d /
BatchNorm1d / ReLU / amax and to the materialised fusion tensor under torch.autograd in fp64) and by
tests/test_pointwise_kernels_gpu.py / tests/test_xcorr_kernels_gpu.py (which pin every export to it).

As in gemm_oracle.py every function takes the fp32 inputs as the fp64 numbers they are and returns a Ref: for every output
the value, the number of terms n of its sum and *_abs, the same sum over the absolute values of every product that enters
a term -- the yardstick of the exactness condition (sum|terms| / spacing < 2^24) and of the rounding bound
(n + 8) * 2^-24 * sum|terms|, both as defined in tests/compact_oracle.py.

The case tables of the two GPU files and the input grids of their exact legs live here too, so that the CPU file can run
the exactness condition of every exact case without a GPU.
"""
from types import SimpleNamespace as Ref

import numpy as np

import compact_oracle as CO
import gemm_oracle as G
from compact_oracle import Dyadic, TWO24  # noqa: F401  (re-exported for the tests)
from gemm_oracle import col, dy_of, f64, pw_dgrad, stats_bwd, stats_fwd, wgrad  # noqa: F401

# grid spacing of the terms of every exactly compared output, for the input grids of the *_inputs functions below
SPACING = {"pw.apply": 0.125, "pw.act0": 0.25, "pw.act1": 1.0 / 16, "pw.gmax": 0.125, "pw.pk0": 0.25, "pw.pk1": 1.0 / 16,
           "pw.cloud": 0.125, "pw.thin_dW": 0.125, "pw.thin_dX": 0.125, "xc.Y0": 0.25, "xc.part0": 0.25, "xc.part1": 1.0 / 16,
           "xc.S": 0.125, "xc.dsim": 1.0 / 16, "xc.dw": 1.0 / 16}
CO.SPACING.update(SPACING)
assert_exact = CO.assert_exact


def pre_act(Y, scale, shift):
    """n = y * scale + shift per row (the BatchNorm in front of the ReLU) -> n, n_abs"""
    Y = f64(Y)
    return Y * col(scale) + col(shift), np.abs(Y * col(scale)) + np.abs(col(shift)) + 0.0 * Y


# ---- materialised activation -------------------------------------------------------------------------------------------
def bn_relu_apply(Y, scale, shift):
    """out (C, P) = relu(Y * scale + shift) -> Ref(out, out_abs, n = 2)"""
    n, na = pre_act(Y, scale, shift)
    on = n > 0
    return Ref(out=np.where(on, n, 0.0), out_abs=np.where(on, na, 0.0), n=2)


def act_bwd_partials(g, Y, scale, shift, mean, tile=128):
    """dN = g where Y * scale + shift > 0 (strict) else 0; part [P/tile][2][C] = {sum dN, sum dN * (Y - mean)} per tile
    -> Ref(dN, dN_abs, n = 1, mask, part, part_abs, part_n = tile)"""
    n, _ = pre_act(Y, scale, shift)
    mask = n > 0
    dN = np.where(mask, f64(g), 0.0)
    r = Ref(dN=dN, dN_abs=np.abs(dN), n=1, mask=mask, part_n=tile)
    r.part, r.part_abs = stats_bwd(dN, np.abs(dN), Y, mean, tile)
    return r


# ---- global max per cloud ------------------------------------------------------------------------------------------------
def gmax_fwd(Y, scale, shift, B, N):
    """out (B, C) = max over the cloud's N columns of relu(Y * scale + shift); argq (B, C) = b*N + the FIRST column at which
    the pre-activation Y * scale + shift is largest (the ReLU plays no part in it); yarg = Y there.
    -> Ref(out, out_abs, argq, yarg, n = 2)"""
    Y = f64(Y)
    C = Y.shape[0]
    n, na = pre_act(Y, scale, shift)
    n3, na3, y3 = n.reshape(C, B, N), na.reshape(C, B, N), Y.reshape(C, B, N)
    rel = n3.argmax(2)                                        # numpy: the first occurrence of the maximum
    pick = lambda a: np.take_along_axis(a, rel[:, :, None], 2)[:, :, 0].T      # noqa: E731
    best = pick(n3)
    on = best > 0
    return Ref(out=np.where(on, best, 0.0), out_abs=np.where(on, pick(na3), 0.0), n=2,
               argq=(rel.T + N * np.arange(B)[:, None]).astype(np.int64), yarg=pick(y3))


def gmax_bwd_pk(dOut, out, argq, yarg, mean, B, N):
    """dOut, out, yarg, argq (B, C) as gmax_fwd returns them -> Ref(pk_g (C, B) = dOut where out > 0 else 0,
    pk_slot (C, B) = argq - b*N (an integer), part [1][2][C] = {sum_b g, sum_b g * (yarg - mean)}, part_abs, part_n = B)"""
    g = np.where(f64(out) > 0, f64(dOut), 0.0)                # (B, C)
    slot = np.asarray(argq, np.int64) - N * np.arange(B)[:, None]
    mu = f64(mean)[None, :]
    part = np.stack([g.sum(0), (g * (f64(yarg) - mu)).sum(0)])[None]
    pabs = np.stack([np.abs(g).sum(0), (np.abs(g) * (np.abs(f64(yarg)) + np.abs(mu))).sum(0)])[None]
    return Ref(pk_g=g.T.copy(), pk_slot=slot.T.copy(), part=part, part_abs=pabs, part_n=B)


def pool_bwd_partials_split(dOut, out, arg, yarg, mean, npoint, nsplit):
    """ONE cloud of npoint balls, pooled tensors (C, npoint); the balls of a channel in nsplit contiguous shares of
    ceil(npoint / nsplit) (a share may be empty: zeros) -> Ref(part [nsplit][2][C], part_abs, part_n = share, pk_g, pk_slot)"""
    g = np.where(f64(out) > 0, f64(dOut), 0.0)                # (C, npoint)
    C = g.shape[0]
    assert g.shape == (C, npoint)
    mu = col(mean)
    q, qa = g * (f64(yarg) - mu), np.abs(g) * (np.abs(f64(yarg)) + np.abs(mu))
    share = -(-npoint // nsplit)
    part, pabs = np.zeros((nsplit, 2, C)), np.zeros((nsplit, 2, C))
    for k in range(nsplit):
        s = slice(min(k * share, npoint), min((k + 1) * share, npoint))
        part[k, 0], part[k, 1] = g[:, s].sum(1), q[:, s].sum(1)
        pabs[k, 0], pabs[k, 1] = np.abs(g[:, s]).sum(1), qa[:, s].sum(1)
    return Ref(part=part, part_abs=pabs, part_n=share, pk_g=g, pk_slot=np.asarray(arg, np.int64).copy())


def expand_pk(pk_g, pk_slot, ns, P):
    """the dense gradient the packed source stands for: dN (C, P), dN[c, j*ns + slot[c, j]] = g[c, j], zero elsewhere"""
    g, slot = f64(pk_g), np.asarray(pk_slot, np.int64)
    C, balls = g.shape
    assert balls * ns == P and slot.shape == g.shape and (slot >= 0).all() and (slot < ns).all()
    dN = np.zeros((C, P))
    dN[np.arange(C)[:, None], np.arange(balls)[None, :] * ns + slot] = g
    return dN


# ---- per-cloud sums and the thin layer 0 ---------------------------------------------------------------------------------
def cloud_sum_dy(dN, Y, A1, A2, A3, B, N):
    """out (C, B) = sum over the N columns of cloud b of dY = A1*dN + A2*Y + A3 -> Ref(out, out_abs, n = N)"""
    dY, dYa = dy_of(dN, Y, A1, A2, A3)
    C = dY.shape[0]
    return Ref(out=dY.reshape(C, B, N).sum(2), out_abs=dYa.reshape(C, B, N).sum(2), n=N)


def thin_bwd(dN, Y, A1, A2, A3, X, W):
    """layer 0 with Cout = 64 and Cin <= 16: dY = A1*dN + A2*Y + A3 (64, P); dW (64, Cin) = dY . X^T (n = P);
    dX (Cin, P) = W^T . dY (n = 64) -> Ref(dW, dW_abs, dW_n, dX, dX_abs, dX_n)"""
    dY, dYa = dy_of(dN, Y, A1, A2, A3)
    X, W = f64(X), f64(W)
    return Ref(dW=dY @ X.T, dW_abs=dYa @ np.abs(X).T, dW_n=dY.shape[1], dX=W.T @ dY, dX_abs=np.abs(W).T @ dYa,
               dX_n=W.shape[0])


# ---- P2B fusion, layer 0 -------------------------------------------------------------------------------------------------
def xcorr_cols(B, M, N):
    """for every column q = (b*N + j)*M + i: its cloud b and its template column b*M + i of Z / S"""
    q = np.arange(B * N * M)
    b, i = q // (N * M), q % M
    return b, b * M + i


def xcorr_expand(Z, sim, W0col, B, M, N, stat_c=None):
    """Y0 (C0, P) with Y0[c, q] = Z[c, b*M + i] + W0col[c] * sim[q]; part [P/256][2][C0] = {sum y, sum (y - stat_c)^2}
    -> Ref(Y0, Y0_abs, n = 2, part, part_abs, part_n = 256)"""
    Z, sim, w = f64(Z), f64(sim).reshape(-1), f64(W0col)
    _, zc = xcorr_cols(B, M, N)
    Y0 = Z[:, zc] + w[:, None] * sim[None, :]
    Ya = np.abs(Z[:, zc]) + np.abs(w[:, None] * sim[None, :])
    r = Ref(Y0=Y0, Y0_abs=Ya, n=2, part_n=256)
    r.part, r.part_abs = stats_fwd(Y0, Ya, 256, stat_c)
    return r


def xcorr_reduce(dN, Y0, A1, A2, A3, sim, W0col, B, M, N):
    """dY0 = A1*dN + A2*Y0 + A3.  S (C0, B*M) = sum over the N search points j (n = N); dsim_part (C0/16, P) = sum over
    each group of 16 channels of W0col[c] * dY0[c, q] (n = 16); dw_part (B, C0) = sum over cloud b's columns of
    dY0[c, q] * sim[q] (n = M*N) -> Ref(S, S_abs, S_n, dsim_part, dsim_abs, dsim_n, dw_part, dw_abs, dw_n)"""
    dY, dYa = dy_of(dN, Y0, A1, A2, A3)
    C0 = dY.shape[0]
    sim, w = f64(sim).reshape(-1), f64(W0col)
    fold = lambda a: a.reshape(C0, B, N, M).sum(2).reshape(C0, B * M)           # noqa: E731
    grp = lambda a: a.reshape(C0 // 16, 16, -1).sum(1)                          # noqa: E731
    cloud = lambda a: a.reshape(C0, B, N * M).sum(2).T                          # noqa: E731
    return Ref(S=fold(dY), S_abs=fold(dYa), S_n=N,
               dsim_part=grp(w[:, None] * dY), dsim_abs=grp(np.abs(w)[:, None] * dYa), dsim_n=16,
               dw_part=cloud(dY * sim[None, :]), dw_abs=cloud(dYa * np.abs(sim)[None, :]), dw_n=M * N)


# ---- hand-written known answers of gmax_fwd ------------------------------------------------------------------------------
def gmax_known_answers():
    """-> [(name, Y (1, B*N), scale, shift, B, N, out (B, 1), argq (B, 1), yarg (B, 1))], every expectation written by hand.
    A lane of the kernel reads 4 consecutive columns, then the 4 columns 256 further on; 64 lanes make a cloud's row."""
    cases = []

    def add(name, Y, scale, shift, B, N, out, argq, yarg):
        cases.append((name, np.asarray(Y, np.float64).reshape(1, B * N), np.array([scale], np.float64),
                      np.array([shift], np.float64), B, N, np.array(out, np.float64).reshape(B, 1),
                      np.array(argq, np.int64).reshape(B, 1), np.array(yarg, np.float64).reshape(B, 1)))

    y = np.full(8, -1.0)
    y[[5, 6]] = 2.0                                           # columns 5 and 6: one group of four columns
    add("tie_in_group_of_four", y, 1.0, 0.5, 1, 8, [2.5], [5], [2.0])
    y = np.full(520, -1.0)
    y[[6, 262]] = 3.0                                         # the same lane, one stride of 256 columns apart
    add("tie_256_apart", y, 0.5, 0.0, 1, 520, [1.5], [6], [3.0])
    y = np.full(2 * 64, -2.0)
    y[[64 + 9, 64 + 41]] = 1.0                                # cloud 1: lanes 2 and 10 of the same row
    y[[3, 60]] = 0.5                                          # cloud 0: lanes 0 and 15
    add("tie_in_two_lanes", y, 2.0, 0.25, 2, 64, [1.25, 2.25], [3, 64 + 9], [0.5, 1.0])
    y = np.arange(2 * 260, dtype=np.float64) - 300.0          # scale 0: every column ties -> the cloud's first column
    add("scale_zero", y, 0.0, 0.75, 2, 260, [0.75, 0.75], [0, 260], [-300.0, -40.0])
    add("scale_zero_negative_shift", y, 0.0, -0.75, 2, 260, [0.0, 0.0], [0, 260], [-300.0, -40.0])
    y = np.array([1.0, -3.0, 2.0, -3.0, 0.0, 1.0, -2.5, 4.0])  # negative scale: the SMALLEST y wins, first of the two -3
    add("negative_scale", y, -1.0, 1.0, 1, 8, [4.0], [1], [-3.0])
    y = np.array([-4.0, -1.0, -2.0, -1.0, -3.0, -5.0, -1.5, -6.0, -2.0, -2.0, -0.5, -7.0])   # all pre-activations negative:
    add("all_negative", y, 1.0, -0.25, 1, 12, [0.0], [10], [-0.5])                          # out 0, argq still the arg-max
    return cases


# ---- case tables of tests/test_pointwise_kernels_gpu.py / tests/test_xcorr_kernels_gpu.py ------------------------------
APPLY_SHAPES = [(1, 4), (5, 1028), (64, 4096)]                             # (C, P)
ACT_C, ACT_P = (1, 7, 8, 9, 64), (128, 384)
GMAX_SHAPES = [(1, 1, 4), (3, 5, 64), (2, 4, 256), (2, 6, 260), (3, 9, 1028), (2, 64, 2048)]      # (B, C, N)
GMAX_BWD_SHAPES = [(1, 5, 64), (3, 9, 1028), (3, 70, 64)]                  # fed by gmax_fwd; C = 70: two workgroups of 64
POOL_C, POOL_NPOINT, POOL_NSPLIT = (16, 80), (12, 1000), (1, 3, 64)
POOL_NS = 32
PK_LAYERS = [(64, 64), (128, 64), (64, 128)]                               # (Cout, Cin)
PK_SHAPES = [(4, 576), (32, 576), (128, 384), (384, 768), (2048, 4096)]    # (ns, P): balls <, == and > a 128-column tile
PK_DGRAD_EXTRA = [(4, 640), (32, 640)]      # the data gradient runs 128-column tiles: P = 576 is refused, 640 = 5 tiles
CLOUD_SHAPES = [(1, 1, 4), (5, 3, 1024), (3, 2, 1028), (64, 2, 2048)]      # (C, B, N)
THIN_CIN = (1, 3, 12, 15, 16)
THIN_GROUPS = (1, 3, 256, 257, 600)                                        # P / 64
XCORR_SHAPES = [(1, 4, 256, 16), (2, 8, 128, 80), (1, 16, 64, 144), (2, 32, 64, 64), (1, 64, 16, 128)]   # (B, M, N, C0)
XCORR_PAD = 3                                                              # ldz = lds = B*M + XCORR_PAD


# ---- inputs: dyadic grids (Dyadic draw) or randn (the GPU files' Randn draw) -----------------------------------------------
def chain_end_inputs(draw, C, P, dead=None):
    """Y, g / dN / dOut-like operands and the per-channel constants of the chain-end kernels; `dead`: a channel whose scale
    is 0 (every column of it ties, the activation is max(shift, 0) everywhere)"""
    scale = draw.coef((C,), zero=False)
    if dead is not None:
        scale[dead] = 0.0
    return Ref(Y=draw.val((C, P), 0.25, 2.0), g=draw.val((C, P), 0.25, 2.0), scale=scale, shift=draw.val((C,), 0.25, 1.0),
               mean=draw.val((C,), 0.25, 0.5), A1=draw.coef((C,)), A2=draw.coef((C,)), A3=draw.coef((C,)))


def pool_split_inputs(draw, C, npoint, ns=POOL_NS):
    """pooled tensors (C, npoint) of one cloud: out >= 0 with zeros among it, arg in [0, ns)"""
    return Ref(dOut=draw.val((C, npoint), 0.25, 2.0), out=np.maximum(draw.val((C, npoint), 0.25, 2.0), 0.0),
               yarg=draw.val((C, npoint), 0.25, 2.0), mean=draw.val((C,), 0.25, 0.5),
               arg=np.random.RandomState(C + npoint).randint(0, ns, size=(C, npoint)))


def pk_source(draw, C, ns, P, seed):
    """a packed source of P / ns balls: g on the grid of gemm_oracle.Inputs.X; a third of the slots is the ball's first, a
    third its last, the rest anywhere (ball 0: first in the even channels, last in the odd ones); ball 1 has g == 0 in
    every channel (with two balls only: the last ball, in every fourth channel)"""
    balls = P // ns
    assert balls >= 2 and balls * ns == P
    rng = np.random.RandomState(seed)
    g = draw.val((C, balls), 0.5, 1.0)
    slot = rng.randint(0, ns, size=(C, balls))
    edge = rng.randint(0, 3, size=(C, balls))
    slot = np.where(edge == 0, 0, np.where(edge == 1, ns - 1, slot))
    slot[:, 0] = np.where(np.arange(C) % 2 == 0, 0, ns - 1)
    if balls > 2:
        g[:, 1] = 0.0
    else:
        g[2::4, -1] = 0.0
    return g, slot


class PkWgradIn:
    """operands of o3d_mlp_conv_wgrad2 on the grids gemm_oracle.SPACING["gemm.dW"] assumes (those of the dense test)"""

    def __init__(self, draw, Cout, Cin, ns, P):
        d = draw
        self.Cout, self.Cin, self.ns, self.P = Cout, Cin, ns, P
        self.g, self.slot = pk_source(d, Cout, ns, P, Cout + Cin + ns)
        self.dN = expand_pk(self.g, self.slot, ns, P)
        self.Y = d.val((Cout, P), 0.5, 1.0)
        self.A1, self.A2, self.A3 = d.coef((Cout,)), d.coef((Cout,)), d.coef((Cout,))
        self.X = d.val((Cin, P), 0.5, 1.0)
        self.in_scale, self.in_shift = d.coef((Cin,), zero=False), d.val((Cin,), 0.25, 0.5)


def pk_dgrad_inputs(draw, Cout, Cin, ns, P):
    """gemm_oracle.Inputs of the data gradient (M = Cin rows out, K = Cout contraction rows) with the packed source in
    place of the dense dN: i.g, i.slot and i.X = expand_pk of them"""
    i = G.Inputs(draw, Cin, Cout, P)
    i.g, i.slot = pk_source(draw, Cout, ns, P, 7 + Cout + Cin + ns)
    i.X = expand_pk(i.g, i.slot, ns, P)
    return i


def thin_inputs(draw, P):
    """the 64-row operands of o3d_thin_bwd at the full Cin = 16 (a case slices X and W); W dense on the coefficient grid"""
    return Ref(dN=draw.val((64, P), 0.5, 1.0), Y=draw.val((64, P), 0.5, 1.0), A1=draw.coef((64,)), A2=draw.coef((64,)),
               A3=draw.coef((64,)), X=draw.val((16, P), 0.5, 1.0), W=draw.coef((64, 16)))


def xcorr_inputs(draw, B, M, N, C0, ldw):
    P, ldz = B * M * N, B * M + XCORR_PAD
    return Ref(Z=draw.val((C0, ldz), 0.5, 1.0), sim=draw.val((P,), 0.5, 1.0), W0=draw.coef((C0, ldw)),
               stat_c=draw.val((C0,), 0.25, 0.5), dN=draw.val((C0, P), 0.25, 2.0), Y0=draw.val((C0, P), 0.25, 2.0),
               A1=draw.coef((C0,)), A2=draw.coef((C0,)), A3=draw.coef((C0,)), ldz=ldz, lds=ldz)


def exact_preconditions():
    """the exactness condition of every exact-leg input set of the two GPU files -> [(name, worst sum|terms| / spacing)];
    raises where a grid is too coarse.  Each GPU case asserts the same condition on its own draw before its launch."""
    seen = []

    def ok(name, abs_sum):
        seen.append((name, assert_exact(name, abs_sum)))

    d = Dyadic(1)
    C, P = max(APPLY_SHAPES)
    i = chain_end_inputs(d, C, P)
    ok("pw.apply", bn_relu_apply(i.Y, i.scale, i.shift).out_abs)
    i = chain_end_inputs(d, max(ACT_C), max(ACT_P))
    r = act_bwd_partials(i.g, i.Y, i.scale, i.shift, i.mean)
    ok("pw.act0", r.part_abs[:, 0]), ok("pw.act1", r.part_abs[:, 1])
    for B, C, N in GMAX_SHAPES + GMAX_BWD_SHAPES:
        i = chain_end_inputs(d, C, B * N)
        f = gmax_fwd(i.Y, i.scale, i.shift, B, N)
        ok("pw.gmax", f.out_abs)
        r = gmax_bwd_pk(i.g[:, :B].T, f.out, f.argq, f.yarg, i.mean, B, N)
        ok("pw.pk0", r.part_abs[:, 0]), ok("pw.pk1", r.part_abs[:, 1])
    for C in POOL_C:
        i = pool_split_inputs(d, C, max(POOL_NPOINT))
        r = pool_bwd_partials_split(i.dOut, i.out, i.arg, i.yarg, i.mean, max(POOL_NPOINT), 1)      # one share: the longest sum
        ok("pw.pk0", r.part_abs[:, 0]), ok("pw.pk1", r.part_abs[:, 1])
    for Cout, Cin in PK_LAYERS:
        for ns, P in PK_SHAPES:
            i = PkWgradIn(d, Cout, Cin, ns, P)
            ok("gemm.dW", wgrad(i.dN, i.X, i.Y, i.A1, i.A2, i.A3, i.in_scale, i.in_shift).dW_abs)
        for ns, P in PK_SHAPES + PK_DGRAD_EXTRA:
            if P % 128:
                continue
            i = pk_dgrad_inputs(d, Cout, Cin, ns, P)
            r = pw_dgrad(i.X, i.W, i.Y, i.A1, i.A2, i.A3, Yprev=i.Yprev, scale_p=i.scale_p, shift_p=i.shift_p, mean_p=i.mean_p,
                         tile=128)
            ok("gemm.G", r.G_abs), ok("gemm.gpart0", r.part_abs[:, 0]), ok("gemm.gpart1", r.part_abs[:, 1])
    C, B, N = CLOUD_SHAPES[-1]
    i = chain_end_inputs(d, C, B * N)
    ok("pw.cloud", cloud_sum_dy(i.g, i.Y, i.A1, i.A2, i.A3, B, N).out_abs)
    i = thin_inputs(d, 64 * max(THIN_GROUPS))
    r = thin_bwd(i.dN, i.Y, i.A1, i.A2, i.A3, i.X, i.W)
    ok("pw.thin_dW", r.dW_abs), ok("pw.thin_dX", r.dX_abs)
    for B, M, N, C0 in XCORR_SHAPES:
        i = xcorr_inputs(d, B, M, N, C0, 5)
        r = xcorr_expand(i.Z, i.sim, i.W0[:, 0], B, M, N, i.stat_c)
        ok("xc.Y0", r.Y0_abs), ok("xc.part0", r.part_abs[:, 0]), ok("xc.part1", r.part_abs[:, 1])
        r = xcorr_reduce(i.dN, i.Y0, i.A1, i.A2, i.A3, i.sim, i.W0[:, 0], B, M, N)
        ok("xc.S", r.S_abs), ok("xc.dsim", r.dsim_abs), ok("xc.dw", r.dw_abs)
    return seen
