"""The kernels around the GEMMs of a per-point stack, called through the C ABI with raw pointers, launch by launch, against
the plain numpy fp64 reference tests/pointwise_oracle.py (tied to Conv1d / BatchNorm1d / ReLU / max-pool under autograd by
tests/test_pointwise_oracle_cpu.py):
  * csrc/pointwise.hip: o3d_bn_relu_apply, o3d_act_bwd_partials, o3d_gmax_fwd, o3d_gmax_bwd_pk, o3d_cloud_sum_dy, o3d_thin_bwd;
  * the packed max-gradient source pk (C, balls, 2) = {masked gradient, bits(arg-max slot)}: its producers o3d_gmax_bwd_pk and
    o3d_pool_bwd_partials_split, and its consumers o3d_mlp_conv_wgrad2(dN = NULL, pk, ns) (POOLED in csrc/mlp_wgrad.hip) and
    o3d_mlp_conv_dgrad_wt(dN = NULL, ..., pk) (B_DYPOOL in csrc/mlp_direct.hip), against the dense GEMM oracle on
    pointwise_oracle.expand_pk(...) and against the dense entry points themselves.
Same method as tests/test_gemm_kernels_gpu.py, whose dense weight-gradient / data-gradient cases these complete:

EXACT leg: every floating-point input lies on a small dyadic grid, so every product and every partial sum of a correct kernel
is exactly representable in fp32 whatever its summation order (asserted before each launch: sum|terms| / spacing < 2^24; the
same condition runs without a GPU in tests/test_pointwise_oracle_cpu.py), and the comparison is EQUALITY -- of the arg-max
columns too: the grids make ties plentiful, and the first maximum is the answer.
ROUNDED leg: torch.randn inputs, |err| <= (n + 8) * 2^-24 * sum|t_i| per output; statistics partials are bounded against the
fp64 sums over the kernel's OWN stored output, read back.  o3d_gmax_fwd: out within 2 fp32 ulp of the fp64 result, yarg ==
Y[argq] bit for bit, argq inside its cloud and a maximiser (the fp64 pre-activation there within 2 fp32 ulp of the fp64
maximum), at every (cloud, channel).  The worst err / bound per kernel is printed and, when O3D_POINTWISE_PINS names a file,
written there together with the rows of tests/test_xcorr_kernels_gpu.py (profiles/pointwise_kernel_pins.txt is such a run).
GUARDS: every output buffer has a 256-element tail and is prefilled with a sentinel; the tail, the statistics rows beyond the
documented count, channels beyond C and the scratch beyond the documented size must still hold it after the call.
"""
import os

import numpy as np
import pytest
import torch

import pointwise_oracle as O

pytestmark = pytest.mark.gpu

SENT = -7.0e37
ISENT = -123456789
TAIL = 256
EINVAL = -1
EXTRA_ROWS = 2             # statistics rows allocated beyond the documented count: must stay untouched
RATIOS = {}


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi
    return capi.load()


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_POINTWISE_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per kernel, rounded legs of tests/test_pointwise_kernels_gpu.py and\n"
                    "# tests/test_xcorr_kernels_gpu.py; bound = (n + 8) * 2^-24 * sum|t_i| (gmax_fwd: 2 ulp of the fp64 result);\n"
                    "# every ratio must be <= 1\n")
            for k in sorted(RATIOS):
                f.write("%-28s %.4f\n" % (k, RATIOS[k]))


def st():
    return torch.cuda.current_stream().cuda_stream


class Randn:
    """torch.randn fp32 values (handed to the oracle as the fp64 numbers they are)"""
    exact = False

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def val(self, shape, step=None, lim=None):
        return torch.randn(shape, generator=self.g, dtype=torch.float32).double().numpy()

    def coef(self, shape, zero=True):
        return self.val(shape)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).cuda()


def devs(*arrays):
    """device copies, to be HELD by the caller until the launch has finished (a temporary's block is free for the next copy)"""
    return [dev(a) for a in arrays]


def devi(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def outbuf(shape):
    """-> (flat buffer with a TAIL of sentinels, view of `shape`)"""
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), SENT, dtype=torch.float32, device="cuda")
    return flat, flat[:n].view(shape)


def ibuf(shape):
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), ISENT, dtype=torch.int32, device="cuda")
    return flat, flat[:n].view(shape)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def tail_intact(*flats):
    for f in flats:
        assert bool((f[-TAIL:] == (ISENT if f.dtype == torch.int32 else SENT)).all()), "write beyond the buffer"


def untouched(t):
    return bool((t == (ISENT if t.dtype == torch.int32 else SENT)).all())


def ptr(t):
    return None if t is None else t.data_ptr()


def pre(draw, abs_sums):
    """before the launch: the exact leg's inputs keep every partial sum of these outputs exact in fp32"""
    if draw.exact:
        for k, v in abs_sums.items():
            O.assert_exact(k, v)


def compare(kernel, got, ref, ref_abs, n, draw):
    """exact leg: equality.  rounded leg: |got - ref| <= (n + 8) * 2^-24 * sum|t_i|, worst ratio recorded"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), kernel
    if draw.exact:
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (kernel, len(bad), bad[:8].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        return
    bound = (np.asarray(n, np.float64) + 8) * 2.0 ** -24 * np.asarray(ref_abs, np.float64)
    err = np.abs(got - ref)
    assert (err[bound == 0] == 0).all(), kernel
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    print("rounded leg %s: worst err/bound %.4f" % (kernel, ratio))
    assert ratio <= 1.0, (kernel, ratio)


def plant_zeros(draw, i):
    """exact leg: column 1 of every live channel sits exactly at 0 before the ReLU (y = -shift / scale lies on Y's grid)"""
    if draw.exact:
        live = i.scale != 0
        i.Y[live, 1] = -i.shift[live] / i.scale[live]
        n, _ = O.pre_act(i.Y, i.scale, i.shift)
        assert (n[live, 1] == 0).all() and (np.abs(i.Y) <= 2).all()


def pack(g, slot):
    """pk (C, balls, 2) on the device: {g, the BITS of the integer slot}"""
    t = torch.empty(g.shape + (2,), dtype=torch.float32)
    t[..., 0] = torch.from_numpy(np.ascontiguousarray(g)).float()
    t.view(torch.int32)[..., 1] = torch.from_numpy(np.ascontiguousarray(slot, dtype=np.int32))
    return t.cuda()


# ---- o3d_bn_relu_apply --------------------------------------------------------------------------------------------------------
def _apply(lib, draw, C, P):
    i = O.chain_end_inputs(draw, C, P, dead=C // 2 if C > 1 else None)
    plant_zeros(draw, i)
    r = O.bn_relu_apply(i.Y, i.scale, i.shift)
    pre(draw, {"pw.apply": r.out_abs})
    Of, out = outbuf((C, P))
    d = devs(i.Y, i.scale, i.shift)
    assert lib.o3d_bn_relu_apply(*map(ptr, d), C, P, ptr(out), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Of)
    got = host(out)
    compare("bn_relu_apply.out", got, r.out, r.out_abs, r.n, draw)
    assert (got >= 0).all() and not got[r.out == 0].any()
    if C > 1:                                                 # the dead channel: max(shift, 0) in every column
        assert (got[C // 2] == max(np.float32(i.shift[C // 2]), 0)).all()


@pytest.mark.parametrize("C,P", O.APPLY_SHAPES)
def test_bn_relu_apply_exact(lib, C, P):
    _apply(lib, O.Dyadic(100 + C), C, P)


def test_bn_relu_apply_rounded(lib):
    for C, P in O.APPLY_SHAPES:
        _apply(lib, Randn(3 + C), C, P)


def test_bn_relu_apply_refuses_p_not_multiple_of_4(lib):
    y, one = torch.zeros(2 * 8, device="cuda"), torch.ones(2, device="cuda")
    Of, out = outbuf((2, 6))
    assert lib.o3d_bn_relu_apply(ptr(y), ptr(one), ptr(one), 2, 6, ptr(out), st()) == EINVAL
    assert lib.o3d_bn_relu_apply(ptr(y), ptr(one), ptr(one), 0, 4, ptr(out), st()) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Of)


# ---- o3d_act_bwd_partials -----------------------------------------------------------------------------------------------------
def _act(lib, draw, C, P):
    i = O.chain_end_inputs(draw, C, P, dead=3 if C > 3 else None)
    plant_zeros(draw, i)
    r = O.act_bwd_partials(i.g, i.Y, i.scale, i.shift, i.mean)
    pre(draw, {"pw.act0": r.part_abs[:, 0], "pw.act1": r.part_abs[:, 1]})
    rows, Cpad = P // 128, (C + 7) // 8 * 8                    # a workgroup covers 8 channels: the surplus ones write nothing
    Df, dN = outbuf((Cpad, P))
    Pf, part = outbuf((rows + EXTRA_ROWS, 2, C))
    d = devs(i.g, i.Y, i.scale, i.shift, i.mean)
    assert lib.o3d_act_bwd_partials(*map(ptr, d), C, P, ptr(dN), ptr(part), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Df, Pf)
    assert untouched(dN[C:]), "a channel beyond C was written"
    assert untouched(part[rows:]), "a statistics row beyond P / 128 was written"
    got, gp = host(dN[:C]), host(part[:rows])
    # the mask is one fmaf in the kernel, whose sign is the exact sign: dN is g or 0 on both legs
    assert np.array_equal(got, r.dN), "act_bwd_partials.dN"
    if draw.exact:
        pr, pa = r.part, r.part_abs
    else:                              # the fp64 sums over the stored dN: what the kernel summed, n = 128
        pr, pa = O.stats_bwd(got, np.abs(got), i.Y, i.mean, 128)
    compare("act_bwd_partials.part_sum", gp[:, 0], pr[:, 0], pa[:, 0], 128, draw)
    compare("act_bwd_partials.part_gy", gp[:, 1], pr[:, 1], pa[:, 1], 128, draw)


@pytest.mark.parametrize("P", O.ACT_P)
@pytest.mark.parametrize("C", O.ACT_C)
def test_act_bwd_partials_exact(lib, C, P):
    _act(lib, O.Dyadic(200 + C + P), C, P)


def test_act_bwd_partials_rounded(lib):
    for C in O.ACT_C:
        for P in O.ACT_P:
            _act(lib, Randn(5 + C), C, P)


def test_act_bwd_partials_refuses_p_not_multiple_of_128(lib):
    z, one = torch.zeros(2 * 192, device="cuda"), torch.ones(2, device="cuda")
    Df, dN = outbuf((2, 192))
    Pf, part = outbuf((2, 2, 2))
    assert lib.o3d_act_bwd_partials(ptr(z), ptr(z), ptr(one), ptr(one), ptr(one), 2, 192, ptr(dN), ptr(part), st()) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Df) and untouched(Pf)


# ---- o3d_gmax_fwd and o3d_gmax_bwd_pk behind it -------------------------------------------------------------------------------
def _gmax_call(lib, Y, scale, shift, B, C, N, with_arg=True):
    Of, out = outbuf((B, C))
    Af, argq = ibuf((B, C))
    Yf, yarg = outbuf((B, C))
    d = devs(Y, scale, shift)
    rc = lib.o3d_gmax_fwd(*map(ptr, d), B, C, N, ptr(out), ptr(argq) if with_arg else None, ptr(yarg) if with_arg else None, st())
    torch.cuda.synchronize()
    assert rc == 0
    tail_intact(Of, Af, Yf)
    if not with_arg:
        assert untouched(Af) and untouched(Yf)
    return out, argq, yarg


def _gmax_fwd(lib, draw, B, C, N):
    """-> (inputs, device out / argq / yarg): checked against the oracle (exact leg) or the properties (rounded leg)"""
    dead = C // 2 if C > 1 else None
    i = O.chain_end_inputs(draw, C, B * N, dead=dead)
    r = O.gmax_fwd(i.Y, i.scale, i.shift, B, N)
    pre(draw, {"pw.gmax": r.out_abs})
    out, argq, yarg = _gmax_call(lib, i.Y, i.scale, i.shift, B, C, N)
    out_only, _, _ = _gmax_call(lib, i.Y, i.scale, i.shift, B, C, N, with_arg=False)
    assert torch.equal(out, out_only), "gmax_fwd: out differs without argq / yarg"
    go, ga, gy = host(out), argq.cpu().numpy().astype(np.int64), host(yarg)
    cloud0 = N * np.arange(B)[:, None]
    assert (ga >= cloud0).all() and (ga < cloud0 + N).all(), "gmax_fwd: argq outside its cloud"
    Y32 = np.asarray(i.Y, np.float32)
    assert np.array_equal(gy.astype(np.float32), Y32.T[ga, np.arange(C)[None, :]]), "gmax_fwd: yarg != Y[argq]"
    if dead is not None:                                      # every column ties exactly, on both legs: the first one
        assert (ga[:, dead] == cloud0[:, 0]).all()
    if draw.exact:
        compare("gmax_fwd.out", go, r.out, r.out_abs, r.n, draw)
        bad = np.argwhere(ga != r.argq)
        assert len(bad) == 0, ("gmax_fwd.argq", len(bad), bad[:8].tolist(), ga[tuple(bad[0])], r.argq[tuple(bad[0])])
        assert np.array_equal(gy, r.yarg), "gmax_fwd.yarg"
        n = (i.Y * i.scale[:, None] + i.shift[:, None]).reshape(C, B, N)
        if N >= 64:
            assert ((n == n.max(2, keepdims=True)).sum(2) > 1).any(), "no tie in this draw"
    else:
        ulp = np.spacing(np.abs(r.out).astype(np.float32)).astype(np.float64)
        ratio = float((np.abs(go - r.out) / (2 * ulp)).max())
        RATIOS["gmax_fwd.out"] = max(RATIOS.get("gmax_fwd.out", 0.0), ratio)
        print("rounded leg gmax_fwd.out: worst err / (2 ulp) %.4f" % ratio)
        assert ratio <= 1.0
        n = (i.Y * i.scale[:, None] + i.shift[:, None]).T      # (P, C) fp64 pre-activations
        best = n.reshape(B, N, C).max(1)
        gap = (best - n[ga, np.arange(C)[None, :]]) / (2 * np.spacing(np.abs(best).astype(np.float32)).astype(np.float64))
        RATIOS["gmax_fwd.argq_gap"] = max(RATIOS.get("gmax_fwd.argq_gap", 0.0), float(gap.max()))
        assert (gap >= 0).all() and gap.max() <= 1.0, "gmax_fwd: argq is not a maximiser"
    return i, out, argq, yarg


@pytest.mark.parametrize("B,C,N", O.GMAX_SHAPES)
def test_gmax_fwd_exact(lib, B, C, N):
    _gmax_fwd(lib, O.Dyadic(300 + B + C + N), B, C, N)


def test_gmax_fwd_rounded(lib):
    for B, C, N in O.GMAX_SHAPES:
        _gmax_fwd(lib, Randn(7 + C), B, C, N)


@pytest.mark.parametrize("case", O.gmax_known_answers(), ids=lambda c: c[0])
def test_gmax_fwd_known_answers(lib, case):
    _, Y, scale, shift, B, N, want_out, want_argq, want_yarg = case
    out, argq, yarg = _gmax_call(lib, Y, scale, shift, B, 1, N)
    assert np.array_equal(host(out), want_out) and np.array_equal(argq.cpu().numpy(), want_argq)
    assert np.array_equal(host(yarg), want_yarg)


def test_gmax_fwd_refusals(lib):
    y, one = torch.zeros(64, device="cuda"), torch.ones(2, device="cuda")
    Of, out = outbuf((1, 2))
    Af, argq = ibuf((1, 2))
    assert lib.o3d_gmax_fwd(ptr(y), ptr(one), ptr(one), 1, 2, 6, ptr(out), None, None, st()) == EINVAL      # N % 4 != 0
    assert lib.o3d_gmax_fwd(ptr(y), ptr(one), ptr(one), 1, 2, 8, ptr(out), ptr(argq), None, st()) == EINVAL  # argq without yarg
    torch.cuda.synchronize()
    assert untouched(Of) and untouched(Af)


def _gmax_bwd(lib, draw, B, C, N):
    i, out, argq, yarg = _gmax_fwd(lib, draw, B, C, N)         # (the exact leg has asserted that these equal the oracle's)
    dOut = np.ascontiguousarray(i.g[:, :B].T)                  # (B, C)
    r = O.gmax_bwd_pk(dOut, host(out), argq.cpu().numpy(), host(yarg), i.mean, B, N)
    pre(draw, {"pw.pk0": r.part_abs[:, 0], "pw.pk1": r.part_abs[:, 1]})
    Kf, pk = outbuf((C, B, 2))
    Pf, part = outbuf((1 + EXTRA_ROWS, 2, C))
    d = devs(dOut, i.mean)
    assert lib.o3d_gmax_bwd_pk(ptr(d[0]), ptr(out), ptr(argq), ptr(yarg), ptr(d[1]), B, C, N, ptr(pk), ptr(part), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Kf, Pf)
    assert untouched(part[1:]), "gmax_bwd_pk: a second statistics row was written"
    assert np.array_equal(host(pk[..., 0]), r.pk_g), "gmax_bwd_pk: masked gradient"
    slots = pk.view(torch.int32)[..., 1].cpu().numpy()
    assert np.array_equal(slots, r.pk_slot) and (slots >= 0).all() and (slots < N).all(), "gmax_bwd_pk: slot bits"
    gp = host(part[:1])
    compare("gmax_bwd_pk.part_sum", gp[:, 0], r.part[:, 0], r.part_abs[:, 0], B, draw)
    compare("gmax_bwd_pk.part_gy", gp[:, 1], r.part[:, 1], r.part_abs[:, 1], B, draw)


@pytest.mark.parametrize("B,C,N", O.GMAX_BWD_SHAPES)
def test_gmax_bwd_pk_exact(lib, B, C, N):
    _gmax_bwd(lib, O.Dyadic(400 + B + C + N), B, C, N)


def test_gmax_bwd_pk_rounded(lib):
    for B, C, N in O.GMAX_BWD_SHAPES:
        _gmax_bwd(lib, Randn(11 + C), B, C, N)


# ---- o3d_pool_bwd_partials_split with pk -------------------------------------------------------------------------------------
def _pool_split(lib, draw, C, npoint, nsplit):
    i = O.pool_split_inputs(draw, C, npoint)
    r = O.pool_bwd_partials_split(i.dOut, i.out, i.arg, i.yarg, i.mean, npoint, nsplit)
    pre(draw, {"pw.pk0": r.part_abs[:, 0], "pw.pk1": r.part_abs[:, 1]})
    d = [dev(a) for a in (i.dOut, i.out, i.yarg, i.mean)]
    arg = devi(i.arg)
    for with_pk in (True, False):
        Pf, part = outbuf((nsplit + EXTRA_ROWS, 2, C))
        Kf, pk = outbuf((C, npoint, 2))
        assert lib.o3d_pool_bwd_partials_split(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), C, npoint, nsplit, ptr(part),
                                               ptr(arg) if with_pk else None, ptr(pk) if with_pk else None, st()) == 0
        torch.cuda.synchronize()
        tail_intact(Pf, Kf)
        assert untouched(part[nsplit:]), "pool_bwd_partials_split: a row beyond nsplit was written"
        gp = host(part[:nsplit])
        compare("pool_bwd_split.part_sum", gp[:, 0], r.part[:, 0], r.part_abs[:, 0], r.part_n, draw)
        compare("pool_bwd_split.part_gy", gp[:, 1], r.part[:, 1], r.part_abs[:, 1], r.part_n, draw)
        if with_pk:
            assert np.array_equal(host(pk[..., 0]), r.pk_g), "pool_bwd_partials_split: masked gradient"
            assert np.array_equal(pk.view(torch.int32)[..., 1].cpu().numpy(), r.pk_slot), "pool_bwd_partials_split: slot bits"
        else:
            assert untouched(Kf)


@pytest.mark.parametrize("nsplit", O.POOL_NSPLIT)
@pytest.mark.parametrize("npoint", O.POOL_NPOINT)
@pytest.mark.parametrize("C", O.POOL_C)
def test_pool_bwd_partials_split_exact(lib, C, npoint, nsplit):
    _pool_split(lib, O.Dyadic(500 + C + npoint + nsplit), C, npoint, nsplit)


def test_pool_bwd_partials_split_rounded(lib):
    for C in O.POOL_C:
        for npoint in O.POOL_NPOINT:
            for nsplit in O.POOL_NSPLIT:
                _pool_split(lib, Randn(13 + nsplit), C, npoint, nsplit)


def test_pool_bwd_partials_split_refuses_65_shares(lib):
    C, npoint = 16, 1000
    i = O.pool_split_inputs(O.Dyadic(1), C, npoint)
    d = [dev(a) for a in (i.dOut, i.out, i.yarg, i.mean)]
    arg = devi(i.arg)
    Pf, part = outbuf((65 + EXTRA_ROWS, 2, C))
    Kf, pk = outbuf((C, npoint, 2))
    a = (ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), C, npoint)
    assert lib.o3d_pool_bwd_partials_split(*a, 65, ptr(part), ptr(arg), ptr(pk), st()) == EINVAL
    assert lib.o3d_pool_bwd_partials_split(*a, 3, ptr(part), None, ptr(pk), st()) == EINVAL             # pk without arg
    torch.cuda.synchronize()
    assert untouched(Pf) and untouched(Kf)


# ---- the packed source in the weight gradient: o3d_mlp_conv_wgrad2(dN = NULL, pk, ns) -----------------------------------------
def _pk_wgrad(lib, draw, Cout, Cin, ns, P):
    i = O.PkWgradIn(draw, Cout, Cin, ns, P)
    assert P % ns == 0 and P % 64 == 0
    if draw.exact:                 # balls that hit their first and their last slot, slots in every quarter of a float4, g == 0
        assert (i.slot == 0).any() and (i.slot == ns - 1).any() and len(np.unique(i.slot % 4)) == 4 and (i.g == 0).any()
    pk, dN = pack(i.g, i.slot), dev(i.dN)
    Y, A1, A2, A3, X, sc, sh = (dev(a) for a in (i.Y, i.A1, i.A2, i.A3, i.X, i.in_scale, i.in_shift))
    n = lib.o3d_mlp_conv_wgrad2_scratch(1, Cin, Cout, P)
    assert n > 0
    kind = "wgrad2_pk.%dx%d" % (128 if Cout % 128 == 0 else 64, 128 if Cin % 128 == 0 else 64)
    for xform in (False, True):
        r = O.wgrad(i.dN, i.X, i.Y, i.A1, i.A2, i.A3, i.in_scale if xform else None, i.in_shift if xform else None)
        pre(draw, {"gemm.dW": r.dW_abs})
        outs = []
        for packed in (True, False):
            Sf, scratch = outbuf((n,))                        # exactly the documented floats, then the guarded tail
            Wf, dW = outbuf((Cout, Cin))
            assert lib.o3d_mlp_conv_wgrad2(None if packed else ptr(dN), ptr(pk) if packed else None, ns if packed else 4, ptr(Y),
                                           ptr(A1), ptr(A2), ptr(A3), ptr(X), ptr(sc) if xform else None,
                                           ptr(sh) if xform else None, 1, Cin, Cout, P, ptr(scratch), ptr(dW), st()) == 0
            torch.cuda.synchronize()
            tail_intact(Sf, Wf)
            compare(kind if packed else "wgrad2_pk.dense", host(dW), r.dW, r.dW_abs, r.n, draw)
            outs.append(Wf)
        # the packed source stands for the same numbers in the same places: same tile plan, same order, same bits
        assert torch.equal(outs[0], outs[1]), kind + ": packed and dense sources differ"


@pytest.mark.parametrize("ns,P", O.PK_SHAPES)
@pytest.mark.parametrize("Cout,Cin", O.PK_LAYERS)
def test_wgrad2_packed_source_exact(lib, Cout, Cin, ns, P):
    _pk_wgrad(lib, O.Dyadic(600 + Cout + 2 * Cin + ns), Cout, Cin, ns, P)


@pytest.mark.parametrize("Cout,Cin", O.PK_LAYERS)
def test_wgrad2_packed_source_rounded(lib, Cout, Cin):
    for ns, P in O.PK_SHAPES:
        _pk_wgrad(lib, Randn(17 + ns), Cout, Cin, ns, P)


def test_wgrad2_packed_source_refuses_ns_not_multiple_of_4(lib):
    Cout = Cin = 64
    i = O.PkWgradIn(O.Dyadic(2), Cout, Cin, 32, 384)
    Y, A1, X = dev(i.Y), dev(i.A1), dev(i.X)
    pk = pack(i.g, i.slot)
    Sf, scratch = outbuf((lib.o3d_mlp_conv_wgrad2_scratch(1, Cin, Cout, 384),))
    Wf, dW = outbuf((Cout, Cin))
    for ns in (6, 2, 0):
        assert lib.o3d_mlp_conv_wgrad2(None, ptr(pk), ns, ptr(Y), ptr(A1), ptr(A1), ptr(A1), ptr(X), None, None, 1, Cin, Cout, 384,
                                       ptr(scratch), ptr(dW), st()) == EINVAL
    assert lib.o3d_mlp_conv_wgrad2(None, None, 32, ptr(Y), ptr(A1), ptr(A1), ptr(A1), ptr(X), None, None, 1, Cin, Cout, 384,
                                   ptr(scratch), ptr(dW), st()) == EINVAL                                 # neither source
    torch.cuda.synchronize()
    assert untouched(Sf) and untouched(Wf)


# ---- the packed source in the data gradient: o3d_mlp_conv_dgrad_wt(dN = NULL, ..., pk) ----------------------------------------
def _dgrad_call(lib, i, dN, pk, ns, Cout, Cin, P, G, part, D):
    return lib.o3d_mlp_conv_dgrad_wt(ptr(dN), None, None, None, ns, ptr(D["Y"]), ptr(D["A1"]), ptr(D["A2"]), ptr(D["A3"]),
                                     ptr(D["W"]), ptr(D["Wt"]), ptr(pk), 1, Cin, Cout, P, ptr(D["Yprev"]), ptr(D["scale_p"]),
                                     ptr(D["shift_p"]), ptr(D["mean_p"]), ptr(G), ptr(part), st())


def _dgrad_dev(i):
    D = {k: dev(getattr(i, k)) for k in ("Y", "A1", "A2", "A3", "Yprev", "scale_p", "shift_p", "mean_p")}
    D["Wt"], D["W"] = dev(i.W), dev(i.W.T)                     # i.W is Wt (Cin, Cout); W (Cout, Cin) for the entry's signature
    return D


def _pk_dgrad(lib, draw, Cout, Cin, ns, P):
    assert P % 128 == 0 and P % ns == 0
    i = O.pk_dgrad_inputs(draw, Cout, Cin, ns, P)
    r = O.pw_dgrad(i.X, i.W, i.Y, i.A1, i.A2, i.A3, Yprev=i.Yprev, scale_p=i.scale_p, shift_p=i.shift_p, mean_p=i.mean_p, tile=128)
    pre(draw, {"gemm.G": r.G_abs, "gemm.gpart0": r.part_abs[:, 0], "gemm.gpart1": r.part_abs[:, 1]})
    D, pk, dN, rows = _dgrad_dev(i), pack(i.g, i.slot), dev(i.X), P // 128
    outs = []
    for packed in (True, False):
        k = "dgrad_wt_pk" if packed else "dgrad_wt_pk.dense"
        Gf, G = outbuf((Cin, P))
        Pf, part = outbuf((rows + EXTRA_ROWS, 2, Cin))
        assert _dgrad_call(lib, i, None if packed else dN, pk if packed else None, ns if packed else 4, Cout, Cin, P, G, part,
                           D) == 0
        torch.cuda.synchronize()
        tail_intact(Gf, Pf)
        assert untouched(part[rows:]), k + ": a statistics row beyond P / 128 was written"
        got, gp = host(G), host(part[:rows])
        compare(k + ".G", got, r.G, r.G_abs, r.n, draw)
        assert not got[~r.mask].any(), k
        pr, pa = (r.part, r.part_abs) if draw.exact else O.stats_bwd(got, np.abs(got), i.Yprev, i.mean_p, 128)
        compare(k + ".part_sum", gp[:, 0], pr[:, 0], pa[:, 0], 128, draw)
        compare(k + ".part_gy", gp[:, 1], pr[:, 1], pa[:, 1], 128, draw)
        outs.append((Gf, Pf))
    if draw.exact:                 # (on randn inputs the dense entry may contract in another order: both meet the bound)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "packed and dense sources differ"


PK_DGRAD_SHAPES = [s for s in O.PK_SHAPES + O.PK_DGRAD_EXTRA if s[1] % 128 == 0]


@pytest.mark.parametrize("ns,P", PK_DGRAD_SHAPES)
@pytest.mark.parametrize("Cout,Cin", O.PK_LAYERS)
def test_dgrad_wt_packed_source_exact(lib, Cout, Cin, ns, P):
    _pk_dgrad(lib, O.Dyadic(700 + Cout + 2 * Cin + ns), Cout, Cin, ns, P)


@pytest.mark.parametrize("Cout,Cin", O.PK_LAYERS)
def test_dgrad_wt_packed_source_rounded(lib, Cout, Cin):
    for ns, P in PK_DGRAD_SHAPES:
        _pk_dgrad(lib, Randn(19 + ns), Cout, Cin, ns, P)


@pytest.mark.parametrize("ns,P", [s for s in O.PK_SHAPES if s[1] % 128] + [(6, 384)])
def test_dgrad_wt_packed_source_refusals(lib, ns, P):
    """the packed source runs 128-column tiles only: P = 576 (4.5 tiles) is refused, as is ns % 4 != 0; nothing is written"""
    Cout = Cin = 64
    i = O.G.Inputs(O.Dyadic(3), Cin, Cout, P)
    D = _dgrad_dev(i)
    pk = torch.zeros((Cout, -(-P // ns), 2), device="cuda")
    Gf, G = outbuf((Cin, P))
    Pf, part = outbuf((P // 128 + EXTRA_ROWS, 2, Cin))
    assert _dgrad_call(lib, i, None, pk, ns, Cout, Cin, P, G, part, D) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Gf) and untouched(Pf)


# ---- o3d_cloud_sum_dy -------------------------------------------------------------------------------------------------------
def _cloud(lib, draw, C, B, N):
    i = O.chain_end_inputs(draw, C, B * N)
    r = O.cloud_sum_dy(i.g, i.Y, i.A1, i.A2, i.A3, B, N)
    pre(draw, {"pw.cloud": r.out_abs})
    Of, out = outbuf((C, B))
    d = devs(i.g, i.Y, i.A1, i.A2, i.A3)
    assert lib.o3d_cloud_sum_dy(*map(ptr, d), C, B, N, ptr(out), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Of)
    compare("cloud_sum_dy.out", host(out), r.out, r.out_abs, N, draw)


@pytest.mark.parametrize("C,B,N", O.CLOUD_SHAPES)
def test_cloud_sum_dy_exact(lib, C, B, N):
    _cloud(lib, O.Dyadic(800 + C + N), C, B, N)


def test_cloud_sum_dy_rounded(lib):
    for C, B, N in O.CLOUD_SHAPES:
        _cloud(lib, Randn(23 + C), C, B, N)


def test_cloud_sum_dy_refuses_n_not_multiple_of_4(lib):
    z, one = torch.zeros(64, device="cuda"), torch.ones(2, device="cuda")
    Of, out = outbuf((2, 2))
    assert lib.o3d_cloud_sum_dy(ptr(z), ptr(z), ptr(one), ptr(one), ptr(one), 2, 2, 6, ptr(out), st()) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Of)


# ---- o3d_thin_bwd -----------------------------------------------------------------------------------------------------------
def _thin(lib, draw, groups):
    """P / 64 = 1: one group; 3: fewer groups than the grid of 256; 256: exactly the grid; 257: one workgroup takes two
    groups; 600: two or three groups per workgroup.  Every Cin of the table on the same 64-row operands."""
    P = 64 * groups
    i = O.thin_inputs(draw, P)
    ns = lib.o3d_thin_bwd_scratch()
    assert ns == 256 * 64 * 16
    dN, Y, A1, A2, A3 = (dev(a) for a in (i.dN, i.Y, i.A1, i.A2, i.A3))
    for Cin in O.THIN_CIN:
        X, W = np.ascontiguousarray(i.X[:Cin]), np.ascontiguousarray(i.W[:, :Cin])
        r = O.thin_bwd(i.dN, i.Y, i.A1, i.A2, i.A3, X, W)
        pre(draw, {"pw.thin_dW": r.dW_abs, "pw.thin_dX": r.dX_abs})
        Xd, Wd = dev(X), dev(W)
        runs = []
        for with_dx in (True, True, False):
            Sf, scratch = outbuf((ns,))
            Wf, dW = outbuf((64, Cin))                        # exactly 64 * Cin floats, then the tail
            Xf, dX = outbuf((Cin, P))
            assert lib.o3d_thin_bwd(ptr(dN), ptr(Y), ptr(A1), ptr(A2), ptr(A3), ptr(Xd), ptr(Wd), Cin, 64, P, ptr(scratch), ptr(dW),
                                    ptr(dX) if with_dx else None, st()) == 0
            torch.cuda.synchronize()
            tail_intact(Sf, Wf, Xf)
            compare("thin_bwd.dW", host(dW), r.dW, r.dW_abs, r.dW_n, draw)
            if with_dx:
                compare("thin_bwd.dX", host(dX), r.dX, r.dX_abs, r.dX_n, draw)
            else:
                assert untouched(Xf)
            runs.append((Wf, Xf))
        # every reduction has a fixed order: two runs on the same inputs are bit-identical, on randn inputs too
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "thin_bwd: two runs differ"


@pytest.mark.parametrize("groups", O.THIN_GROUPS)
def test_thin_bwd_exact(lib, groups):
    _thin(lib, O.Dyadic(900 + groups), groups)


@pytest.mark.parametrize("groups", O.THIN_GROUPS)
def test_thin_bwd_rounded(lib, groups):
    _thin(lib, Randn(29 + groups), groups)


def test_thin_bwd_refusals(lib):
    z, one = torch.zeros(64 * 128, device="cuda"), torch.ones(64, device="cuda")
    Sf, scratch = outbuf((lib.o3d_thin_bwd_scratch(),))
    Wf, dW = outbuf((64, 17))
    Xf, dX = outbuf((17, 128))
    for Cin, Cout, P in ((17, 64, 128), (0, 64, 128), (16, 128, 128), (16, 64, 96)):
        assert lib.o3d_thin_bwd(ptr(z), ptr(z), ptr(one), ptr(one), ptr(one), ptr(z), ptr(z), Cin, Cout, P, ptr(scratch), ptr(dW),
                                ptr(dX), st()) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Sf) and untouched(Wf) and untouched(Xf)
