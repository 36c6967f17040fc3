"""The inner-layer GEMM entry points of the compact (distinct-neighbour) layout -- o3d_mlp_conv_fwd_c, o3d_mlp_conv_dgrad_c
(csrc/mlp_direct.hip), o3d_mlp_conv_wgrad2_c, o3d_mlp_conv_bwd_fused_c (csrc/mlp_wgrad.hip) -- called through the C ABI with raw
pointers, launch by launch and per LAUNCH CLASS, against the plain numpy fp64 reference tests/compact_gemm_oracle.py (tied to
Conv2d / BatchNorm2d / ReLU under autograd by tests/test_compact_gemm_oracle_cpu.py).  Same method as
tests/test_gemm_kernels_gpu.py:

EXACT leg: dyadic inputs, sparse weights; the exactness condition of every case is asserted before the launch (and, without a
GPU, by the CPU file over the same inputs); the comparison is EQUALITY -- of the output on every written column, of every
statistics row with the oracle's row for ITS column range, and of everything else with the sentinel: dead tiles, unused extra
rows, the other segment's slot block.
ROUNDED leg: torch.randn inputs, |err| <= (n + 8) * 2^-24 * sum|t_i| per output; the statistics are bounded against the fp64 sums
over the kernel's OWN stored output.  The worst err / bound per kernel and class is printed and, when O3D_COMPACT_GEMM_PINS
names a file, written there (profiles/compact_gemm_kernel_pins.txt is such a run).
POISON: every column the contract says is never read (beyond live256 of each segment) holds NaN in X, Y, dN and Yprev.
CLASS: every forward / data-gradient case first asserts o3d_direct_class(ldp, M, K, tile) -- 2 = 64 x 64 wave tile, 3 = 64 x
128, 4 = split-K -- and, for the 128-column class, o3d_direct_tail_slots(M): 0 for the plain launch, the slot count whose plan
the oracle restates for the remainder split (forced through fused.set_tail_split, or the device's natural one).
FINALIZE: the o3d_bn_finalize / o3d_bn_bwd_finalize job of fused.bn_fin_job / fused.bn_bwd_fin_job (meta, tile 128) runs over the
sentinel-prefilled rows the GEMM just filled; on the exact leg its outputs are bit-identical between no split and every split
(dyadic partials, fp64 sums: the order cannot matter -- a sentinel row read or a written row missed can), and within 1e-5 of the
tensor scale of the oracle's batch statistics.
"""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import compact_gemm_oracle as G

pytestmark = pytest.mark.gpu

SENT = -7.0e37
SENT32 = float(np.float32(SENT))
TAIL = 256
EINVAL = -1
EXTRA_ROWS = 2             # statistics rows allocated beyond the plan's: must stay untouched
EPS, MOMENTUM = 1e-5, 0.1
RATIOS = {}


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi, fused, fused_heads, fused_pointwise  # noqa: F401  (register the signatures)
    return capi.load()


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_COMPACT_GEMM_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per kernel and launch class, rounded leg of tests/test_compact_gemm_kernels_gpu.py\n"
                    "# bound = (n + 8) * 2^-24 * sum|t_i|; every ratio must be <= 1\n"
                    "# c2 = 64 x 64 wave tile, c4 = split-K, c3 = 64 x 128 plain, c3split = 64 x 128 with the remainder split\n")
            for k in sorted(RATIOS):
                f.write("%-34s %.4f\n" % (k, RATIOS[k]))


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


def outbuf(shape):
    """-> (flat buffer with a TAIL of sentinels, view of `shape`)"""
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), SENT, dtype=torch.float32, device="cuda")
    return flat, flat[:n].view(shape)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def tail_intact(*flats):
    for f in flats:
        assert bool((f[-TAIL:] == SENT).all()), "write beyond the buffer"


def untouched(t):
    return bool((t == SENT).all())


def ptr(t):
    return None if t is None else t.data_ptr()


def compare(kernel, got, ref, ref_abs, n, draw):
    """where the oracle holds NaN nothing may have been written (the sentinel is still there); elsewhere -- exact leg:
    equality; rounded leg: |got - ref| <= (n + 8) * 2^-24 * sum|t_i|, worst ratio recorded"""
    got, ref, ref_abs = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(ref_abs, np.float64)
    assert got.shape == ref.shape, kernel
    live = ~np.isnan(ref)
    assert (got[~live] == SENT32).all(), kernel + ": written where nothing may be written"
    assert np.isfinite(got[live]).all() and not (got[live] == SENT32).any(), kernel + ": not written / not finite"
    if draw.exact:
        bad = np.argwhere(live & (got != ref))
        assert len(bad) == 0, (kernel, len(bad), bad[:8].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        return
    bound = ((np.asarray(n, np.float64) + 8) * 2.0 ** -24 * ref_abs)[live]
    err = np.abs(got - ref)[live]
    assert (err[bound == 0] == 0).all(), kernel
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    print("rounded leg %s: worst err/bound %.4f" % (kernel, ratio))
    assert ratio <= 1.0, (kernel, ratio)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def D(i, name):
    """device copy of an operand of compact_gemm_oracle.Inputs (or of its layout: cw, meta), made once"""
    cache = i.__dict__.setdefault("_dev", {})
    if name not in cache:
        if name == "meta":
            cache[name] = torch.from_numpy(np.ascontiguousarray(i.L.meta).astype(np.int32)).cuda()
        elif name == "cw":
            cache[name] = dev(i.L.cw)
        else:
            cache[name] = dev(getattr(i, name))
    return cache[name]


class slots:
    """with slots(lib, S, M): the remainder split forced to S slots (0: off; None: the device's own count) -> the count in
    force for M output rows; always restored"""

    def __init__(self, lib, S, M):
        self.lib, self.S, self.M = lib, S, M

    def __enter__(self):
        from open3dsot_amd import fused
        if self.S is not None:
            fused.set_tail_split(self.S)
        got = self.lib.o3d_direct_tail_slots(self.M)
        if self.S is None:
            assert got > 0, "the natural slot count of %d output rows no longer arms the remainder split" % self.M
        else:
            assert got == self.S
        return got

    def __exit__(self, *exc):
        from open3dsot_amd import fused
        fused.set_tail_split(-1)


def expect_class(lib, cls, ldp, M, K, tile):
    got = lib.o3d_direct_class(ldp, M, K, tile)
    assert got == cls, "this case was written for launch class %d; (ldp, M, K, tile) = (%d, %d, %d, %d) now launches class %d" % (
        cls, ldp, M, K, tile, got)


# ---- one forward / data-gradient launch ------------------------------------------------------------------------------------
def run_fwd(lib, i, tile, S, draw, key):
    L, Cin, Cout = i.L, i.Cin, i.Cout
    r = G.ref_fwd(i, tile, S)
    if draw.exact:
        G.exact_fwd(r)
    Yf, Y = outbuf((Cout, L.ldp))
    Pf, part = outbuf((r.nrows + EXTRA_ROWS, 2, Cout))
    assert lib.o3d_mlp_conv_fwd_c(ptr(D(i, "X")), ptr(D(i, "W")), ptr(D(i, "in_scale")), ptr(D(i, "in_shift")), Cin, Cout, L.ldp,
                                  ptr(D(i, "cw")), ptr(D(i, "meta")), L.start1, tile, ptr(Y), ptr(part), ptr(D(i, "stat_c")),
                                  st()) == 0
    torch.cuda.synchronize()
    tail_intact(Yf, Pf)
    got, gp = host(Y), host(part)
    compare(key + ".Y", got, r.Y, r.Y_abs, r.n, draw)
    assert untouched(part[r.nrows:]), key + ": a statistics row beyond the plan's was written"
    if draw.exact:
        pr, pa = r.part, r.part_abs
    else:                          # the fp64 sums over the stored output: what the epilogue summed
        pr, pa, _ = G.stats_fwd_rows(L, got, np.abs(got), i.stat_c, r.rows, r.nrows)
    n = r.part_n[:, None]
    compare(key + ".part_sum", gp[:r.nrows, 0], pr[:, 0], pa[:, 0], n, draw)
    compare(key + ".part_var", gp[:r.nrows, 1], pr[:, 1], pa[:, 1], n, draw)
    return SimpleNamespace(ref=r, Yf=Yf, part=part[:r.nrows], got=got)


def run_dgrad(lib, i, tile, S, draw, key):
    L, Cin, Cout = i.L, i.Cin, i.Cout
    r = G.ref_dgrad(i, tile, S)
    if draw.exact:
        G.exact_dgrad(r)
    Gf, Gd = outbuf((Cin, L.ldp))
    Pf, part = outbuf((r.nrows + EXTRA_ROWS, 2, Cin))
    assert lib.o3d_mlp_conv_dgrad_c(ptr(D(i, "dN")), ptr(D(i, "Y")), ptr(D(i, "A1")), ptr(D(i, "A2")), ptr(D(i, "A3")),
                                    ptr(D(i, "Wt")), Cin, Cout, L.ldp, ptr(D(i, "cw")), ptr(D(i, "meta")), L.start1, tile,
                                    ptr(D(i, "X")), ptr(D(i, "in_scale")), ptr(D(i, "in_shift")), ptr(D(i, "in_mean")), ptr(Gd),
                                    ptr(part), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Gf, Pf)
    got, gp = host(Gd), host(part)
    compare(key + ".G", got, r.G, r.G_abs, r.n, draw)
    assert not got[~r.mask & ~np.isnan(r.G)].any(), key + ": the ReLU mask"
    assert not got[:, G.padding(L)].any(), key + ": padding columns must come out as zeros"
    assert untouched(part[r.nrows:]), key + ": a statistics row beyond the plan's was written"
    if draw.exact:
        pr, pa = r.part, r.part_abs
    else:
        pr, pa, _ = G.stats_bwd_rows(L, got, np.abs(got), i.X, i.in_mean, r.rows, r.nrows)
    n = r.part_n[:, None]
    compare(key + ".part_sum", gp[:r.nrows, 0], pr[:, 0], pa[:, 0], n, draw)
    compare(key + ".part_gy", gp[:r.nrows, 1], pr[:, 1], pa[:, 1], n, draw)
    return SimpleNamespace(ref=r, Gf=Gf, part=part[:r.nrows], got=got)


RUN = {"fwd": run_fwd, "dgrad": run_dgrad}


# ---- the finalize job over the rows a tile-128 launch just filled -------------------------------------------------------------
def finalize_fwd(lib, i, part):
    """-> (outputs as one tensor list for the bitwise comparison, dict for the oracle)"""
    from open3dsot_amd import fused
    L, C = i.L, i.Cout
    rm0, rv0 = np.asarray(i.stat_c[:C]), np.ones(C)
    bn = SimpleNamespace(running_mean=dev(rm0), running_var=dev(rv0), momentum=MOMENTUM, eps=EPS)
    gamma, beta = dev(i.gamma_o), dev(i.beta_o)
    Vf, vec = outbuf((4, L.nseg, C))
    job = fused.bn_fin_job(part, G.seg_caps(L), G.counts_of(L), bn, gamma, beta, vec, D(i, "stat_c").view(L.nseg, C),
                           D(i, "meta"), 128)
    assert lib.o3d_bn_finalize(ctypes.addressof(job), 1, st()) == 0
    torch.cuda.synchronize()
    tail_intact(Vf)
    got = dict(mean=host(vec[0]), invstd=host(vec[1]), scale=host(vec[2]), shift=host(vec[3]),
               running_mean=host(bn.running_mean), running_var=host(bn.running_var))
    return [vec.clone(), bn.running_mean, bn.running_var], got, (rm0, rv0)


def check_finalize_fwd(i, ref, got, rm_rv, key):
    want = G.bn_fin_ref(ref.tot, G.counts_of(i.L), i.gamma_o, i.beta_o, EPS, i.stat_c, rm_rv[0], rm_rv[1], MOMENTUM)
    for k, v in want.items():
        assert np.isfinite(got[k]).all() and rel(got[k], v) <= 1e-5, (key, k, rel(got[k], v))


def finalize_bwd(lib, i, part, rows=None):
    """the data gradient's rows are the producer's: C = Cin, its gamma / mean / invstd.  rows: the fused entry's part_s
    (rows per segment block, every one live, no meta)"""
    from open3dsot_amd import fused
    L, C = i.L, i.Cin
    gamma, mean, invstd = dev(i.gamma_i), D(i, "in_mean").view(L.nseg, C), dev(i.invstd_i).view(L.nseg, C)
    live = (D(i, "meta"), 128) if rows is None else ()
    job, coef = fused.bn_bwd_fin_job(part, G.seg_caps(L) if rows is None else [rows] * L.nseg, G.counts_of(L), gamma, mean,
                                     invstd, *live)
    assert lib.o3d_bn_bwd_finalize(ctypes.addressof(job), 1, st()) == 0
    torch.cuda.synchronize()
    got = dict(dgamma=host(coef[0, 0]), dbeta=host(coef[1, 0]), A1=host(coef[2]), A2=host(coef[3]), A3=host(coef[4]))
    return [coef[0, 0].clone(), coef[1, 0].clone(), coef[2:].clone()], got


def check_finalize_bwd(i, tot, got, key):
    want = G.bn_bwd_fin_ref(tot, G.counts_of(i.L), i.gamma_i, i.in_mean, i.invstd_i)
    for k, v in want.items():
        assert np.isfinite(got[k]).all() and rel(got[k], v) <= 1e-5, (key, k, rel(got[k], v))


def launch_and_finalize(lib, kind, i, S, M, draw, key):
    with slots(lib, S, M) as s_eff:
        run = RUN[kind](lib, i, 128, s_eff, draw, key)
        if kind == "fwd":
            outs, got, rm_rv = finalize_fwd(lib, i, run.part)
            check_finalize_fwd(i, run.ref, got, rm_rv, key)
        else:
            outs, got = finalize_bwd(lib, i, run.part)
            check_finalize_bwd(i, run.ref.tot, got, key)
    return run, outs, s_eff


# ---- the classes ---------------------------------------------------------------------------------------------------------------
def _plain(lib, kind, case, draw):
    fam, M, K, tile, cls = case
    L = G.layout(fam)
    expect_class(lib, cls, L.ldp, M, K, tile)
    Cin, Cout = G.kind_dims(kind, M, K)
    i = G.Inputs(draw, L, Cin, Cout)
    key = "%s_c.c%d" % (kind, cls)
    if tile == 128:
        launch_and_finalize(lib, kind, i, 0, M, draw, key)
    else:
        RUN[kind](lib, i, tile, 0, draw, key)


def _split(lib, kind, case, draw):
    fam, S, M, K = case
    L = G.layout(fam)
    expect_class(lib, 3, L.ldp, M, K, 128)
    Cin, Cout = G.kind_dims(kind, M, K)
    i = G.Inputs(draw, L, Cin, Cout)
    split, outs, s_eff = launch_and_finalize(lib, kind, i, S, M, draw, "%s_c.c3split" % kind)
    if not draw.exact:
        return
    plain, outs0, _ = launch_and_finalize(lib, kind, i, 0, M, draw, "%s_c.c3" % kind)
    # the same MFMA chains on the same operands: the stored output is the same, bit for bit
    assert torch.equal(split.Yf if kind == "fwd" else split.Gf, plain.Yf if kind == "fwd" else plain.Gf)
    for a, b in zip(outs, outs0):
        assert torch.equal(a, b), "the finalize over the split launch's rows differs from the one over the plain launch's"
    why = G.plan_reasons(L, s_eff)
    if any(w in ("f4", "f2") for w, _ in why):
        assert len(split.ref.rows) > len(plain.ref.rows) and not torch.equal(split.part[:L.ldp // 128], plain.part)


@pytest.mark.parametrize("case", G.PLAIN_CASES, ids=lambda c: "%s-%dx%d-t%d-c%d" % c)
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_plain_exact(lib, kind, case):
    fam, M, K, _, _ = case
    _plain(lib, kind, case, G.Dyadic(G.case_seed(kind, fam, M, K)))


@pytest.mark.parametrize("case", G.SPLIT_CASES, ids=lambda c: "%s-S%s-%dx%d" % c)
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_remainder_split_exact(lib, kind, case):
    fam, _, M, K = case
    _split(lib, kind, case, G.Dyadic(G.case_seed(kind, fam, M, K)))


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_plain_rounded(lib, kind):
    for n, case in enumerate(G.PLAIN_CASES):
        _plain(lib, kind, case, Randn(61 + n))


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_remainder_split_rounded(lib, kind):
    for n, case in enumerate(G.SPLIT_CASES):
        _split(lib, kind, case, Randn(71 + n))


def test_split_cases_reach_every_branch_on_this_device(lib):
    """the CPU file asserts the coverage for 256 compute units; here with the slot counts of the device in use"""
    cases = [(f, S if S is not None else lib.o3d_direct_tail_slots(M), M, K) for f, S, M, K in G.SPLIT_CASES]
    assert G.split_coverage(cases) == G.SPLIT_BRANCHES


def test_direct_class_rules(lib):
    """the export itself, at the edges of every rule of csrc/mlp_direct.hip it restates"""
    c = lib.o3d_direct_class
    assert [c(6144, 64, 16, 64), c(6144, 64, 48, 64), c(6144, 64, 64, 64), c(65536, 256, 64, 64)] == [2, 2, 4, 4]
    assert c(65536, 512, 64, 64) == 2                          # M * ldp above splitk_max(): back on the unsplit tile
    assert [c(6144, 64, 64, 128), c(6144, 256, 16, 128), c(1 << 20, 64, 64, 128)] == [3, 3, 3]
    assert [c(0, 64, 64, 64), c(6144 + 64, 64, 64, 64), c(6144, 32, 64, 64), c(6144, 64, 8, 64), c(6144, 64, 64, 32),
            c(6144, 64, 64, 256), c(1 << 31, 64, 64, 128)] == [-1] * 7
    assert lib.o3d_direct_tile(65536, 64, 1) == 64 and lib.o3d_direct_tile(65536 + 128, 64, 1) == 128


# ---- weight gradient -----------------------------------------------------------------------------------------------------------
def run_wgrad(lib, i, draw, key):
    L, Cin, Cout = i.L, i.Cin, i.Cout
    r = G.ref_wgrad(i)
    if draw.exact:
        G.assert_exact("cg.dW", r.dW_abs)
    n = lib.o3d_mlp_conv_wgrad2_scratch(1, Cin, Cout, L.ldp)
    assert n > 0
    Sf, scratch = outbuf((n,))                                # exactly the documented floats, then the guarded tail
    Wf, dW = outbuf((Cout, Cin))
    assert lib.o3d_mlp_conv_wgrad2_c(ptr(D(i, "dN")), ptr(D(i, "Y")), ptr(D(i, "A1")), ptr(D(i, "A2")), ptr(D(i, "A3")),
                                     ptr(D(i, "X")), ptr(D(i, "in_scale")), ptr(D(i, "in_shift")), Cin, Cout, L.ldp,
                                     ptr(D(i, "cw")), ptr(D(i, "meta")), L.start1, ptr(scratch), ptr(dW), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Sf, Wf)
    compare(key, host(dW), r.dW, r.dW_abs, r.n, draw)
    return Wf


def _wg_key(Cout, Cin):
    return "wgrad2_c.%dx%d" % (128 if Cout % 128 == 0 else 64, 128 if Cin % 128 == 0 else 64)


@pytest.mark.parametrize("case", G.WGRAD_CASES, ids=lambda c: "%s-%dx%d" % c)
def test_wgrad2_c_exact(lib, case):
    fam, Cout, Cin = case
    run_wgrad(lib, G.Inputs(G.Dyadic(G.case_seed("wgrad", fam, Cout, Cin)), G.layout(fam), Cin, Cout), G.Dyadic(0), _wg_key(Cout, Cin))


def test_wgrad2_c_rounded(lib):
    for n, (fam, Cout, Cin) in enumerate(G.WGRAD_CASES):
        draw = Randn(81 + n)
        run_wgrad(lib, G.Inputs(draw, G.layout(fam), Cin, Cout), draw, _wg_key(Cout, Cin))


# ---- data + weight gradient in one launch ----------------------------------------------------------------------------------
def _fused(lib, case, draw):
    fam, Cout, dead = case
    Cin = 64
    dense = not isinstance(fam, str)
    L = G.Dense(fam) if dense else G.layout(fam)
    i = G.Inputs(draw, L, Cin, Cout, dead_channel=dead)
    r, rw = G.ref_dgrad(i, 64), G.ref_wgrad(i)
    if draw.exact:
        G.exact_dgrad(r), G.exact_fused(i, r), G.assert_exact("cg.dW", rw.dW_abs)
    rows = lib.o3d_mlp_conv_bwd_fused_rows(Cin, Cout, L.ldp)
    nscr = lib.o3d_mlp_conv_bwd_fused_scratch(Cin, Cout, L.ldp)
    assert rows > 0 and nscr > 0
    Sf, scratch = outbuf((nscr,))
    Wf, dW = outbuf((Cout, Cin))
    Pf, part_s = outbuf((2, rows, 2, Cin))
    Gf, Gd = outbuf((Cin, L.ldp))
    cw, meta = (None, None) if dense else (ptr(D(i, "cw")), ptr(D(i, "meta")))
    assert lib.o3d_mlp_conv_bwd_fused_c(ptr(D(i, "dN")), ptr(D(i, "Y")), ptr(D(i, "A1")), ptr(D(i, "A2")), ptr(D(i, "A3")),
                                        ptr(D(i, "X")), ptr(D(i, "in_scale")), ptr(D(i, "in_shift")), ptr(D(i, "in_mean")),
                                        ptr(D(i, "Wt")), Cin, Cout, L.ldp, cw, meta, L.start1, ptr(scratch), ptr(dW),
                                        ptr(part_s), ptr(Gd), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Sf, Wf, Pf, Gf)
    key = "bwd_fused_c.%d%s" % (Cout, "dense" if dense else "")
    compare(key + ".dW", host(dW), rw.dW, rw.dW_abs, rw.n, draw)
    got = host(Gd)
    compare(key + ".G", got, r.G, r.G_abs, r.n, draw)
    assert not got[~r.mask & ~np.isnan(r.G)].any() and not got[:, G.padding(L)].any()
    ps = host(part_s)
    # the finalize reads all `rows` rows of a used segment block (meta = NULL): every one must have been written
    assert np.isfinite(ps[:L.nseg]).all() and not (ps[:L.nseg] == SENT32).any(), key + ": an unwritten row of part_s"
    tot = ps[:L.nseg].sum(1)                                                         # (nseg, 2, Cin), fp64 sums of fp32 rows
    if draw.exact:
        want, want_abs = r.tot, r.tot_abs
    else:
        want, want_abs, _ = G.stats_bwd_rows(L, got, np.abs(got), i.X, i.in_mean, *G.seg_rows(L))
        want_abs[:, 1] = G.fused_second_abs(L, np.abs(got), i.X, i.in_scale, i.in_shift, i.in_mean)[2]
    n = np.asarray(L.live256, np.float64)[:, None]
    compare(key + ".part_sum", tot[:, 0], want[:, 0], want_abs[:, 0], n, draw)
    compare(key + ".part_gy", tot[:, 1], want[:, 1], want_abs[:, 1], n, draw)
    _, fin = finalize_bwd(lib, i, part_s, rows=rows)
    check_finalize_bwd(i, r.tot, fin, key)
    if draw.exact and not dense:       # "replaces the pair o3d_mlp_conv_wgrad2_c + o3d_mlp_conv_dgrad_c": the same numbers
        tile = lib.o3d_direct_tile(L.ldp, Cin, 1)
        Wf2 = run_wgrad(lib, i, draw, _wg_key(Cout, Cin))
        pair = run_dgrad(lib, i, tile, 0, draw, "dgrad_c.c%d" % lib.o3d_direct_class(L.ldp, Cin, Cout, tile))
        assert torch.equal(Wf, Wf2) and torch.equal(Gf, pair.Gf)
        pp, ptot = host(pair.part), np.zeros_like(tot)
        for row, _, _, sg in pair.ref.rows:
            ptot[sg] += pp[row]
        assert np.array_equal(ptot, tot)


@pytest.mark.parametrize("case", G.FUSED_CASES, ids=lambda c: "%s-%d-%s" % c)
def test_bwd_fused_c_exact(lib, case):
    _fused(lib, case, G.Dyadic(G.case_seed("fused", case[0], case[1])))


def test_bwd_fused_c_rounded(lib):
    for n, case in enumerate(G.FUSED_CASES):
        _fused(lib, case, Randn(91 + n))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched(lib):
    L = G.layout("paired")
    i = G.Inputs(G.Dyadic(3), L, 64, 64)
    Yf, Y = outbuf((64, L.ldp))
    Pf, part = outbuf((L.ldp // 64, 2, 64))
    Wf, dW = outbuf((64, 64))
    Sf, scr = outbuf((lib.o3d_mlp_conv_wgrad2_scratch(1, 64, 64, L.ldp),))
    X, W, sc, sh, cw, meta, stc = (ptr(D(i, n)) for n in ("X", "W", "in_scale", "in_shift", "cw", "meta", "stat_c"))

    def fwd(X=X, W=W, sc=sc, sh=sh, Cin=64, Cout=64, ldp=L.ldp, cw=cw, meta=meta, tile=64, Yp=ptr(Y)):
        return lib.o3d_mlp_conv_fwd_c(X, W, sc, sh, Cin, Cout, ldp, cw, meta, L.start1, tile, Yp, ptr(part), stc, st())
    for bad in (dict(X=None), dict(W=None), dict(sc=None), dict(sh=None), dict(cw=None), dict(meta=None), dict(Yp=None),
                dict(tile=32), dict(tile=256), dict(tile=0), dict(ldp=L.ldp + 64), dict(ldp=0), dict(ldp=1 << 31),
                dict(Cout=32), dict(Cout=96), dict(Cin=8)):
        assert fwd(**bad) == EINVAL, bad
    dN, Yl, A1, A2, A3, Wt, mu = (ptr(D(i, n)) for n in ("dN", "Y", "A1", "A2", "A3", "Wt", "in_mean"))

    def dgrad(dN=dN, A1=A1, Wt=Wt, Cin=64, Cout=64, ldp=L.ldp, cw=cw, meta=meta, tile=64, Yprev=X, sp=sc, mp=mu, out=ptr(Y),
              pp=ptr(part)):
        return lib.o3d_mlp_conv_dgrad_c(dN, Yl, A1, A2, A3, Wt, Cin, Cout, ldp, cw, meta, L.start1, tile, Yprev, sp, sh, mp, out,
                                        pp, st())
    for bad in (dict(dN=None), dict(A1=None), dict(Wt=None), dict(cw=None), dict(meta=None), dict(Yprev=None), dict(sp=None),
                dict(mp=None), dict(out=None), dict(pp=None), dict(tile=32), dict(tile=192), dict(ldp=L.ldp + 64),
                dict(ldp=1 << 31), dict(Cin=32), dict(Cout=8)):
        assert dgrad(**bad) == EINVAL, bad

    def wgrad(dN=dN, Yl=Yl, X=X, sc=sc, sh=sh, Cin=64, Cout=64, ldp=L.ldp, cw=cw, meta=meta, start1=L.start1, s=ptr(scr), o=ptr(dW)):
        return lib.o3d_mlp_conv_wgrad2_c(dN, Yl, A1, A2, A3, X, sc, sh, Cin, Cout, ldp, cw, meta, start1, s, o, st())
    for bad in (dict(dN=None), dict(Yl=None), dict(X=None), dict(sc=None), dict(sh=None), dict(cw=None), dict(meta=None),
                dict(s=None), dict(o=None), dict(start1=L.start1 + 128), dict(start1=-256), dict(ldp=L.ldp + 32), dict(ldp=0),
                dict(ldp=1 << 31), dict(Cin=48), dict(Cout=96)):
        assert wgrad(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert untouched(Yf) and untouched(Pf) and untouched(Wf) and untouched(Sf)
