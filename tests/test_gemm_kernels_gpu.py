"""The flat-layout (C, P) GEMM entry points -- o3d_pw_fwd, o3d_pw_dgrad, their pairs, o3d_pw_fwd_cloud (csrc/mlp_direct.hip),
o3d_mlp_conv_wgrad2 (B = 1, dense dN) and o3d_mlp_conv_wgrad2_group (csrc/mlp_wgrad.hip) -- called through the C ABI with raw
pointers, launch by launch and per LAUNCH CLASS, against the plain numpy fp64 reference tests/gemm_oracle.py (tied to
Conv1d / BatchNorm1d / ReLU under autograd by tests/test_gemm_oracle_cpu.py).  The packed max-gradient source of the weight and
data gradient (dN = NULL, pk) is pinned next to its producers in tests/test_pointwise_kernels_gpu.py.  Same method as
tests/test_compact_kernels_gpu.py:

EXACT leg: every floating-point input lies on a small dyadic grid (sparse weights for the larger K), so every product and
every partial sum of a correct kernel is exactly representable in fp32 whatever its summation order (asserted before each
launch: sum|terms| / spacing < 2^24), and the comparison is EQUALITY.  A reordered sum -- the split-K kernel's four quarters,
the weight gradient's slices -- still passes; a dropped, duplicated or misplaced term does not.
ROUNDED leg: torch.randn inputs, |err| <= (n + 8) * 2^-24 * sum|t_i| per output.  The statistics partials are bounded against
the fp64 sums over the kernel's OWN stored output, read back (the stored fp32 values are exactly what the epilogue summed:
n = columns per tile); the stored output is itself bounded against the oracle.  The worst err / bound per kernel and class is
printed and, when O3D_GEMM_PINS names a file, written there (profiles/gemm_kernel_pins.txt is such a run).
GUARDS: every output buffer has a 256-element tail and is prefilled with a sentinel; the tail, the statistics rows beyond
P / tile, the scratch beyond o3d_mlp_conv_wgrad2_scratch(...) and everything outside a compact (out_rows, out_cols) gradient
must still hold it after the call.
CLASS: every forward / data-gradient case first asserts o3d_pw_class(P, M, K), the launcher's own rule (2 = 64 x 64 wave
tile, 3 = 64 x 128, 4 = split-K, 5 = 32-row narrow tile): when a threshold is retuned the case that lost its class fails by
name instead of silently testing another kernel.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import gemm_oracle as O

pytestmark = pytest.mark.gpu

SENT = -7.0e37
TAIL = 256
EINVAL = -1
RATIOS = {}
P_BIG = 65664              # the first multiple of 128 above the 64-column threshold of o3d_direct_tile


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi, fused, fused_heads, fused_pointwise  # noqa: F401  (register the signatures)
    return capi.load()


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_GEMM_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per kernel and launch class, rounded leg of tests/test_gemm_kernels_gpu.py\n"
                    "# bound = (n + 8) * 2^-24 * sum|t_i|; every ratio must be <= 1\n"
                    "# pair rows carry the class of the single launches (c5: the pair itself runs 64-row waves)\n")
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


def pre(draw, **abs_sums):
    """before the launch: the exact leg's inputs keep every partial sum of these outputs exact in fp32"""
    if draw.exact:
        for k, v in abs_sums.items():
            O.assert_exact("gemm." + k, v)


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


def expect_class(lib, cls, P, M, K):
    got = lib.o3d_pw_class(P, M, K)
    assert got == cls, "this case was written for launch class %d; (P, M, K) = (%d, %d, %d) now launches class %d" % (
        cls, P, M, K, got)
    tile = lib.o3d_pw_tile(P, M)
    assert tile == (64 if cls in (2, 4) else 128)
    return tile


def D(i, name):
    """device copy of an operand of gemm_oracle.Inputs, made once"""
    cache = i.__dict__.setdefault("_dev", {})
    if name not in cache:
        cache[name] = dev(getattr(i, name))
    return cache[name]


# ---- one forward / data-gradient problem: operands, reference, output buffers, the call, the check --------------------------
FWD_EPI = ("part", "none", "bias", "resid", "bias+resid")
FWD_VARIANTS = [(x, e) for x in (False, True) for e in FWD_EPI]
DG_EPI = ("mask", "plain", "resid")
DG_VARIANTS = [(y, e) for y in (False, True) for e in DG_EPI]
EXTRA_ROWS = 2             # statistics rows allocated beyond P / tile: must stay untouched


class Fwd:
    """o3d_pw_fwd: Y (M, P) = W (M, K) . f(X); xform: f = relu(x * in_scale + in_shift) (and a stat_c), else identity"""
    entry, pair_entry = "o3d_pw_fwd", "o3d_pw_fwd_pair"

    def __init__(self, lib, draw, cls, M, K, P, xform, epi, inputs=None, like=None):
        self.tile = expect_class(lib, cls, P, M, K)
        self.draw, self.cls, self.M, self.K, self.P, self.epi = draw, cls, M, K, P, epi
        self.i = i = inputs if inputs is not None else O.Inputs(draw, M, K, P)
        self.stat_c = i.stat_c if xform else None
        sc, sh = (i.in_scale, i.in_shift) if xform else (None, None)
        if like is None:                   # (like: a second launch of the same problem shares its reference)
            self.ref = r = O.pw_fwd(i.X, i.W, sc, sh, i.bias if "bias" in epi else None, i.resid if "resid" in epi else None,
                                    tile=self.tile if epi == "part" else None, stat_c=self.stat_c)
            pre(draw, Y=r.Y_abs)
            if epi == "part":
                pre(draw, part0=r.part_abs[:, 0], part1=r.part_abs[:, 1])
        else:
            self.ref = like.ref
        self.Yf, self.Y = outbuf((M, P))
        self.Pf, self.part = outbuf((P // self.tile + EXTRA_ROWS, 2, M))
        self.fields = (ptr(D(i, "X")), ptr(D(i, "W")), ptr(D(i, "in_scale")) if xform else None,
                       ptr(D(i, "in_shift")) if xform else None, ptr(D(i, "bias")) if "bias" in epi else None,
                       ptr(D(i, "resid")) if "resid" in epi else None, K, M, P, ptr(self.Y),
                       ptr(self.part) if epi == "part" else None, ptr(D(i, "stat_c")) if xform else None)

    def struct(self):
        from open3dsot_amd.fused_heads import _PwFwdArgs
        return _PwFwdArgs(*self.fields)

    def check(self, what):
        tail_intact(self.Yf, self.Pf)
        r, k = self.ref, "%s.c%d" % (what, self.cls)
        self.got = got = host(self.Y)
        compare(k + ".Y", got, r.Y, r.Y_abs, r.n, self.draw)
        if self.epi != "part":
            assert untouched(self.part), k
            return
        rows = self.P // self.tile
        gp = host(self.part)
        assert untouched(self.part[rows:]), k + ": a statistics row beyond P / tile was written"
        if self.draw.exact:
            pr, pa = r.part, r.part_abs
        else:                          # the fp64 sums over the stored output: what the epilogue summed, n = tile
            pr, pa = O.stats_fwd(got, np.abs(got), self.tile, self.stat_c)
        compare(k + ".part_sum", gp[:rows, 0], pr[:, 0], pa[:, 0], self.tile, self.draw)
        compare(k + ".part_var", gp[:rows, 1], pr[:, 1], pa[:, 1], self.tile, self.draw)


class Dgrad:
    """o3d_pw_dgrad: G (M, P) = Wt (M, K) . dY; with_y: dY = A1*dN + A2*Y + A3, else dN; epi mask / plain / resid"""
    entry, pair_entry = "o3d_pw_dgrad", "o3d_pw_dgrad_pair"

    def __init__(self, lib, draw, cls, M, K, P, with_y, epi, inputs=None, like=None):
        self.tile = expect_class(lib, cls, P, M, K)
        self.draw, self.cls, self.M, self.K, self.P, self.epi = draw, cls, M, K, P, epi
        self.i = i = inputs if inputs is not None else O.Inputs(draw, M, K, P)
        ya = dict(Y=i.Y, A1=i.A1, A2=i.A2, A3=i.A3) if with_y else {}
        if like is not None:
            self.ref = like.ref
        elif epi == "mask":
            self.ref = r = O.pw_dgrad(i.X, i.W, Yprev=i.Yprev, scale_p=i.scale_p, shift_p=i.shift_p, mean_p=i.mean_p,
                                      tile=self.tile, **ya)
            pre(draw, G=r.G_abs, gpart0=r.part_abs[:, 0], gpart1=r.part_abs[:, 1])
        else:
            self.ref = r = O.pw_dgrad(i.X, i.W, resid=i.resid if epi == "resid" else None, **ya)
            pre(draw, G=r.G_abs)
        self.Gf, self.G = outbuf((M, P))
        self.Pf, self.part = outbuf((P // self.tile + EXTRA_ROWS, 2, M))
        m = epi == "mask"
        self.fields = (ptr(D(i, "X")),) + tuple(ptr(D(i, n)) if with_y else None for n in ("Y", "A1", "A2", "A3")) + (
            ptr(D(i, "W")), M, K, P) + tuple(ptr(D(i, n)) if m else None for n in ("Yprev", "scale_p", "shift_p", "mean_p")) + (
            ptr(D(i, "resid")) if epi == "resid" else None, ptr(self.G), ptr(self.part) if m else None)

    def struct(self):
        from open3dsot_amd.fused_heads import _PwDgradArgs
        return _PwDgradArgs(*self.fields)

    def check(self, what):
        tail_intact(self.Gf, self.Pf)
        r, k = self.ref, "%s.c%d" % (what, self.cls)
        self.got = got = host(self.G)
        compare(k + ".G", got, r.G, r.G_abs, r.n, self.draw)
        if self.epi != "mask":
            assert untouched(self.part), k
            return
        # the mask: one fmaf in the kernel, whose sign is the exact sign; the oracle evaluates the same expression in fp64
        assert not got[~r.mask].any(), k
        rows = self.P // self.tile
        gp = host(self.part)
        assert untouched(self.part[rows:]), k + ": a statistics row beyond P / tile was written"
        if self.draw.exact:
            pr, pa = r.part, r.part_abs
        else:
            pr, pa = O.stats_bwd(got, np.abs(got), self.i.Yprev, self.i.mean_p, self.tile)
        compare(k + ".part_sum", gp[:rows, 0], pr[:, 0], pa[:, 0], self.tile, self.draw)
        compare(k + ".part_gy", gp[:rows, 1], pr[:, 1], pa[:, 1], self.tile, self.draw)


def single(lib, prob):
    assert getattr(lib, prob.entry)(*prob.fields, st()) == 0
    torch.cuda.synchronize()
    prob.check(prob.entry[4:])


def sweep(lib, draw, kind, cls, Ms, Ks, Ps, variants):
    for M in Ms:
        for K in Ks:
            for P in Ps:
                i = O.Inputs(draw, M, K, P)
                for a, epi in variants:
                    single(lib, kind(lib, draw, cls, M, K, P, a, epi, inputs=i))


# ---- class 2 (unsplit, 64 columns: K < 64) and class 4 (split-K) ---------------------------------------------------------
C2 = dict(Ks=(16, 48), Ms=(64, 128, 192, 256), Ps=(64, 192))        # M / 64 = 1, 2, 3, 4: 1, 2, 1 (x3) and 4 waves
C4 = dict(Ks=(64, 80, 96, 272), Ms=(64, 192), Ps=(64, 192))        # 80, 272: the 16-k pairs do not divide over the 4 waves
KINDS = {"fwd": (Fwd, FWD_VARIANTS), "dgrad": (Dgrad, DG_VARIANTS)}


@pytest.mark.parametrize("K", C2["Ks"])
@pytest.mark.parametrize("M", C2["Ms"])
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_class2_exact(lib, kind, M, K):
    sweep(lib, O.Dyadic(1000 + M + K), KINDS[kind][0], 2, (M,), (K,), C2["Ps"], KINDS[kind][1])


@pytest.mark.parametrize("K", C4["Ks"])
@pytest.mark.parametrize("M", C4["Ms"])
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_class4_splitk_exact(lib, kind, M, K):
    sweep(lib, O.Dyadic(2000 + M + K), KINDS[kind][0], 4, (M,), (K,), C4["Ps"], KINDS[kind][1])


@pytest.mark.parametrize("cls,shapes", [(2, C2), (4, C4)])
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_class2_class4_rounded(lib, kind, cls, shapes):
    sweep(lib, Randn(31 + cls), KINDS[kind][0], cls, shapes["Ms"], shapes["Ks"], shapes["Ps"], KINDS[kind][1])


# ---- classes 3 and 5 (128 columns: P > 65536) --------------------------------------------------------------------------
def _big(lib, draw, cls, M):
    i = O.Inputs(draw, M, 16, P_BIG)
    single(lib, Fwd(lib, draw, cls, M, 16, P_BIG, True, "part", inputs=i))
    single(lib, Fwd(lib, draw, cls, M, 16, P_BIG, False, "bias+resid", inputs=i))
    single(lib, Dgrad(lib, draw, cls, M, 16, P_BIG, True, "mask", inputs=i))
    single(lib, Dgrad(lib, draw, cls, M, 16, P_BIG, False, "plain", inputs=i))


@pytest.mark.parametrize("cls,M", [(3, 192), (3, 256), (5, 64), (5, 128)])
def test_class3_class5_exact(lib, cls, M):
    _big(lib, O.Dyadic(3000 + M), cls, M)


@pytest.mark.parametrize("cls,M", [(3, 192), (3, 256), (5, 64), (5, 128)])
def test_class3_class5_rounded(lib, cls, M):
    _big(lib, Randn(37 + M), cls, M)


def test_128_column_class_refuses_p_not_multiple_of_128(lib):
    P, M, K = 65600, 64, 16
    assert P % 64 == 0 and lib.o3d_pw_class(P, M, K) == -1
    i = O.Inputs(O.Dyadic(5), M, K, 64)
    x = torch.zeros(K * P, device="cuda")
    Yf, Y = outbuf((M, P))
    Pf, part = outbuf((P // 64, 2, M))
    assert lib.o3d_pw_fwd(ptr(x), ptr(D(i, "W")), None, None, None, None, K, M, P, ptr(Y), ptr(part), None, st()) == EINVAL
    assert lib.o3d_pw_dgrad(ptr(x), None, None, None, None, ptr(D(i, "W")), M, K, P, None, None, None, None, None, ptr(Y), None,
                            st()) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Yf) and untouched(Pf)


def test_pw_class_rules(lib):
    """the export itself, at the edges of every rule of csrc/mlp_direct.hip it restates"""
    c = lib.o3d_pw_class
    assert [c(64, 64, 16), c(64, 64, 48), c(64, 64, 64), c(65536, 256, 64)] == [2, 2, 4, 4]
    assert c(65536, 512, 64) == 2                               # M * P above splitk_max(): back on the unsplit tile
    assert [c(P_BIG, 64, 16), c(P_BIG, 128, 272), c(P_BIG, 192, 16), c(P_BIG, 256, 272)] == [5, 5, 3, 3]
    assert [c(0, 64, 16), c(96, 64, 16), c(64, 32, 16), c(64, 64, 8), c(65600, 64, 16), c(1 << 31, 64, 16)] == [-1] * 6


# ---- o3d_pw_fwd_cloud ------------------------------------------------------------------------------------------------------
def _cloud(lib, draw, B, N, Cout, with_c):
    Cin, P = 16, B * N
    i = O.Inputs(draw, Cout, Cin, P)
    cb = draw.val((Cout, B), 0.125, 1.0) + 2.0 * np.arange(B)[None, :]      # a distinct bias per cloud: the cloud index shows
    stat_c = i.stat_c if with_c else None
    r = O.pw_fwd_cloud(i.X, i.W, cb, N, stat_c)
    pre(draw, Y=r.Y_abs, part0=r.part_abs[:, 0], part1=r.part_abs[:, 1])
    Yf, Y = outbuf((Cout, P))
    Pf, part = outbuf((P // 128 + EXTRA_ROWS, 2, Cout))
    cbd = dev(cb)
    assert lib.o3d_pw_fwd_cloud(ptr(D(i, "X")), ptr(D(i, "W")), ptr(cbd), B, N, Cin, Cout, ptr(Y), ptr(part),
                                ptr(D(i, "stat_c")) if with_c else None, st()) == 0
    torch.cuda.synchronize()
    tail_intact(Yf, Pf)
    got, gp, rows = host(Y), host(part), P // 128
    compare("pw_fwd_cloud.Y", got, r.Y, r.Y_abs, r.n, draw)
    assert untouched(part[rows:])
    pr, pa = (r.part, r.part_abs) if draw.exact else O.stats_fwd(got, np.abs(got), 128, stat_c)
    compare("pw_fwd_cloud.part_sum", gp[:rows, 0], pr[:, 0], pa[:, 0], 128, draw)
    compare("pw_fwd_cloud.part_var", gp[:rows, 1], pr[:, 1], pa[:, 1], 128, draw)


@pytest.mark.parametrize("with_c", [False, True])
@pytest.mark.parametrize("Cout", [64, 192])
@pytest.mark.parametrize("B,N", [(1, 128), (3, 128), (2, 256)])
def test_pw_fwd_cloud_exact(lib, B, N, Cout, with_c):
    _cloud(lib, O.Dyadic(4000 + B + N + Cout), B, N, Cout, with_c)


@pytest.mark.parametrize("with_c", [False, True])
@pytest.mark.parametrize("Cout", [64, 192])
def test_pw_fwd_cloud_rounded(lib, Cout, with_c):
    for B, N in ((1, 128), (3, 128), (2, 256)):
        _cloud(lib, Randn(41 + B), B, N, Cout, with_c)


# ---- pairs ---------------------------------------------------------------------------------------------------------------
def _pair(lib, kind, draw, cls_a, cls_b, pa, pb):
    """pa / pb = (M, K, P, operand flag, epilogue): the pair launch against the oracle, and bit for bit against the two
    single launches (include/o3dsot.h: "the numbers are the same either way")"""
    probs, singles = [], []
    for cls, (M, K, P, a, epi) in ((cls_a, pa), (cls_b, pb)):
        i = O.Inputs(draw, M, K, P)
        probs.append(kind(lib, draw, cls, M, K, P, a, epi, inputs=i))
        singles.append(kind(lib, draw, cls, M, K, P, a, epi, inputs=i, like=probs[-1]))
    sa, sb = probs[0].struct(), probs[1].struct()
    assert getattr(lib, kind.pair_entry)(ctypes.addressof(sa), ctypes.addressof(sb), st()) == 0
    torch.cuda.synchronize()
    for p, s in zip(probs, singles):
        p.check(kind.pair_entry[4:])
        assert getattr(lib, s.entry)(*s.fields, st()) == 0
        torch.cuda.synchronize()
        out_p, out_s = (p.Yf, s.Yf) if kind is Fwd else (p.Gf, s.Gf)      # (whole buffers: tails and spare rows included)
        assert torch.equal(out_p, out_s) and torch.equal(p.Pf, s.Pf), "pair and single launches differ"


PAIR_CASES = {
    # one launch, 1-wave branch (1 and 4 row slabs): the smaller problem's surplus row blocks must write nothing
    "class2": (2, 2, (64, 16, 192), (256, 16, 192)),
    "class4": (4, 4, (64, 80, 192), (192, 80, 192)),
    "class3": (3, 3, (256, 16, P_BIG), (256, 16, P_BIG)),
    # M <= 128 over 128-column tiles: the pair runs 64-row waves (class 3), the single launches 32-row waves (class 5); the
    # header's "same numbers" is held to bit for bit here too -- what that proves on randn inputs: test_pair_rounded
    "narrow": (5, 5, (128, 16, P_BIG), (64, 16, P_BIG)),
    "different_classes": (2, 4, (64, 48, 192), (64, 64, 192)),      # two single launches
}


@pytest.mark.parametrize("case", list(PAIR_CASES))
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_pair_exact(lib, kind, case):
    ca, cb, a, b = PAIR_CASES[case]
    k = KINDS[kind][0]
    variants = [(True, "part" if kind == "fwd" else "mask")] if case in ("class3", "narrow") else \
        [(True, "part"), (False, "bias+resid")] if kind == "fwd" else [(True, "mask"), (False, "resid"), (False, "mask")]
    for flag, epi in variants:
        _pair(lib, k, O.Dyadic(5000 + a[0] + b[0]), ca, cb, a + (flag, epi), b + (flag, epi))


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_pair_different_epilogues_exact(lib, kind):
    """same class, different operand mode / epilogue: the entry issues the two single launches"""
    k = KINDS[kind][0]
    e0, e1 = ("part", "bias") if kind == "fwd" else ("mask", "plain")
    _pair(lib, k, O.Dyadic(5500), 2, 2, (64, 16, 192, True, e0), (128, 16, 192, True, e1))
    _pair(lib, k, O.Dyadic(5501), 4, 4, (64, 64, 192, True, e0), (64, 64, 192, False, e0))


@pytest.mark.parametrize("case", ["class2", "class4", "class3", "narrow"])
@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_pair_rounded(lib, kind, case):
    """randn inputs: here the order of a sum shows in the last bit, so pair == single launches (checked in _pair with
    torch.equal) says that both contract k in the same order -- in "narrow" across two different instantiations (the pair's
    64-row waves, the single launches' 32-row waves).  Rows of the pins file are named by the class of the single launches."""
    k = KINDS[kind][0]
    epi = "part" if kind == "fwd" else "mask"
    ca, cb, a, b = PAIR_CASES[case]
    _pair(lib, k, Randn(43), ca, cb, a + (True, epi), b + (True, epi))


# ---- weight gradient -----------------------------------------------------------------------------------------------------
WG_SHAPES = [(64, 64), (64, 128), (128, 64), (128, 128), (192, 64)]      # (Cout, Cin): the four tile kernels, + 3 row tiles
WG_P = (64, 576, 4160)     # one chunk; a chunk count the slice count does not divide; enough chunks for several slices


class WgIn:
    def __init__(self, draw, Cout, Cin, P):
        d = draw
        self.Cout, self.Cin, self.P = Cout, Cin, P
        self.dN, self.Y = d.val((Cout, P), 0.5, 1.0), d.val((Cout, P), 0.5, 1.0)
        self.A1, self.A2, self.A3 = d.coef((Cout,)), d.coef((Cout,)), d.coef((Cout,))
        self.X = d.val((Cin, P), 0.5, 1.0)
        self.in_scale, self.in_shift = d.coef((Cin,), zero=False), d.val((Cin,), 0.25, 0.5)
        self.one, self.zero = np.ones(Cout), np.zeros(Cout)


class WgJob:
    """one weight gradient: xform (in_scale given) x general (A1..A3 and Y) or Y == dN with A = (1, 0, 0)"""

    def __init__(self, lib, draw, i, xform, general, out=None):
        self.i, self.draw = i, draw
        Y, A = ("Y", ("A1", "A2", "A3")) if general else ("dN", ("one", "zero", "zero"))
        sc, sh = (i.in_scale, i.in_shift) if xform else (None, None)
        self.ref = O.wgrad(i.dN, i.X, getattr(i, Y), *(getattr(i, a) for a in A), in_scale=sc, in_shift=sh)
        pre(draw, dW=self.ref.dW_abs)
        n = lib.o3d_mlp_conv_wgrad2_scratch(1, i.Cin, i.Cout, i.P)
        assert n > 0
        self.Sf, self.scratch = outbuf((n,))                  # exactly the documented floats, then the guarded tail
        self.out = out
        self.Wf, self.dW = outbuf((i.Cout, i.Cin))            # a compact gradient: the top-left block, packed at the front
        self.ptrs = (ptr(D(i, "dN")), ptr(D(i, Y))) + tuple(ptr(D(i, a)) for a in A) + (
            ptr(D(i, "X")), ptr(D(i, "in_scale")) if xform else None, ptr(D(i, "in_shift")) if xform else None)

    def job(self):
        from open3dsot_amd.fused_heads import _WgradJob
        i, (r, c) = self.i, self.out or (0, 0)
        return _WgradJob(*self.ptrs, i.Cin, i.Cout, i.P, ptr(self.scratch), ptr(self.dW), r, c)

    def check(self, what):
        tail_intact(self.Sf, self.Wf)
        r, i = self.ref, self.i
        if self.out:
            rows, cols = self.out
            assert untouched(self.Wf[rows * cols:]), what + ": a write outside the compact block"
            got = host(self.Wf[:rows * cols].view(rows, cols))
            compare(what, got, r.dW[:rows, :cols], r.dW_abs[:rows, :cols], r.n, self.draw)
        else:
            compare(what, host(self.dW), r.dW, r.dW_abs, r.n, self.draw)


class RowSumJob:
    def __init__(self, draw, C, P):
        self.draw = draw
        self.dN = draw.val((C, P), 0.5, 1.0)
        self.ref = O.row_sum(self.dN)
        pre(draw, rowsum=self.ref.dW_abs)
        self.d = dev(self.dN)
        self.Wf, self.dW = outbuf((C,))
        self.C, self.P = C, P

    def job(self):
        from open3dsot_amd.fused_heads import _WgradJob
        return _WgradJob(ptr(self.d), None, None, None, None, None, None, None, 0, self.C, self.P, None, ptr(self.dW), 0, 0)

    def check(self, what):
        tail_intact(self.Wf)
        compare(what + ".row_sum", host(self.dW), self.ref.dW, self.ref.dW_abs, self.ref.n, self.draw)


def _wgrad_single(lib, draw, Cout, Cin):
    for P in WG_P:
        i = WgIn(draw, Cout, Cin, P)
        for xform in (False, True):
            for general in (False, True):
                j = WgJob(lib, draw, i, xform, general)
                p = j.ptrs
                assert lib.o3d_mlp_conv_wgrad2(p[0], None, 4, p[1], p[2], p[3], p[4], p[5], p[6], p[7], 1, Cin, Cout, P,
                                               ptr(j.scratch), ptr(j.dW), st()) == 0
                torch.cuda.synchronize()
                j.check("wgrad2.%dx%d" % (128 if Cout % 128 == 0 else 64, 128 if Cin % 128 == 0 else 64))


@pytest.mark.parametrize("Cout,Cin", WG_SHAPES)
def test_wgrad2_exact(lib, Cout, Cin):
    _wgrad_single(lib, O.Dyadic(6000 + Cout + 2 * Cin), Cout, Cin)


def test_wgrad2_rounded(lib):
    for Cout, Cin in WG_SHAPES:
        _wgrad_single(lib, Randn(47), Cout, Cin)


def _group(lib, jobs):
    from open3dsot_amd.fused_heads import _WgradJob
    arr = (_WgradJob * len(jobs))(*[j.job() for j in jobs])
    rc = lib.o3d_mlp_conv_wgrad2_group(ctypes.addressof(arr), len(jobs), st())
    torch.cuda.synchronize()
    return rc


def _mixed_jobs(lib, draw):
    """eight jobs: every tile kind, three P, row sums first, in the middle and last"""
    def wg(Cout, Cin, P, xform, general):
        return WgJob(lib, draw, WgIn(draw, Cout, Cin, P), xform, general)
    return [RowSumJob(draw, 5, 576), wg(64, 64, 4160, True, True), wg(128, 64, 576, False, False), RowSumJob(draw, 64, 64),
            wg(64, 128, 64, True, False), wg(128, 128, 4160, False, True), wg(192, 64, 576, True, True),
            RowSumJob(draw, 256, 4160)]


def _group_cases(lib, draw):
    one = [WgJob(lib, draw, WgIn(draw, 128, 64, 576), True, True)]
    assert _group(lib, one) == 0
    one[0].check("wgrad2_group")
    jobs = _mixed_jobs(lib, draw)
    assert _group(lib, jobs) == 0
    for j in jobs:
        j.check("wgrad2_group")
    # a compact (5, 259) gradient inside a (64, 320) zero-padded problem, next to a full one
    jobs = [WgJob(lib, draw, WgIn(draw, 64, 320, 576), True, True, out=(5, 259)), WgJob(lib, draw, WgIn(draw, 64, 64, 64), False, True)]
    assert _group(lib, jobs) == 0
    for j in jobs:
        j.check("wgrad2_group")


def test_wgrad2_group_exact(lib):
    _group_cases(lib, O.Dyadic(7000))


def test_wgrad2_group_rounded(lib):
    _group_cases(lib, Randn(53))


def test_wgrad2_group_refuses_nine_jobs(lib):
    draw = O.Dyadic(7001)
    jobs = [RowSumJob(draw, 64, 64) for _ in range(9)]
    assert _group(lib, jobs) == EINVAL
    assert all(untouched(j.Wf) for j in jobs)
    assert _group(lib, jobs[:8]) == 0
    for j in jobs[:8]:
        j.check("wgrad2_group")
