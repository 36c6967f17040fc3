"""The batched (B, C, P) GEMM entry points of csrc/mlp.hip -- o3d_mlp_conv_fwd, o3d_mlp_conv_dgrad, o3d_mlp_conv_dgrad_wt,
o3d_mlp_conv_dgrad_plain, o3d_mlp_conv_wgrad, o3d_bn_relu_maxpool_fwd -- and o3d_row_sum (csrc/heads.hip), called through the
C ABI with raw pointers, launch by launch and per LAUNCH CLASS, against the plain numpy fp64 reference
tests/batched_gemm_oracle.py (tests/gemm_oracle.py on the rearranged operands; tied to Conv2d / BatchNorm2d / ReLU / max under
autograd by tests/test_batched_gemm_oracle_cpu.py).  Same method as tests/test_gemm_kernels_gpu.py:

EXACT leg: every floating-point input lies on a small dyadic grid (sparse weights for the larger K), so every product and
every partial sum of a correct kernel is exactly representable in fp32 whatever its summation order (asserted before each
launch: sum|terms| / spacing < 2^24), and the comparison is EQUALITY.
ROUNDED leg: torch.randn inputs, |err| <= (n + 8) * 2^-24 * sum|t_i| per output, n the length of the sum that produced it
(Cin forward, Cout data gradients, B*P for dW, 128 for a statistics row, 2 for the pool).  The statistics rows are bounded
against the fp64 sums over the kernel's OWN stored output; the stored output is itself bounded against the oracle.  The worst
err / bound per kernel and class is printed and, when O3D_BATCHED_GEMM_PINS names a file, written there
(profiles/batched_gemm_kernel_pins.txt is such a run).
GUARDS: every output buffer has a 256-element tail and is prefilled with a sentinel; the tail, the statistics rows beyond
B*P/128 and the scratch beyond nslices*Cout*Cin must still hold it after the call.  Every input buffer carries a 256-element
tail of NaN, so a read past an operand poisons an output.
CLASS: every forward / data-gradient case first asserts o3d_mlp_conv_class(entry, B, M, K, P, part), the entries' own rule
(64 / 128 / 256 = rows per workgroup of the LDS-staged generic kernel; 2064 / 4064 / 3128 = class and tile of the direct
kernel at this B): when a dispatch rule is retuned the case that lost its class fails by name.
"""
import os

import numpy as np
import pytest
import torch

import batched_gemm_oracle as BO

pytestmark = pytest.mark.gpu

SENT = -7.0e37
SENT_I = -77777
TAIL = 256
EINVAL = -1
E24 = 2.0 ** -24
RATIOS = {}
EXTRA_ROWS = 2             # statistics rows allocated beyond B*P/128: must stay untouched
BP = ((3, 128), (2, 384))  # one tile per cloud; three tiles per cloud


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi
    return capi.load()


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_BATCHED_GEMM_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per kernel and launch class, rounded leg of tests/test_batched_gemm_kernels_gpu.py\n"
                    "# bound = (n + 8) * 2^-24 * sum|t_i|; every ratio must be <= 1\n"
                    "# g64 / g128 / g256: conv_fwd_kernel / conv_dgrad_kernel<BM>; d2064 / d4064 / d3128: the direct kernels at B > 1\n")
            for k in sorted(RATIOS):
                f.write("%-44s %.4f\n" % (k, RATIOS[k]))


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
    """device copy of an fp32 operand, followed by TAIL NaNs no correct kernel may read"""
    a = np.ascontiguousarray(a)
    flat = torch.full((a.size + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    flat[:a.size] = torch.from_numpy(a.reshape(-1)).to(torch.float32).cuda()
    return flat[:a.size].view(a.shape)


def dev_i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    flat = torch.full((a.size + TAIL,), 0x7fffffff, dtype=torch.int32, device="cuda")
    flat[:a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return flat[:a.size].view(a.shape)


def outbuf(shape, dtype=torch.float32):
    """-> (flat buffer with a TAIL of sentinels, view of `shape`)"""
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), SENT if dtype == torch.float32 else SENT_I, dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def sent_of(t):
    return SENT if t.dtype == torch.float32 else SENT_I


def tail_intact(*flats):
    for f in flats:
        assert bool((f[-TAIL:] == sent_of(f)).all()), "write beyond the buffer"


def untouched(t):
    return bool((t == sent_of(t)).all())


def ptr(t):
    return None if t is None else t.data_ptr()


def pre(draw, **abs_sums):
    """before the launch: the exact leg's inputs keep every partial sum of these outputs exact in fp32"""
    if draw.exact:
        for k, v in abs_sums.items():
            BO.assert_exact(k if "." in k else "gemm." + k, v)


def compare(kernel, got, ref, ref_abs, n, exact, ratios=RATIOS):
    """exact leg: equality.  rounded leg: |got - ref| <= (n + 8) * 2^-24 * sum|t_i|, worst ratio recorded"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), kernel
    if exact:
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (kernel, len(bad), bad[:8].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        return
    bound = (np.asarray(n, np.float64) + 8) * E24 * np.asarray(ref_abs, np.float64)
    err = np.abs(got - ref)
    assert (err[bound == 0] == 0).all(), kernel
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    ratios[kernel] = max(ratios.get(kernel, 0.0), ratio)
    print("rounded leg %s: worst err/bound %.4f" % (kernel, ratio))
    assert ratio <= 1.0, (kernel, ratio)


def compare_int(kernel, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    bad = np.argwhere(got != ref)
    assert got.shape == ref.shape and len(bad) == 0, (kernel, len(bad), bad[:8].tolist())


def cname(cls):
    return ("g%d" if cls < 1000 else "d%d") % cls


def expect_class(lib, entry, B, M, K, P, part, cls):
    if lib is None:                                           # (reference only: tests/test_batched_gemm_oracle_cpu.py)
        return
    got = lib.o3d_mlp_conv_class(entry, B, M, K, P, int(part))
    assert got == cls, "this case was written for launch class %d; entry %d (B, M, K, P, part) = (%d, %d, %d, %d, %d) now " \
        "launches class %d" % (cls, entry, B, M, K, P, part, got)


def generic_class(rows):
    return 256 if rows > 128 else 128 if rows > 64 else 64


def D(i, name):
    """device copy of an operand of an input record, made once"""
    cache = i.__dict__.setdefault("_dev", {})
    if name not in cache:
        cache[name] = dev(getattr(i, name))
    return cache[name]


def make_draw(exact, seed):
    return BO.Dyadic(seed) if exact else Randn(seed)


# ==== o3d_mlp_conv_fwd ========================================================================================================
FWD_MODES = ("none", "part_c", "part")                       # part NULL; part with stat_c; part with stat_c NULL
FWD_GENERIC_COUT = (1, 37, 64, 65, 100, 128, 129, 200, 256, 300)
FWD_GENERIC_CIN = (3, 19, 20)                                # one partial chunk; a second partial chunk; float4 loads, short last
FWD_GENERIC_K48 = (37, 100, 300)                             # Cin = 48: the k loop three chunks deep (Cout % 64 != 0: not direct)
FWD_DIRECT = ((16, 64), (64, 128), (128, 256))              # (Cin, Cout)


def fwd_direct_class(Cin, part):
    return 3128 if part else (2064 if Cin < 64 else 4064)


def fwd_ref(draw, i, xform, mode):
    sc, sh = (i.in_scale, i.in_shift) if xform else (None, None)
    r = BO.fwd(i.X, i.W, sc, sh, part=mode != "none", stat_c=i.stat_c if mode == "part_c" else None)
    pre(draw, Y=r.Y_abs)
    if mode != "none":
        pre(draw, part0=r.part_abs[:, 0], part1=r.part_abs[:, 1])
    return r


def run_fwd(lib, draw, i, xform, mode, cls):
    B, Cin, Cout, P = i.B, i.Cin, i.Cout, i.P
    expect_class(lib, 0, B, Cout, Cin, P, mode != "none", cls)
    r = fwd_ref(draw, i, xform, mode)
    if lib is None:
        return
    Yf, Y = outbuf((B, Cout, P))
    rows = B * P // 128
    Pf, part = outbuf((rows + EXTRA_ROWS, 2, Cout))
    rc = lib.o3d_mlp_conv_fwd(ptr(D(i, "X")), ptr(D(i, "W")), ptr(D(i, "in_scale")) if xform else None,
                              ptr(D(i, "in_shift")) if xform else None, B, Cin, Cout, P, ptr(Y),
                              ptr(part) if mode != "none" else None, ptr(D(i, "stat_c")) if mode == "part_c" else None, st())
    assert rc == 0
    torch.cuda.synchronize()
    tail_intact(Yf, Pf)
    k = "fwd.%s.%s" % (cname(cls), "xform" if xform else "plain")
    got = host(Y)
    compare(k + ".Y", got, r.Y, r.Y_abs, r.n, draw.exact)
    if mode == "none":
        assert untouched(part), k
        return
    assert untouched(part[rows:]), k + ": a statistics row beyond B*P/128 was written"
    gp = host(part[:rows])
    pr, pa = (r.part, r.part_abs) if draw.exact else BO.stats_fwd(got, i.stat_c if mode == "part_c" else None)
    compare(k + ".part_sum", gp[:, 0], pr[:, 0], pa[:, 0], 128, draw.exact)
    compare(k + ".part_var", gp[:, 1], pr[:, 1], pa[:, 1], 128, draw.exact)


def fwd_generic_shapes(Cout):
    return [(Cin, Cout) for Cin in FWD_GENERIC_CIN] + ([(48, Cout)] if Cout in FWD_GENERIC_K48 else [])


def _fwd_generic(lib, exact, Cout):
    for Cin, _ in fwd_generic_shapes(Cout):
        for B, P in BP:
            draw = make_draw(exact, 100 + Cin + Cout + B)
            i = BO.Inputs(draw, B, Cin, Cout, P)
            for xform in (False, True):
                for mode in FWD_MODES:
                    run_fwd(lib, draw, i, xform, mode, generic_class(Cout))


@pytest.mark.parametrize("Cout", FWD_GENERIC_COUT)
def test_fwd_generic_exact(lib, Cout):
    _fwd_generic(lib, True, Cout)


@pytest.mark.parametrize("Cout", FWD_GENERIC_COUT)
def test_fwd_generic_rounded(lib, Cout):
    _fwd_generic(lib, False, Cout)


def _fwd_direct(lib, exact, Cin, Cout):
    for B, P in BP:
        draw = make_draw(exact, 200 + Cin + B)
        i = BO.Inputs(draw, B, Cin, Cout, P)
        for xform in (False, True):
            for mode in ("none", "part_c"):
                run_fwd(lib, draw, i, xform, mode, fwd_direct_class(Cin, mode != "none"))


@pytest.mark.parametrize("Cin,Cout", FWD_DIRECT)
def test_fwd_direct_batched_exact(lib, Cin, Cout):
    _fwd_direct(lib, True, Cin, Cout)


@pytest.mark.parametrize("Cin,Cout", FWD_DIRECT)
def test_fwd_direct_batched_rounded(lib, Cin, Cout):
    _fwd_direct(lib, False, Cin, Cout)


def test_fwd_refuses_one_sided_transform(lib):
    """exactly one of in_scale / in_shift NULL: refused on the generic and on the direct shape, nothing written"""
    for Cin, Cout in ((3, 37), (16, 64)):
        i = BO.Inputs(BO.Dyadic(1), 2, Cin, Cout, 128)
        Yf, Y = outbuf((2, Cout, 128))
        Pf, part = outbuf((2, 2, Cout))
        for sc, sh in ((D(i, "in_scale"), None), (None, D(i, "in_shift"))):
            assert lib.o3d_mlp_conv_fwd(ptr(D(i, "X")), ptr(D(i, "W")), ptr(sc), ptr(sh), 2, Cin, Cout, 128, ptr(Y), ptr(part),
                                        None, st()) == EINVAL
        assert lib.o3d_mlp_conv_fwd(ptr(D(i, "X")), ptr(D(i, "W")), None, None, 2, Cin, Cout, 64, ptr(Y), None, None, st()) == EINVAL
        torch.cuda.synchronize()
        assert untouched(Yf) and untouched(Pf)


def test_conv_class_rules(lib):
    """the export itself, at the edges of the rules it restates"""
    c = lib.o3d_mlp_conv_class
    assert [c(0, 2, M, 3, 128, 1) for M in (1, 64, 65, 128, 129, 300)] == [64, 64, 128, 128, 256, 256]
    assert [c(2, 2, M, 16, 128, 1) for M in (64, 128, 256)] == [64, 128, 256]          # no direct dispatch without Wt
    assert [c(0, 2, 64, 16, 128, 1), c(0, 2, 64, 16, 128, 0), c(0, 2, 64, 64, 128, 0), c(0, 2, 64, 64, 128, 1)] == \
        [3128, 2064, 4064, 3128]
    assert c(0, 2, 64, 64, 65536, 0) == 3128                  # B*P above the 64-column threshold of o3d_direct_tile
    assert c(0, 2, 64, 17, 128, 0) == 64 and c(0, 2, 96, 16, 128, 0) == 128            # unaligned: generic
    assert [c(1, 2, 64, 16, 128, 0), c(1, 2, 65, 16, 128, 0), c(1, 2, 64, 17, 128, 0)] == [3128, 128, 64]
    assert [c(3, 2, 64, 16, 128, 0), c(0, 0, 64, 16, 128, 0), c(0, 2, 64, 16, 96, 0), c(0, 2, 0, 16, 128, 0)] == [-1] * 4


# ==== data gradients ========================================================================================================
DG_M = (3, 20, 64, 65, 128, 129, 300)                        # M = Cin: output rows
DG_COUT = (5, 16, 17, 40)
DG_NS = (0, 4, 8, 32)                                        # 0: the dense source


class DgIn(BO.Inputs):
    """the data gradient contracts over Cout: its exact leg wants few non-zeros per COLUMN of W"""

    def __init__(self, draw, B, Cin, Cout, P):
        super().__init__(draw, B, Cin, Cout, P)
        if draw.exact:
            nnz = min(Cout, max(16, -(-Cout // Cin)))
            self.W = BO.sparse_rows(draw, Cin, Cout, nnz).T.copy()
        self.Wt = np.ascontiguousarray(self.W.T)


def dg_source(draw, i, ns):
    """-> dN (dense, for the oracle), the pooled triple or None"""
    if ns == 0:
        return i.dN, None
    dOut, out, arg = i.pooled(draw, ns)
    return BO.pooled_dense(dOut, out, arg, ns), (dOut, out, arg)


def dgrad_ref(draw, i, dN):
    r = BO.dgrad(dN, i.W, i.Y, i.A1, i.A2, i.A3, i.Yprev, i.scale_p, i.shift_p, i.mean_p)
    assert np.array_equal(r.mask, BO.mask_fp32(i.Yprev, i.scale_p, i.shift_p))
    pre(draw, G=r.G_abs, gpart0=r.part_abs[:, 0], gpart1=r.part_abs[:, 1])
    return r


def check_dgrad(k, draw, i, r, Gf, Gv, Pf, part):
    tail_intact(Gf, Pf)
    rows = i.B * i.P // 128
    got = host(Gv)
    compare(k + ".G", got, r.G, r.G_abs, r.n, draw.exact)
    assert not got[~r.mask].any(), k + ": the ReLU mask"
    assert untouched(part[rows:]), k + ": a statistics row beyond B*P/128 was written"
    gp = host(part[:rows])
    pr, pa = (r.part, r.part_abs) if draw.exact else BO.stats_bwd(got, i.Yprev, i.mean_p)
    compare(k + ".part_sum", gp[:, 0], pr[:, 0], pa[:, 0], 128, draw.exact)
    compare(k + ".part_gy", gp[:, 1], pr[:, 1], pa[:, 1], 128, draw.exact)


def run_dgrad(lib, draw, i, ns, via):
    """via: "dgrad" (o3d_mlp_conv_dgrad), "wt_null" (o3d_mlp_conv_dgrad_wt, Wt NULL), "wt" (Wt given: falls through when the
    shape is unaligned, or when the pooled source comes without pk)"""
    B, Cin, Cout, P = i.B, i.Cin, i.Cout, i.P
    cls = generic_class(Cin)
    expect_class(lib, 2, B, Cin, Cout, P, 1, cls)
    if via == "wt" and ns == 0:
        expect_class(lib, 1, B, Cin, Cout, P, 1, cls)         # (an aligned shape would take the direct kernel)
    dN, pooled = dg_source(draw, i, ns)
    r = dgrad_ref(draw, i, dN)
    if lib is None:
        return
    Gf, Gv = outbuf((B, Cin, P))
    Pf, part = outbuf((B * P // 128 + EXTRA_ROWS, 2, Cin))
    if pooled is None:
        src = (ptr(D(i, "dN")), None, None, None, 4)
    else:
        keep = (dev(pooled[0]), dev(pooled[1]), dev_i(pooled[2]))     # (alive until the launch has run)
        src = (None, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ns)
    yA = tuple(ptr(D(i, n)) for n in ("Y", "A1", "A2", "A3"))
    end = (B, Cin, Cout, P) + tuple(ptr(D(i, n)) for n in ("Yprev", "scale_p", "shift_p", "mean_p")) + (ptr(Gv), ptr(part), st())
    if via == "dgrad":
        rc = lib.o3d_mlp_conv_dgrad(*src, *yA, ptr(D(i, "W")), *end)
    else:
        rc = lib.o3d_mlp_conv_dgrad_wt(*src, *yA, ptr(D(i, "W")), ptr(D(i, "Wt")) if via == "wt" else None, None, *end)
    assert rc == 0
    torch.cuda.synchronize()
    check_dgrad("dgrad.%s.%s" % (cname(cls), "pooled" if ns else "dense"), draw, i, r, Gf, Gv, Pf, part)


def dgrad_generic_cases(M):
    """(Cout, (B, P), ns, via) for output rows M: every Cout with every source; the entry variants spread over them"""
    cases = []
    for n, Cout in enumerate(DG_COUT):
        for m, ns in enumerate(DG_NS):
            B, P = BP[(n + m) % 2]
            aligned = M % 64 == 0 and Cout % 16 == 0
            via = ("dgrad", "wt_null", "wt")[(n + m) % 3]
            if via == "wt" and aligned and ns == 0:
                via = "wt_null"                               # (Wt given on an aligned dense shape: the direct kernel, below)
            cases.append((Cout, (B, P), ns, via))
    return cases


def _dgrad_generic(lib, exact, M):
    for Cout, (B, P), ns, via in dgrad_generic_cases(M):
        draw = make_draw(exact, 300 + M + Cout + ns)
        run_dgrad(lib, draw, DgIn(draw, B, M, Cout, P), ns, via)


@pytest.mark.parametrize("M", DG_M)
def test_dgrad_generic_exact(lib, M):
    _dgrad_generic(lib, True, M)


@pytest.mark.parametrize("M", DG_M)
def test_dgrad_generic_rounded(lib, M):
    _dgrad_generic(lib, False, M)


def test_dgrad_entry_variants_cover_every_path():
    vias = {(M, ns > 0, via) for M in DG_M for _, _, ns, via in dgrad_generic_cases(M)}
    for M in DG_M:
        for pooled in (False, True):
            assert (M, pooled, "dgrad") in vias and (M, pooled, "wt_null") in vias
    assert (65, False, "wt") in vias and (64, True, "wt") in vias     # unaligned with Wt; pooled without pk


# ---- o3d_mlp_conv_dgrad_wt: the direct kernel at B = 2 -------------------------------------------------------------------------
DG_DIRECT = ((64, 16), (128, 64), (256, 128))                # (Cin, Cout)


def pack_pk(pooled):
    dOut, out, arg = pooled
    g = np.where(out > 0, dOut, 0.0).astype(np.float32)
    return np.stack([g, arg.astype(np.int32).view(np.float32)], axis=-1)      # (B, Cout, npoint, 2)


def _dgrad_direct(lib, exact, Cin, Cout, ns):
    B, P = 2, 384 if ns in (0, 4) else 128
    draw = make_draw(exact, 400 + Cin + ns)
    i = DgIn(draw, B, Cin, Cout, P)
    expect_class(lib, 1, B, Cin, Cout, P, 1, 3128)
    expect_class(lib, 1, 1, Cin, Cout, P, 1, 3128)
    dN, pooled = dg_source(draw, i, ns)
    r = dgrad_ref(draw, i, dN)
    if lib is None:
        return
    pk = dev_i(pack_pk(pooled).reshape(B, Cout, -1).view(np.int32)).view(torch.float32) if pooled is not None else None
    tpb = P // 128

    def call(b0, nb, Gv, part):
        sl = lambda t: None if t is None else t[b0:b0 + nb]
        return lib.o3d_mlp_conv_dgrad_wt(ptr(sl(D(i, "dN"))) if pooled is None else None, None, None, None, ns or 4,
                                         ptr(sl(D(i, "Y"))), ptr(D(i, "A1")), ptr(D(i, "A2")), ptr(D(i, "A3")), ptr(D(i, "W")),
                                         ptr(D(i, "Wt")), ptr(sl(pk)), nb, Cin, Cout, P, ptr(sl(D(i, "Yprev"))),
                                         ptr(D(i, "scale_p")), ptr(D(i, "shift_p")), ptr(D(i, "mean_p")), ptr(Gv[b0:b0 + nb]),
                                         ptr(part[b0 * tpb:]), st())
    Gf, Gv = outbuf((B, Cin, P))
    Pf, part = outbuf((B * tpb + EXTRA_ROWS, 2, Cin))
    assert call(0, B, Gv, part) == 0
    torch.cuda.synchronize()
    check_dgrad("dgrad_wt.d3128.%s" % ("pk" if ns else "dense"), draw, i, r, Gf, Gv, Pf, part)
    Gf1, Gv1 = outbuf((B, Cin, P))
    Pf1, part1 = outbuf((B * tpb + EXTRA_ROWS, 2, Cin))
    for b in range(B):
        assert call(b, 1, Gv1, part1) == 0
    torch.cuda.synchronize()
    assert torch.equal(Gf, Gf1) and torch.equal(Pf, Pf1), "the batched launch and the cloud-by-cloud launches differ"


@pytest.mark.parametrize("ns", [0, 4, 32])
@pytest.mark.parametrize("Cin,Cout", DG_DIRECT)
def test_dgrad_wt_direct_batched_exact(lib, Cin, Cout, ns):
    _dgrad_direct(lib, True, Cin, Cout, ns)


@pytest.mark.parametrize("ns", [0, 4, 32])
@pytest.mark.parametrize("Cin,Cout", DG_DIRECT)
def test_dgrad_wt_direct_batched_rounded(lib, Cin, Cout, ns):
    _dgrad_direct(lib, False, Cin, Cout, ns)


# ---- o3d_mlp_conv_dgrad_plain --------------------------------------------------------------------------------------------------
PLAIN_CIN = (3, 19, 131, 259, 100)                           # the [xyz ; feats] operand widths; 100: the 128-row kernel
PLAIN_COUT = (64, 128)
PLAIN_BP = ((1, 256), (2, 128))


def plain_ref(draw, i):
    r = BO.dgrad_plain(i.dN, i.W, i.Y, i.A1, i.A2, i.A3)
    pre(draw, G=r.G_abs)
    return r


def plain_call(lib, i, dX, **null):
    a = {n: ptr(D(i, n)) for n in ("dN", "Y", "A1", "A2", "A3", "W")}
    a.update(null)
    return lib.o3d_mlp_conv_dgrad_plain(a["dN"], a["Y"], a["A1"], a["A2"], a["A3"], a["W"], i.B, i.Cin, i.Cout, i.P, ptr(dX), st())


def _plain(lib, exact, Cin):
    for Cout in PLAIN_COUT:
        for B, P in PLAIN_BP:
            draw = make_draw(exact, 500 + Cin + Cout + B)
            i = DgIn(draw, B, Cin, Cout, P)
            cls = generic_class(Cin)
            expect_class(lib, 2, B, Cin, Cout, P, 0, cls)
            r = plain_ref(draw, i)
            if lib is None:
                continue
            Xf, dX = outbuf((B, Cin, P))
            assert plain_call(lib, i, dX) == 0
            torch.cuda.synchronize()
            tail_intact(Xf)
            compare("dgrad_plain.%s.dX" % cname(cls), host(dX), r.G, r.G_abs, r.n, draw.exact)


@pytest.mark.parametrize("Cin", PLAIN_CIN)
def test_dgrad_plain_exact(lib, Cin):
    _plain(lib, True, Cin)


@pytest.mark.parametrize("Cin", PLAIN_CIN)
def test_dgrad_plain_rounded(lib, Cin):
    _plain(lib, False, Cin)


def test_dgrad_plain_refusals(lib):
    i = DgIn(BO.Dyadic(2), 2, 19, 64, 128)
    Xf, dX = outbuf((2, 19, 128))
    for name in ("dN", "Y", "A1", "A2", "A3", "W"):
        assert plain_call(lib, i, dX, **{name: None}) == EINVAL, name
    assert plain_call(lib, i, None) == EINVAL
    i.P = 64                                                  # P % 128 != 0 (the operands are larger than that)
    assert plain_call(lib, i, dX) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Xf)


# ==== o3d_mlp_conv_wgrad ========================================================================================================
WG_SHAPES = ((3, 64), (19, 37), (128, 128), (131, 129), (259, 64))      # (Cin, Cout): 1x1, 2x2 and 3x1 output tiles of 128
# (B, P, nslices): one slice; 8 chunks over 3 slices (3, 3, 2); the XCD remapping (nslices % 8 == 0) with and without empty
# slices; more slices than chunks, remapped (4 chunks, 8 slices) and not (4 chunks, 5 slices); P % 128 != 0
WG_SLICES = ((2, 128, 1), (2, 128, 3), (2, 128, 8), (2, 384, 16), (3, 128, 16), (1, 128, 8), (1, 128, 5), (2, 96, 3), (3, 96, 8))
WG_INST = tuple((pooled, xform) for pooled in (False, True) for xform in (False, True))


def wgrad_ref(draw, i, dN, xform):
    sc, sh = (i.in_scale, i.in_shift) if xform else (None, None)
    r = BO.wgrad(dN, i.X, i.Y, i.A1, i.A2, i.A3, in_scale=sc, in_shift=sh)
    pre(draw, dW=r.dW_abs)
    return r


def wgrad_call(lib, i, src, xform, nslices, scratch, dW, **over):
    a = dict(X=ptr(D(i, "X")), sc=ptr(D(i, "in_scale")) if xform else None, sh=ptr(D(i, "in_shift")) if xform else None, P=i.P)
    a.update(over)
    return lib.o3d_mlp_conv_wgrad(*src, ptr(D(i, "Y")), ptr(D(i, "A1")), ptr(D(i, "A2")), ptr(D(i, "A3")), a["X"], a["sc"], a["sh"],
                                  i.B, i.Cin, i.Cout, a["P"], nslices, ptr(scratch), ptr(dW), st())


def _wgrad(lib, exact, Cin, Cout):
    for n, (B, P, nslices) in enumerate(WG_SLICES):
        draw = make_draw(exact, 600 + Cin + n)
        i = BO.Inputs(draw, B, Cin, Cout, P)
        ns = (4, 8, 32)[n % 3]
        dense, pooled = dg_source(draw, i, ns)
        keep = (dev(pooled[0]), dev(pooled[1]), dev_i(pooled[2])) if lib is not None else (None,) * 3
        psrc = (None, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ns)
        for is_pooled, xform in WG_INST:
            r = wgrad_ref(draw, i, dense if is_pooled else i.dN, xform)
            if lib is None:
                continue
            Sf, scratch = outbuf(((nslices + 16) * Cout * Cin,))
            Wf, dW = outbuf((Cout, Cin))
            src = psrc if is_pooled else (ptr(D(i, "dN")), None, None, None, 4)
            assert wgrad_call(lib, i, src, xform, nslices, scratch, dW) == 0
            torch.cuda.synchronize()
            tail_intact(Sf, Wf)
            assert untouched(scratch[nslices * Cout * Cin:]), "scratch beyond nslices * Cout * Cin was written"
            k = "wgrad.%s.%s" % ("pooled" if is_pooled else "dense", "xform" if xform else "plain")
            compare(k + ".dW", host(dW), r.dW, r.dW_abs, r.n, draw.exact)
            chunks = B * P // 32
            per = -(-chunks // nslices)
            first_empty = -(-chunks // per)
            if first_empty < nslices:                         # slices without a chunk: zeros, not stale memory
                assert not scratch[first_empty * Cout * Cin:nslices * Cout * Cin].any(), k + ": an empty slice is not zero"


@pytest.mark.parametrize("Cin,Cout", WG_SHAPES)
def test_wgrad_exact(lib, Cin, Cout):
    _wgrad(lib, True, Cin, Cout)


@pytest.mark.parametrize("Cin,Cout", WG_SHAPES)
def test_wgrad_rounded(lib, Cin, Cout):
    _wgrad(lib, False, Cin, Cout)


def test_wgrad_slice_table_has_every_branch():
    t = [(B * P // 32, ns) for B, P, ns in WG_SLICES]
    assert any(ns == 1 for _, ns in t) and (8, 3) in t
    assert any(ns % 8 == 0 and c >= ns for c, ns in t) and any(ns % 8 == 0 and c < ns for c, ns in t)
    assert any(ns % 8 and c < ns for c, ns in t) and any(P % 128 for _, P, _ in WG_SLICES)


def test_wgrad_refusals(lib):
    i = BO.Inputs(BO.Dyadic(3), 2, 19, 37, 128)
    Sf, scratch = outbuf((17 * 37 * 19,))
    Wf, dW = outbuf((37, 19))
    src = (ptr(D(i, "dN")), None, None, None, 4)
    assert wgrad_call(lib, i, src, True, 1, scratch, dW, sh=None) == EINVAL          # in_scale without in_shift
    assert wgrad_call(lib, i, src, True, 1, scratch, dW, sc=None) == EINVAL          # in_shift without in_scale
    assert wgrad_call(lib, i, src, False, 1, scratch, dW, X=None) == EINVAL
    assert wgrad_call(lib, i, src, False, 1, scratch, dW, P=48) == EINVAL             # P % 32 != 0
    assert wgrad_call(lib, i, src, False, 0, scratch, dW) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Sf) and untouched(Wf)


# ==== o3d_bn_relu_maxpool_fwd =================================================================================================
POOL_NS = (4, 8, 32, 36, 64)
POOL_SHAPES = ((1, 1, 3), (2, 5, 7), (3, 5, 32))             # (B, C, npoint): 3 and 70 centres (dead lanes), 480 (none)


def pool_inputs(draw, B, C, npoint, ns):
    Y = draw.val((B, C, npoint * ns), 0.25, 2.0)
    scale, shift = draw.coef((C,), zero=False), draw.val((C,), 0.25, 1.0)
    if C >= 4:
        scale[1] = -abs(scale[1])                             # a negative scale: the smallest y wins
        scale[2] = 0.0                                        # every slot ties: arg = 0
        Y[:, 3] = -np.abs(Y[:, 3]) - 0.25                     # an all-negative channel ...
        scale[3], shift[3] = abs(scale[3]), -abs(shift[3])    # ... stays negative: out = 0, arg / yarg of the largest
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # (the oracle sees the fp32 values the kernel sees)
    return f32(Y), f32(scale), f32(shift)


def pool_ref(draw, Y, scale, shift, ns):
    r = BO.pool_fwd(Y, scale, shift, ns)
    pre(draw, **{"bg.pool": r.out_abs})
    return r


def run_pool(lib, draw, Y, scale, shift, ns, want=True, r=None):
    B, C, P = Y.shape
    npoint = P // ns
    r = r or pool_ref(draw, Y, scale, shift, ns)
    if lib is None:
        return None
    Of, out = outbuf((B, C, npoint))
    Af, arg = outbuf((B, C, npoint), torch.int32)
    Yf, yarg = outbuf((B, C, npoint))
    dY, ds, dh = dev(Y), dev(scale), dev(shift)
    assert lib.o3d_bn_relu_maxpool_fwd(ptr(dY), ptr(ds), ptr(dh), B, C, npoint, ns, ptr(out),
                                       ptr(arg) if want else None, ptr(yarg) if want else None, st()) == 0
    torch.cuda.synchronize()
    tail_intact(Of, Af, Yf)
    compare("pool_fwd.out", host(out), r.out, r.out_abs, r.n, draw.exact)
    if want:
        compare_int("pool_fwd.arg", arg.cpu().numpy(), r.arg)
        assert np.array_equal(host(yarg), r.yarg), "pool_fwd.yarg"
    else:
        assert untouched(Af) and untouched(Yf)
    return out, arg, yarg


def _pool(lib, ns, exact):
    for B, C, npoint in POOL_SHAPES:
        draw = make_draw(exact, 700 + ns + C)
        Y, scale, shift = pool_inputs(draw, B, C, npoint, ns)
        run_pool(lib, draw, Y, scale, shift, ns)
        run_pool(lib, draw, Y, scale, shift, ns, want=False)
        if C >= 4:                                            # the oracle on the planted channels: dead scale, all negative
            r = BO.pool_fwd(Y, scale, shift, ns)
            assert not r.arg[:, 2].any() and (r.out[:, 2] == max(shift[2], 0.0)).all() and not r.out[:, 3].any()


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("ns", POOL_NS)
def test_pool_fwd(lib, ns, exact):
    _pool(lib, ns, exact)


def pool_ties():
    """hand-written known answers: (ns, {ball: ([slots holding the maximum], winner)}) -- the lowest k wins every time.
    Lane e of a ball reads float4 e, e + 8, ...: slots 4e .. 4e + 3, then 32 + 4e .. 32 + 4e + 3"""
    return [(8, {0: ([1, 2], 1), 1: ([3, 4], 3), 2: ([7, 0], 0)}),                     # inside one float4; across two lanes
            (32, {0: ([5, 9], 5), 1: ([30, 3], 3), 2: ([13, 14, 31], 13), 3: ([28, 24, 20, 16, 12, 8, 4], 4)}),
            (36, {0: ([32, 1], 1), 1: ([35, 34], 34), 2: ([33, 4], 4)}),               # lane 0's second round against round one
            (64, {0: ([33, 2], 2), 1: ([63, 31], 31), 2: ([36, 5, 40], 5), 3: ([62, 61, 60], 60), 4: ([32, 28], 28)})]


@pytest.mark.parametrize("case", range(4))
def test_pool_fwd_ties_known_answers(lib, case):
    ns, plants = pool_ties()[case]
    npoint, C = len(plants), 2
    Y = np.zeros((1, C, npoint, ns))
    Y[0, 0] = -1.0 - 0.25 * np.arange(ns)[None, :]
    Y[0, 1] = 1.0 + 0.25 * np.arange(ns)[None, :]             # channel 1 has scale -1: the SMALLEST y is the maximum
    for j, (slots, win) in plants.items():
        Y[0, 0, j, slots] = 3.0
        Y[0, 1, j, slots] = -3.0
    scale, shift = np.array([1.0, -1.0]), np.array([0.5, 0.5])
    out, arg, yarg = run_pool(lib, BO.Dyadic(0), Y.reshape(1, C, npoint * ns), scale, shift, ns)
    want = np.array([[plants[j][1] for j in range(npoint)]] * C)
    assert np.array_equal(arg.cpu().numpy()[0], want)
    assert (host(out) == 3.5).all() and np.array_equal(host(yarg)[0], np.array([[3.0] * npoint, [-3.0] * npoint]))


def test_pool_fwd_refusals(lib):
    Y, scale, shift = pool_inputs(BO.Dyadic(4), 1, 1, 3, 8)
    Of, out = outbuf((1, 1, 3))
    Af, arg = outbuf((1, 1, 3), torch.int32)
    dY, ds, dh = dev(Y), dev(scale), dev(shift)
    f = lib.o3d_bn_relu_maxpool_fwd
    assert f(ptr(dY), ptr(ds), ptr(dh), 1, 1, 3, 8, ptr(out), ptr(arg), None, st()) == EINVAL        # arg without yarg
    assert f(ptr(dY), ptr(ds), ptr(dh), 1, 1, 4, 6, ptr(out), None, None, st()) == EINVAL            # ns % 4 != 0
    assert f(None, ptr(ds), ptr(dh), 1, 1, 3, 8, ptr(out), None, None, st()) == EINVAL
    assert f(ptr(dY), ptr(ds), ptr(dh), 1, 1, 3, 8, None, None, None, st()) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Of) and untouched(Af)


# ==== o3d_row_sum ===============================================================================================================
ROW_SUM_P = (4, 1020, 1024, 1028, 4100)                      # the stride-1024 walk: one lane; 255 lanes; all; a second round


def row_sum_ref(draw, C, P):
    Gm = draw.val((C, P), 0.5, 1.0)
    r = BO.row_sum(Gm)
    pre(draw, rowsum=r.dW_abs)
    return Gm, r


def _row_sum(lib, C, exact):
    for P in ROW_SUM_P:
        draw = make_draw(exact, 800 + P)
        Gm, r = row_sum_ref(draw, C, P)
        if lib is None:
            continue
        Of, out = outbuf((C,))
        dG = dev(Gm)
        assert lib.o3d_row_sum(ptr(dG), C, P, ptr(out), st()) == 0
        torch.cuda.synchronize()
        tail_intact(Of)
        compare("row_sum", host(out), r.dW, r.dW_abs, r.n, draw.exact)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("C", [1, 7])
def test_row_sum(lib, C, exact):
    _row_sum(lib, C, exact)


def test_row_sum_refusals(lib):
    Of, out = outbuf((2,))
    g = dev(np.zeros((2, 8)))
    assert lib.o3d_row_sum(ptr(g), 2, 6, ptr(out), st()) == EINVAL                    # P % 4 != 0
    assert lib.o3d_row_sum(None, 2, 8, ptr(out), st()) == EINVAL and lib.o3d_row_sum(ptr(g), 2, 8, None, st()) == EINVAL
    assert lib.o3d_row_sum(ptr(g), 0, 8, ptr(out), st()) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Of)
