"""Every export of csrc/compact.hip, called through the C ABI with arguments the test can check, against the plain numpy fp64
reference tests/compact_oracle.py (tied to the slot-wise operator by tests/test_compact_oracle_cpu.py).

The layout on the device comes from o3d_compact_build (one segment) / o3d_compact_build2 (two); it is read back once per
index family and compared in full with the oracle's, and the kernels under test take those device buffers.

EXACT leg: all floating-point inputs lie on small dyadic grids, so every product and every partial sum of a correct kernel is
exactly representable in fp32 whatever its summation order (asserted before each launch: sum|terms| / spacing < 2^24), and the
comparison is EQUALITY.  A reordered sum still passes; a dropped, duplicated or misplaced term does not.
ROUNDED leg: torch.randn inputs, |err| <= (n + 8) * 2^-24 * sum|t_i| per output (n terms; sum|t_i| over the absolute values of
every product that enters a term, from the oracle; the 8 covers the roundings inside one term).  The worst err / bound per kernel
is printed and, when O3D_COMPACT_PINS names a file, written there (profiles/compact_kernel_pins.txt is such a run).
GUARDS: every output buffer has a 256-element tail and is prefilled with a sentinel; the tail, the columns beyond meta[0] and the
dead statistics rows must still hold it after the call.
"""
import os

import numpy as np
import pytest
import torch

import compact_oracle as O

pytestmark = pytest.mark.gpu

FAMILIES = ["singles", "full", "mixed", "paired", "wide"]
SENT = -7.0e37
SENT_I = O.FILL_I
TAIL = 256
EINVAL = -1
RATIOS = {}


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi, fused  # noqa: F401  (registers the signatures)
    return capi.load()


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_COMPACT_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per kernel, rounded leg of tests/test_compact_kernels_gpu.py\n"
                    "# bound = (n + 8) * 2^-24 * sum|t_i| (pool forward: 2 ulp of the fp64 result); every ratio must be <= 1\n")
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


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def outbuf(shape, dtype=torch.float32):
    """-> (flat buffer with a TAIL of sentinels, view of `shape`)"""
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), SENT if dtype == torch.float32 else SENT_I, dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def host(t):
    a = t.detach().cpu().numpy()
    return a.astype(np.float64) if a.dtype == np.float32 else a.astype(np.int64)


def tail_intact(*flats):
    for f in flats:
        assert bool((f[-TAIL:] == (SENT if f.dtype == torch.float32 else SENT_I)).all()), "write beyond the buffer"


def ptr(t):
    return None if t is None else t.data_ptr()


def pre(draw, **abs_sums):
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


_DL = {}


def dlayout(lib, name):
    """the family's layout built ON THE DEVICE, read back once and compared in full with the oracle's"""
    if name in _DL:
        return _DL[name]
    fam, L = O.family(name), O.family_layout(name)
    idx = [dev(s[0], torch.int32) for s in fam["segs"]]
    fs = {}
    t = {}
    for k, n, dt in (("ball_cnt", L.nballs, torch.int32), ("ball_off", L.nballs + 1, torch.int32), ("gp", L.ldp, torch.int32),
                     ("cball", L.ldp, torch.int32), ("cw", L.ldp, torch.float32), ("meta", L.nseg * 4, torch.int32)):
        fs[k], t[k] = outbuf((n,), dt)
    t["cw"].fill_(float(SENT_I))
    if L.nseg == 1:
        rc = lib.o3d_compact_build(idx[0].data_ptr(), L.B, L.npoint[0], L.ns, L.ld[0], 0, 0, 0, L.dummy_ball, ptr(t["ball_cnt"]),
                                   ptr(t["ball_off"]), ptr(t["gp"]), ptr(t["cball"]), ptr(t["cw"]), ptr(t["meta"]), st())
    else:
        rc = lib.o3d_compact_build2(idx[0].data_ptr(), L.npoint[0], L.ld[0], idx[1].data_ptr(), L.npoint[1], L.ld[1], L.B, L.ns,
                                    L.start1, L.pt_base[1], L.dummy_ball, ptr(t["ball_cnt"]), ptr(t["ball_off"]), ptr(t["gp"]),
                                    ptr(t["cball"]), ptr(t["cw"]), ptr(t["meta"]), st())
    assert rc == 0
    torch.cuda.synchronize()
    tail_intact(*fs.values())
    assert np.array_equal(host(t["ball_cnt"]), L.ball_cnt)
    assert np.array_equal(host(t["ball_off"])[:L.nballs], L.ball_off)
    assert np.array_equal(host(t["meta"]).reshape(L.nseg, 4), L.meta)
    assert np.array_equal(host(t["gp"]), L.gp) and np.array_equal(host(t["cball"]), L.cball)        # every column, the
    assert np.array_equal(host(t["cw"]), L.cw)                                                      # unwritten ones too
    t["L"], t["_keep"] = L, (fs, idx)
    _DL[name] = t
    return t


@pytest.mark.parametrize("name", FAMILIES)
def test_layout_matches_oracle(lib, name):
    dlayout(lib, name)


def test_compact_build_one_segment_at_a_base(lib):
    """o3d_compact_build with non-zero column / point / ball bases (how a paired call builds segment 1 on its own) gives what
    o3d_compact_build2 gives"""
    fam, L = O.family("paired"), O.family_layout("paired")
    gf, gp = outbuf((L.ldp,), torch.int32)
    bf, cball = outbuf((L.ldp,), torch.int32)
    wf, cw = outbuf((L.ldp,))
    cf, cnt = outbuf((L.nballs,), torch.int32)
    of, off = outbuf((L.nballs + 1,), torch.int32)
    mf, meta = outbuf((8,), torch.int32)
    for s in range(2):
        idx = dev(fam["segs"][s][0], torch.int32)
        assert lib.o3d_compact_build(idx.data_ptr(), L.B, L.npoint[s], L.ns, L.ld[s], L.start[s], L.pt_base[s], L.ball_base[s],
                                     L.dummy_ball, cnt[L.ball_base[s]:].data_ptr(), off[L.ball_base[s]:].data_ptr(), ptr(gp),
                                     ptr(cball), ptr(cw), meta[4 * s:].data_ptr(), st()) == 0
    torch.cuda.synchronize()
    tail_intact(gf, bf, wf, cf, of, mf)
    w = L.written
    assert np.array_equal(host(gp)[w], L.gp[w]) and np.array_equal(host(cball)[w], L.cball[w])
    assert np.array_equal(host(cw)[w], L.cw[w]) and bool((gp[torch.from_numpy(L.unwritten()).cuda()] == SENT_I).all())
    assert np.array_equal(host(cnt), L.ball_cnt) and np.array_equal(host(off)[:L.nballs], L.ball_off)
    assert np.array_equal(host(meta).reshape(2, 4), L.meta)


def test_compact_build_one_block_segment(lib):
    """A segment of ONE count workgroup (1 cloud x 8 balls x 32 slots = 256 slots, plus its padding workgroup): the smallest
    grid at which the build kernels' pick of a segment from blockIdx.x can go wrong.  Built alone (o3d_compact_build) and
    next to a copy of itself (o3d_compact_build2: once as segment 0, once as segment 1), each compared in full with the
    oracle's layout of the same indices -- every column, the unwritten ones included, sentinel tails intact."""
    B, npoint, ns, N, ld = 1, 8, 32, 40, 64
    rng = np.random.RandomState(20)
    cnts = rng.permutation(np.arange(1, ns + 1))[:npoint]
    idx = np.empty((B, npoint, ns), np.int64)
    for j, c in enumerate(cnts):             # c distinct points, then copies of the first hit (ball_query's padding)
        hits = rng.permutation(N)[:c]
        idx[0, j] = np.concatenate([hits, np.full(ns - c, hits[0])])
    assert np.array_equal(O.ball_counts(idx), cnts)
    didx = dev(idx, torch.int32)
    for nseg in (1, 2):
        L = O.Layout([(idx, ld)] * nseg)
        assert L.ldp == 256 * nseg and L.start1 == 256 * (nseg - 1)
        fs, t = {}, {}
        for k, n, dt in (("ball_cnt", L.nballs, torch.int32), ("ball_off", L.nballs + 1, torch.int32), ("gp", L.ldp, torch.int32),
                         ("cball", L.ldp, torch.int32), ("cw", L.ldp, torch.float32), ("meta", nseg * 4, torch.int32)):
            fs[k], t[k] = outbuf((n,), dt)
        t["cw"].fill_(float(SENT_I))
        out = [ptr(t[k]) for k in ("ball_cnt", "ball_off", "gp", "cball", "cw", "meta")]
        if nseg == 1:
            rc = lib.o3d_compact_build(didx.data_ptr(), B, npoint, ns, ld, 0, 0, 0, L.dummy_ball, *out, st())
        else:
            rc = lib.o3d_compact_build2(didx.data_ptr(), npoint, ld, didx.data_ptr(), npoint, ld, B, ns, L.start1, L.pt_base[1],
                                        L.dummy_ball, *out, st())
        assert rc == 0
        torch.cuda.synchronize()
        tail_intact(*fs.values())
        assert np.array_equal(host(t["ball_cnt"]), L.ball_cnt)
        assert np.array_equal(host(t["ball_off"])[:L.nballs], L.ball_off)
        assert np.array_equal(host(t["meta"]).reshape(nseg, 4), L.meta)
        assert np.array_equal(host(t["gp"]), L.gp) and np.array_equal(host(t["cball"]), L.cball)
        assert np.array_equal(host(t["cw"]), L.cw)


# ---- expand ------------------------------------------------------------------------------------------------------------
def _expand(lib, name, C0, draw):
    d = dlayout(lib, name)
    L = d["L"]
    i = O.expand_inputs(L, C0, draw)
    ldw = i["W0"].shape[1]
    Z, X3, ctr, W0, stat = dev(i["Z"]), dev(i["X3"]), dev(i["centers"]), dev(i["W0"]), dev(i["stat_c"])
    unw = L.unwritten()
    for form in ("z", "z_nocenters", "x3", "z_nopart"):
        centers = None if form == "z_nocenters" else i["centers"]
        Yr, Ya = O.expand(L, i["W0"], centers, **(dict(X3=i["X3"]) if form == "x3" else dict(Z=i["Z"])))
        Pr, Pa, live = O.expand_part(L, Yr, Ya, i["stat_c"])
        pre(draw, Y0=Ya, part0=Pa[:, 0], part1=Pa[:, 1])
        Yf, Y = outbuf((C0, L.ldp))
        Pf, P = outbuf((L.ldp // 256, 2, C0))
        part = None if form == "z_nopart" else P
        if form == "x3":
            rc = lib.o3d_group_expand_c3(ptr(X3), L.ldz, ptr(d["gp"]), ptr(d["cball"]), ptr(d["cw"]), ptr(ctr), ptr(W0), ldw, C0,
                                         ptr(d["meta"]), L.start1, L.ldp, ptr(Y), ptr(part), ptr(stat), st())
        else:
            rc = lib.o3d_group_expand_c(ptr(Z), L.ldz, ptr(d["gp"]), ptr(d["cball"]), ptr(d["cw"]),
                                        None if centers is None else ptr(ctr), ptr(W0), ldw, C0, ptr(d["meta"]), L.start1, L.ldp,
                                        ptr(Y), ptr(part), ptr(stat), st())
        assert rc == 0, form
        torch.cuda.synchronize()
        tail_intact(Yf, Pf)
        got, gpart = host(Y), host(P)
        k = "expand_c3" if form == "x3" else "expand_c"
        compare(k + ".Y0", got[:, L.real], Yr[:, L.real], Ya[:, L.real], 4, draw)
        assert np.isfinite(got[:, L.written]).all()                  # padding columns: any finite value
        assert (got[:, unw] == np.float32(SENT)).all(), form          # columns beyond meta[0]
        if part is None:
            assert (gpart == np.float32(SENT)).all()
            continue
        compare(k + ".part_sum", gpart[live, 0], Pr[live, 0], Pa[live, 0], 256, draw)
        compare(k + ".part_var", gpart[live, 1], Pr[live, 1], Pa[live, 1], 256, draw)
        assert (gpart[~live] == np.float32(SENT)).all(), form         # dead rows


@pytest.mark.parametrize("C0", [5, 64, 136])          # one per channel-split branch (1, 2, 4 ranges)
@pytest.mark.parametrize("name", FAMILIES)
def test_expand_exact(lib, name, C0):
    _expand(lib, name, C0, O.Dyadic(100 + C0))


@pytest.mark.parametrize("name", ["mixed", "paired"])
def test_expand_rounded(lib, name):
    _expand(lib, name, 64, Randn(7))


# ---- pool forward --------------------------------------------------------------------------------------------------------
def _pool_call(lib, d, kind, Y, scale, shift, C, want_arg=True):
    L = d["L"]
    n = C * L.nballs
    of, out = outbuf((n,))
    af, arg = outbuf((n,), torch.int32)
    yf, yarg = outbuf((n,))
    np1 = L.npoint[1] if L.nseg == 2 else 0
    if kind == "c":
        rc = lib.o3d_pool_fwd_c(ptr(Y), L.ldp, ptr(scale), ptr(shift), ptr(d["ball_off"]), ptr(d["ball_cnt"]), L.B, C, L.npoint[0],
                                np1, ptr(out), ptr(arg) if want_arg else None, ptr(yarg) if want_arg else None, st())
    else:
        rc = lib.o3d_pool_fwd_ct(ptr(Y), L.ldp, ptr(scale), ptr(shift), ptr(d["ball_off"]), ptr(d["ball_cnt"]), ptr(d["cball"]),
                                 ptr(d["meta"]), L.start1, L.B, C, L.npoint[0], np1, L.ns, ptr(out),
                                 ptr(arg) if want_arg else None, ptr(yarg) if want_arg else None, st())
    if rc != 0:
        return rc, None
    torch.cuda.synchronize()
    tail_intact(of, af, yf)
    if not want_arg:
        assert bool((arg == SENT_I).all()) and bool((yarg == SENT).all())
    return rc, (L.from_pooled(host(out), C), L.from_pooled(host(arg), C), L.from_pooled(host(yarg), C))


def _pool_fwd_exact(lib, name, C, kinds):
    d = dlayout(lib, name)
    L = d["L"]
    i = O.pool_inputs(L, C, O.Dyadic(200 + C))
    plants = O.plant_pool(L, i["Y"], i["scale"], i["shift"])
    seg = L.seg_of_col(L.real)
    O.assert_exact("pool", np.abs(i["Y"][:, L.real] * L.per_channel(i["scale"], C, seg)) + np.abs(L.per_channel(i["shift"], C, seg)))
    out, argq, yarg = O.pool_fwd(L, i["Y"], i["scale"], i["shift"])
    Y, scale, shift = dev(i["Y"]), dev(i["scale"]), dev(i["shift"])
    res = {}
    for kind in kinds:
        rc, got = _pool_call(lib, d, kind, Y, scale, shift, C)
        assert rc == 0
        res[kind] = got
        for what, c, ball, q, o in plants:              # named first: the planted edges
            assert got[0][c, ball] == o and (q is None or got[1][c, ball] == q), (kind, what, c, ball, got[1][c, ball], q)
        for g, r, what in zip(got, (out, argq, yarg), ("out", "argq", "yarg")):
            bad = np.argwhere(g != r)
            assert len(bad) == 0, (kind, what, len(bad), bad[:8].tolist())
    if len(res) == 2:
        assert all(np.array_equal(a, b) for a, b in zip(res["c"], res["ct"]))
    if "ct" in kinds:                                   # argq = yarg = NULL: out alone
        rc, got = _pool_call(lib, d, "ct", Y, scale, shift, C, want_arg=False)
        assert rc == 0 and np.array_equal(got[0], out)


@pytest.mark.parametrize("C", [12, 32])               # 12: not a multiple of POOL_CH = 8
@pytest.mark.parametrize("name", FAMILIES)
def test_pool_fwd_c_exact(lib, name, C):
    _pool_fwd_exact(lib, name, C, ["c", "ct"] if C == 32 and name != "wide" else ["c"])


@pytest.mark.parametrize("name", [f for f in FAMILIES if f != "wide"])
def test_pool_fwd_ct_exact_96_channels(lib, name):
    _pool_fwd_exact(lib, name, 96, ["ct"])


def test_pool_fwd_ct_rejects_more_than_32_columns_per_ball(lib):
    d = dlayout(lib, "wide")
    L = d["L"]
    Y, one = torch.zeros(32, L.ldp, device="cuda"), torch.ones(32, device="cuda")
    rc, _ = _pool_call(lib, d, "ct", Y, one, one, 32)
    assert rc == EINVAL


@pytest.mark.parametrize("kind", ["c", "ct"])
def test_pool_fwd_rounded(lib, kind):
    d = dlayout(lib, "mixed")
    L = d["L"]
    C = 32
    i = O.pool_inputs(L, C, Randn(11))
    out, _, _ = O.pool_fwd(L, i["Y"], i["scale"], i["shift"])
    rc, (gout, garg, gy) = _pool_call(lib, d, kind, dev(i["Y"]), dev(i["scale"]), dev(i["shift"]), C)
    assert rc == 0
    ulp = np.spacing(np.abs(out).astype(np.float32)).astype(np.float64)
    ratio = float((np.abs(gout - out) / (2 * ulp)).max())
    RATIOS["pool_fwd_%s.out" % kind] = ratio
    print("rounded leg pool_fwd_%s: worst err / (2 ulp) %.4f" % (kind, ratio))
    assert ratio <= 1.0
    assert (garg >= L.ball_off[None, :]).all() and (garg < (L.ball_off + L.ball_cnt)[None, :]).all()
    assert np.array_equal(gy, np.take_along_axis(i["Y"], garg, axis=1))             # bitwise: both are fp32 values


# ---- pool backward -------------------------------------------------------------------------------------------------------
def _pool_bwd(lib, name, C, draw):
    d = dlayout(lib, name)
    L = d["L"]
    i = O.pool_inputs(L, C, draw)
    if draw.exact:
        O.plant_pool(L, i["Y"], i["scale"], i["shift"])
    out, argq, yarg = O.pool_fwd(L, i["Y"], i["scale"], i["shift"])
    out = out.astype(np.float32).astype(np.float64)       # what the forward hands on (exact leg: no change)
    zero1 = i["dOut"].copy()
    if L.nseg == 2:
        zero1[:, L.ball_base[1]:] = 0.0
    unw = L.unwritten()
    o_d, a_d, y_d = dev(L.to_pooled(out)), dev(L.to_pooled(argq), torch.int32), dev(L.to_pooled(yarg))
    mean = dev(i["mean"])
    n0 = L.nballs_s[0] * C
    np0, np1 = L.npoint[0], (L.npoint[1] if L.nseg == 2 else 0)

    def check(kernel, D, part_tot, dOut):
        Dr, tot, tabs, cnt = O.pool_bwd(L, dOut, out, argq, yarg, i["mean"])
        got = host(D)
        assert np.array_equal(got[:, L.written], Dr[:, L.written]), kernel         # a copy: exact on both legs
        assert (got[:, unw] == np.float32(SENT)).all(), kernel
        compare(kernel + ".sum_g", part_tot[:, 0], tot[:, 0], tabs[:, 0], cnt[:, None], draw)
        compare(kernel + ".sum_gy", part_tot[:, 1], tot[:, 1], tabs[:, 1], cnt[:, None], draw)

    _, _, tabs, _ = O.pool_bwd(L, i["dOut"], out, argq, yarg, i["mean"])
    pre(draw, bwd0=tabs[:, 0], bwd1=tabs[:, 1])
    # o3d_pool_bwd_c: zero fill + scatter, 8 statistics rows per segment
    dO = dev(L.to_pooled(i["dOut"]))
    Df, D = outbuf((C, L.ldp))
    Pf, P = outbuf((L.nseg, 8, 2, C))
    assert lib.o3d_pool_bwd_c(ptr(dO), ptr(o_d), ptr(a_d), ptr(y_d), ptr(mean), L.B, C, np0, np1, ptr(d["meta"]), L.start1, L.ldp,
                              ptr(D), ptr(P), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Df, Pf)
    check("pool_bwd_c", D, host(P).sum(1), i["dOut"])
    # o3d_pool_bwd_dense: one pass, one statistics row per live 512-column chunk
    rows = L.ldp // 512
    live = np.zeros(rows, bool)
    live[L.written[::256] // 512] = True
    rseg = L.seg_of_col(np.arange(rows) * 512)
    big = torch.full((L.B, C + 3, np0 + 5), 9.0, device="cuda")
    view = big[:, 1:C + 1, 2:np0 + 2]
    view.copy_(dO[:n0].view(L.B, C, np0))
    variants = [("contiguous", (ptr(dO), C * np0, np0), (dO[n0:].data_ptr(), C * np1, np1) if L.nseg == 2 else (None, 0, 0),
                 i["dOut"]),
                ("strided dOut0", (view.data_ptr(), big.stride(0), big.stride(1)),
                 (dO[n0:].data_ptr(), C * np1, np1) if L.nseg == 2 else (None, 0, 0), i["dOut"]),
                ("dOut1 NULL", (ptr(dO), C * np0, np0), (None, 0, 0), zero1)]
    for what, g0, g1, ref_dOut in variants:
        Df, D = outbuf((C, L.ldp))
        Pf, P = outbuf((rows, 2, C))
        assert lib.o3d_pool_bwd_dense(g0[0], g0[1], g0[2], g1[0], g1[1], g1[2], ptr(o_d), ptr(a_d), ptr(y_d), ptr(mean),
                                      ptr(d["cball"]), ptr(d["ball_off"]), ptr(d["meta"]), L.start1, L.ldp, L.B, C, np0, np1, ptr(D),
                                      ptr(P), st()) == 0, what
        torch.cuda.synchronize()
        tail_intact(Df, Pf)
        gp_ = host(P)
        assert (gp_[~live] == np.float32(SENT)).all(), what                          # dead rows
        assert L.nseg == 1 or np.nonzero(live & (rseg == 1))[0][0] == L.start1 // 512
        tot = np.stack([gp_[live & (rseg == s)].sum(0) for s in range(L.nseg)])
        check("pool_bwd_dense", D, tot, ref_dOut)


@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("name", FAMILIES)
def test_pool_bwd_exact(lib, name, C):
    _pool_bwd(lib, name, C, O.Dyadic(200 + C))


@pytest.mark.parametrize("name", ["mixed", "paired"])
def test_pool_bwd_rounded(lib, name):
    _pool_bwd(lib, name, 24, Randn(13))


# ---- layer-0 backward sums, dw0_xyz ----------------------------------------------------------------------------------------
def _layer0(lib, name, C0, draw):
    d = dlayout(lib, name)
    L = d["L"]
    i = O.layer0_inputs(L, C0, draw)
    dY, dYa = O.layer0_dy(L, i["dN"], i["Y0"], i["A1"], i["A2"], i["A3"])
    S, T = O.reduce_sums(L, dY)
    Sa, Ta = O.reduce_sums(L, dYa)
    nS, _ = O.reduce_sums(L, np.ones((1, len(L.real))))
    W, Wa = O.dw0_xyz(L, dY, i["X"], i["centers"]), O.dw0_xyz(L, dYa, i["X"], i["centers"], absolute=True)
    pre(draw, S=Sa, T=Ta, dW0=Wa)
    dN, Y0, A1, A2, A3 = (dev(i[k]) for k in ("dN", "Y0", "A1", "A2", "A3"))
    X, ctr = dev(i["X"]), dev(i["centers"])
    np1, ld1 = (L.npoint[1], L.ld[1]) if L.nseg == 2 else (0, 0)
    span = max(L.npoint) * L.ns
    npo = lib.o3d_group_reduce_gather_scratch(L.B, L.nseg, L.npoint[0], L.ld[0], np1, ld1, span)
    assert npo > 0
    for what in ("gather", "gather T NULL", "atomic"):
        Sf, Sd = outbuf((C0, L.ldz))
        Tf, Td = outbuf((C0, L.nballs))
        Tp = None if what == "gather T NULL" else Td
        if what == "atomic":
            rc = lib.o3d_group_reduce_c(ptr(dN), ptr(Y0), L.ldp, ptr(A1), ptr(A2), ptr(A3), ptr(d["gp"]), ptr(d["cball"]), ptr(d["cw"]),
                                        ptr(d["ball_off"]), ptr(d["ball_cnt"]), L.B, L.nseg, L.npoint[0], L.ld[0], np1, ld1, C0,
                                        ptr(Sd), ptr(Tp), st())
        else:
            pf, perm = outbuf((L.ldp,), torch.int32)
            qf, poff = outbuf((npo,), torch.int32)
            rc = lib.o3d_group_reduce_gather(ptr(dN), ptr(Y0), L.ldp, ptr(A1), ptr(A2), ptr(A3), ptr(d["gp"]), ptr(d["cw"]),
                                             ptr(d["ball_off"]), ptr(d["ball_cnt"]), L.B, L.nseg, L.npoint[0], L.ld[0], np1, ld1, C0,
                                             span, ptr(perm), ptr(poff), ptr(Sd), ptr(Tp), st())
        assert rc == 0, what
        torch.cuda.synchronize()
        tail_intact(Sf, Tf)
        if what != "atomic":
            tail_intact(pf, qf)
        k = "reduce_c" if what == "atomic" else "reduce_gather"
        compare(k + ".S", host(Sd), S, Sa, nS, draw)                 # unreferenced points (N .. ld-1 among them): exactly 0
        if Tp is None:
            assert bool((Td == SENT).all())
        else:
            compare(k + ".T", host(Td), T, Ta, L.ball_cnt[None, :], draw)
    Pf, P = outbuf((L.ldp // 256, C0, 3))
    Wf, Wd = outbuf((C0, 3))
    assert lib.o3d_group_dw0_xyz(ptr(dN), ptr(Y0), L.ldp, ptr(A1), ptr(A2), ptr(A3), ptr(d["gp"]), ptr(d["cball"]), ptr(d["cw"]),
                                 ptr(X), L.ldz, ptr(ctr), ptr(d["meta"]), L.start1, C0, ptr(P), ptr(Wd), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Pf, Wf)
    compare("dw0_xyz.dW0", host(Wd), W, Wa, len(L.real), draw)


@pytest.mark.parametrize("C0", [5, 64])               # 5: odd, the clamped last row of the 2-channel slab
@pytest.mark.parametrize("name", FAMILIES)
def test_layer0_sums_exact(lib, name, C0):
    _layer0(lib, name, C0, O.Dyadic(300 + C0))


@pytest.mark.parametrize("name", ["mixed", "paired"])
def test_layer0_sums_rounded(lib, name):
    _layer0(lib, name, 64, Randn(17))


def test_unreferenced_points_get_zero(lib):
    """mixed: points N .. ld-1 of every cloud are in no ball: S there is 0 (not merely small)"""
    d = dlayout(lib, "mixed")
    L = d["L"]
    N, ld = O.family("mixed")["segs"][0][1:]
    dead = np.concatenate([b * ld + np.arange(N, ld) for b in range(L.B)])
    assert not np.isin(dead, L.gp[L.real]).any()
    i = O.layer0_inputs(L, 5, O.Dyadic(1))
    dY, _ = O.layer0_dy(L, i["dN"], i["Y0"], i["A1"], i["A2"], i["A3"])
    assert (O.reduce_sums(L, dY)[0][:, dead] == 0).all()            # (the device result equals this oracle in the tests above)


def test_reduce_gather_refuses_what_does_not_fit(lib):
    assert lib.o3d_group_reduce_gather_scratch(1, 1, 1024, 16384, 0, 0, 32768) == -1
    t = torch.zeros(1024, device="cuda")
    ti = torch.zeros(1024, device="cuda", dtype=torch.int32)
    rc = lib.o3d_group_reduce_gather(ptr(t), ptr(t), 32768, ptr(t), ptr(t), ptr(t), ptr(ti), ptr(t), ptr(ti), ptr(ti), 1, 1, 1024,
                                     16384, 0, 0, 1, 32768, ptr(ti), ptr(ti), ptr(t), None, st())
    assert rc == EINVAL


# ---- centre terms --------------------------------------------------------------------------------------------------------
def _center(lib, nballs, draw):
    C0, ldw, ncols = 7, 6, 5
    i = O.center_inputs(nballs, C0, ldw, draw)
    ta = O.center_term(i["T"], i["centers"], i["dW"], absolute=True)
    ga = O.center_grad(i["T"], i["W0"], 0.5, absolute=True)
    pre(draw, center_term=ta, center_grad=ga)
    T, ctr, W0 = dev(i["T"]), dev(i["centers"]), dev(i["W0"])
    ref = O.center_term(i["T"], i["centers"], i["dW"])
    n = np.full((C0, ldw), 1.0)
    n[:, :3] = nballs + 1
    # in place
    Wf, dW = outbuf((C0, ldw))
    dW.copy_(dev(i["dW"]))
    assert lib.o3d_center_term(ptr(T), ptr(ctr), C0, nballs, ldw, ptr(dW), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Wf)
    compare("center_term", host(dW), ref, ta, n, draw)
    assert np.array_equal(host(dW)[:, 3:], i["dW"][:, 3:])
    # into a compact gradient: dW untouched
    dW.copy_(dev(i["dW"]))
    of, out = outbuf((C0, ncols))
    assert lib.o3d_center_term_out(ptr(T), ptr(ctr), C0, nballs, ldw, ptr(dW), ncols, ptr(out), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Wf, of)
    assert np.array_equal(host(dW), i["dW"])
    compare("center_term_out", host(out), ref[:, :ncols], ta[:, :ncols], n[:, :ncols], draw)
    gf, g = outbuf((3, nballs))
    assert lib.o3d_center_grad(ptr(T), ptr(W0), ldw, C0, nballs, 0.5, ptr(g), st()) == 0
    torch.cuda.synchronize()
    tail_intact(gf)
    compare("center_grad", host(g), O.center_grad(i["T"], i["W0"], 0.5), ga, C0, draw)


@pytest.mark.parametrize("nballs", [1, 1025])         # one more than a multiple of the 1024-thread stride
def test_center_terms_exact(lib, nballs):
    _center(lib, nballs, O.Dyadic(400 + nballs))


def test_center_terms_rounded(lib):
    _center(lib, 1025, Randn(19))


# ---- pack_points ---------------------------------------------------------------------------------------------------------
def _pack(lib, two, nxyz, draw):
    B, C = 2, 3
    inv_r = 0.5 if draw.exact else float(np.float32(0.3))          # (the C ABI takes a float)
    i = O.pack_inputs(two, draw, B, C)
    N0, ld0, N1, ld1, xyz, feats = (i[k] for k in ("N0", "ld0", "N1", "ld1", "xyz", "feats"))
    rows = nxyz + C + 2
    ref = O.pack_points(xyz[0], feats[0], N0, ld0, xyz[1], feats[1], N1, ld1, B, nxyz, C, inv_r, rows)
    pre(draw, pack=np.abs(ref))
    x0, f0 = dev(xyz[0]), dev(feats[0])
    x1, f1 = (dev(xyz[1]), dev(feats[1])) if two else (None, None)
    Xf, X = outbuf(ref.shape)
    assert lib.o3d_pack_points(ptr(x0) if nxyz else None, ptr(f0), N0, ld0, ptr(x1) if nxyz else None, ptr(f1), N1, ld1, B, nxyz,
                               C, inv_r, rows, ptr(X), st()) == 0
    torch.cuda.synchronize()
    tail_intact(Xf)
    got = host(X)
    compare("pack_points", got, ref, np.abs(ref), 1, draw)
    assert (got[nxyz + C:] == 0).all() and (got[:, N0:ld0] == 0).all() and (got[:, ld0 + N0:2 * ld0] == 0).all()
    if two:
        assert (got[:, 2 * ld0 + N1:2 * ld0 + ld1] == 0).all() and (got[:, 2 * ld0 + ld1 + N1:] == 0).all()


@pytest.mark.parametrize("nxyz", [0, 3])
@pytest.mark.parametrize("two", [False, True])
def test_pack_points_exact(lib, two, nxyz):
    _pack(lib, two, nxyz, O.Dyadic(500 + nxyz + two))


def test_pack_points_rounded(lib):
    _pack(lib, True, 3, Randn(23))
