"""o3d_group_reduce_gather_ordered (deterministic mode's layer-0 list sums) through the C ABI.

INDEX       poff equals the default entry's, perm equals the oracle's sorted index (every list ascending), on every family.
EXACT leg   dyadic inputs: S and T equal compact_oracle's fp64 sums by equality (no term dropped, doubled or misplaced).
ORDER leg   randn dN with A1 = 1, A2 = A3 = 0 (dY is dN exactly, no fused multiply-add in the comparison): S and T equal the
            float32 restatement of the written order (tests/ordered_reduce_oracle.py) BIT FOR BIT.  This pins the order; the
            default kernels cannot pass it.
INVARIANCES three launches byte-identical; S the same with T NULL; rows 0..4 of a C0 = 64 launch equal a C0 = 5 launch.
Every output buffer carries a sentinel tail (as tests/test_compact_kernels_gpu.py).
"""
import numpy as np
import pytest
import torch

import compact_oracle as O
import ordered_reduce_oracle as R

pytestmark = pytest.mark.gpu

OLD = ["singles", "full", "mixed", "paired", "wide"]
FAMILIES = OLD + R.NEW_FAMILIES
ORDER_FAMILIES = ["mixed", "paired", "wide"] + R.NEW_FAMILIES
SENT = -7.0e37
SENT_I = O.FILL_I
TAIL = 256
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi, fused  # noqa: F401
    return capi.load()


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def outbuf(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), SENT if dtype == torch.float32 else SENT_I, dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def tail_intact(*flats):
    for f in flats:
        assert bool((f[-TAIL:] == (SENT if f.dtype == torch.float32 else SENT_I)).all()), "write beyond the buffer"


def ptr(t):
    return None if t is None else t.data_ptr()


def randn32(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32).numpy()


_DL = {}


def dlayout(lib, name):
    """the family's layout built on the device, compared in full with the oracle's"""
    if name in _DL:
        return _DL[name]
    fam, L = R.family(name), R.family_layout(name)
    idx = [dev(s[0], torch.int32) for s in fam["segs"]]
    fs, t = {}, {}
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
    assert np.array_equal(t["ball_cnt"].cpu().numpy(), L.ball_cnt)
    assert np.array_equal(t["ball_off"].cpu().numpy()[:L.nballs], L.ball_off)
    assert np.array_equal(t["gp"].cpu().numpy(), L.gp) and np.array_equal(t["cw"].cpu().numpy().astype(np.float64), L.cw)
    t["L"], t["_keep"] = L, (fs, idx)
    _DL[name] = t
    return t


def dims(L):
    np1, ld1 = (L.npoint[1], L.ld[1]) if L.nseg == 2 else (0, 0)
    return (L.B, L.nseg, L.npoint[0], L.ld[0], np1, ld1), max(L.npoint) * L.ns


def launch(lib, d, i, C0, with_T=True, ordered=True):
    """one call of the ordered (or the default) entry on float32 host inputs i = dict(dN, Y0 (C0, ldp), A1..A3 (nseg*C0,))
    -> S, T (float32 host arrays; T None when not asked for), perm, poff (int32 host arrays, sentinels where nothing is written)"""
    L = d["L"]
    rd, span = dims(L)
    scratch = lib.o3d_group_reduce_gather_ordered_scratch if ordered else lib.o3d_group_reduce_gather_scratch
    npo = scratch(*rd, span)
    assert npo > 0
    dN, Y0, A1, A2, A3 = (dev(i[k]) for k in ("dN", "Y0", "A1", "A2", "A3"))
    Sf, Sd = outbuf((C0, L.ldz))
    Tf, Td = outbuf((C0, L.nballs))
    pf, perm = outbuf((L.ldp,), torch.int32)
    qf, poff = outbuf((npo,), torch.int32)
    entry = lib.o3d_group_reduce_gather_ordered if ordered else lib.o3d_group_reduce_gather
    rc = entry(ptr(dN), ptr(Y0), L.ldp, ptr(A1), ptr(A2), ptr(A3), ptr(d["gp"]), ptr(d["cw"]), ptr(d["ball_off"]),
               ptr(d["ball_cnt"]), *rd, C0, span, ptr(perm), ptr(poff), ptr(Sd), ptr(Td if with_T else None), st())
    assert rc == 0
    torch.cuda.synchronize()
    tail_intact(Sf, Tf, pf, qf)
    if not with_T:
        assert bool((Td == SENT).all())
    return Sd.cpu().numpy(), (Td.cpu().numpy() if with_T else None), perm.cpu().numpy(), poff.cpu().numpy()


def f32_inputs(i):
    return {k: np.asarray(i[k]).astype(np.float32) for k in ("dN", "Y0", "A1", "A2", "A3")}


def general_inputs(L, C0, seed):
    return dict(dN=randn32(seed, (C0, L.ldp)), Y0=randn32(seed + 1, (C0, L.ldp)), A1=randn32(seed + 2, (L.nseg * C0,)),
                A2=randn32(seed + 3, (L.nseg * C0,)), A3=randn32(seed + 4, (L.nseg * C0,)))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", FAMILIES)
def test_index_is_the_default_offsets_and_the_sorted_lists(lib, name):
    d = dlayout(lib, name)
    L = d["L"]
    i = general_inputs(L, 2, 40)
    _, _, perm_d, poff_d = launch(lib, d, i, 2, ordered=False)
    _, _, perm, poff = launch(lib, d, i, 2)
    assert np.array_equal(poff, poff_d)
    want_perm, want_poff = R.ordered_index(L)
    assert np.array_equal(poff.reshape(want_poff.shape), want_poff)
    assert np.array_equal(perm, want_perm)
    # the default fill holds the same entries list by list, in whatever order its atomics handed out
    nchunk = R.nchunk_of(L)
    for c, _, _, _, ld, q0, q1, _ in R.clouds(L):
        po = want_poff[c]
        assert np.array_equal(np.sort(perm_d[q0:q1]), np.sort(perm[q0:q1]))
        for b in range(nchunk * ld):
            lst = perm[q0 + po[b]:q0 + po[b + 1]]
            assert (np.diff(lst) > 0).all()


@pytest.mark.parametrize("C0", [5, 64])
@pytest.mark.parametrize("name", FAMILIES)
def test_exact_leg(lib, name, C0):
    d = dlayout(lib, name)
    L = d["L"]
    i = O.layer0_inputs(L, C0, O.Dyadic(300 + C0))
    dY, dYa = O.layer0_dy(L, i["dN"], i["Y0"], i["A1"], i["A2"], i["A3"])
    S, T = O.reduce_sums(L, dY)
    Sa, Ta = O.reduce_sums(L, dYa)
    O.assert_exact("S", Sa)
    O.assert_exact("T", Ta)
    Sd, Td, _, _ = launch(lib, d, f32_inputs(i), C0)
    assert np.isfinite(Sd).all() and np.isfinite(Td).all()
    assert np.array_equal(Sd.astype(np.float64), S)
    assert np.array_equal(Td.astype(np.float64), T)


_ORDER_REF = {}


def order_case(name):
    """inputs and the float32 restatement for the order leg: computed once per family"""
    if name not in _ORDER_REF:
        L, C0 = R.family_layout(name), 5
        i = dict(dN=randn32(70, (C0, L.ldp)), Y0=randn32(71, (C0, L.ldp)), A1=np.ones(L.nseg * C0, np.float32),
                 A2=np.zeros(L.nseg * C0, np.float32), A3=np.zeros(L.nseg * C0, np.float32))
        _ORDER_REF[name] = (i, R.ordered_sums(L, i["dN"][:, L.real]))
    return _ORDER_REF[name]


@pytest.mark.parametrize("name", ORDER_FAMILIES)
def test_order_leg_bit_for_bit(lib, name):
    d = dlayout(lib, name)
    i, (S, T) = order_case(name)
    Sd, Td, _, _ = launch(lib, d, i, 5)
    bad = np.argwhere(bits(Sd) != bits(S))
    assert len(bad) == 0, ("S", len(bad), bad[:8].tolist(), Sd[tuple(bad[0])], S[tuple(bad[0])])
    bad = np.argwhere(bits(Td) != bits(T))
    assert len(bad) == 0, ("T", len(bad), bad[:8].tolist(), Td[tuple(bad[0])], T[tuple(bad[0])])


@pytest.mark.parametrize("name", ["mixed", "hubrun", "misaligned"])
def test_invariances(lib, name):
    d = dlayout(lib, name)
    L = d["L"]
    i = general_inputs(L, 64, 90)
    runs = [launch(lib, d, i, 64) for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert a.tobytes() == b.tobytes()
    S0 = runs[0][0]
    Sn, Tn, _, _ = launch(lib, d, i, 64, with_T=False)
    assert Tn is None and Sn.tobytes() == S0.tobytes()
    i5 = dict(dN=i["dN"][:5], Y0=i["Y0"][:5])
    for k in ("A1", "A2", "A3"):
        i5[k] = np.ascontiguousarray(i[k].reshape(L.nseg, 64)[:, :5]).reshape(-1)
    S5, T5, _, _ = launch(lib, d, i5, 5)
    assert S5.tobytes() == S0[:5].tobytes() and T5.tobytes() == runs[0][1][:5].tobytes()


def test_refuses_what_does_not_fit(lib):
    assert lib.o3d_group_reduce_gather_ordered_scratch(1, 1, 1024, 16384, 0, 0, 32768) == -1
    t = torch.zeros(1024, device="cuda")
    ti = torch.zeros(1024, device="cuda", dtype=torch.int32)
    rc = lib.o3d_group_reduce_gather_ordered(ptr(t), ptr(t), 32768, ptr(t), ptr(t), ptr(t), ptr(ti), ptr(t), ptr(ti), ptr(ti), 1, 1,
                                             1024, 16384, 0, 0, 1, 32768, ptr(ti), ptr(ti), ptr(t), None, st())
    assert rc == EINVAL
