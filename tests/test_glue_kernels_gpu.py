"""The glue in front of the GEMMs -- o3d_sample_query and the grid-stride wrap of o3d_ball_query (csrc/index_ops.hip),
o3d_gather_rows2, o3d_pack_rows / o3d_pack_rows_ld, o3d_prep_weights (csrc/heads.hip) and o3d_cosine_sim_fwd /
o3d_cosine_sim_bwd (csrc/xcorr.hip) -- called through the C ABI with raw pointers against tests/glue_oracle.py (tied to
nn.CosineSimilarity under autograd by tests/test_glue_oracle_cpu.py) and, for the ball query, oracle.ops.ball_query on centres
gathered in numpy.  Everything but the cosine map moves values or indices without arithmetic: the comparison is EQUALITY
(floats bit for bit) and every output is prefilled with a sentinel, tails and never-written padding included; every input
carries a tail of NaN (floats) or of indices that point into such a tail.
The cosine map has two legs like the GEMM pins.  EXACT: columns of four entries +-2^k (forward) and power-of-two norms with
dyadic values elsewhere (backward; the test supplies sim, tn, sn, dsim itself): equality.  ROUNDED, stage by stage: the
stored tn / sn against fp64, sim against fp64 over the STORED norms, dt / ds against fp64 over the fp32 inputs handed to the
backward; the bounds are derived in tests/glue_oracle.py (division and square root are correctly rounded in this build).
The worst err / bound per kernel is printed and, when O3D_GLUE_PINS names a file, written there
(profiles/glue_kernel_pins.txt is such a run).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import glue_oracle as GO

pytestmark = pytest.mark.gpu

SENT = -7.0e37
SENT_I = -77777
TAIL = 256
EINVAL = -1
RATIOS = {}


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi
    return capi.load()


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_GLUE_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per output, rounded leg of the cosine map in tests/test_glue_kernels_gpu.py\n"
                    "# bounds: tests/glue_oracle.py (u = 2^-24; division and square root correctly rounded: one rounding each,\n"
                    "# no measured allowance); every ratio must be <= 1.  Every other entry of that file is compared for equality.\n")
            for k in sorted(RATIOS):
                f.write("%-28s %.4f\n" % (k, RATIOS[k]))


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a, pad=float("nan")):
    """device copy of an fp32 operand, followed by TAIL NaNs no correct kernel may read"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    flat = torch.full((a.size + TAIL,), pad, dtype=torch.float32, device="cuda")
    flat[:a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return flat[:a.size].view(a.shape)


def dev_i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    flat = torch.zeros((a.size + TAIL,), dtype=torch.int32, device="cuda")
    flat[:a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return flat[:a.size].view(a.shape)


def outbuf(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), SENT if dtype == torch.float32 else SENT_I, dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def sent_of(t):
    return SENT if t.dtype == torch.float32 else SENT_I


def tail_intact(*flats):
    for f in flats:
        assert bool((f[-TAIL:] == sent_of(f)).all()), "write beyond the buffer"


def untouched(t):
    return bool((t == sent_of(t)).all())


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(what, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(bits(got) != bits(ref)) if got.dtype.kind == "f" else np.argwhere(got != ref)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())


def compare(kernel, got, ref, bound, exact, ratios=RATIOS):
    """exact leg: equality.  rounded leg: |got - ref| <= bound (an array, derived in glue_oracle), worst ratio recorded"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), kernel
    if exact:
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (kernel, len(bad), bad[:8].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        return
    err = np.abs(got - ref)
    assert (err[bound == 0] == 0).all(), kernel
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    ratios[kernel] = max(ratios.get(kernel, 0.0), ratio)
    print("rounded leg %s: worst err/bound %.4f" % (kernel, ratio))
    assert ratio <= 1.0, (kernel, ratio)


# ==== o3d_sample_query / o3d_ball_query =========================================================================================
def cloud(rng, B, N):
    return rng.rand(B, N, 3).astype(np.float32)


def sq_call(lib, sets, B, radius, nsample, idx, centers, over=None):
    """sets: [(xyz dev, sidx dev | None, N, npoint)], one or two; over: {name: value} of arguments to replace"""
    s0 = sets[0]
    s1 = sets[1] if len(sets) > 1 else (None, None, 0, 0)
    a = dict(xyz0=ptr(s0[0]), sidx0=ptr(s0[1]), N0=s0[2], np0=s0[3], idx0=ptr(idx[0]), xyz1=ptr(s1[0]), sidx1=ptr(s1[1]), N1=s1[2],
             np1=s1[3], idx1=ptr(idx[1]) if len(idx) > 1 else None, B=B, nsample=nsample, centers=ptr(centers))
    a.update(over or {})
    return lib.o3d_sample_query(a["xyz0"], a["sidx0"], a["N0"], a["np0"], a["idx0"], a["xyz1"], a["sidx1"], a["N1"], a["np1"],
                                a["idx1"], a["B"], radius, a["nsample"], a["centers"], st())


def run_sq(lib, sets, radius, nsample):
    """sets: [(xyz (B, N, 3) float32, sidx (B, npoint) | None, npoint)] -> checks centres bit for bit and both index blocks"""
    from oracle import ops
    B = sets[0][0].shape[0]
    ref_c, per = GO.sample_query_centers(sets)
    dsets = [(dev(x), dev_i(si) if si is not None else None, x.shape[1], npnt) for x, si, npnt in sets]
    flats, idx = zip(*[outbuf((B, npnt, nsample), torch.int32) for _, _, npnt in sets])
    Cf, centers = outbuf(ref_c.shape)
    assert sq_call(lib, dsets, B, radius, nsample, idx, centers) == 0
    torch.cuda.synchronize()
    tail_intact(Cf, *flats)
    same_bits("centers", centers.cpu().numpy(), ref_c)
    for k, ((x, _, _), c) in enumerate(zip(sets, per)):
        same_bits("idx%d" % k, idx[k].cpu().numpy(), ops.ball_query(c, x, radius, nsample))
    return [i.cpu().numpy() for i in idx]


def sidx_of(rng, B, N, npoint, mode="random"):
    if mode == "dups":                                        # duplicates, out of order, the last point first
        s = rng.randint(0, N, size=(B, npoint))
        s[:, 0] = N - 1
        if npoint > 2:
            s[:, 1] = s[:, 2]
        return s.astype(np.int32)
    return np.stack([rng.permutation(N)[:npoint] for _ in range(B)]).astype(np.int32)


@pytest.mark.parametrize("nsample", [1, 16, 70])
def test_sample_query_sets_and_index_sources(lib, nsample):
    rng = np.random.RandomState(10 + nsample)
    B, N0, N1 = 3, 65, 200
    x0, x1 = cloud(rng, B, N0), cloud(rng, B, N1)
    radius = 0.9 if nsample == 70 else 0.3                     # 0.9: more than 64 hits in the cloud of 200 (a second ballot)
    run_sq(lib, [(x0, sidx_of(rng, B, N0, 33), 33), (x1, sidx_of(rng, B, N1, 1), 1)], radius, nsample)      # both sampled
    run_sq(lib, [(x0, None, 33), (x1, None, 1)], radius, nsample)                                            # both prefixes
    run_sq(lib, [(x0, None, 1), (x1, sidx_of(rng, B, N1, 33, "dups"), 33)], radius, nsample)                 # one of each
    run_sq(lib, [(x1, sidx_of(rng, B, N1, 33, "dups"), 33), (x0, None, 65)], radius, nsample)
    got = run_sq(lib, [(x1, sidx_of(rng, B, N1, 33), 33)], radius, nsample)                                  # npoint1 = 0, NULLs
    if nsample == 70:
        assert (np.diff(got[0][:, :, :66].astype(np.int64), axis=-1) > 0).all(-1).any(), "no ball reached a second ballot"


def test_sample_query_edges(lib):
    # d2 == r2 is excluded, d2 < r2 included; a radius of 0 hits nothing, not even the centre itself: the row is all 0
    x = np.array([[[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 1, 0], [0, 0, 0.75], [3, 3, 3]]], np.float32)
    got = run_sq(lib, [(x, None, 6)], 1.0, 4)[0]
    assert got[0, 0].tolist() == [0, 2, 4, 0] and got[0, 5].tolist() == [5, 5, 5, 5] and got[0, 1].tolist() == [1, 2, 1, 1]
    got = run_sq(lib, [(x, np.array([[5, 0]], np.int32), 2)], 0.0, 3)[0]
    assert not got.any()
    # duplicated points: every copy is a hit of its own
    d = np.repeat(np.array([[[0.25, 0.5, 0.75], [0.5, 0.5, 0.5]]], np.float32), 5, axis=1)
    got = run_sq(lib, [(d, None, 10)], 0.1, 8)[0]
    assert got[0, 0].tolist() == [0, 1, 2, 3, 4, 0, 0, 0] and got[0, 9].tolist() == [5, 6, 7, 8, 9, 5, 5, 5]
    # N = 1, in both sets
    one = np.array([[[0.5, 0.25, 0.125]], [[1, 2, 3]]], np.float32)
    got = run_sq(lib, [(one, None, 1), (one, np.zeros((2, 4), np.int32), 4)], 0.5, 2)
    assert not got[0].any() and not got[1].any()


def test_sample_query_refusals(lib):
    rng = np.random.RandomState(3)
    B, N = 2, 8
    x = dev(cloud(rng, B, N))
    si = dev_i(sidx_of(rng, B, N, 4))
    If, idx0 = outbuf((B, 9, 4), torch.int32)
    Jf, idx1 = outbuf((B, 9, 4), torch.int32)
    Cf, centers = outbuf((B * 18 + 1, 3))
    good = [(x, si, N, 4), (x, si, N, 4)]
    assert sq_call(lib, good, B, 0.3, 4, (idx0, idx1), centers) == 0
    torch.cuda.synchronize()
    for f in (If, Jf, Cf):
        f.fill_(sent_of(f))
    for over in (dict(B=0), dict(N0=0), dict(np0=0), dict(nsample=0), dict(xyz0=None), dict(idx0=None), dict(centers=None),
                 dict(np1=-1), dict(xyz1=None), dict(idx1=None), dict(N1=0),
                 dict(sidx0=None, np0=9),                     # a prefix longer than the cloud
                 dict(sidx1=None, np1=9)):
        assert sq_call(lib, good, B, 0.3, 4, (idx0, idx1), centers, over) == EINVAL, over
    torch.cuda.synchronize()
    assert untouched(If) and untouched(Jf) and untouched(Cf)


WRAP_B, WRAP_NPOINT, WRAP_N, WRAP_NS = 2, 32770, 8, 4          # 65 540 centres: 16 385 blocks of 4, one more than the grid cap


def test_grid_stride_wrap_of_both_ball_queries(lib):
    from oracle import ops
    rng = np.random.RandomState(4)
    x = cloud(rng, WRAP_B, WRAP_N)
    si = rng.randint(0, WRAP_N, size=(WRAP_B, WRAP_NPOINT)).astype(np.int32)
    assert WRAP_B * WRAP_NPOINT == 65540 and (WRAP_B * WRAP_NPOINT + 3) // 4 > 16384
    got = run_sq(lib, [(x, si, WRAP_NPOINT)], 0.4, WRAP_NS)[0]
    c = GO.sample_centres(x, si, WRAP_NPOINT)
    If, idx = outbuf((WRAP_B, WRAP_NPOINT, WRAP_NS), torch.int32)
    dc, dx = dev(c), dev(x)
    assert lib.o3d_ball_query(ptr(dc), ptr(dx), WRAP_B, WRAP_N, WRAP_NPOINT, 0.4, WRAP_NS, ptr(idx), st()) == 0
    torch.cuda.synchronize()
    tail_intact(If)
    same_bits("ball_query", idx.cpu().numpy(), ops.ball_query(c, x, 0.4, WRAP_NS))
    same_bits("ball_query == sample_query", idx.cpu().numpy(), got)


# ==== o3d_gather_rows2 ==========================================================================================================
def g2_call(lib, a, Da, b, Db, idx, ld, B, N, npoint, oa, ob):
    return lib.o3d_gather_rows2(ptr(a), Da, ptr(b), Db, ptr(idx), ld, B, N, npoint, ptr(oa), ptr(ob), st())


@pytest.mark.parametrize("Da,Db", [(3, 1), (1, 0), (9, 3)])
def test_gather_rows2(lib, Da, Db):
    rng = np.random.RandomState(20 + Da)
    B, N = 3, 20
    a = rng.randn(B, N, Da).astype(np.float32)
    b = rng.randn(B, N, Db).astype(np.float32) if Db else None
    da, db = dev(a), dev(b) if Db else None
    for npoint, ld in ((7, 7), (7, 11), (1, 4), (20, 23)):
        idx = rng.randint(0, N, size=(B, ld)).astype(np.int32)
        idx[:, npoint:] = N + 1 + np.arange(ld - npoint)[None, :]      # beyond npoint: rows inside the NaN tail of a / b
        if npoint > 2:
            idx[:, 2] = idx[:, 0]                                       # a duplicated index
        ra, rb = GO.gather_rows2(a, b, idx, npoint)
        Af, oa = outbuf((B, npoint, Da))
        Bf, ob = outbuf((B, npoint, max(Db, 1)))
        di = dev_i(idx)
        assert g2_call(lib, da, Da, db, Db, di, ld, B, N, npoint, oa, ob if Db else None) == 0
        torch.cuda.synchronize()
        tail_intact(Af, Bf)
        same_bits("outa", oa.cpu().numpy(), ra)
        if Db:
            same_bits("outb", ob.cpu().numpy(), rb)
        else:
            assert untouched(Bf)
    # npoint = 0: OK, nothing written; ld_idx < npoint and missing operands: refused
    Af, oa = outbuf((B, 7, Da))
    Bf, ob = outbuf((B, 7, max(Db, 1)))
    di = dev_i(rng.randint(0, N, size=(B, 7)))
    assert g2_call(lib, da, Da, db, Db, di, 7, B, N, 0, oa, ob if Db else None) == 0
    assert g2_call(lib, da, Da, db, Db, di, 6, B, N, 7, oa, ob if Db else None) == EINVAL
    assert g2_call(lib, None, Da, db, Db, di, 7, B, N, 7, oa, ob if Db else None) == EINVAL
    assert g2_call(lib, da, Da, db, Db, None, 7, B, N, 7, oa, ob if Db else None) == EINVAL
    assert g2_call(lib, da, Da, da, 1, di, 7, B, N, 7, oa, None) == EINVAL
    torch.cuda.synchronize()
    assert untouched(Af) and untouched(Bf)


# ==== o3d_pack_rows / o3d_pack_rows_ld ========================================================================================
def rows_src(tensors):
    from open3dsot_amd import capi
    arr = (capi.struct("o3d_rows_src") * len(tensors))()
    for i, t in enumerate(tensors):
        sb, sc, sn = t.stride()
        arr[i].p, arr[i].sb, arr[i].sc, arr[i].sn, arr[i].C = t.data_ptr(), sb, sc, sn, t.shape[1]
    return arr


def pack_sources(rng, B, N):
    """four (B, C_i, N) views with the strides the trackers pass: a transposed (B, N, 3), a (C, B, N) buffer seen as
    (B, C, N), a strided slice (every second column, channels 1..5 of 7), a contiguous one"""
    xyz = dev(rng.randn(B, N, 3))
    cbn = dev(rng.randn(5, B, N))
    wide = dev(rng.randn(B, 7, 2 * N))
    plain = dev(rng.randn(B, 2, N))
    return [xyz.transpose(1, 2), cbn.permute(1, 0, 2), wide[:, 1:6, ::2], plain]


@pytest.mark.parametrize("B,N", [(1, 1), (3, 85), (2, 128), (1, 257)])
def test_pack_rows(lib, B, N):
    rng = np.random.RandomState(30 + N)
    srcs = pack_sources(rng, B, N)
    assert B * N in (1, 255, 256, 257)
    for nsrc in (1, 2, 3, 4):
        use = srcs[:nsrc]
        total = sum(t.shape[1] for t in use)
        arr = rows_src(use)
        for rows in (total, total + 3):
            ref = GO.pack_rows([t.cpu().numpy() for t in use], rows)
            Xf, X = outbuf((rows, B * N))
            assert lib.o3d_pack_rows(ctypes.addressof(arr), nsrc, B, N, rows, ptr(X), st()) == 0
            torch.cuda.synchronize()
            tail_intact(Xf)
            same_bits("pack_rows", X.cpu().numpy(), ref)
            # the same into a column block in the middle of a wider operand, and with ld == B*N
            for ld, col0 in ((B * N + 9, 4), (B * N, 0)):
                Wf, Wd = outbuf((rows, ld))
                assert lib.o3d_pack_rows_ld(ctypes.addressof(arr), nsrc, B, N, rows, ptr(Wd[0, col0:]), ld, st()) == 0
                torch.cuda.synchronize()
                tail_intact(Wf)
                got = Wd.cpu().numpy()
                same_bits("pack_rows_ld", got[:, col0:col0 + B * N], ref)
                assert (got[:, :col0] == SENT).all() and (got[:, col0 + B * N:] == SENT).all()
        Xf, X = outbuf((total, B * N))
        assert lib.o3d_pack_rows(ctypes.addressof(arr), nsrc, B, N, total - 1, ptr(X), st()) == EINVAL      # sum C > rows
        assert lib.o3d_pack_rows_ld(ctypes.addressof(arr), nsrc, B, N, total - 1, ptr(X), B * N, st()) == EINVAL
        assert lib.o3d_pack_rows_ld(ctypes.addressof(arr), nsrc, B, N, total, ptr(X), B * N - 1, st()) == EINVAL   # ld < B*N
        assert lib.o3d_pack_rows(ctypes.addressof(arr), 5, B, N, total, ptr(X), st()) == EINVAL
        assert lib.o3d_pack_rows(ctypes.addressof(arr), nsrc, B, N, total, None, st()) == EINVAL
        torch.cuda.synchronize()
        assert untouched(Xf)


# ==== o3d_prep_weights ==========================================================================================================
PREP_SHAPES = ((1, 1), (1, 8191), (8191, 1), (64, 128), (3, 2731), (130, 130), (1, 16385))      # rows * cols = 1, 8191, 8192, 8193, > 2 * 8192


def prep_jobs(rng, shapes):
    """-> [(src numpy, rows, cols, ld, transpose)]: plain and transposed, ld equal to and larger than the copied width"""
    jobs = []
    for n, (r, c) in enumerate(shapes):
        for tr in (0, 1):
            width = r if tr else c
            jobs.append((rng.randn(r, c).astype(np.float32), r, c, width + (0, 5)[(n + tr) % 2], tr))
    return jobs


def run_prep(lib, jobs):
    keep, table, checks = [], [], []
    for src, r, c, ld, tr in jobs:
        d = dev(src)
        n = (c if tr else r) * ld
        Df, dst = outbuf((n,))
        keep.append((d, Df))
        table.append([d.data_ptr(), dst.data_ptr(), r, c, ld, tr])
        checks.append((Df, dst, GO.prep_weights(np.full(n, SENT, np.float32), src, ld, tr)))
    t = torch.tensor(table, dtype=torch.int64, device="cuda")
    assert lib.o3d_prep_weights(t.data_ptr(), len(jobs), st()) == 0
    torch.cuda.synchronize()
    for Df, dst, ref in checks:
        tail_intact(Df)
        same_bits("prep_weights", dst.cpu().numpy(), ref)       # (the padding of dst keeps the sentinel: it is part of ref)


def test_prep_weights(lib):
    rng = np.random.RandomState(40)
    jobs = prep_jobs(rng, PREP_SHAPES)
    run_prep(lib, jobs[:1])
    run_prep(lib, jobs[1:4])
    run_prep(lib, jobs)                                        # 14 jobs, every size
    small = prep_jobs(rng, [(1 + k % 5, 1 + k % 7) for k in range(16)]) + [(rng.randn(1, 40).astype(np.float32), 1, 40, 40, 0)]
    assert len(small) == 33
    run_prep(lib, small)                                       # a table of 33, a vector as (1, n) last
    assert lib.o3d_prep_weights(None, 1, st()) == EINVAL
    t = torch.zeros((1, 6), dtype=torch.int64, device="cuda")
    assert lib.o3d_prep_weights(t.data_ptr(), 0, st()) == EINVAL


# ==== o3d_cosine_sim_fwd / o3d_cosine_sim_bwd =================================================================================
COS_SHAPES = ((32, 4, 1), (32, 12, 31), (96, 60, 32), (32, 64, 33), (96, 12, 100), (96, 64, 128), (32, 60, 128), (96, 4, 100))
COS_LAYOUTS = ("flat", "contiguous", "point_major")


def lay_out(t, s, layout):
    """t (B, f, M), s (B, f, N) numpy -> device views with the strides of `layout`.  flat: both are column blocks of one
    (f, ld) matrix, columns in (b, point) order -- how the trackers pass the conv_final output; point_major: (B, K, f)"""
    B, f, M = t.shape
    N = s.shape[2]
    if layout == "contiguous":
        return dev(t), dev(s)
    if layout == "point_major":
        return dev(t.transpose(0, 2, 1)).transpose(1, 2), dev(s.transpose(0, 2, 1)).transpose(1, 2)
    ld = B * M + B * N + 3
    flat = np.full((f, ld), np.nan, np.float32)
    flat[:, :B * M] = t.transpose(1, 0, 2).reshape(f, B * M)
    flat[:, B * M:B * M + B * N] = s.transpose(1, 0, 2).reshape(f, B * N)
    d = dev(flat)
    return (d[:, :B * M].view(f, B, M).permute(1, 0, 2), d[:, B * M:B * M + B * N].view(f, B, N).permute(1, 0, 2))


def cos_fwd(lib, dt_, ds_, dims, over=None):
    """dims = (B, f, M, N); over: {name: value} of arguments to replace"""
    B, f, M, N = dims
    Sf, sim = outbuf((B, N, M))
    Tf, tn = outbuf((B, M))
    Nf, sn = outbuf((B, N))
    a = dict(t=ptr(dt_), s=ptr(ds_), f=f, M=M, N=N, sim=ptr(sim), tn=ptr(tn), sn=ptr(sn))
    a.update(over or {})
    rc = lib.o3d_cosine_sim_fwd(a["t"], *dt_.stride(), a["s"], *ds_.stride(), B, a["f"], a["M"], a["N"], a["sim"], a["tn"], a["sn"],
                                st())
    torch.cuda.synchronize()
    return rc, (Sf, Tf, Nf), (sim, tn, sn)


def cos_bwd(lib, dsim, sim, tn, sn, dt_, ds_, dims, over=None):
    B, f, M, N = dims
    Af, gt = outbuf((B, f, M))
    Bf, gs = outbuf((B, f, N))
    a = dict(dsim=ptr(dsim), sim=ptr(sim), tn=ptr(tn), sn=ptr(sn), t=ptr(dt_), s=ptr(ds_), f=f, M=M, N=N, dt=ptr(gt), ds=ptr(gs))
    a.update(over or {})
    rc = lib.o3d_cosine_sim_bwd(a["dsim"], a["sim"], a["tn"], a["sn"], a["t"], *dt_.stride(), a["s"], *ds_.stride(), B, a["f"],
                                a["M"], a["N"], a["dt"], a["ds"], st())
    torch.cuda.synchronize()
    return rc, (Af, Bf), (gt, gs)


def h(t):
    return t.detach().cpu().numpy().astype(np.float64)


def zero_cols(M, N):
    """a zero template column and a zero search column where the shape has room for one beside a live one"""
    return ((1,) if M > 1 else ()), ((0,) if N > 1 else ())


def check_fwd(r, flats, outs, exact, zt, zs):
    tail_intact(*flats)
    sim, tn, sn = (h(o) for o in outs)
    compare("cosine_fwd.tn", tn, r.tn, r.tn_bound, exact)
    compare("cosine_fwd.sn", sn, r.sn, r.sn_bound, exact)
    for cols, n in ((zt, tn), (zs, sn)):
        for k in cols:
            assert (n[:, k] == GO.EPS).all()                  # the clamped norm, exactly
    return sim, tn, sn


@pytest.mark.parametrize("layout", COS_LAYOUTS)
@pytest.mark.parametrize("B", [1, 3])
def test_cosine_sim_exact(lib, B, layout):
    for n, (f, M, N) in enumerate(COS_SHAPES):
        rng = np.random.RandomState(50 + n)
        zt, zs = zero_cols(M, N)
        t, s = GO.pow2_columns(rng, B, f, M, zt), GO.pow2_columns(rng, B, f, N, zs)
        r = GO.cosine_sim(t, s)
        dt_, ds_ = lay_out(t, s, layout)
        rc, flats, outs = cos_fwd(lib, dt_, ds_, (B, f, M, N))
        assert rc == 0
        sim, _, _ = check_fwd(r, flats, outs, True, zt, zs)
        compare("cosine_fwd.sim", sim, r.sim, None, True)
        # backward on inputs of its own: power-of-two norms (also all below eps: no gradient through them), dyadic values
        for clamped in (False, True):
            i = GO.exact_bwd_inputs(rng, B, f, M, N, clamped_t=clamped)
            rb = GO.cosine_sim_bwd(i.dsim, i.sim, i.tn, i.sn, i.t, i.s)
            GO.assert_exact_bwd(i, rb)
            bt, bs = lay_out(i.t, i.s, layout)
            keep = [dev(i.dsim), dev(i.sim), dev(i.tn), dev(i.sn)]
            rc, flats, (gt, gs) = cos_bwd(lib, *keep, bt, bs, (B, f, M, N))
            assert rc == 0
            tail_intact(*flats)
            compare("cosine_bwd.dt", h(gt), rb.dt, None, True)
            compare("cosine_bwd.ds", h(gs), rb.ds, None, True)


@pytest.mark.parametrize("layout", COS_LAYOUTS)
@pytest.mark.parametrize("B", [1, 3])
def test_cosine_sim_rounded(lib, B, layout):
    for n, (f, M, N) in enumerate(COS_SHAPES):
        g = torch.Generator().manual_seed(60 + n)
        zt, zs = zero_cols(M, N)
        t = torch.randn((B, f, M), generator=g).numpy().astype(np.float32)
        s = torch.randn((B, f, N), generator=g).numpy().astype(np.float32)
        t[:, :, list(zt)], s[:, :, list(zs)] = 0.0, 0.0
        dt_, ds_ = lay_out(t, s, layout)
        rc, flats, outs = cos_fwd(lib, dt_, ds_, (B, f, M, N))
        assert rc == 0
        sim, tn, sn = check_fwd(GO.cosine_sim(t, s), flats, outs, False, zt, zs)
        r = GO.cosine_sim(t, s, tn=tn, sn=sn)                   # over the stored norms
        compare("cosine_fwd.sim", sim, r.sim, r.sim_bound, False)
        assert not sim[:, :, list(zt)].any() and not sim[:, list(zs), :].any()
        dsim = torch.randn((B, N, M), generator=g).numpy().astype(np.float32)
        dd = dev(dsim)
        rc, flats, (gt, gs) = cos_bwd(lib, dd, outs[0], outs[1], outs[2], dt_, ds_, (B, f, M, N))
        assert rc == 0
        tail_intact(*flats)
        rb = GO.cosine_sim_bwd(dsim, sim, tn, sn, t, s)         # over the fp32 inputs handed to the backward
        compare("cosine_bwd.dt", h(gt), rb.dt, rb.dt_bound, False)
        compare("cosine_bwd.ds", h(gs), rb.ds, rb.ds_bound, False)


def test_cosine_sim_backward_lds_sizes():
    """M = 64 (and 60) with N = 128 takes the backward above 48 KB of dynamic LDS, the opt-in path; the others stay below"""
    lds = lambda M, N: 4 * (N * (M + 1) + 32 * (N + 1) + 32 * (M + 1) + M + N)
    assert {(M, N) for _, M, N in COS_SHAPES if lds(M, N) > 48 * 1024} == {(64, 128), (60, 128)}


def test_cosine_sim_refusals(lib):
    B, f, M, N = 2, 32, 8, 16
    rng = np.random.RandomState(7)
    t, s = dev(rng.randn(B, f, M)), dev(rng.randn(B, f, N))
    for over in (dict(f=33), dict(f=0), dict(M=6), dict(M=68), dict(N=129), dict(N=0), dict(t=None), dict(s=None), dict(sim=None),
                 dict(tn=None), dict(sn=None)):
        rc, flats, _ = cos_fwd(lib, t, s, (B, f, M, N), over)
        assert rc == EINVAL and all(untouched(x) for x in flats), over
    dsim, sim, tn, sn = dev(rng.randn(B, N, M)), dev(rng.randn(B, N, M)), dev(np.ones((B, M))), dev(np.ones((B, N)))
    for over in (dict(f=33), dict(M=68), dict(N=129), dict(M=0), dict(dsim=None), dict(sim=None), dict(tn=None), dict(sn=None),
                 dict(t=None), dict(s=None), dict(dt=None), dict(ds=None)):
        rc, flats, _ = cos_bwd(lib, dsim, sim, tn, sn, t, s, (B, f, M, N), over)
        assert rc == EINVAL and all(untouched(x) for x in flats), over
