"""The index operators at the C ABI, per call -- o3d_furthest_point_sampling / _shfl / _pair (csrc/fps.hip), o3d_ball_query,
o3d_group_points[_grad], o3d_gather_points[_grad], o3d_gather_rows, o3d_three_nn, o3d_three_interpolate[_grad], o3d_knn
(csrc/index_ops.hip) and o3d_boxcloud (csrc/boxcloud.hip) -- with raw pointers, every output prefilled with a sentinel and
followed by a sentinel tail that is checked after every call.
Indices and pure moves are compared for EQUALITY with oracle.ops (floats bit for bit).  Input tails are DECOYS, not NaN: behind a
sampled cloud a point at 1e4 (an over-read makes it the winner), behind a queried cloud copies of the centre / the query (an
over-read is a hit with an index >= N), behind an index indices of the row past the operand.  Only the last cloud has a tail, so
every such case runs with B = 1 and with B = 2, where cloud 1 begins with the decoys of cloud 0.
The arithmetic outputs have two legs against tests/index_oracle.py (fp64; tied to torch by tests/test_index_oracle_cpu.py).
EXACT: the three scatter-adds on multiples of 2^-6 (weights powers of two), at most 4096 terms per destination, one
destination receiving all 4096 and one none (it reads 0, not the sentinel: the zero fill); BoxCloud on signed permutation
matrices with points a Pythagorean quadruple away from each landmark in turn: equality.  ROUNDED: randn / general rotations with
centres up to 2000 m out, |got - ref| <= a bound derived in index_oracle; the worst err / bound per kernel is printed and, when
O3D_INDEX_PINS names a file, written there (profiles/index_kernel_pins.txt is such a run).
No case passes an index outside its range.
"""
import os

import numpy as np
import pytest
import torch

import index_oracle as IO
from test_glue_kernels_gpu import (EINVAL, SENT, TAIL, compare, dev, lib, outbuf, ptr, same_bits, st, tail_intact,  # noqa: F401
                                   untouched)

pytestmark = pytest.mark.gpu

RATIOS = {}
DTAIL = 288                  # floats / ints of a decoy tail: whole rows of 3 and of 9


@pytest.fixture(scope="module", autouse=True)
def _index_pins():
    yield
    path = os.environ.get("O3D_INDEX_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per kernel, rounded legs of tests/test_index_kernels_gpu.py\n"
                    "# bounds: tests/index_oracle.py (u = 2^-24; scatter-adds gamma_n sum|t_i| for any order of the atomics, interpolation\n"
                    "# 3 u sum|f_i w_i|, BoxCloud propagated per operation, valid with and without contraction, sqrtf correctly rounded);\n"
                    "# every ratio must be <= 1.  Every index and every pure move of that file is compared for equality.\n")
            for k in sorted(RATIOS):
                f.write("%-28s %.4f\n" % (k, RATIOS[k]))


def devt(a, tail, dtype=np.float32):
    """device copy of an operand followed by DTAIL elements repeating `tail` -- the decoys a correct kernel never reads"""
    a = np.ascontiguousarray(a, dtype=dtype)
    t = np.resize(np.asarray(tail, dtype=dtype).reshape(-1), DTAIL)
    flat = torch.from_numpy(np.concatenate([a.reshape(-1), t])).cuda()
    return flat[:a.size].view(a.shape)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def batches(x):
    """the B = 1 form (cloud 0 alone in front of the tail) and the whole batch"""
    return (x[:1], x) if x.shape[0] > 1 else (x,)


# ==== furthest point sampling ===========================================================================================================
DECOY_ROW = np.full(3, IO.FPS_DECOY, np.float32)


def fps_fn(lib, variant):
    return lib.o3d_furthest_point_sampling if variant == "dpp" else lib.o3d_furthest_point_sampling_shfl


def run_fps(lib, cloud, npoint):
    """both variants against the oracle; the cloud's tail is the 1e4 decoy"""
    from oracle import ops
    B, N, _ = cloud.shape
    want = ops.furthest_point_sampling(cloud, npoint)
    assert want.min() >= 0 and want.max() < N
    x = devt(cloud, DECOY_ROW)
    for variant in ("dpp", "shfl"):
        flat, idx = outbuf((B, npoint), torch.int32)
        tflat, temp = outbuf((B, N)) if N > 8192 else (None, None)
        assert fps_fn(lib, variant)(ptr(x), B, N, npoint, ptr(temp), ptr(idx), st()) == 0
        same_bits("fps %s B=%d N=%d" % (variant, B, N), host(idx), want)
        tail_intact(flat)
        if tflat is not None:
            tail_intact(tflat)
    return want


@pytest.mark.parametrize("N", IO.FPS_SIZES)
def test_fps_dispatch_edges(lib, N):
    npoint = min(N, 24)
    for kind in IO.FPS_KINDS:
        cloud = IO.lead_with(IO.fps_cloud(kind, 2, N, 1000 + N), DECOY_ROW, 1)
        for c in batches(cloud):
            want = run_fps(lib, c, npoint)
            if kind == "last" and N > 1:
                assert want[0, 1] == N - 1          # the last slot of the last wave won round 1
            if kind == "normal" and N >= 24:
                assert len(set(want[0].tolist())) == npoint


FAR_CASES = ((300, 40), (2049, 24), (8193, 24))


@pytest.mark.parametrize("N,npoint", FAR_CASES)
def test_fps_far_coordinates_are_decided_by_rank(lib, N, npoint):
    cloud = IO.fps_cloud("far", 2, N, 7)
    for c in batches(cloud):
        want = run_fps(lib, c, npoint)
        assert len(set(want[0].tolist())) == npoint
    exact = IO.fps_cloud("fargrid", 2, N, 8)
    for c in batches(exact):
        run_fps(lib, c, npoint)


def test_fps_far_cloud_of_300_begins_as_the_rank_orders(lib):
    """a line of points 4e5 apart: no pair closer than 1e10, every running minimum stays where it started, and the samples
    come in ascending rank (N = 300, bs = 256: 0, 256, 128, 64, 192, 32, 288, 160 by hand)"""
    cloud = (np.arange(300, dtype=np.float64)[None, :, None] * np.array([4.0e5, 0.0, 0.0]) + np.array([0.0, 1.0, 0.0])).astype(np.float32)
    want = run_fps(lib, cloud, 40)
    assert want[0, :8].tolist() == [0, 256, 128, 64, 192, 32, 288, 160]
    assert want[0].tolist() == np.argsort(IO.upstream_rank(300))[:40].tolist()


@pytest.mark.parametrize("N,npoint", [(5, 9), (65, 70)])
def test_fps_more_samples_than_points(lib, N, npoint):
    """after every point is taken all minima are 0: the winner is the lowest rank among the valid points"""
    for kind in ("normal", "grid"):
        for zero_first in (False, True):
            cloud = IO.fps_cloud(kind, 2, N, 50 + N) + np.float32(3.0 if kind == "grid" else 0.0)
            if zero_first:
                cloud[:, 0] = 0.0                    # point 0 inside the near-origin rule: the start, but never a winner
            for c in batches(IO.lead_with(cloud, DECOY_ROW, 1)):
                want = run_fps(lib, c, npoint)
                if kind == "normal":             # (duplicated grid points may be passed over for a taken one of lower rank)
                    assert len(set(want[0, :N].tolist())) == N
                if zero_first:
                    assert (want[0, 1:] != 0).all()


@pytest.mark.parametrize("N", (1, 65, 2049, 8193))
def test_fps_all_points_near_the_origin_gives_zeros(lib, N):
    cloud = (np.random.RandomState(N).rand(2, N, 3) * 0.01).astype(np.float32)
    for c in batches(cloud):
        assert not run_fps(lib, c, min(N, 9)).any()


def test_fps_scratch_is_required_beyond_8192_points(lib):
    cloud = devt(IO.fps_cloud("normal", 1, 8193, 3), DECOY_ROW)
    for variant in ("dpp", "shfl"):
        flat, idx = outbuf((1, 4), torch.int32)
        assert fps_fn(lib, variant)(ptr(cloud), 1, 8193, 4, None, ptr(idx), st()) == EINVAL
        torch.cuda.synchronize()
        assert untouched(flat)


PAIR_SIZES = ((256, 257), (257, 256), (512, 513), (64, 2048), (2048, 1))


@pytest.mark.parametrize("N0,N1", PAIR_SIZES)
def test_fps_pair_entry(lib, N0, N1):
    from oracle import ops
    np0, np1 = min(N0, 24), min(N1, 17)
    for kind in IO.FPS_KINDS:
        a = IO.lead_with(IO.fps_cloud(kind, 2, N0, 300 + N0), DECOY_ROW, 1)
        b = IO.lead_with(IO.fps_cloud(kind, 2, N1, 400 + N1), DECOY_ROW, 1)
        for ca, cb in zip(batches(a), batches(b)):
            B = ca.shape[0]
            wa, wb = ops.furthest_point_sampling(ca, np0), ops.furthest_point_sampling(cb, np1)
            xa, xb = devt(ca, DECOY_ROW), devt(cb, DECOY_ROW)
            fa, ia = outbuf((B, np0), torch.int32)
            fb, ib = outbuf((B, np1), torch.int32)
            assert lib.o3d_furthest_point_sampling_pair(ptr(xa), N0, np0, ptr(ia), ptr(xb), N1, np1, ptr(ib), B, st()) == 0
            same_bits("pair set 0", host(ia), wa)
            same_bits("pair set 1", host(ib), wb)
            tail_intact(fa, fb)
            fs, isingle = outbuf((B, np0), torch.int32)
            assert lib.o3d_furthest_point_sampling(ptr(xa), B, N0, np0, None, ptr(isingle), st()) == 0
            same_bits("pair vs single", host(ia), host(isingle))
            tail_intact(fs)


# ==== ball query =========================================================================================================================
def run_bq(lib, centers, cloud, radius, nsample, null_xyz=False):
    """decoys: behind the last cloud copies of its last centre; the caller leads cloud 1 with cloud 0's"""
    from oracle import ops
    B, N, _ = cloud.shape
    npoint = centers.shape[1]
    want = ops.ball_query(centers, cloud, radius, nsample)
    assert want.min() >= 0 and want.max() < max(N, 1)
    x = None if null_xyz else devt(cloud, centers[-1, -1])
    c = dev(centers)
    flat, idx = outbuf((B, npoint, nsample), torch.int32)
    assert lib.o3d_ball_query(ptr(c), ptr(x), B, N, npoint, float(radius), nsample, ptr(idx), st()) == 0
    same_bits("ball query N=%d nsample=%d r=%g" % (N, nsample, radius), host(idx), want)
    tail_intact(flat)
    return want


BQ_NSAMPLE = (1, 63, 64, 65, 129)
BQ_N = (0, 1, 63, 64, 65, 130)


@pytest.mark.parametrize("nsample", BQ_NSAMPLE)
def test_ball_query_sizes(lib, nsample):
    """half-integer coordinates in [-1, 1]: duplicated points and d2 == r2 = 1 throughout; radius 10 takes every point"""
    for N in BQ_N:
        rng = np.random.RandomState(10 * N + nsample)
        cloud = (rng.randint(-2, 3, size=(2, N, 3)) * 0.5).astype(np.float32)
        centers = (rng.randint(-2, 3, size=(2, 5, 3)) * 0.5).astype(np.float32)
        cloud = IO.lead_with(cloud, centers[:-1, -1], 3)
        for radius in (1.0, 10.0):
            for c, x in zip(batches(centers), batches(cloud)):
                want = run_bq(lib, c, x, radius, nsample)
                if radius == 10.0 and N > 0:
                    assert (want[..., :min(N, nsample)] == np.arange(min(N, nsample))).all()


def marked_cloud(N, hits, B=1):
    """the origin at the indices `hits`, (9, 9, 9) elsewhere"""
    cloud = np.full((B, N, 3), 9.0, np.float32)
    cloud[:, list(hits)] = 0.0
    return cloud


def test_ball_query_ballots_and_early_stop(lib):
    zero = np.zeros((1, 1, 3), np.float32)
    # exactly nsample hits inside the first ballot, decoy hits behind the stop in both later ballots
    assert run_bq(lib, zero, marked_cloud(130, (3, 10, 20, 40, 70, 129)), 0.5, 4)[0, 0].tolist() == [3, 10, 20, 40]
    # nsample reached in the second ballot, one more hit in it and one in the third
    assert run_bq(lib, zero, marked_cloud(130, (5, 60, 64, 100, 101, 129)), 0.5, 4)[0, 0].tolist() == [5, 60, 64, 100]
    # the 64th hit is the last lane of the first ballot; 65 asks the second ballot for one more
    assert run_bq(lib, zero, marked_cloud(130, range(0, 130)), 0.5, 64)[0, 0].tolist() == list(range(64))
    assert run_bq(lib, zero, marked_cloud(130, range(0, 130)), 0.5, 65)[0, 0].tolist() == list(range(65))
    # fewer hits than nsample across three ballots: padded with the first hit, over two rounds of the pad loop
    got = run_bq(lib, zero, marked_cloud(130, (7, 64, 129)), 0.5, 129)[0, 0]
    assert got[:3].tolist() == [7, 64, 129] and (got[3:] == 7).all()
    # an empty ball, and B = 2 with the decoys of cloud 0 at the head of cloud 1
    assert not run_bq(lib, zero, marked_cloud(130, ()), 0.5, 65).any()
    two = marked_cloud(65, (64,), B=2)
    two[1, :3] = 0.0
    got = run_bq(lib, np.zeros((2, 2, 3), np.float32), two, 0.5, 3)
    assert got[0].tolist() == [[64, 64, 64]] * 2 and got[1].tolist() == [[0, 1, 2]] * 2


def test_ball_query_radius_is_strict_and_empty_cloud(lib):
    cloud = np.array([[[0.5, 0, 0], [0, 0.5, 0], [0.25, 0, 0], [0, 0, 0.5]]], np.float32)
    zero = np.zeros((1, 1, 3), np.float32)
    assert run_bq(lib, zero, cloud, 0.5, 3)[0, 0].tolist() == [2, 2, 2]              # d2 == r2 is outside
    assert run_bq(lib, zero, cloud, 0.25, 3)[0, 0].tolist() == [0, 0, 0]             # d2 == r2 again: empty
    assert not run_bq(lib, np.zeros((2, 3, 3), np.float32), np.zeros((2, 0, 3), np.float32), 1.0, 5, null_xyz=True).any()


# ==== group / gather / gather_rows =========================================================================================================
MOVE_C = (1, 15, 16, 17, 33)
MOVE_Q = (1, 255, 256, 257)
MOVE_SPLIT = {1: (1, 1), 255: (15, 17), 256: (16, 16), 257: (1, 257)}
ROWS_D = (1, 3, 9)


def move_idx(rng, B, Q, N):
    idx = rng.randint(0, N, size=(B, Q)).astype(np.int32)
    idx[:, 0] = N - 1
    idx[:, -1] = idx[:, 0]                           # a duplicate, and the last index of the range
    if Q > 2:
        idx[:, 1] = idx[:, 2]
    return idx


@pytest.mark.parametrize("C", MOVE_C)
def test_group_and_gather_points(lib, C):
    from oracle import ops
    N = 7
    for Q in MOVE_Q:
        rng = np.random.RandomState(C * 1000 + Q)
        feats, idx = rng.randn(2, C, N).astype(np.float32), move_idx(rng, 2, Q, N)
        npoint, nsample = MOVE_SPLIT[Q]
        for f, i in zip(batches(feats), batches(idx)):
            B = f.shape[0]
            fd, idd = dev(f), devt(i, [N], np.int32)        # feats: NaN tail; idx: the row past the operand
            flat, out = outbuf((B, C, npoint, nsample))
            assert lib.o3d_group_points(ptr(fd), ptr(idd), B, C, N, npoint, nsample, ptr(out), st()) == 0
            same_bits("group C=%d Q=%d" % (C, Q), host(out), ops.group_points(f, i.reshape(B, npoint, nsample)))
            tail_intact(flat)
            flat, out = outbuf((B, C, Q))
            assert lib.o3d_gather_points(ptr(fd), ptr(idd), B, C, N, Q, ptr(out), st()) == 0
            same_bits("gather C=%d Q=%d" % (C, Q), host(out), ops.gather_points(f, i))
            tail_intact(flat)


@pytest.mark.parametrize("D", ROWS_D)
def test_gather_rows(lib, D):
    N = 7
    for Q in MOVE_Q:
        rng = np.random.RandomState(D * 1000 + Q)
        src, idx = rng.randn(2, N, D).astype(np.float32), move_idx(rng, 2, Q, N)
        for s, i in zip(batches(src), batches(idx)):
            B = s.shape[0]
            flat, out = outbuf((B, Q, D))
            assert lib.o3d_gather_rows(ptr(dev(s)), ptr(devt(i, [N], np.int32)), B, N, D, Q, ptr(out), st()) == 0
            same_bits("gather_rows D=%d Q=%d" % (D, Q), host(out), np.stack([s[b][i[b]] for b in range(B)]))
            tail_intact(flat)


def test_group_and_gather_at_the_grid_limit(lib):
    """B = 65535 clouds of one element each on grid.z; 65536 is refused"""
    B = 65535
    feats = np.arange(B, dtype=np.float32).reshape(B, 1, 1)
    fd, idd = dev(feats), devt(np.zeros((B, 1), np.int32), [1], np.int32)
    for call in (lambda o, b: lib.o3d_group_points(ptr(fd), ptr(idd), b, 1, 1, 1, 1, ptr(o), st()),
                 lambda o, b: lib.o3d_gather_points(ptr(fd), ptr(idd), b, 1, 1, 1, ptr(o), st())):
        flat, out = outbuf((B, 1, 1))
        assert call(out, B) == 0
        same_bits("B = 65535", host(out), feats)
        tail_intact(flat)
        flat, out = outbuf((B, 1, 1))
        assert call(out, B + 1) == EINVAL
        torch.cuda.synchronize()
        assert untouched(flat)


# ==== the three scatter-adds ==================================================================================================================
def run_group_grad(lib, g, idx, N, exact, gather=False):
    B, C = g.shape[:2]
    s = IO.group_points_grad(g, idx, N)
    gd, idd = dev(g), devt(idx, [N], np.int32)
    flat, out = outbuf((B, C, N))
    if gather:
        rc = lib.o3d_gather_points_grad(ptr(gd), ptr(idd), B, C, N, idx.shape[1], ptr(out), st())
    else:
        rc = lib.o3d_group_points_grad(ptr(gd), ptr(idd), B, C, N, idx.shape[1], idx.shape[2], ptr(out), st())
    assert rc == 0
    got = host(out)
    tail_intact(flat)
    assert (got[s.cnt == 0] == 0).all()              # a destination nothing lands on reads the zero fill, not the sentinel
    compare("gather_points_grad" if gather else "group_points_grad", got, s.ref, s.bound, exact, ratios=RATIOS)
    return s


def exact_scatter_inputs():
    """-> (group / gather (g (B, C, Q), idx (B, Q), N), interpolation (g, idx, w, m)); shared with the CPU file"""
    rng = np.random.RandomState(21)
    B, C, N, Q = 2, 17, 5, IO.EXACT_TERMS
    idx = IO.exact_scatter_idx(rng, B, Q, N, skip=4)
    g = IO.dyadic(rng, (B, C, Q))
    return (g, idx, N), IO.exact_interp_inputs(rng, B, 17, IO.EXACT_TERMS, 9) + (9,)


def test_scatter_adds_exact(lib):
    (g, idx, N), (gi, ii3, wi, m) = exact_scatter_inputs()
    C, Q, n = g.shape[1], g.shape[2], gi.shape[2]
    for gg, ii in zip(batches(g), batches(idx)):
        b = gg.shape[0]
        s = run_group_grad(lib, gg.reshape(b, C, 64, 64), ii.reshape(b, 64, 64), N, True)
        IO.assert_exact_scatter(s, 2.0 ** -6)
        assert s.cnt.max() == Q and s.cnt.min() == 0
        run_group_grad(lib, gg, ii, N, True, gather=True)
    for gg, ii, ww in zip(batches(gi), batches(ii3), batches(wi)):
        s = run_interp_grad(lib, gg, ii, ww, m, True)
        IO.assert_exact_scatter(s, 2.0 ** -8)
        assert s.cnt.max() == n and s.cnt.min() == 0


def run_interp_grad(lib, g, idx, w, m, exact):
    B, c, n = g.shape
    s = IO.three_interpolate_grad(g, idx, w, m)
    flat, out = outbuf((B, c, m))
    assert lib.o3d_three_interpolate_grad(ptr(dev(g)), ptr(devt(idx, [m], np.int32)), ptr(dev(w)), B, c, n, m, ptr(out), st()) == 0
    got = host(out)
    tail_intact(flat)
    assert (got[s.cnt == 0] == 0).all()
    compare("three_interpolate_grad", got, s.ref, s.bound, exact, ratios=RATIOS)
    return s


def rounded_scatter_inputs():
    """-> (group (g, idx, N), gather (g, idx, N), interpolation (g, idx, w, m)); shared with the CPU file"""
    rng = np.random.RandomState(22)
    grp = (rng.randn(2, 17, 33, 9).astype(np.float32), rng.randint(0, 40, size=(2, 33, 9)).astype(np.int32), 41)
    gat = (rng.randn(2, 5, 300).astype(np.float32), rng.randint(0, 30, size=(2, 300)).astype(np.int32), 31)
    w = rng.rand(2, 300, 3)
    itp = (rng.randn(2, 17, 300).astype(np.float32), rng.randint(0, 20, size=(2, 300, 3)).astype(np.int32),
           (w / w.sum(-1, keepdims=True)).astype(np.float32), 21)
    return grp, gat, itp


def test_scatter_adds_rounded(lib):
    grp, gat, itp = rounded_scatter_inputs()
    for b in (slice(1, 2), slice(0, 2)):
        run_group_grad(lib, grp[0][b], grp[1][b], grp[2], False)
        run_group_grad(lib, gat[0][b], gat[1][b], gat[2], False, gather=True)
        run_interp_grad(lib, itp[0][b], itp[1][b], itp[2][b], itp[3], False)


# ==== 3-NN and the interpolation ==============================================================================================================
NN_M = (0, 1, 2, 3, 257)
NN_N = (1, 256, 257)


@pytest.mark.parametrize("m", NN_M)
def test_three_nn(lib, m):
    from oracle import ops
    for n in NN_N:
        for kind in ("grid", "normal"):
            rng = np.random.RandomState(100 * m + n)
            draw = (lambda s: rng.randint(-3, 4, size=s) * 0.5) if kind == "grid" else (lambda s: rng.randn(*s))
            unknown, known = draw((2, n, 3)).astype(np.float32), draw((2, m, 3)).astype(np.float32)
            known = IO.lead_with(known, unknown[:-1, 0], 3)
            for u, k in zip(batches(unknown), batches(known)):
                B = u.shape[0]
                wd, wi = ops.three_nn(u, k)
                assert wi.min() >= 0 and wi.max() < max(m, 1)
                if m < 3:
                    assert np.isinf(wd[..., m:]).all() and not wi[..., m:].any()
                fd, dist = outbuf((B, n, 3))
                fi, idx = outbuf((B, n, 3), torch.int32)
                assert lib.o3d_three_nn(ptr(dev(u)), ptr(devt(k, u[-1, 0])), B, n, m, ptr(dist), ptr(idx), st()) == 0
                same_bits("three_nn idx m=%d n=%d" % (m, n), host(idx), wi)
                same_bits("three_nn dist2 m=%d n=%d" % (m, n), host(dist), wd)
                tail_intact(fd, fi)


def interp_inputs(c, m, n, seed):
    rng = np.random.RandomState(seed)
    w = rng.rand(2, n, 3)
    idx = rng.randint(0, m, size=(2, n, 3)).astype(np.int32)
    idx[:, 0] = m - 1
    return rng.randn(2, c, m).astype(np.float32), idx, (w / w.sum(-1, keepdims=True)).astype(np.float32)


INTERP_SHAPES = [(c, m, n) for c in (1, 17, 33) for m in (1, 3, 20) for n in (1, 256, 257)]


def test_three_interpolate(lib):
    from oracle import ops
    for c, m, n in INTERP_SHAPES:
        feats, idx, w = interp_inputs(c, m, n, c * 100 + m * 10 + n)
        for f, i, ww in zip(batches(feats), batches(idx), batches(w)):
            B = f.shape[0]
            flat, out = outbuf((B, c, n))
            assert lib.o3d_three_interpolate(ptr(dev(f)), ptr(devt(i, [m], np.int32)), ptr(dev(ww)), B, c, m, n, ptr(out), st()) == 0
            got = host(out)
            tail_intact(flat)
            same_bits("three_interpolate c=%d m=%d n=%d" % (c, m, n), got, ops.three_interpolate(f, i, ww))
            ref, bound = IO.three_interpolate(f, i, ww)
            compare("three_interpolate", got, ref, bound, False, ratios=RATIOS)


# ==== kNN ================================================================================================================================
KNN_CASES = ([(9, k, R) for k in (1, 2, 3, 4) for R in (1365, 1366)] + [(9, 5, 20), (9, 4, 4), (9, 4, 64), (9, 4, 65)] +
             [(3, k, 40) for k in (7, 8, 9, 16, 17, 31, 32)] + [(3, 32, 32), (0, 3, 5), (1, 2, 7), (1, 1, 1)])
KNN_Q = (1, 128, 129)


def half_integers(rng, shape):
    return (np.round(rng.randn(*shape) * 2) / 2).astype(np.float32)


def run_knn(lib, q, r, k):
    from oracle import ops
    B, Q, D = q.shape
    R = r.shape[1]
    want = ops.knn(q, r, k)
    assert want.min() >= 0 and want.max() < R
    flat, idx = outbuf((B, Q, k), torch.int32)
    tail = q[-1, 0] if D > 0 else [0.0]
    assert lib.o3d_knn(ptr(devt(q, [9.0e3])), ptr(devt(r, tail)), B, Q, R, D, k, ptr(idx), st()) == 0
    got = host(idx)
    same_bits("knn D=%d k=%d R=%d Q=%d B=%d" % (D, k, R, Q, B), got, want)
    tail_intact(flat)
    return got


@pytest.mark.parametrize("D,k,R", KNN_CASES)
def test_knn(lib, D, k, R):
    for Q in KNN_Q:
        rng = np.random.RandomState(D * 7 + k * 131 + R + Q)
        q, r = half_integers(rng, (2, Q, D)), half_integers(rng, (2, R, D))
        if D > 0:
            r = IO.lead_with(r, q[:-1, 0], 3)
        for qq, rr in zip(batches(q), batches(r)):
            got = run_knn(lib, qq, rr, k)
            if D == 0:
                assert (got == np.arange(k)).all()


def test_knn_matches_across_the_lds_edge(lib):
    """the same 1365 references through the LDS-staged kernel, and with a 1366th far row through the generic one"""
    rng = np.random.RandomState(5)
    q, r = half_integers(rng, (2, 129, 9)), half_integers(rng, (2, 1365, 9))
    far = np.concatenate([r, np.full((2, 1, 9), 100.0, np.float32)], axis=1)
    for k in (1, 4):
        same_bits("knn across the LDS edge", run_knn(lib, q, far, k), run_knn(lib, q, r, k))


# ==== BoxCloud ===========================================================================================================================
def run_boxcloud(lib, case):
    p, c, s, R = case["points"], case["center"], case["wlh"], case["rot"]
    B, N, _ = p.shape
    flat, out = outbuf((B, N, 9))
    assert lib.o3d_boxcloud(ptr(dev(p)), ptr(dev(c)), ptr(dev(s)), ptr(dev(R)), float(case["factor"]), B, N, ptr(out), st()) == 0
    got = host(out)
    tail_intact(flat)
    return got


@pytest.mark.parametrize("case", range(3))
def test_boxcloud_exact(lib, case):
    c = IO.exact_boxcloud_case(case)
    got = run_boxcloud(lib, c)
    pinned = np.take_along_axis(got, c["chan"][None, :, None].repeat(got.shape[0], 0), axis=2)[..., 0]
    compare("boxcloud", pinned, c["want"], None, True)
    ref = IO.boxcloud(c["points"], c["center"], c["wlh"], c["rot"], c["factor"])
    compare("boxcloud (exact inputs)", got, ref, IO.boxcloud_bound(c["points"], c["center"], c["wlh"], c["rot"], c["factor"]),
            False, ratios={})


BOX_N = (1, 255, 256, 257)


@pytest.mark.parametrize("N", BOX_N)
def test_boxcloud_rounded(lib, N):
    for B, seed in ((3, N), (1, N + 1)):
        c = IO.rounded_boxcloud_case(B, N, seed)
        got = run_boxcloud(lib, c)
        ref = IO.boxcloud(c["points"], c["center"], c["wlh"], c["rot"], c["factor"])
        compare("boxcloud", got, ref, IO.boxcloud_bound(c["points"], c["center"], c["wlh"], c["rot"], c["factor"]), False,
                ratios=RATIOS)


# ==== refusals ===========================================================================================================================
# entry -> (arguments in order, the sizes of a call that would be accepted, outputs, one override per clause of the entry's `if`);
# every argument without a size is a pointer.  Shared with the CPU file, which runs the table on host memory: a refusal comes
# before anything touches the device.
_NEG5 = [dict(B=-1), dict(C=-1), dict(N=-1), dict(npoint=-1), dict(B=65536)]
REFUSALS = {
    "o3d_furthest_point_sampling": (("xyz", "B", "N", "npoint", "temp", "idx"), dict(B=1, N=8, npoint=2, temp=None), ("idx",),
                                    [dict(B=-1), dict(N=0), dict(npoint=-1), dict(xyz=None), dict(idx=None), dict(N=8193)]),
    "o3d_furthest_point_sampling_shfl": (("xyz", "B", "N", "npoint", "temp", "idx"), dict(B=1, N=8, npoint=2, temp=None), ("idx",),
                                         [dict(B=-1), dict(N=0), dict(npoint=-1), dict(xyz=None), dict(idx=None), dict(N=8193)]),
    "o3d_furthest_point_sampling_pair": (("xyz0", "N0", "npoint0", "idx0", "xyz1", "N1", "npoint1", "idx1", "B"),
                                         dict(N0=8, npoint0=2, N1=8, npoint1=2, B=1), ("idx0", "idx1"),
                                         [dict(B=0), dict(N0=0), dict(N1=0), dict(npoint0=0), dict(npoint1=0), dict(N0=2049),
                                          dict(N1=2049), dict(xyz0=None), dict(xyz1=None), dict(idx0=None), dict(idx1=None)]),
    "o3d_ball_query": (("new_xyz", "xyz", "B", "N", "npoint", "radius", "nsample", "idx"),
                       dict(B=1, N=4, npoint=2, radius=1.0, nsample=3), ("idx",),
                       [dict(B=-1), dict(N=-1), dict(npoint=-1), dict(nsample=-1), dict(new_xyz=None), dict(idx=None), dict(xyz=None)]),
    "o3d_group_points": (("feats", "idx", "B", "C", "N", "npoint", "nsample", "out"), dict(B=1, C=2, N=4, npoint=3, nsample=2),
                         ("out",), _NEG5 + [dict(nsample=-1), dict(feats=None), dict(idx=None), dict(out=None), dict(N=0),
                                            dict(npoint=65536, nsample=32768)]),
    "o3d_group_points_grad": (("grad_out", "idx", "B", "C", "N", "npoint", "nsample", "grad_feats"),
                              dict(B=1, C=2, N=4, npoint=3, nsample=2), ("grad_feats",),
                              _NEG5 + [dict(nsample=-1), dict(grad_feats=None), dict(grad_out=None), dict(idx=None),
                                       dict(npoint=65536, nsample=32768)]),
    "o3d_gather_points": (("feats", "idx", "B", "C", "N", "npoint", "out"), dict(B=1, C=2, N=4, npoint=3), ("out",),
                          _NEG5 + [dict(feats=None), dict(idx=None), dict(out=None), dict(N=0)]),
    "o3d_gather_points_grad": (("grad_out", "idx", "B", "C", "N", "npoint", "grad_feats"), dict(B=1, C=2, N=4, npoint=3),
                               ("grad_feats",), _NEG5 + [dict(grad_feats=None), dict(grad_out=None), dict(idx=None)]),
    "o3d_gather_rows": (("src", "idx", "B", "N", "D", "npoint", "out"), dict(B=1, N=4, D=3, npoint=3), ("out",),
                        [dict(B=-1), dict(N=-1), dict(D=0), dict(npoint=-1), dict(src=None), dict(idx=None), dict(out=None), dict(N=0)]),
    "o3d_three_nn": (("unknown", "known", "B", "n", "m", "dist2", "idx"), dict(B=1, n=3, m=4), ("dist2", "idx"),
                     [dict(B=-1), dict(n=-1), dict(m=-1), dict(B=65536), dict(unknown=None), dict(dist2=None), dict(idx=None),
                      dict(known=None)]),
    "o3d_three_interpolate": (("feats", "idx", "weight", "B", "c", "m", "n", "out"), dict(B=1, c=2, m=4, n=3), ("out",),
                              [dict(B=-1), dict(c=-1), dict(m=-1), dict(n=-1), dict(B=65536), dict(feats=None), dict(idx=None),
                               dict(weight=None), dict(out=None), dict(m=0)]),
    "o3d_three_interpolate_grad": (("grad_out", "idx", "weight", "B", "c", "n", "m", "grad_feats"), dict(B=1, c=2, n=3, m=4),
                                   ("grad_feats",),
                                   [dict(B=-1), dict(c=-1), dict(m=-1), dict(n=-1), dict(B=65536), dict(grad_feats=None),
                                    dict(grad_out=None), dict(idx=None), dict(weight=None)]),
    "o3d_knn": (("query", "ref", "B", "Q", "R", "D", "k", "idx"), dict(B=1, Q=2, R=5, D=3, k=2), ("idx",),
                [dict(B=-1), dict(Q=-1), dict(R=-1), dict(D=-1), dict(k=0), dict(k=33), dict(k=6), dict(B=65536), dict(idx=None),
                 dict(query=None), dict(ref=None)]),
    "o3d_boxcloud": (("points", "center", "wlh", "rot", "wlh_factor", "B", "N", "out"), dict(wlh_factor=1.0, B=1, N=4), ("out",),
                     [dict(B=-1), dict(N=-1), dict(B=65536), dict(points=None), dict(center=None), dict(wlh=None), dict(rot=None),
                      dict(out=None)]),
}


def refused_everywhere(lib, entry, in_ptr, new_out, is_untouched, stream):
    """every override of REFUSALS[entry] returns O3D_EINVAL with every output untouched.  in_ptr: address of a readable buffer;
    new_out() -> (handle, address) of a sentinel-filled output; is_untouched(handle)"""
    names, sizes, outputs, overrides = REFUSALS[entry]
    for over in overrides:
        outs = {o: new_out() for o in outputs}
        a = {n: (sizes[n] if n in sizes else (outs[n][1] if n in outs else in_ptr)) for n in names}
        assert all(k in a for k in over), (entry, over)
        a.update(over)
        rc = getattr(lib, entry)(*([a[n] for n in names] + [stream]))
        assert rc == EINVAL, (entry, over, rc)
        for o in outputs:
            assert is_untouched(outs[o][0]), (entry, over, o)


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_refusals_leave_every_output_untouched(lib, entry):
    src = torch.zeros(4096, dtype=torch.float32, device="cuda")

    def new_out():
        flat, _ = outbuf((64,))
        return flat, flat.data_ptr()

    def is_untouched(flat):
        torch.cuda.synchronize()
        return untouched(flat)

    refused_everywhere(lib, entry, src.data_ptr(), new_out, is_untouched, st())
