"""tests/index_oracle.py against the operators it restates, and tests/test_index_kernels_gpu.py against itself:
  * the three scatter-adds tied, to 1e-12, to index_add_ / gather under autograd in fp64, the interpolation to gather + sum,
    BoxCloud to the reference's get_point_to_box_distance (tests/golden/ref_boxcloud.npz);
  * the plain-numpy FPS / ball query / kNN (tie rules as parameters) equal to oracle.ops on the exact inputs they are used on;
  * every exactness precondition of the GPU file, the Pythagorean placements included, and its case tables as a checklist;
  * the far-coordinate clouds really have more than 90 % of their pairs above 1e10;
  * every formula evaluated in float32 on the GPU file's own rounded-leg inputs lies inside its bound;
  * the refusal table of the GPU file on host memory: a refusal comes before anything touches the device;
  * sensitivity: plausible mistakes applied to the references are rejected by the GPU file's comparisons.
No GPU."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import index_oracle as IO
import test_index_kernels_gpu as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def rejected(name, got, ref, bound, exact):
    with pytest.raises(AssertionError):
        K.compare(name, got, ref, bound, exact, ratios={})
    return True


def differs(what, got, ref):
    with pytest.raises(AssertionError):
        K.same_bits(what, got, ref)
    return True


# ---- the fp64 helpers against torch --------------------------------------------------------------------------------------------
def test_scatter_adds_vs_torch_autograd():
    grp, gat, itp = K.rounded_scatter_inputs()
    for g, idx, N in (grp, gat):
        B, C = g.shape[:2]
        feats = torch.zeros(B, C, N, dtype=torch.float64, requires_grad=True)
        ii = torch.from_numpy(idx.reshape(B, 1, -1).astype(np.int64)).expand(B, C, -1)
        out = torch.gather(feats, 2, ii)                                    # the forward: out[b, c, q] = feats[b, c, idx[b, q]]
        out.backward(torch.from_numpy(g.reshape(B, C, -1).astype(np.float64)))
        s = IO.group_points_grad(g, idx, N)
        assert rel(s.ref, feats.grad.numpy()) <= 1e-12
        acc = torch.zeros(C, N, dtype=torch.float64)
        acc.index_add_(1, torch.from_numpy(idx[0].reshape(-1).astype(np.int64)), torch.from_numpy(g[0].reshape(C, -1).astype(np.float64)))
        assert rel(s.ref[0], acc.numpy()) <= 1e-12
        assert s.cnt.sum() == B * C * idx[0].size and (s.abs >= np.abs(s.ref) - 1e-12).all()
    g, idx, w, m = itp
    B, c, n = g.shape
    feats = torch.randn(B, c, m, dtype=torch.float64, requires_grad=True)
    ii = torch.from_numpy(idx.astype(np.int64))
    out = sum(torch.gather(feats, 2, ii[:, None, :, t].expand(B, c, n)) * torch.from_numpy(w.astype(np.float64))[:, None, :, t]
              for t in range(3))
    out.backward(torch.from_numpy(g.astype(np.float64)))
    s = IO.three_interpolate_grad(g, idx, w, m)
    assert rel(s.ref, feats.grad.numpy()) <= 1e-12
    fwd, bound = IO.three_interpolate(feats.detach().numpy().astype(np.float32), idx, w)
    want = sum(torch.gather(feats.detach().float().double(), 2, ii[:, None, :, t].expand(B, c, n)) *
               torch.from_numpy(w.astype(np.float64))[:, None, :, t] for t in range(3))
    assert rel(fwd, want.numpy()) <= 1e-12 and (bound > 0).all()


@pytest.mark.parametrize("i", range(4))
def test_boxcloud_vs_the_references_fixture(i):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ref_boxcloud.npz"))
    c, s, r, f = gold["center_%d" % i], gold["wlh_%d" % i], gold["rot_%d" % i], float(gold["factor_%d" % i])
    p = gold["points_%d" % i]
    got = IO.boxcloud(p[None], c[None], s[None], r[None], f)[0]
    assert float(np.float32(f)) == f and rel(got, gold["bc_%d" % i]) <= 1e-12
    assert rel(IO.landmarks(c[None], s[None], r[None], f)[0, 1:].T, gold["corners_%d" % i]) <= 1e-12


# ---- the plain-numpy operators against oracle.ops ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 2, 65, 129, 300, 513))
def test_fps_numpy_is_the_oracle_on_exact_clouds(N):
    from oracle import ops
    for kind in ("grid", "fargrid"):
        cloud = IO.fps_cloud(kind, 2, N, 11 + N)
        npoint = min(N, 24) + (3 if N < 10 else 0)
        assert np.array_equal(IO.fps_numpy(cloud, npoint), ops.furthest_point_sampling(cloud, npoint))


def test_ball_query_and_knn_numpy_are_the_oracle_on_half_integers():
    from oracle import ops
    rng = np.random.RandomState(3)
    cloud = (rng.randint(-2, 3, size=(2, 130, 3)) * 0.5).astype(np.float32)
    centers = (rng.randint(-2, 3, size=(2, 5, 3)) * 0.5).astype(np.float32)
    for ns in (1, 64, 129):
        assert np.array_equal(IO.ball_query_numpy(centers, cloud, 1.0, ns), ops.ball_query(centers, cloud, 1.0, ns))
    q, r = K.half_integers(rng, (2, 9, 9)), K.half_integers(rng, (2, 70, 9))
    for k in (1, 4, 17):
        assert np.array_equal(IO.knn_numpy(q, r, k), ops.knn(q, r, k))


# ---- exactness preconditions and case tables ----------------------------------------------------------------------------------------
def test_exact_scatter_inputs_keep_every_partial_sum_representable():
    (g, idx, N), (gi, ii, wi, m) = K.exact_scatter_inputs()
    assert np.array_equal(g * 64, np.round(g * 64)) and np.abs(g).max() <= 4
    s = IO.group_points_grad(g, idx, N)
    assert IO.assert_exact_scatter(s, 2.0 ** -6) < 2.0 ** 24
    assert s.cnt[0, 0].tolist() == [0, 0, IO.EXACT_TERMS, 0, 0] and (s.cnt[1, :, 4] == 0).all() and s.cnt[1].max() <= IO.EXACT_TERMS
    assert set(np.unique(wi).tolist()) <= {0.25, 0.5, 1.0}
    s = IO.three_interpolate_grad(gi, ii, wi, m)
    assert IO.assert_exact_scatter(s, 2.0 ** -8) < 2.0 ** 24
    assert s.cnt[0, 0, 2] == IO.EXACT_TERMS and not s.cnt[0, :, 7:].any() and not s.cnt[1, :, m - 1].any()
    # 4096 terms in two orders, in float32: the same bits
    t = (gi[0, 0].astype(np.float64) * wi[0, :, 0]).astype(np.float32)
    fwd, bwd = np.float32(0), np.float32(0)
    for v in t:
        fwd = np.float32(fwd + v)
    for v in t[::-1]:
        bwd = np.float32(bwd + v)
    assert fwd == bwd == np.float32(s.ref[0, 0, 2])


def test_exact_boxcloud_placements():
    seen = set()
    for case in range(3):
        c = IO.exact_boxcloud_case(case)
        R = c["rot"]
        for b in range(len(R)):
            assert np.array_equal(np.abs(R[b]).sum(0), np.ones(3)) and np.array_equal(np.abs(R[b]).sum(1), np.ones(3))
            assert abs(round(float(np.linalg.det(R[b].astype(np.float64))))) == 1
            seen.add(tuple(int(np.argmax(np.abs(R[b][i]))) for i in range(3)))
        assert float(np.log2(c["factor"])).is_integer()
        assert np.array_equal(c["center"] * 16, np.round(c["center"] * 16)) and np.array_equal(c["wlh"] * 8, np.round(c["wlh"] * 8))
        assert set(c["chan"].tolist()) == set(range(9))
        lm = IO.landmarks(c["center"], c["wlh"], c["rot"], c["factor"])
        d = c["points"].astype(np.float64) - lm[:, c["chan"], :]                               # (B, N, 3)
        q = np.sort(np.abs(d), axis=-1)
        q = q / (q[..., :1])                                                                   # smallest component -> 1, 2 or 4
        fams = {tuple(sorted(v)) for v in (np.array(x[:3], float) / x[0] for x in IO.QUADS)}
        assert {tuple(v) for v in q.reshape(-1, 3).tolist()} == fams
        assert np.array_equal(np.sqrt((d * d).sum(-1)), c["want"])
        ref = IO.boxcloud(c["points"], c["center"], c["wlh"], c["rot"], c["factor"])
        pinned = np.take_along_axis(ref, c["chan"][None, :, None].repeat(len(R), 0), axis=2)[..., 0]
        assert np.array_equal(pinned, c["want"])
        f32 = IO.boxcloud_f32(c["points"], c["center"], c["wlh"], c["rot"], c["factor"])
        K.compare("boxcloud", np.take_along_axis(f32, c["chan"][None, :, None].repeat(len(R), 0), axis=2)[..., 0], c["want"], None, True)
        # two corners exchanged / a sign flipped breaks the equality outright
        sw = ref[..., [0, 2, 1, 3, 4, 5, 6, 7, 8]]
        assert rejected("boxcloud", np.take_along_axis(sw, c["chan"][None, :, None].repeat(len(R), 0), axis=2)[..., 0], c["want"], None, True)
    assert seen == set(IO.AXIS_ORDERS)


def test_no_point_is_a_quadruple_away_from_all_nine_landmarks():
    """why the exact leg pins one landmark per point: integer half-sizes up to 6, offsets up to 16 (the full search went to 12 / 28)"""
    Rr, H = 16, 6
    M = Rr + H
    ax = np.arange(-M, M + 1)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    S = X * X + Y * Y + Z * Z
    rt = np.round(np.sqrt(S)).astype(np.int64)
    isq = (rt * rt == S) & (X != 0) & (Y != 0) & (Z != 0)
    n = 2 * Rr + 1
    for hx, hy, hz in itertools.product(range(1, H + 1), repeat=3):
        ok = isq[H:H + n, H:H + n, H:H + n].copy()
        for sx, sy, sz in itertools.product((1, -1), repeat=3):
            ok &= isq[H - sx * hx:H - sx * hx + n, H - sy * hy:H - sy * hy + n, H - sz * hz:H - sz * hz + n]
        assert not ok.any()


def test_far_clouds_have_most_pairs_above_1e10():
    for N, npoint in K.FAR_CASES:
        for kind in ("far", "fargrid"):
            cloud = IO.fps_cloud(kind, 2, N, 7 if kind == "far" else 8)
            frac = IO.far_fraction(cloud[0, :600])
            assert frac > 0.9, (kind, N, frac)
    line = np.arange(300)[:, None] * np.array([4.0e5, 0, 0]) + np.array([0, 1.0, 0])
    assert IO.far_fraction(line.astype(np.float32)) == 1.0
    from oracle import ops
    got = ops.furthest_point_sampling(IO.fps_cloud("far", 1, 300, 7), 40)
    assert len(set(got[0].tolist())) == 40 and got[0, :3].tolist() == [0, 256, 128]


def test_case_tables_promise_what_the_issue_lists():
    assert IO.FPS_SIZES == (1, 2, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)
    assert set(IO.FPS_KINDS) == {"normal", "grid", "last"} and [n for n, _ in K.FAR_CASES] == [300, 2049, 8193]
    assert K.PAIR_SIZES == ((256, 257), (257, 256), (512, 513), (64, 2048), (2048, 1))
    assert K.BQ_NSAMPLE == (1, 63, 64, 65, 129) and K.BQ_N == (0, 1, 63, 64, 65, 130)
    assert K.MOVE_C == (1, 15, 16, 17, 33) and K.MOVE_Q == (1, 255, 256, 257) and K.ROWS_D == (1, 3, 9)
    assert all(a * b == q for q, (a, b) in K.MOVE_SPLIT.items())
    assert K.NN_M == (0, 1, 2, 3, 257) and K.NN_N == (1, 256, 257) and K.KNN_Q == (1, 128, 129) and K.BOX_N == (1, 255, 256, 257)
    cases = set(K.KNN_CASES)
    assert {(9, k, R) for k in (1, 2, 3, 4) for R in (1365, 1366)} <= cases and {(9, 4, 64), (9, 4, 65), (9, 4, 4)} <= cases
    assert {k for D, k, _ in cases if D == 3} >= {7, 8, 9, 16, 17, 31, 32} and any(D == 9 and k == 5 for D, k, _ in cases)
    assert {0, 1} <= {D for D, _, _ in cases} and all(k <= R for _, k, R in cases)
    assert 1365 * 36 <= 48 * 1024 < 1366 * 36
    for entry, (names, sizes, outputs, overrides) in K.REFUSALS.items():
        assert set(outputs) <= set(names) and set(sizes) <= set(names) and all(set(o) <= set(names) for o in overrides)


# ---- float32 evaluations lie inside the bounds ----------------------------------------------------------------------------------------
def f32_scatter(terms32, dest, N):
    out = np.zeros(terms32.shape[:2] + (N,), np.float32)
    for b in range(len(out)):
        np.add.at(out[b], (slice(None), dest[b]), terms32[b])               # unbuffered, in index order, in float32
    return out


def test_float32_evaluations_are_inside_the_bounds():
    grp, gat, itp = K.rounded_scatter_inputs()
    for name, (g, idx, N) in (("group_points_grad", grp), ("gather_points_grad", gat)):
        B, C = g.shape[:2]
        s = IO.group_points_grad(g, idx, N)
        r = {}
        K.compare(name, f32_scatter(g.reshape(B, C, -1), idx.reshape(B, -1), N), s.ref, s.bound, False, ratios=r)
        K.compare(name, f32_scatter(g.reshape(B, C, -1)[:, :, ::-1], idx.reshape(B, -1)[:, ::-1], N), s.ref, s.bound, False, ratios=r)
        assert 0 < r[name] <= 1
    g, idx, w, m = itp
    B, c, n = g.shape
    s = IO.three_interpolate_grad(g, idx, w, m)
    K.compare("three_interpolate_grad", f32_scatter((g[:, :, :, None] * w[:, None, :, :]).reshape(B, c, -1), idx.reshape(B, -1), m),
              s.ref, s.bound, False, ratios={})
    for cc, mm, nn in K.INTERP_SHAPES:
        f, i, ww = K.interp_inputs(cc, mm, nn, cc * 100 + mm * 10 + nn)
        ref, bound = IO.three_interpolate(f, i, ww)
        p = [np.stack([f[b][:, i[b, :, t]] * ww[b, :, t][None, :] for b in range(2)]) for t in range(3)]
        assert p[0].dtype == np.float32
        K.compare("three_interpolate", (p[0] + p[1]) + p[2], ref, bound, False, ratios={})
    for N in K.BOX_N:
        for B, seed in ((3, N), (1, N + 1)):
            c = IO.rounded_boxcloud_case(B, N, seed)
            assert c["factor"] != 1.0
            a = (c["points"], c["center"], c["wlh"], c["rot"], c["factor"])
            r = {}
            K.compare("boxcloud", IO.boxcloud_f32(*a), IO.boxcloud(*a), IO.boxcloud_bound(*a), False, ratios=r)
            assert r["boxcloud"] <= 1
            if B == 3:
                d = np.linalg.norm(c["center"].astype(np.float64), axis=1)
                assert d[1] > 399 and d[2] > 1999


# ---- the refusal table on host memory ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(K.REFUSALS))
def test_refusals_come_before_the_device(entry):
    from open3dsot_amd import capi
    lib = capi.load()
    src = (ctypes.c_float * 4096)()
    keep = []

    def new_out():
        buf = np.full(64 + K.TAIL, K.SENT, np.float32)
        keep.append(buf)
        return buf, buf.ctypes.data

    K.refused_everywhere(lib, entry, ctypes.addressof(src), new_out, lambda buf: bool((buf == np.float32(K.SENT)).all()), None)


def test_the_three_closed_holes_by_name():
    from open3dsot_amd import capi
    lib = capi.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.o3d_three_interpolate(p, p, p, 1, 2, 0, 3, p, None) == K.EINVAL                 # m == 0 with work to do
    assert lib.o3d_three_interpolate(p, p, p, 1, 2, 0, 0, p, None) == 0                        # ... and without
    assert lib.o3d_group_points(p, p, 1, 2, 0, 3, 2, p, None) == K.EINVAL                      # N == 0 with work to do
    assert lib.o3d_gather_points(p, p, 1, 2, 0, 3, p, None) == K.EINVAL
    assert lib.o3d_gather_points(p, p, 1, 2, 0, 0, p, None) == 0
    assert lib.o3d_boxcloud(p, p, p, p, 1.0, 65536, 4, p, None) == K.EINVAL                    # B beyond grid.y
    assert lib.o3d_boxcloud(p, p, p, p, 1.0, 65536, 0, p, None) == K.EINVAL
    # a refused scatter-add writes nothing: the operands are checked before the zero fill
    assert lib.o3d_group_points_grad(None, p, 1, 2, 4, 3, 2, p, None) == K.EINVAL
    assert lib.o3d_three_interpolate_grad(p, None, p, 1, 2, 3, 4, p, None) == K.EINVAL


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------
def test_rejects_wrong_ball_queries():
    rng = np.random.RandomState(4)
    cloud = (rng.randint(-2, 3, size=(2, 65, 3)) * 0.5).astype(np.float32)
    centers = (rng.randint(-2, 3, size=(2, 5, 3)) * 0.5).astype(np.float32)
    ref = IO.ball_query_numpy(centers, cloud, 1.0, 65)
    K.same_bits("ball", ref, ref)
    assert differs("pad with 0", IO.ball_query_numpy(centers, cloud, 1.0, 65, pad_first=False), ref)
    assert differs("<= at the radius", IO.ball_query_numpy(centers, cloud, 1.0, 65, strict=False), ref)
    strict = np.array([[[0.5, 0, 0], [0, 0.5, 0], [0.25, 0, 0], [0, 0, 0.5]]], np.float32)
    assert IO.ball_query_numpy(np.zeros((1, 1, 3)), strict, 0.5, 3)[0, 0].tolist() == [2, 2, 2]
    assert IO.ball_query_numpy(np.zeros((1, 1, 3)), strict, 0.5, 3, strict=False)[0, 0].tolist() == [0, 1, 2]


def test_rejects_wrong_fps_tie_orders():
    for kind, N in (("grid", 129), ("grid", 513), ("fargrid", 300)):
        cloud = IO.fps_cloud(kind, 1, N, 5)
        ref = IO.fps_numpy(cloud, 24)
        assert differs("last maximum", IO.fps_numpy(cloud, 24, last_max=True), ref)
        assert differs("plain rank", IO.fps_numpy(cloud, 24, rank=np.arange(N)), ref)
    line = (np.arange(300)[None, :, None] * np.array([4.0e5, 0, 0]) + np.array([0, 1.0, 0])).astype(np.float32)
    assert IO.fps_numpy(line, 8)[0].tolist() == [0, 256, 128, 64, 192, 32, 288, 160]
    assert IO.fps_numpy(line, 8, rank=np.arange(300))[0].tolist() == list(range(8))


def test_rejects_an_unstable_knn():
    rng = np.random.RandomState(6)
    q, r = K.half_integers(rng, (2, 9, 3)), K.half_integers(rng, (2, 40, 3))
    ref = IO.knn_numpy(q, r, 8)
    assert differs("unstable", IO.knn_numpy(q, r, 8, stable=False), ref)
    d = ((q[:, :, None] - r[:, None]) ** 2).sum(-1)
    assert np.array_equal(np.take_along_axis(d, IO.knn_numpy(q, r, 8, stable=False).astype(np.int64), 2),
                          np.take_along_axis(d, ref.astype(np.int64), 2))                      # (the same distances: only the tie order)


def test_rejects_wrong_scatters():
    (g, idx, N), (gi, ii, wi, m) = K.exact_scatter_inputs()
    s = IO.group_points_grad(g, idx, N)
    K.compare("exact", s.ref.astype(np.float32), s.ref, s.bound, True, ratios={})
    dropped = IO.group_points_grad(g[:, :, 1:], idx[:, 1:], N)               # one duplicate's contribution lost
    assert rejected("exact", dropped.ref, s.ref, s.bound, True)
    nofill = s.ref.copy()
    nofill[s.cnt == 0] = K.SENT                                              # no zero fill: untouched destinations keep the sentinel
    assert rejected("exact", nofill, s.ref, s.bound, True)
    assert not (nofill[s.cnt == 0] == 0).all()
    grp, gat, itp = K.rounded_scatter_inputs()
    s = IO.group_points_grad(*grp)
    g2, i2 = grp[0].copy(), grp[1]
    q = int(np.argmin(np.abs(g2[0, 0].reshape(-1))))                         # the SMALLEST contribution of a row, dropped
    small = g2[0, 0].reshape(-1)[q]
    assert 0 < abs(small) < 1e-2
    g2[0, 0].reshape(-1)[q] = 0
    assert rejected("rounded", IO.group_points_grad(g2, i2, grp[2]).ref, s.ref, s.bound, False)
    doubled = grp[0].copy()
    doubled[0, 0].reshape(-1)[q] *= 2
    assert rejected("rounded", IO.group_points_grad(doubled, i2, grp[2]).ref, s.ref, s.bound, False)
    s = IO.three_interpolate_grad(*itp)
    off = s.ref.copy()
    at = tuple(np.argwhere(s.bound > 0)[0])
    off[at] += 2 * s.bound[at]
    assert rejected("rounded", off, s.ref, s.bound, False)


def test_rejects_wrong_boxclouds_and_one_element_off():
    c = IO.rounded_boxcloud_case(3, 257, 257)
    a = (c["points"], c["center"], c["wlh"], c["rot"], c["factor"])
    ref, bound = IO.boxcloud(*a), IO.boxcloud_bound(*a)
    K.compare("boxcloud", ref, ref, bound, False, ratios={})
    assert rejected("corners exchanged", ref[..., [0, 2, 1, 3, 4, 5, 6, 7, 8]], ref, bound, False)
    assert rejected("corners exchanged", ref[..., [0, 1, 2, 3, 4, 5, 6, 8, 7]], ref, bound, False)
    assert rejected("w and l swapped", IO.boxcloud(*a, swap_wl=True), ref, bound, False)
    assert rejected("factor dropped", IO.boxcloud(*a[:4], 1.0), ref, bound, False)
    for at in ((0, 0, 0), (1, 100, 3), (2, 256, 8)):
        off = ref.copy()
        off[at] += 2 * bound[at] if bound[at] > 0 else 1e-7
        assert rejected("one element", off, ref, bound, False)
    f, i, w = K.interp_inputs(17, 20, 257, 1)
    r, b = IO.three_interpolate(f, i, w)
    off = r.copy()
    off[1, 16, 256] += 2 * b[1, 16, 256]
    assert rejected("one element", off, r, b, False)
