"""o3d_scene_pair_scores (csrc/metrics.hip) and o3d_scene_manage (csrc/scene.hip) through the C ABI, per call, against the numpy
restatement tests/scene_manage_oracle.py: every output array equal."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_manage_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
STATE = ("cur", "yaw_state", "canon_wlh", "results", "active", "slot", "next_id", "bank_state_next", "lanes", "ids_log", "match_log",
         "dropped_log")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def box(x, y=0.0, z=0.0, wlh=(2.0, 4.0, 1.5), yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([x, y, z, *wlh, c, -s, 0, s, c, 0, 0, 0, 1], np.float32)


def scene(rng, K, D, n_new):
    """K track boxes on a 6 m grid with random yaws and sizes; D detections: jittered copies of tracks (overlaps of every size),
    then n_new boxes far from every track"""
    tracks = np.stack([box(6.0 * (k % 12), 6.0 * (k // 12), 0.1 * (k % 3), wlh=1.5 + rng.random(3), yaw=rng.uniform(-3, 3))
                       for k in range(K)])
    dets = []
    for d in range(D - n_new):
        b = tracks[rng.integers(0, K)].copy()
        b[:3] += rng.normal(scale=0.6, size=3).astype(np.float32)
        dets.append(b)
    dets += [box(1000.0 + 10.0 * j, -50.0, 0.0, yaw=0.3 * j) for j in range(n_new)]
    return tracks, np.stack(dets).astype(np.float32) if dets else np.zeros((0, 15), np.float32)


def to_camera(boxes):
    """z-up boxes -> the camera frame (y down): x' = x, y' = -z, z' = y; the xy footprint becomes the xz footprint"""
    P = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    out = np.array(boxes, np.float32).reshape(-1, 15)
    out[:, :3] = out[:, :3] @ P.T
    out[:, 6:15] = (P @ out[:, 6:15].reshape(-1, 3, 3)).reshape(-1, 9)
    return out


def state_of(rng, K, T, tracks, active):
    """a mid-sequence state: ids, misses, starved, start per slot, sentinels where a call must not write"""
    s = SO.new_state(K, T, tracks)
    s["active"][:] = active
    s["slot"][:, 0] = np.where(active != 0, 10 + np.arange(K), -1)
    s["slot"][:, 1:3] = rng.integers(0, 3, (K, 2)) * (active != 0)[:, None]
    s["next_id"][0] = 10 + K
    s["results"][:] = rng.normal(size=s["results"].shape).astype(np.float32)
    s["bank_state_next"][:] = 7
    s["lanes"][:] = -5
    s["ids_log"][:], s["match_log"][:], s["dropped_log"][:] = -7, -8, -9
    return s


def device_scores(dev, tracks, active, dets, n_det, dim, up):
    from open3dsot_amd import points_utils as PU
    up_t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    return PU.scene_pair_scores(up_t(tracks, np.float32), up_t(active, np.int32), up_t(dets, np.float32),
                                torch.tensor([n_det], dtype=torch.int32, device=dev), dim, up)


def device_step(dev, state, dets, n_det, counts, t, dim=3, up=2, has_dets=1, count_col=0, rule=2, scores=None, **params):
    """the two launches on an upload of `state` (with scores = (overlaps, distances): o3d_scene_manage alone, on these matrices)
    -> (the state read back, the two matrices)"""
    from open3dsot_amd import points_utils as PU
    g = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in state.items() if v is not None}
    d_dev = torch.from_numpy(np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 15)).to(dev)
    n_dev = torch.tensor([n_det], dtype=torch.int32, device=dev)
    K, D = state["cur"].shape[0], d_dev.shape[0]
    ov, di = torch.full((K, D), 9.0, device=dev), torch.full((K, D), 9.0, device=dev)
    if scores is not None:
        ov, di = (torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(dev) for m in scores)
    elif D:
        PU.scene_pair_scores(g["cur"], g["active"], d_dev, n_dev, dim, up, out=(ov, di))
    p = dict(SO.PARAMS)
    p.update(params)
    PU.scene_manage(ov, di, d_dev, n_dev, g["cur"], g["yaw_state"], g["canon_wlh"], g["results"],
                    torch.tensor([t + 1], dtype=torch.int32, device=dev), g["active"], g["slot"], g["next_id"],
                    torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(dev), count_col, g.get("bank_state_next"),
                    g["lanes"], {0: "first", 1: "previous", 2: "firstandprevious", 3: "all", -1: None}[rule], g["ids_log"],
                    g["match_log"], g["dropped_log"], has_dets=has_dets, **p)
    out = {k: (None if state[k] is None else g[k].cpu().numpy()) for k in state}
    return out, ov.cpu().numpy(), di.cpu().numpy()


def assert_step(dev, state, dets, n_det, counts, t, what, **kw):
    got, ov, di = device_step(dev, state, dets, n_det, counts, t, **kw)
    want, match, det_match = SO.step(state, dets, n_det, counts, t, **kw)
    for name in STATE:
        if want[name] is None:
            assert got[name] is None
            continue
        assert got[name].dtype == want[name].dtype and np.array_equal(bits(got[name]), bits(want[name])), (what, name)
    return got, want, match, det_match


# ---- o3d_scene_pair_scores ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("K,D", [(1, 1), (5, 6), (65, 70), (130, 3)])
def test_pair_scores_carry_the_bits_of_o3d_track_score_and_equal_the_oracle(dev, K, D, dim):
    from open3dsot_amd import metrics
    rng = np.random.default_rng(100 * K + D)
    tracks, dets = scene(rng, K, D, min(D, 2) - 1)
    active = np.ones((K,), np.int32)
    active[1::4] = 0                                       # K = 1 stays active
    n_det = D if D < 3 else D - 2
    up = 2 if K != 5 else 1                                # one case in the camera frame
    if up == 1:
        tracks, dets = to_camera(tracks), to_camera(dets)
    ov, di = device_scores(dev, tracks, active, dets, n_det, dim, up)
    assert ov.shape == (K, D) and ov.dtype == torch.float32
    a = torch.from_numpy(tracks).to(dev)[:, None, :].expand(K, D, 15).contiguous()
    b = torch.from_numpy(dets).to(dev)[None, :, :].expand(K, D, 15).contiguous()
    so, sd = metrics.score_boxes(a, b, dim, (0, 0, 1) if up == 2 else (0, -1, 0))
    live = torch.from_numpy((active[:, None] != 0) & (np.arange(D)[None, :] < n_det)).to(dev)
    assert torch.equal(ov[live].view(torch.int32), so[live].view(torch.int32))
    assert torch.equal(di[live].view(torch.int32), sd[live].view(torch.int32))
    assert bool((ov[~live] == -1).all()) and bool(torch.isinf(di[~live]).all()) and bool((di[~live] > 0).all())
    want_ov, want_di = SO.pair_scores(tracks, active, dets, n_det, dim, up)
    assert np.array_equal(bits(ov.cpu().numpy()), bits(want_ov)) and np.array_equal(bits(di.cpu().numpy()), bits(want_di))
    if K > 1:
        assert 0 < float(ov[live].max()) < 1 and int((ov[live] > 0).sum()) >= 1                # real overlaps, not all 0


def test_pair_scores_clamp_n_det(dev):
    rng = np.random.default_rng(1)
    tracks, dets = scene(rng, 3, 4, 0)
    for n, want in ((-2, 0), (9, 4)):
        ov, _ = device_scores(dev, tracks, np.ones(3, np.int32), dets, n, 3, 2)
        assert int((ov >= 0).sum()) == 3 * want


# ---- o3d_scene_manage ----------------------------------------------------------------------------------------------------------------
def test_manage_without_detections_k1_d0(dev):
    s = state_of(np.random.default_rng(0), 1, 4, box(0.0)[None], np.ones(1, np.int32))
    s["slot"][0] = 10, 2, 0, 0
    got, _, _, _ = assert_step(dev, s, np.zeros((0, 15), np.float32), 0, np.zeros((1, 2), np.int32), 2, "(1,0)", max_misses=2)
    assert got["active"].tolist() == [0] and got["slot"].tolist() == [[-1, 3, 0, 0]] and got["ids_log"][2].tolist() == [10]


def test_manage_duplicated_detections_and_exact_ties(dev):
    rng = np.random.default_rng(5)
    tracks = np.stack([box(0.0), box(0.0), box(20.0), box(40.0, yaw=0.4), box(60.0)])          # tracks 0 and 1 on one box
    dets = np.stack([box(20.0), box(0.0), box(0.0), box(20.0), box(40.3, yaw=0.4), box(0.0)])   # exact copies, twice and thrice
    s = state_of(rng, 5, 4, tracks, np.array([1, 1, 1, 1, 0], np.int32))
    got, _, match, det_match = assert_step(dev, s, dets, 6, np.zeros((5, 2), np.int32), 1, "(5,6)", min_iou=0.1, max_dist=3.0)
    assert match.tolist() == [1, 2, 0, 4, -1] and det_match.tolist() == [2, 0, 1, -1, 3, -1]
    assert got["match_log"][1].tolist() == [1, 2, 0, 4, -1]
    assert got["slot"][4].tolist() == [15, 0, 0, 1] and np.array_equal(got["cur"][4], dets[3]) and got["dropped_log"][1] == 1


@pytest.mark.parametrize("K,D,n_new,n_free", [(65, 70, 20, 5), (130, 3, 2, 1)])
def test_manage_across_a_wave_with_more_detections_than_free_slots(dev, K, D, n_new, n_free):
    rng = np.random.default_rng(K)
    tracks, dets = scene(rng, K, D, n_new)
    active = np.ones((K,), np.int32)
    active[rng.choice(K, n_free, replace=False)] = 0
    s = state_of(rng, K, 4, tracks, active)
    if D < K:
        s["slot"][:, 1] = 0                                # nobody is retired: the one free slot is all there is
    counts = rng.integers(0, 40, (K, 2)).astype(np.int32)
    got, want, match, det_match = assert_step(dev, s, dets, D, counts, 3, (K, D), min_iou=0.05, max_dist=2.5, max_misses=1)
    assert (match >= 0).sum() >= 1 and got["dropped_log"][3] > 0 and got["next_id"][0] > 10 + K
    assert (got["active"] != s["active"]).any() and (got["lanes"][:, 1] == 1).sum() >= n_free
    # the same call again from the same state: the same bits
    again, ov, di = device_step(dev, s, dets, D, counts, 3, min_iou=0.05, max_dist=2.5, max_misses=1)
    for name in STATE:
        assert np.array_equal(bits(again[name]), bits(got[name])), name
    # and with ties everywhere: every detection a copy of ONE track's box, every track on that box
    same = np.tile(tracks[0], (K, 1))
    s2 = state_of(rng, K, 4, same, np.ones((K,), np.int32))
    got2, _, match2, _ = assert_step(dev, s2, np.tile(tracks[0], (D, 1)), D, counts, 1, (K, D, "ties"))
    assert match2.tolist() == list(range(min(K, D))) + [-1] * (K - min(K, D))


def test_manage_no_free_slot_drops_every_new_detection(dev):
    rng = np.random.default_rng(9)
    tracks, dets = scene(rng, 6, 9, 4)
    s = state_of(rng, 6, 4, tracks, np.ones((6,), np.int32))
    s["slot"][:, 1] = 0
    got, _, _, det_match = assert_step(dev, s, dets, 9, np.zeros((6, 2), np.int32), 2, "full", min_iou=0.0, max_dist=2.5, max_misses=5)
    assert got["dropped_log"][2] == (det_match < 0).sum() >= 4 and got["next_id"][0] == 16 and not got["lanes"][:, 1].any()
    assert np.array_equal(bits(got["cur"]), bits(s["cur"]))


def test_manage_skips_a_non_finite_detection(dev):
    rng = np.random.default_rng(11)
    tracks = np.stack([box(0.0), box(20.0), box(40.0)])
    dets = np.stack([box(500.0), box(600.0), box(700.0), box(0.2)])
    dets[0, 7] = np.nan
    dets[1, 0] = np.inf
    s = state_of(rng, 3, 4, tracks, np.array([1, 0, 0], np.int32))
    got, _, _, _ = assert_step(dev, s, dets, 4, np.zeros((3, 2), np.int32), 1, "nan", max_dist=3.0)
    assert got["slot"][:, 0].tolist() == [10, 13, -1] and np.array_equal(got["cur"][1], dets[2]) and got["dropped_log"][1] == 0


@pytest.mark.parametrize("count_col,rule", [(0, 0), (1, -1)])
def test_manage_min_points_rule_and_has_dets_0(dev, count_col, rule):
    rng = np.random.default_rng(13)
    tracks, dets = scene(rng, 7, 5, 2)
    s = state_of(rng, 7, 4, tracks, np.array([1, 1, 1, 0, 1, 1, 1], np.int32))
    if rule < 0:
        s["bank_state_next"] = None                        # the motion tracker: no bank
    counts = np.array([[3, 30], [30, 3], [10, 10], [0, 0], [9, 11], [11, 9], [0, 50]], np.int32)
    kw = dict(count_col=count_col, rule=rule, min_points=10, max_starved=1, max_misses=2, max_dist=2.5)
    got, _, _, _ = assert_step(dev, s, dets, 5, counts, 2, "min_points", **kw)
    quiet, _, match, _ = assert_step(dev, s, dets, 5, counts, 2, "has_dets = 0", has_dets=0, **kw)
    assert (match < 0).all() and quiet["slot"][:, 1].tolist() == s["slot"][:, 1].tolist() and quiet["next_id"][0] == s["next_id"][0]
    assert (quiet["slot"][:, 2] != s["slot"][:, 2]).any() and quiet["lanes"][:, 2].tolist() == [int(rule != 0)] * 7
    # beyond the results buffer (t >= T): the state advances, no row is written
    late, _, _, _ = assert_step(dev, s, dets, 5, counts, 4, "t = T", **kw)
    assert (late["ids_log"] == -7).all() and np.array_equal(bits(late["results"]), bits(s["results"])) and late["next_id"][0] > s["next_id"][0]


# ---- the match on given matrices: rows in contention for a detection that is one row's second choice ------------------------------------
def assert_manage_on(dev, state, ov, di, dets, n_det, counts, t, what, **kw):
    """o3d_scene_manage on uploaded matrices against scene_manage_oracle.manage on the same ones: every array equal"""
    got, _, _ = device_step(dev, state, dets, n_det, counts, t, scores=(ov, di), **kw)
    want, match, det_match = SO.manage(state, ov, di, dets, n_det, counts, t, **kw)
    for name in STATE:
        assert got[name].dtype == want[name].dtype and np.array_equal(bits(got[name]), bits(want[name])), (what, name)
    return got, match, det_match


def test_manage_gives_a_contested_detection_to_the_track_the_walk_gives_it_to(dev):
    """tracks at x = 0, 3, 14, detections at x = 1, 8, every overlap 0, the default gates: the walk takes (0,0) at distance 1, then
    (1,1) at 5 -- track 1's SECOND choice, which is track 2's first (6)"""
    rng = np.random.default_rng(2)
    ov = np.zeros((3, 2), np.float32)
    di = np.array([[1, 8], [2, 5], [13, 6]], np.float32)
    s = state_of(rng, 3, 4, np.stack([box(0.0), box(3.0), box(14.0)]), np.ones((3,), np.int32))
    got, match, det_match = assert_manage_on(dev, s, ov, di, np.stack([box(1.0), box(8.0)]), 2, np.zeros((3, 2), np.int32), 1, "3x2")
    assert match.tolist() == [0, 1, -1] and det_match.tolist() == [0, 1] and got["match_log"][1].tolist() == [0, 1, -1]


@pytest.mark.parametrize("K,D", [(5, 6), (24, 24), (65, 70), (130, 3)])
def test_manage_on_random_matrices_with_ties_equals_the_oracle(dev, K, D):
    """random (K,D) overlap and distance matrices, from a small set of values (exact ties) or continuous, tight and loose gates, a
    random active mask and n_det: second choices collide with first choices all over"""
    rng = np.random.default_rng(1000 * K + D)
    tracks, dets = scene(rng, K, D, 0)
    contested = 0
    for trial in range(6):
        pick = (lambda m: rng.integers(0, 4, m) / 4.0) if trial % 2 == 0 else (lambda m: rng.random(m))
        ov = pick(K * D).reshape(K, D).astype(np.float32)
        di = (4.0 * pick(K * D)).reshape(K, D).astype(np.float32)
        active = (rng.random(K) < 0.8).astype(np.int32)
        n_det = D if trial < 2 else int(rng.integers(0, D + 1))
        gates = dict(min_iou=0.25, max_dist=3.0) if trial % 3 else {}
        s = state_of(rng, K, 4, tracks, active)
        counts = rng.integers(0, 40, (K, 2)).astype(np.int32)
        got, match, det_match = assert_manage_on(dev, s, ov, di, dets, n_det, counts, 2, (K, D, trial), max_misses=1, **gates)
        assert got["match_log"][2].tolist() == match.tolist()
        ok = SO.admissible(ov, di, active, n_det, gates.get("min_iou", 0.0), gates.get("max_dist", np.inf))
        for k in np.flatnonzero(match >= 0):               # a track that did not get the first pair of its row
            row = [(-ov[k, d], di[k, d], d) for d in np.flatnonzero(ok[k])]
            contested += min(row)[2] != match[k]
    print("tracks on a later choice than their row's first, (K,D) = (%d,%d): %d" % (K, D, contested))
    assert contested >= 1 or D < 5, "no track fell back to a later choice: the case this test is for did not occur"
