"""The scene trackers' device-side lifecycle without a GPU: the properties of the numpy restatement
(tests/scene_manage_oracle.py) that the GPU tests compare the kernels with, the argument checks of the two entry points, and
the refusals of the managed tracker classes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_manage_oracle as SO  # noqa: E402


def box(x, y=0.0, z=0.0, wlh=(2.0, 4.0, 1.5), yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([x, y, z, *wlh, c, -s, 0, s, c, 0, 0, 0, 1], np.float32)


def random_case(rng, K, D, ties=True):
    """score matrices with many exact ties (values from a small set), a random active mask and n_det"""
    pick = (lambda n: rng.integers(0, 4, n) / 4.0) if ties else (lambda n: rng.random(n))
    ov = pick(K * D).reshape(K, D).astype(np.float32)
    di = (4.0 * pick(K * D)).reshape(K, D).astype(np.float32)
    return ov, di, (rng.random(K) < 0.8).astype(np.int32), int(rng.integers(0, D + 1))


@pytest.mark.parametrize("K,D", [(1, 1), (5, 6), (17, 9), (9, 17), (24, 24)])
def test_the_match_is_one_to_one_admissible_and_maximal(K, D):
    rng = np.random.default_rng(K * 100 + D)
    for trial in range(20):
        ov, di, active, n = random_case(rng, K, D, ties=trial % 2 == 0)
        ok = SO.admissible(ov, di, active, n, 0.25, 3.0)
        match, det_match = SO.greedy_match(ov, di, ok)
        taken = [(k, d) for k, d in enumerate(match) if d >= 0]
        assert len({d for _, d in taken}) == len(taken)                                       # one to one
        assert all(det_match[d] == k for k, d in taken) and (det_match >= 0).sum() == len(taken)
        assert all(ok[k, d] for k, d in taken)                                                # every taken pair is admissible
        for k, d in zip(*np.nonzero(ok)):                                                     # nothing admissible is left open
            assert match[k] >= 0 or det_match[d] >= 0, (k, d)
        assert not ok[active == 0].any() and not ok[:, n:].any()
        for k, d in taken:                    # greedy: a taken pair is first, in the written order, among the pairs that were still open
            for k2, d2 in zip(*np.nonzero(ok)):
                if (k2, d2) != (k, d) and (-ov[k2, d2], di[k2, d2], k2, d2) < (-ov[k, d], di[k, d], k, d):
                    assert (match[k2] >= 0 and (-ov[k2, match[k2]], di[k2, match[k2]], k2, match[k2]) < (-ov[k, d], di[k, d], k, d)) or \
                        (det_match[d2] >= 0 and (-ov[det_match[d2], d2], di[det_match[d2], d2], det_match[d2], d2) < (-ov[k, d], di[k, d], k, d))


def test_nan_is_never_admissible_and_the_bounds_are_inclusive():
    ov = np.array([[np.nan, 0.5, 0.25, 0.2]], np.float32)
    di = np.array([[0.0, np.nan, 3.0, 0.0]], np.float32)
    assert SO.admissible(ov, di, [1], 4, 0.25, 3.0).tolist() == [[False, False, True, False]]


def test_exact_ties_between_duplicated_detections_fall_to_the_lowest_k_and_d():
    tracks = np.stack([box(0.0), box(50.0)])
    dets = np.stack([box(50.0), box(0.0), box(0.0), box(50.0)])                              # each track's box twice
    ov, di = SO.pair_scores(tracks, [1, 1], dets, 4)
    assert ov[0, 1] == ov[0, 2] == 1.0 and ov[1, 0] == ov[1, 3] == 1.0 and di[0, 1] == 0.0
    match, det_match = SO.greedy_match(ov, di, SO.admissible(ov, di, [1, 1], 4, 0.0, np.inf))
    assert match.tolist() == [1, 0] and det_match.tolist() == [1, 0, -1, -1]
    # two tracks on one box and one detection: the lower k takes it
    ov, di = SO.pair_scores(np.stack([box(0.0), box(0.0)]), [1, 1], box(0.0)[None], 1)
    match, _ = SO.greedy_match(ov, di, SO.admissible(ov, di, [1, 1], 1, 0.5, np.inf))
    assert match.tolist() == [0, -1]


def test_pair_scores_mark_inactive_rows_and_columns_beyond_n_det():
    tracks, dets = np.stack([box(0.0), box(1.0), box(2.0)]), np.stack([box(0.5), box(1.5)])
    ov, di = SO.pair_scores(tracks, [1, 0, 1], dets, 1)
    assert ov.dtype == np.float32 and ov.shape == (3, 2)
    assert (ov[1] == -1).all() and np.isinf(di[1]).all() and (ov[:, 1] == -1).all() and np.isinf(di[:, 1]).all()
    assert 0 < ov[0, 0] < 1 and di[0, 0] == 0.5 and ov[2, 0] > 0 and di[2, 0] == 1.5
    assert SO.clamp_n(-3, 2) == 0 and SO.clamp_n(9, 2) == 2


def scenario():
    """K = 3: slots 0 and 1 follow objects, slot 2 is free"""
    s = SO.new_state(3, 8, np.stack([box(0.0), box(30.0)]))
    assert s["active"].tolist() == [1, 1, 0] and s["slot"][:, 0].tolist() == [0, 1, -1] and s["next_id"].tolist() == [2]
    assert s["ids_log"][0].tolist() == [0, 1, -1] and s["cur"][2].tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    return s


def test_retire_then_reuse_in_one_call_and_dropped_is_counted():
    s = scenario()
    counts = np.zeros((3, 2), np.int32)
    # frame 1: slot 1 has no detection (one miss), three new objects for one free slot
    dets = np.stack([box(0.1), box(100.0), box(200.0), box(300.0)])
    s1, match, det_match = SO.step(s, dets, 4, counts, 1, max_misses=1, max_dist=3.0)
    assert match.tolist() == [0, -1, -1] and det_match.tolist() == [0, -1, -1, -1]
    assert s1["slot"].tolist() == [[0, 0, 0, 0], [1, 1, 0, 0], [2, 0, 0, 1]] and s1["active"].tolist() == [1, 1, 1]
    assert s1["dropped_log"][1] == 2 and s1["next_id"].tolist() == [3] and s1["ids_log"][1].tolist() == [0, 1, 2]
    assert np.array_equal(s1["cur"][2], dets[1]) and np.array_equal(s1["results"][1, 2], dets[1])
    assert np.array_equal(s1["yaw_state"][2], np.r_[dets[1, 6:15], 0]) and np.array_equal(s1["canon_wlh"][2], dets[1, 3:6])
    assert s1["lanes"].tolist() == [[1, 0, 1, 0, -1, -1, 0], [1, 0, 1, 0, -1, -1, 0], [1, 1, 1, 0, -1, -1, 0]]
    assert s["active"].tolist() == [1, 1, 0] and s["next_id"].tolist() == [2]                # a pure function
    # frame 2: slot 1 misses again (2 > max_misses = 1): retired and taken by the new detection in the same call
    dets = np.stack([box(0.2), box(100.0), box(400.0)])
    s1["bank_state_next"][:] = 7
    s2, match, _ = SO.step(s1, dets, 3, counts, 2, max_misses=1, max_dist=3.0, rule=0)
    assert match.tolist() == [0, -1, 1]
    assert s2["slot"].tolist() == [[0, 0, 0, 0], [3, 0, 0, 2], [2, 0, 0, 1]] and s2["active"].tolist() == [1, 1, 1]
    assert s2["ids_log"][2].tolist() == [0, 3, 2] and s2["match_log"][2].tolist() == [0, -1, 1] and s2["dropped_log"][2] == 0
    assert np.array_equal(s2["cur"][1], dets[2]) and s2["bank_state_next"].tolist() == [[7, 7], [0, 0], [7, 7]]
    assert s2["lanes"][:, :3].tolist() == [[1, 0, 0], [1, 1, 1], [1, 0, 0]]                   # rule `first`: has_crop = first
    # enroll off: the retired slot stays free, nothing is dropped
    s3, _, _ = SO.step(s1, dets, 3, counts, 2, max_misses=1, max_dist=3.0, enroll=0)
    assert s3["active"].tolist() == [1, 0, 1] and s3["slot"][1].tolist() == [-1, 2, 0, 0] and s3["dropped_log"][2] == 0
    assert s3["ids_log"][2].tolist() == [0, 1, 2] and np.array_equal(s3["cur"][1], s1["cur"][1])


def test_has_dets_0_leaves_the_misses_alone_and_the_starvation_rule_runs_on_every_frame():
    s = scenario()
    s["slot"][1, 1] = 2
    counts = np.array([[5, 50], [50, 5], [0, 0]], np.int32)
    dets = np.stack([box(0.0)])
    a, match, _ = SO.step(s, dets, 1, counts, 1, has_dets=0, max_misses=2, min_points=10, max_starved=1)
    assert match.tolist() == [-1, -1, -1] and a["slot"].tolist() == [[0, 0, 1, 0], [1, 2, 0, 0], [-1, 0, 0, 0]]
    assert a["active"].tolist() == [1, 1, 0] and a["next_id"].tolist() == [2]                 # nothing enrolled either
    b, _, _ = SO.step(a, dets, 1, counts, 2, has_dets=0, max_misses=2, min_points=10, max_starved=1)
    assert b["active"].tolist() == [0, 1, 0] and b["slot"][0].tolist() == [-1, 0, 2, 0]      # starved 2 > 1: retired
    c, _, _ = SO.step(s, dets, 1, counts, 1, has_dets=0, count_col=1, min_points=10, max_starved=0)
    assert c["active"].tolist() == [1, 0, 0]                                                  # the motion tracker's column
    d, _, _ = SO.step(s, dets, 1, counts, 1, has_dets=1, max_misses=2)                        # with detections slot 1 misses a third time
    assert d["slot"].tolist() == [[0, 0, 0, 0], [-1, 3, 0, 0], [-1, 0, 0, 0]] and d["ids_log"][1].tolist() == [0, 1, -1]
    e, _, _ = SO.step(s, np.zeros((0, 15), np.float32), 0, counts, 1, has_dets=1, max_misses=2)      # D = 0 still counts
    assert e["slot"][:, 1].tolist() == [1, 3, 0] and e["active"].tolist() == [1, 0, 0]


def test_a_non_finite_detection_is_not_enrolled_and_not_dropped():
    s = scenario()
    bad = box(100.0)
    bad[4] = np.nan
    s1, _, det_match = SO.step(s, np.stack([bad, box(200.0)]), 2, np.zeros((3, 2), np.int32), 1, max_dist=3.0)
    assert det_match.tolist() == [-1, -1] and s1["dropped_log"][1] == 0 and np.array_equal(s1["cur"][2], box(200.0))


def test_both_entry_points_validate_before_any_hip_call():
    from open3dsot_amd import capi
    lib = capi.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = capi.CONSTANTS["O3D_EINVAL"]
    KMAX, DMAX = capi.CONSTANTS["O3D_CROP_MULTI_MAX_TARGETS"], capi.CONSTANTS["O3D_SCENE_MAX_DETECTIONS"]
    assert (DMAX, capi.CONSTANTS["O3D_SCENE_SLOT_COLS"]) == (1024, 4)

    def scores(tracks=p, active=p, K=2, dets=p, n_det=p, D=3, dim=3, up=2, ov=p, di=p):
        return lib.o3d_scene_pair_scores(tracks, active, K, dets, n_det, D, dim, up, ov, di, None)
    for bad in (dict(tracks=None), dict(active=None), dict(dets=None), dict(n_det=None), dict(ov=None), dict(di=None), dict(K=0),
                dict(K=KMAX + 1), dict(D=-1), dict(D=DMAX + 1), dict(dim=1), dict(dim=4), dict(up=0), dict(up=3)):
        assert scores(**bad) == EINVAL, bad
    assert scores(D=0, dets=None, n_det=None, ov=None, di=None) == 0                          # nothing to score: no launch

    def manage(ov=p, di=p, dets=p, n_det=p, K=2, D=3, cur=p, yaw=p, wlh=p, results=p, T=4, frame=p, active=p, slot=p, next_id=p,
               counts=p, count_col=0, bank=p, lanes=p, rule=2, ids=p, match=p, dropped=p):
        return lib.o3d_scene_manage(ov, di, dets, n_det, K, D, cur, yaw, wlh, results, T, frame, active, slot, next_id, counts,
                                    count_col, bank, lanes, rule, ids, match, dropped, 0.0, 1.0, 2, 0, 0, 1, 1, None)
    for name in ("ov", "di", "dets", "n_det", "cur", "yaw", "wlh", "results", "frame", "active", "slot", "next_id", "counts", "lanes",
                 "ids", "match", "dropped"):
        assert manage(**{name: None}) == EINVAL, name
    for bad in (dict(K=0), dict(K=KMAX + 1), dict(D=-1), dict(D=DMAX + 1), dict(T=0), dict(count_col=2), dict(rule=-2), dict(rule=4),
                dict(D=0, cur=None)):
        assert manage(**bad) == EINVAL, bad


def test_the_managed_classes_refuse_cpu_models_ref_boxes_and_too_many_detections():
    from open3dsot_amd import trackers, tracking
    assert issubclass(tracking.ManagedSceneTracker, tracking.SceneTracker)
    assert issubclass(tracking.ManagedMotionSceneTracker, tracking.MotionSceneTracker)
    bat = trackers.get_model("BAT")(trackers.make_config(dict(trackers.BAT_CAR)))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        tracking.ManagedSceneTracker(bat, 4)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        tracking.managed_scene_tracker_for(bat, 4, manage=dict(max_misses=1))
    with pytest.raises(TypeError):
        tracking.ManagedMotionSceneTracker(bat, 4)
    # update()'s own checks come before anything touches a device: an instance without a device shows them
    for cls in (tracking.ManagedSceneTracker, tracking.ManagedMotionSceneTracker):
        trk = object.__new__(cls)
        trk.max_detections, trk.t = 4, 1
        with pytest.raises(ValueError, match="ref_boxes"):
            trk.update(torch.zeros(8, 3), ref_boxes=np.zeros((4, 15), np.float32))
        for dets in (np.zeros((5, 15), np.float32), torch.zeros(5, 15), [np.zeros(15, np.float32)] * 5):
            with pytest.raises(ValueError, match="max_detections"):
                trk.update(torch.zeros(8, 3), detections=dets)
        with pytest.raises(RuntimeError, match="CPU not supported"):                           # a CPU frame, after the checks
            trk.update(torch.zeros(8, 3), detections=np.zeros((4, 15), np.float32))
    assert tracking._unit_box().tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1]
