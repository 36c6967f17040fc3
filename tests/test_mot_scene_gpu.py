"""Scoring a managed scene on the device end to end (metrics.ClearMOT, _Managed.score_mot, tracking.evaluate_managed_scene;
DESIGN.md section 12k), on the 3-target, 6-frame scene of ref_multi_tracking.npz with K = 4 slots and the scripted events of
test_scene_manage_gpu.py: target 2 is enrolled at frame 1 (it is MISSED at frame 0), slot 1 loses its detection at frame 2 and is
retired at frame 3, where a box 500 m away takes the slot in the same call (a hypothesis WITHOUT ground truth from then on).
The weights are random: no quality threshold is asserted, only that the device's bookkeeping is the oracle's on the same boxes."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fixture_io  # noqa: E402
import mot_oracle as MOT  # noqa: E402
import test_free_running_tracking_gpu as FR  # noqa: E402  (host_stops, the motion model of case kitti)
import test_scene_manage_gpu as SM  # noqa: E402  (the scripted scenario: make, plain_tracker, frame_detections, host_events)
import test_scene_tracking_gpu as ST  # noqa: E402  (count_uploads)

pytestmark = pytest.mark.gpu
K = SM.K
COUNTS = ("frames",) + MOT.FRAME_COLS + ("objects",)
RATES = ("mota", "motp_dist", "motp_iou", "recall", "precision", "mostly_tracked", "mostly_lost")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scene(dev):
    from open3dsot_amd import synth
    gold = fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_multi_tracking.npz"))
    frames, gt = synth.make_scene(int(gold["scene_seed"]), int(gold["n_frames"]), int(gold["n_points"]), int(gold["n_targets"]))
    assert gt.shape[:2] == (6, 3)
    return [torch.from_numpy(f).to(dev) for f in frames], gt


@pytest.fixture(scope="module")
def run(dev, scene):
    """the scripted managed run, once for the module -> (the tracker, gt (T,3,15), valid (T,3): target 1 has no annotation in
    the last frame)"""
    from open3dsot_amd import tracking
    frames, gt = scene
    model, kw, _ = SM.make("bat_fap", "table", dev)
    man = tracking.managed_scene_tracker_for(model, K, manage=SM.MANAGE, **kw)
    plain = SM.plain_tracker(model, kw, frames, gt)
    man.init(frames[0], gt[0, :2])
    for t in range(1, len(frames)):
        pb = plain.update(frames[t]).cpu().numpy()
        dets, _ = SM.frame_detections(t, pb, gt)
        man.update(frames[t], torch.from_numpy(dets).to(dev))
        SM.host_events(plain, t, gt)
    assert man.events()[0].tolist() == [[0, 1, -1, -1], [0, 1, 2, -1], [0, 1, 2, -1], [0, 3, 2, -1], [0, 3, 2, -1], [0, 3, 2, -1]]
    valid = np.ones(gt.shape[:2], np.int32)
    valid[5, 1] = 0
    return man, np.ascontiguousarray(gt, dtype=np.float32), valid


def oracle_of(trk, gt, valid, **gates):
    """the oracle on the tracker's read-back state -> (summary dict, the walk's rows)"""
    p = dict(MOT.GATES)
    p.update(gates)
    res, ids = trk.results(), trk.events()[0]
    ov, di = MOT.pair_scores_frames(gt, valid, res, ids, trk.score_dim, trk.score_up)
    rows = MOT.walk(ov, di, valid, ids, **p)
    return MOT.summary(rows["per_frame"], rows["match_slot"], rows["match_ov"], rows["match_di"], valid), rows


def assert_same(got, want, what):
    assert set(got) == set(COUNTS + RATES) == set(want), (what, sorted(got), sorted(want))
    for n in COUNTS:
        assert got[n] == want[n] and isinstance(got[n], int), (what, n, got[n], want[n])
    for n in RATES:
        assert got[n] == pytest.approx(want[n], rel=1e-12, abs=0), (what, n, got[n], want[n])


def invariants(d):
    assert d["tp"] + d["fn"] == d["gt"] and d["tp"] + d["fp"] == d["hyp"]
    assert d["mota"] == pytest.approx(1.0 - (d["fn"] + d["fp"] + d["idsw"]) / d["gt"], rel=1e-12)
    assert 0.0 <= d["mostly_tracked"] <= 1.0 and 0.0 <= d["mostly_lost"] <= 1.0 and d["mostly_tracked"] + d["mostly_lost"] <= 1.0


def test_score_mot_equals_the_oracle_on_the_read_back_run(dev, run):
    man, gt, valid = run
    for gates in (dict(), dict(min_iou=0.0, max_dist=np.inf), dict(min_iou=0.3, max_dist=1.0)):
        m = man.score_mot(gt, valid, keep_logs=True, **gates)
        got = m.compute()
        want, rows = oracle_of(man, gt, valid, **gates)
        assert_same(got, want, gates)
        invariants(got)
        logs = {n: t.cpu().numpy() for n, t in m.logs().items()}
        for n in ("match_slot", "match_id", "match_ov", "match_di"):
            assert np.array_equal(SM.bits(logs[n]), SM.bits(rows[n])), (gates, n)
        print("scripted run, gates %s: %s" % (gates, got))
        if not gates:
            # by construction, under the default 2 m gate: target 2 is not followed at frame 0; the far box follows no object
            # from frame 3 on
            assert got["fn"] > 0 and got["fp"] >= 3 and rows["match_slot"][0, 2] == -1 and (rows["match_slot"][3:] != 1).all()
            assert got["gt"] == int(valid.sum()) == 17 and got["hyp"] == 2 + 3 * 5 and got["frames"] == 6
    with pytest.raises(ValueError, match="gt_boxes"):
        man.score_mot(gt[:3])
    with pytest.raises(ValueError, match="gates"):
        man.score_mot(gt, valid, metrics=m, max_dist=1.0)


def test_frame_by_frame_equals_at_once_and_chunks_equal_one_launch(dev, run, monkeypatch):
    from open3dsot_amd import metrics
    man, gt, valid = run
    T, G = gt.shape[:2]
    g_dev, v_dev = torch.from_numpy(gt).to(dev), torch.from_numpy(valid).to(dev)
    kw = dict(dim=man.score_dim, up_axis=(0, 0, 1), max_dist=float("inf"), keep_logs=True)
    sot = [metrics.SuccessPrecision(device=dev) for _ in range(3)]
    once = metrics.ClearMOT(G, dev, sot=sot[0], **kw)
    once.update(g_dev, v_dev, man.boxes[:T], man.ids_log[:T])
    single = metrics.ClearMOT(G, dev, sot=sot[1], **kw)
    for t in range(T):
        single.update(g_dev[t:t + 1], v_dev[t:t + 1], man.boxes[t:t + 1], man.ids_log[t:t + 1])
    monkeypatch.setattr(metrics, "MOT_CHUNK_BYTES", 8 * G * K * 2)             # two frames per chunk
    chunked = metrics.ClearMOT(G, dev, sot=sot[2], **kw)
    assert chunked.chunk_frames(K) == 2 and once.chunk_frames(K) == 2          # (read at the call)
    chunked.update(g_dev, v_dev, man.boxes[:T], man.ids_log[:T])
    want = once.compute()
    for other, what in ((single, "frame by frame"), (chunked, "chunks of two")):
        assert_same(other.compute(), want, what)
        assert torch.equal(other.state, once.state) and torch.equal(other.counts, once.counts), what
        for n, t in other.logs().items():
            assert t.shape == (T, G) and torch.equal(t.view(torch.int32), once.logs()[n].view(torch.int32)), (what, n)
    # the single-object metric of the matched pairs, through SuccessPrecision's own update()
    logs = once.logs()
    hit = logs["match_slot"] >= 0
    ref = metrics.SuccessPrecision(device=dev)
    ref.update(logs["match_ov"][hit], logs["match_di"][hit])
    assert int(hit.sum()) == want["tp"] > 0
    for s in sot:
        assert torch.equal(s.counts, ref.counts)
    # reset() brings back the empty metric; valid=None means every object annotated in every frame
    once.reset()
    assert once.compute()["gt"] == 0 and once.compute()["mota"] == 0.0 and once.logs()["match_slot"].shape == (0, G)
    once.update(g_dev, None, man.boxes[:T], man.ids_log[:T])
    assert once.compute()["gt"] == T * G


def test_score_mot_makes_no_host_stop_and_no_upload(dev, run, monkeypatch):
    from open3dsot_amd import metrics
    man, gt, valid = run
    g_dev, v_dev = torch.from_numpy(gt).to(dev), torch.from_numpy(valid).to(dev)
    man.score_mot(g_dev, v_dev)                            # the first call may load the library
    m = metrics.ClearMOT(gt.shape[1], dev, dim=man.score_dim, sot=metrics.SuccessPrecision(device=dev))
    uploads = []
    with FR.host_stops(monkeypatch) as stops:
        ST.count_uploads(monkeypatch, uploads, lambda: "upload")
        man.score_mot(g_dev, v_dev, metrics=m)
        man.score_mot(g_dev, None, keep_logs=True).logs()
    assert stops.calls == [] and uploads == [], (stops.calls, uploads)
    with FR.host_stops(monkeypatch) as stops:               # the control, and compute()'s one read-back
        got = m.compute()
    assert stops.calls.count("cpu") == 1 and not {"synchronize", "item"} & set(stops.calls), stops.calls
    assert_same(got, oracle_of(man, gt, valid)[0], "after the harness")


@pytest.mark.parametrize("case", ["bat_fap", FR.MOTION])
def test_evaluate_managed_scene_equals_the_oracle_on_its_own_run(dev, scene, case):
    from open3dsot_amd import tracking
    frames, gt = scene
    gt = np.ascontiguousarray(gt, dtype=np.float32)
    T = len(frames)
    valid = np.ones((T, 3), np.int32)
    valid[0, 2] = 0                                        # target 2 appears at frame 1: enrolled from its detection
    valid[4:, 1] = 0                                       # target 1 leaves: its slot misses, and is retired
    model, kw, motion = SM.make(case, "table", dev)
    got, trk = tracking.evaluate_managed_scene(model, frames, gt, valid, n_targets=K, manage=SM.MANAGE, mot=dict(max_dist=3.0), **kw)
    assert isinstance(trk, tracking.ManagedMotionSceneTracker if motion else tracking.ManagedSceneTracker) and trk.t == T
    ids = trk.events()[0]
    assert ids[0].tolist() == [0, 1, -1, -1] and ids.max() >= 2                             # target 2 was enrolled from its detection
    want, rows = oracle_of(trk, gt, valid, max_dist=3.0)
    assert_same(got, want, case)
    invariants(got)
    assert got["frames"] == T and got["gt"] == int(valid.sum()) and got["hyp"] == int((ids >= 0).sum()) and got["tp"] > 0
    # detections given by the caller: the same boxes, as a device tensor with counts
    order = np.argsort(valid == 0, axis=1, kind="stable")
    dets = torch.from_numpy(np.take_along_axis(gt, order[:, :, None], axis=1)).to(dev)
    again, trk2 = tracking.evaluate_managed_scene(model, frames, gt, valid, detections=dets, n_detections=valid.sum(1), n_targets=K,
                                                  manage=SM.MANAGE, mot=dict(max_dist=3.0), **kw)
    assert_same(again, got, case + ", detections passed")
    assert np.array_equal(SM.bits(trk2.results()), SM.bits(trk.results()))
    print("evaluate_managed_scene %s: %s" % (case, got))
