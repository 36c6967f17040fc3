"""The managed scene trackers end to end on the GPU (tracking.ManagedSceneTracker / ManagedMotionSceneTracker; DESIGN.md section
12j), on the fixture scene of ref_multi_tracking.npz (3 targets, 6 frames).

The scenario.  K = 4 slots, init with the ground truth of targets 0 and 1, max_misses = 1, max_dist = 3.  A plain SceneTracker
runs every frame first; its boxes are read back and the frame's detections are copies of them (a copy has overlap 1 and distance
0 and therefore matches its track, whatever the random-weight network does), then the managed tracker runs the frame with these
detections.  Target 2's ground-truth box is added at frame 1, slot 1's detection is left out from frame 2 on, and a box 500 m away
is added at frame 3.  Every new detection is farther than 20 m from every track box (asserted), so the decisions are fixed by
construction: slot 2 is enrolled at frame 1, slot 1 is retired at frame 3 and taken by the far box in the same call, slot 3 is
never used.  The plain tracker makes exactly these decisions with host calls (retire / enroll); the two must then agree bit for
bit.  What is compared on which slots: boxes, yaw state, canonical wlh, `active`, results() and counts() on all K slots; every
network input and bank_state on the slots that follow an object; on the FREE slots the inputs that `first` does not enter -- the
search input on every frame (matching trackers), every input from frame 2 on (motion tracker).  A free slot's template input and
its bank_state row are never compared: at frame 1 the plain tracker's init marks all K slots `first`, the managed one the occupied
slots only, so the unit box's model crop (1 point here) is banked by another branch and the bank's `fixed` differs from then on;
the motion tracker's prior-targetness column shows the same flag at frame 1.  Both trackers share one model and run interleaved:
neither disturbs the other."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fixture_io  # noqa: E402
import scene_manage_oracle as SO  # noqa: E402
import test_free_running_tracking_gpu as FR  # noqa: E402  (host_stops, bits, the motion model of case kitti)
import test_multi_tracking_gpu as MT  # noqa: E402  (the matching models by mode)

pytestmark = pytest.mark.gpu
bits, host_stops = FR.bits, FR.host_stops
CAP, K, FAR = 4096, 4, 500.0
MANAGE = dict(max_misses=1, max_dist=3.0)
CASES = [("bat_fap", "table"), ("bat_first", "device"), (FR.MOTION, "table")]


def tbits(t):
    return t.contiguous().view(torch.int32)


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


def test_the_fixture_targets_are_far_apart(scene):
    _, gt = scene
    for t in range(gt.shape[0]):
        d = np.linalg.norm(gt[t, :, None, :3] - gt[t, None, :, :3], axis=-1)[np.triu_indices(3, 1)]
        assert d.min() > 20.0 and d.max() < 60.0, (t, d)


def make(case, sampling, dev, **kw):
    """-> (model, the keywords of both trackers, is it the motion case)"""
    motion = case == FR.MOTION
    model = FR.make_model(case, dev)[0] if motion else MT.make_model(case, dev)[0]
    caps = dict(capacity=CAP) if motion else dict(search_capacity=CAP, model_capacity=CAP, bank_capacity=CAP)
    return model, dict(sampling=sampling, seed=2, **caps, **kw), motion


def far_box(gt):
    b = np.array(gt[3, 0], np.float32)
    b[0] += FAR
    return b


def plain_tracker(model, kw, frames, gt):
    """a plain scene tracker in the managed tracker's initial state: free slots hold the unit box and are retired"""
    from open3dsot_amd import tracking
    plain = tracking.scene_tracker_for(model, K, **kw)
    plain.init(frames[0], np.stack([gt[0, 0], gt[0, 1], tracking._unit_box(), tracking._unit_box()]))
    plain.retire(2)
    plain.retire(3)
    return plain


def frame_detections(t, pb, gt):
    """the frame's detection set from the plain tracker's boxes pb (K,15) of frame t -> (dets (D,15), the new ones)"""
    new = {1: [gt[1, 2]], 3: [far_box(gt)]}.get(t, [])
    followed = [0, 1] if t < 2 else [0, 2] if t < 4 else [0, 1, 2]         # slot 1: left out from frame 2 on, the far object from 4 on
    return np.stack([pb[k] for k in followed] + new).astype(np.float32), new


def host_events(plain, t, gt):
    """the scenario's decisions as host calls on the plain tracker, after its frame t"""
    if t == 1:
        plain.enroll(2, gt[1, 2])
    if t == 3:
        plain.retire(1)
        plain.enroll(1, far_box(gt))


@pytest.mark.parametrize("case,sampling", CASES)
def test_managed_tracker_equals_the_host_driven_scene_tracker_and_the_oracle(dev, scene, case, sampling):
    from open3dsot_amd import points_utils as PU, tracking
    frames, gt = scene
    T = len(frames)
    model, kw, motion = make(case, sampling, dev)
    man = tracking.managed_scene_tracker_for(model, K, manage=MANAGE, **kw)
    assert isinstance(man, tracking.ManagedMotionSceneTracker if motion else tracking.ManagedSceneTracker)
    plain = plain_tracker(model, kw, frames, gt)
    first = man.init(frames[0], gt[0, :2])
    assert first.shape == (K, 15) and torch.equal(tbits(man.cur), tbits(plain.cur)) and torch.equal(man.active, plain.active)
    st = man.status()
    assert st["ids"].tolist() == [0, 1, -1, -1] and st["active"].tolist() == [1, 1, 0, 0]
    oracle = SO.new_state(K, man.boxes.shape[0], gt[0, :2], matching=not motion)
    occupied = [0, 1]
    zeros = np.zeros((K, 2), np.int32)
    rule = -1 if motion else PU.BANK_RULES[man.aggregation]
    for t in range(1, T):
        pb = plain.update(frames[t]).cpu().numpy()
        dets, new = frame_detections(t, pb, gt)
        live = np.flatnonzero(oracle["active"])
        for b in new:                                      # the scenario's premise
            assert np.linalg.norm(pb[live, :3] - b[None, :3], axis=1).min() > 20.0, t
        n_det = torch.tensor([len(dets)], dtype=torch.int32, device=dev) if t % 2 else None
        mb = man.update(frames[t], torch.from_numpy(dets).to(dev) if t != 2 else dets, n_det)      # frame 2: a host array
        host_events(plain, t, gt)
        # every network input and the bank, on the slots that followed an object through this frame
        assert sorted(man.inputs) == sorted(plain.inputs)
        for name in man.inputs:
            assert torch.equal(tbits(man.inputs[name][occupied]), tbits(plain.inputs[name][occupied])), (case, t, name)
        if not motion:                                     # all K slots where `first` does not enter (the module docstring)
            assert torch.equal(tbits(man.inputs["search_points"]), tbits(plain.inputs["search_points"])), (case, t, "free slots")
        elif t >= 2:
            for name in man.inputs:
                assert torch.equal(tbits(man.inputs[name]), tbits(plain.inputs[name])), (case, t, name, "free slots")
        occupied = {1: [0, 1, 2]}.get(t, occupied)
        if not motion:
            assert torch.equal(man.bank_state[:, occupied], plain.bank_state[:, occupied]), (case, t)
        assert mb.shape == (K, 15) and torch.equal(tbits(man.cur), tbits(plain.cur)), (case, t)
        assert torch.equal(tbits(man.yaw_state), tbits(plain.yaw_state)) and torch.equal(tbits(man.canon_wlh), tbits(plain.canon_wlh))
        assert torch.equal(man.active, plain.active), (case, t)
        # the oracle on the same inputs: the boxes of the frame, then steps 1 to 8
        oracle["cur"][live] = pb[live]
        oracle["results"][t] = oracle["cur"]
        oracle, _, _ = SO.step(oracle, dets, len(dets), zeros, t, dim=man.score_dim, up=man.score_up, rule=rule, **MANAGE)
        assert np.array_equal(bits(man.cur.cpu().numpy()), bits(oracle["cur"])), (case, t)
    res = man.results()
    assert res.shape == (T, K, 15) and np.array_equal(bits(res), bits(plain.results()))
    assert np.array_equal(bits(res), bits(oracle["results"][:T]))
    mc, pc = man.counts(), plain.counts()
    assert np.array_equal(mc[:, :, 0], pc[:, :, 0]) and (mc[1:] >= 0).all()
    logged = pc[:, :, 1] >= 0
    assert logged[1:].any() and np.array_equal(mc[:, :, 1][logged], pc[:, :, 1][logged])
    # the scenario's decisions, and the logs against the oracle
    ids, match, dropped = man.events()
    assert np.array_equal(ids, oracle["ids_log"][:T]) and np.array_equal(match, oracle["match_log"][:T])
    assert np.array_equal(dropped, oracle["dropped_log"][:T]) and not dropped.any()
    assert ids.tolist() == [[0, 1, -1, -1], [0, 1, 2, -1], [0, 1, 2, -1], [0, 3, 2, -1], [0, 3, 2, -1], [0, 3, 2, -1]]
    assert match[1:].tolist() == [[0, 1, -1, -1], [0, -1, 1, -1], [0, -1, 1, -1], [0, 1, 2, -1], [0, 1, 2, -1]]
    st = man.status()
    assert np.array_equal(st["active"], oracle["active"]) and st["active"].tolist() == [1, 1, 1, 0]
    assert np.array_equal(np.stack([st["ids"], st["misses"], st["starved"], st["start"]], 1), oracle["slot"])
    assert st["ids"].tolist() == [0, 3, 2, -1] and st["start"].tolist() == [0, 3, 1, 0]
    tracks = man.tracks()
    assert sorted(tracks) == [0, 1, 2, 3] and [tracks[i][0] for i in range(4)] == [0, 0, 1, 3]
    assert [len(tracks[i][1]) for i in range(4)] == [6, 3, 5, 3]
    assert np.array_equal(bits(tracks[1][1]), bits(res[:3, 1])) and np.array_equal(bits(tracks[3][1]), bits(res[3:, 1]))
    assert np.array_equal(bits(tracks[2][1][0]), bits(gt[1, 2])) and np.array_equal(bits(res[3, 1]), bits(far_box(gt)))
    assert man.overflow() == plain.overflow() and man._start.tolist() == [0, 3, 1, 0] == plain._start.tolist()
    assert np.abs(res[1:, 0, :3] - res[:-1, 0, :3]).max() > 1e-3                           # the boxes do move
    print("managed %s / %s: graphs %s, counts of frame 1 %s" % (case, sampling, [man.graph is not None, plain.graph is not None],
                                                               mc[1].tolist()))


def scripted(gt, dev):
    """detections known before the run: per frame t the ground truth of the 3 targets, on the device, with a device count"""
    return [(torch.from_numpy(np.ascontiguousarray(gt[t])).to(dev), torch.tensor([3], dtype=torch.int32, device=dev))
            for t in range(gt.shape[0])]


def test_graph_replay_equals_eager(dev, scene):
    from open3dsot_amd import tracking
    frames, gt = scene
    runs = []
    for use_graph in (False, True):
        model, kw, _ = make("bat_fap", "table", dev, use_graph=use_graph)
        man = tracking.ManagedSceneTracker(model, K, **kw)  # the default gates admit every pair: a track takes its nearest detection
        man.init(frames[0], gt[0, :2])
        for t, (dets, n) in enumerate(scripted(gt, dev)):
            if t:
                man.update(frames[t], dets, n)
        assert (man.graph is not None) == use_graph
        runs.append((man.results(), man.events(), man.status()))
    (ra, ea, sa), (rb, eb, sb) = runs
    assert np.array_equal(bits(ra), bits(rb)) and all(np.array_equal(x, y) for x, y in zip(ea, eb))
    assert all(np.array_equal(sa[k], sb[k]) for k in sa) and sa["ids"].tolist()[:3] == [0, 1, 2]      # target 2 was enrolled at frame 1
    assert not np.array_equal(ra[1], ra[0])


@pytest.mark.parametrize("case", ["bat_fap", FR.MOTION])
def test_no_host_stop_and_no_upload_with_device_detections(dev, scene, case, monkeypatch):
    from open3dsot_amd import tracking
    import test_scene_tracking_gpu as ST                   # count_uploads: the harness of the scene tracker's own test
    frames, gt = scene
    T = len(frames)
    model, kw, _ = make(case, "table", dev, use_graph=True)
    man = tracking.managed_scene_tracker_for(model, K, **kw)      # the default gates admit every pair: a track takes its nearest detection
    man.init(frames[0], gt[0, :2])
    dets = scripted(gt, dev)
    none_at = 4                                            # a frame without a detection set
    man.update(frames[1], dets[1][0][:2].contiguous(), dets[1][1])                          # the capture may synchronise
    uploads = []
    with host_stops(monkeypatch) as stops:
        ST.count_uploads(monkeypatch, uploads, lambda: man.t)
        for t in range(2, T):
            if t == none_at:
                man.update(frames[t])
            else:
                man.update(frames[t], dets[t][0], None if t == 3 else dets[t][1])           # frame 3: n_detections = D, an int fill
    assert stops.calls == [] and uploads == [], (stops.calls, uploads)
    assert man.graph is not None
    ids, match, _ = man.events()
    assert ids[1].tolist() == [0, 1, -1, -1] and ids[2].tolist() == [0, 1, 2, -1]            # target 2 was enrolled on the device at frame 2
    assert match[none_at].tolist() == [-1] * K and ids[none_at].tolist() == ids[none_at - 1].tolist()
    assert man.status()["misses"].tolist() == [0, 0, 0, 0]
    # the control: the plain tracker uploads its lane table after an enroll
    plain = plain_tracker(model, kw, frames, gt)
    plain.update(frames[1])
    uploads = []
    with host_stops(monkeypatch) as stops:
        ST.count_uploads(monkeypatch, uploads, lambda: plain.t)
        for t in range(2, T):
            plain.update(frames[t])
            if t == 2:
                plain.enroll(2, dets[2][0][2])
    assert stops.calls == [] and len(uploads) >= 2, uploads


def test_manual_enroll_and_retire_write_the_managed_state(dev, scene):
    from open3dsot_amd import tracking
    frames, gt = scene
    model, kw, _ = make("bat_fap", "table", dev)
    man = tracking.ManagedSceneTracker(model, K, manage=dict(enroll=False, max_misses=100), **kw)
    man.init(frames[0], gt[0, :2])
    man.update(frames[1])
    man.retire(0)
    man.enroll(3, gt[1, 2])
    st = man.status()
    assert st["active"].tolist() == [0, 1, 0, 1] and st["ids"].tolist() == [-1, 1, -1, 2] and st["start"].tolist() == [0, 0, 0, 1]
    assert man.lanes[:, :3].cpu().tolist() == [[1, 0, 1], [1, 0, 1], [1, 0, 1], [1, 1, 1]]
    assert man._pending == set() and int(man.next_id) == 3 and man.events()[0][1].tolist() == [0, 1, -1, 2]
    man.update(frames[2], gt[2])                           # enroll = False: the detections match or are ignored
    assert man.status()["ids"].tolist() == [-1, 1, -1, 2] and man.lanes[:, 1].cpu().tolist() == [0, 0, 0, 0]
    tracks = man.tracks()
    assert sorted(tracks) == [0, 1, 2] and tracks[2][0] == 1 and len(tracks[2][1]) == 2 and len(tracks[0][1]) == 2
    with pytest.raises(ValueError, match="ref_boxes"):
        man.update(frames[3], ref_boxes=gt[2])
    with pytest.raises(ValueError, match="max_detections"):
        tracking.ManagedSceneTracker(model, K, manage=dict(max_detections=0), **kw)
    with pytest.raises(ValueError, match="manage has no"):
        tracking.ManagedSceneTracker(model, K, manage=dict(max_miss=1), **kw)
