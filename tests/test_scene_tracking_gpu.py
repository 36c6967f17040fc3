"""K targets of one live scene, free-running, on the GPU (tracking.SceneTracker / MotionSceneTracker, track_scene,
evaluate_scene).

  sampling="table"    against MultiTargetTracker / MultiMotionTracker (sampling="reference") on the same scene from the same
                      boxes, closed loop: inputs, proposal, indices, boxes, results and counts torch.equal -- both loops run the
                      same batch-K network on the same inputs; also with reference_BB previous_gt, retire and set_box in
                      mid-sequence, with K = 33 (one more than a crop chunk), and through evaluate_scene
  sampling="device"   row k against a single free-running tracker, teacher-forced: inputs, counts and indices bit for bit, the
                      chosen proposal equal, the centre within FEATURE_BOUND (batch K and batch 1 take different GEMM paths)
  enroll              the enrolled slot against a single tracker initialised on the frame it was enrolled on; the others against
                      a run without the enrolment
  host stops          none after the first update(), no upload on a frame without an event; the control is MultiTargetTracker
  capacities          a cut is reported for the slot it happened in, and the cut row is still the single tracker's

Every tracker here has capacities of 4096 where nothing is meant to be cut (tests/test_table_sampling_gpu.py: the draw tables are
the cached 8 / 17 MB ones)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fixture_io  # noqa: E402
import motion_oracle as MO  # noqa: E402
import tracking_oracle as TO  # noqa: E402
import test_free_running_tracking_gpu as FR  # noqa: E402  (host_stops, the motion model of case kitti)
import test_lane_tracking_gpu as LT  # noqa: E402  (tbits)
import test_multi_tracking_gpu as MT  # noqa: E402  (the matching models by mode, turned, FEATURE_BOUND)

pytestmark = pytest.mark.gpu
tbits, bits, host_stops = LT.tbits, FR.bits, FR.host_stops
FEATURE_BOUND = MT.FEATURE_BOUND                   # 1e-4
CAP = 4096
MATCHING_KW = dict(search_capacity=CAP, model_capacity=CAP, bank_capacity=CAP)
MOTION_KW = dict(capacity=CAP)
MODES, MOTION = list(MT.MODES), list(MO.CASES)     # bat_fap, bat_first, bat_previous, bat_all, p2b; kitti, no_bc
FAR = 500.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_multi_tracking.npz"))


@pytest.fixture(scope="module")
def motion_gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_motion_tracking.npz"))


@pytest.fixture(scope="module")
def scene(gold, dev):
    """the matching fixture's scene: (frames on the device, gt (T,K,15) on the host, gt on the device)"""
    from open3dsot_amd import synth
    frames, gt = synth.make_scene(int(gold["scene_seed"]), int(gold["n_frames"]), int(gold["n_points"]), int(gold["n_targets"]))
    return [torch.from_numpy(f).to(dev) for f in frames], gt, torch.from_numpy(gt).to(dev)


def far(box):
    b = np.array(box, np.float32)
    b[0] += FAR
    return b


def motion_targets(box):
    """three pairwise different targets: the box, the box shifted and turned a little (other crops), the box 500 m away (empty
    crops, zero-filled inputs)"""
    return np.stack([np.asarray(box, np.float32), MT.turned(box, 0.3, 10.0), far(box)])


def motion_scene(motion_gold, case, dev):
    """-> (frames on the device, gt (T,15) of the fixture's target)"""
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(int(motion_gold[case + ".seq_seed"]), MO.SEQ_FRAMES, MO.SEQ_POINTS)
    return [torch.from_numpy(f).to(dev) for f in frames], gt


_MOTION_MODELS = {}


def motion_model(case, dev):
    if case == FR.MOTION:
        return FR.make_model(case, dev)
    if case not in _MOTION_MODELS:
        from open3dsot_amd import m2track
        cfg = MO.case_config(case)
        _MOTION_MODELS[case] = (MO.init_weights(m2track.M2TRACK(**cfg)).to(dev).eval(), cfg)
    return _MOTION_MODELS[case]


def previous_gt_model(dev):
    from open3dsot_amd import trackers
    cfg = dict(trackers.BAT_CAR)
    cfg.update(MT.KEYS)
    cfg["reference_BB"] = "previous_gt"
    return TO.init_weights(trackers.get_model("BAT")(trackers.make_config(cfg))).to(dev).eval()


def drawn(n, S):
    """tracking.draw_indices(n, S) as the (S,) int32 array `used` must hold (-1: the zero-fill case)"""
    from open3dsot_amd import tracking
    idx = tracking.draw_indices(int(n), S)
    return np.full((S,), -1, np.int32) if idx is None else idx.astype(np.int32)


def same_inputs(a, b, what, rows=None):
    assert sorted(a.inputs) == sorted(b.inputs)
    for name in a.inputs:
        x, y = (a.inputs[name], b.inputs[name]) if rows is None else (a.inputs[name][rows], b.inputs[name][rows])
        assert torch.equal(tbits(x), tbits(y)), (what, name)


# ---- 5. "table" equals the reference K-target loops, closed loop --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_table_scene_equals_the_multi_target_tracker_closed_loop(dev, scene, mode):
    from open3dsot_amd import tracking
    model, _ = MT.make_model(mode, dev)
    frames, gt, _ = scene
    T, K = gt.shape[:2]
    scn = tracking.SceneTracker(model, K, sampling="table", record_indices=True, **MATCHING_KW)
    ref = tracking.MultiTargetTracker(model, K)
    assert scn.free_running and scn.tabled and scn.lanes.shape == (K, 7)
    for trk in (scn, ref):
        assert trk.init(frames[0], gt[0]).shape == (K, 15)
    M, N = int(scn.template_size), int(scn.search_size)
    want_counts = [[[-1, -1]] * K]
    for t in range(1, T):
        a, b = scn.update(frames[t]), ref.update(frames[t])
        same_inputs(scn, ref, (mode, t))
        assert torch.equal(scn.out[1], ref.out[1]), (mode, t)                              # the chosen proposal
        ns, nm, nt = ref.log[-1]
        assert scn.bank_state[t & 1, :, 1].cpu().tolist() == [int(v) for v in nt], (mode, t)
        for k in range(K):
            assert np.array_equal(scn.used_t[k].cpu().numpy(), drawn(nt[k], M)), (mode, t, k)
            assert np.array_equal(scn.used_s[k].cpu().numpy(), drawn(ns[k], N)), (mode, t, k)
        assert a.shape == (K, 15) and torch.equal(tbits(a), tbits(b)), (mode, t)
        want_counts.append([[int(ns[k]), -1 if nm is None else int(nm[k])] for k in range(K)])
    res = scn.results()
    assert res.shape == (T, K, 15) and np.array_equal(bits(res), bits(ref.results()))
    counts = scn.counts()
    assert counts.shape == (T, K, 2) and counts.dtype == np.int32 and counts.tolist() == want_counts
    assert scn.overflow() == (0, 0, 0) and not scn.overflow(per_target=True).any() and scn.log == []
    assert scn.crop_calls == T - 1 and scn.lane_uploads == 2                               # t = 1, and the frame after it
    assert np.abs(res[1:, :, :3] - res[:-1, :, :3]).max() > 1e-3                           # the boxes do move
    print("scene table %s: counts of frame 1 %s; graphs %s" % (mode, counts[1].tolist(), [scn.graph is not None, ref.graph is not None]))


@pytest.mark.parametrize("case", MOTION)
def test_table_motion_scene_equals_the_multi_motion_tracker_closed_loop(dev, motion_gold, case):
    from open3dsot_amd import tracking
    model, _ = motion_model(case, dev)
    frames, gt = motion_scene(motion_gold, case, dev)
    boxes0 = motion_targets(gt[0])
    K, T = 3, len(frames)
    scn = tracking.MotionSceneTracker(model, K, sampling="table", record_indices=True, **MOTION_KW)
    ref = tracking.MultiMotionTracker(model, K)
    for trk in (scn, ref):
        trk.init(frames[0], boxes0)
    N = int(scn.point_sample_size)
    want_counts = [[[-1, -1]] * K]
    for t in range(1, T):
        a, b = scn.update(frames[t]), ref.update(frames[t])
        same_inputs(scn, ref, (case, t))
        n_prev, n_this = ref.log[-1]
        for k in range(K):
            assert np.array_equal(scn.used[k].cpu().numpy(), np.concatenate([drawn(n_prev[k], N), drawn(n_this[k], N)])), (case, t, k)
        assert torch.equal(tbits(a), tbits(b)), (case, t)
        want_counts.append([[int(n_prev[k]), int(n_this[k])] for k in range(K)])
    assert np.array_equal(bits(scn.results()), bits(ref.results()))
    counts = scn.counts()
    assert counts.tolist() == want_counts and scn.overflow() == (0, 0, 0)
    # three pairwise different rows: a swapped stride would show
    assert counts[1, 0].tolist() != counts[1, 1].tolist() and min(counts[1, 0]) > 2 and min(counts[1, 1]) > 2
    assert counts[1:, 2].max() == 0 and not bool(scn.inputs["points"][2, :, :3].any())


# ---- 6. reference boxes from the caller, retire and set_box in mid-sequence ---------------------------------------------------------
def test_table_scene_with_previous_gt_retire_and_set_box(dev, scene):
    from open3dsot_amd import tracking
    model = previous_gt_model(dev)
    frames, gt, gt_dev = scene
    T, K = gt.shape[:2]
    scn = tracking.SceneTracker(model, K, sampling="table", **MATCHING_KW)
    ref = tracking.MultiTargetTracker(model, K)
    for trk in (scn, ref):
        trk.init(frames[0], gt[0])
    with pytest.raises(ValueError, match="ref_boxes"):
        scn.update(frames[1])
    moved = MT.turned(gt[3, 0], 0.2, 5.0)
    for t in range(1, T):
        mine = gt_dev[t - 1].clone()
        a, b = scn.update(frames[t], ref_boxes=mine), ref.update(frames[t], ref_boxes=gt[t - 1])
        assert torch.equal(tbits(mine), tbits(gt_dev[t - 1]))                               # the caller's tensor is read only
        same_inputs(scn, ref, t)
        assert torch.equal(tbits(a), tbits(b)), t
        if t == 2:
            for trk in (scn, ref):
                trk.retire(1)
        if t == 3:
            for trk in (scn, ref):
                trk.set_box(0, moved)
    res = scn.results()
    assert np.array_equal(bits(res), bits(ref.results()))
    assert all(np.array_equal(bits(res[t, 1]), bits(res[2, 1])) for t in range(3, T))       # the retired row ignores ref_boxes
    assert not np.array_equal(bits(gt[2, 1]), bits(res[2, 1])) and np.array_equal(bits(res[3, 0]), bits(moved))
    assert scn.counts()[1:, :, 0].tolist() == [[int(v) for v in e[0]] for e in ref.log]


# ---- 7. "device": row k is the single free-running tracker's ------------------------------------------------------------------------
def assert_matching_row(scn, k, one, box, sbox, what, with_model_crop):
    """slot k of a SceneTracker after a frame against a SequenceTracker after the same frame -> the centre difference"""
    for name in one.inputs:
        assert torch.equal(tbits(scn.inputs[name][k]), tbits(one.inputs[name][0])), (what, name)
    n = 2 if with_model_crop else 1
    assert torch.equal(scn.counts2[k, :n], one.counts_dev[:n]), what
    assert torch.equal(scn.used_t[k], one.used_t) and torch.equal(scn.used_s[k], one.used_s), what
    assert int(scn.out[1][k].item()) == int(one.out[1].item()), what                        # the chosen proposal
    d = float((box[:3] - sbox[:3]).abs().max())
    assert d <= FEATURE_BOUND, (what, d)
    assert torch.equal(tbits(box[3:6]), tbits(sbox[3:6])), what
    return d


@pytest.mark.parametrize("mode", ["bat_fap", "bat_first", "p2b"])
def test_device_scene_rows_are_the_single_free_running_trackers(gold, dev, scene, mode):
    from open3dsot_amd import tracking
    model, _ = MT.make_model(mode, dev)
    frames, gt, _ = scene
    T, K = gt.shape[:2]
    kw = dict(sampling="device", seed=5, record_indices=True, use_graph=False, **MATCHING_KW)
    scn = tracking.SceneTracker(model, K, **kw)
    assert not scn.limit_box and scn.keys == tracking.draw_keys(5)
    scn.init(frames[0], gt[0])
    singles = [tracking.SequenceTracker(model, **kw) for _ in range(K)]
    for k, s in enumerate(singles):
        s.init(frames[0], gt[0, k])
    worst = 0.0
    for t in range(1, T):
        for k, s in enumerate(singles):
            teacher = gold["t%d.f%d.ref_box" % (k, t)]
            scn.set_box(k, teacher)
            s.set_box(teacher)
        boxes = scn.update(frames[t])
        for k, s in enumerate(singles):
            sbox = s.update(frames[t])
            worst = max(worst, assert_matching_row(scn, k, s, boxes[k], sbox, (mode, t, k), t == 1 or scn.aggregation != "first"))
            assert torch.equal(scn.bank_state[t & 1, k], s.bank_state[t & 1]), (mode, t, k)
    print("scene device %s: worst centre difference to the single trackers %.2e m" % (mode, worst))
    counts = scn.counts()
    for k, s in enumerate(singles):
        assert counts[:, k].tolist() == s.counts().tolist(), (mode, k)
    assert scn.overflow() == (0, 0, 0)


def assert_motion_row(scn, k, one, box, sbox, what):
    for name in one.inputs:
        assert torch.equal(tbits(scn.inputs[name][k]), tbits(one.inputs[name][0])), (what, name)
    assert torch.equal(scn.counts2[k], one.counts_dev) and torch.equal(scn.used[k], one.used), what
    d = float((box[:3] - sbox[:3]).abs().max())
    assert d <= FEATURE_BOUND, (what, d)
    assert torch.equal(tbits(box[3:6]), tbits(sbox[3:6])), what
    return d


@pytest.mark.parametrize("case", MOTION)
def test_device_motion_scene_rows_are_the_single_free_running_trackers(dev, motion_gold, case):
    from open3dsot_amd import tracking
    model, _ = motion_model(case, dev)
    frames, gt = motion_scene(motion_gold, case, dev)
    K, T = 3, len(frames)
    kw = dict(sampling="device", seed=5, record_indices=True, use_graph=False, **MOTION_KW)
    scn = tracking.MotionSceneTracker(model, K, **kw)
    assert not scn.limit_box
    scn.init(frames[0], motion_targets(gt[0]))
    singles = [tracking.MotionSequenceTracker(model, **kw) for _ in range(K)]
    for s, box in zip(singles, motion_targets(gt[0])):
        s.init(frames[0], box)
    worst = 0.0
    for t in range(1, T):
        teacher = motion_targets(motion_gold["%s.f%d.ref_box" % (case, t)])
        for k, s in enumerate(singles):
            scn.set_box(k, teacher[k])
            s.set_box(teacher[k])
        boxes = scn.update(frames[t])
        for k, s in enumerate(singles):
            worst = max(worst, assert_motion_row(scn, k, s, boxes[k], s.update(frames[t]), (case, t, k)))
    print("motion scene device %s: worst centre difference to the single trackers %.2e m" % (case, worst))
    counts = scn.counts()
    for k, s in enumerate(singles):
        assert counts[:, k].tolist() == s.counts().tolist(), (case, k)
    assert scn.overflow() == (0, 0, 0)


# ---- 8. enroll --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,sampling", [("bat_fap", "table"), ("bat_all", "device")])
def test_enroll_starts_a_slot_as_init_starts_a_single_tracker(gold, dev, scene, mode, sampling):
    """slot 2 holds a far-away dummy box until it is enrolled on the fixture's target 2 after frame 2; teacher-forced"""
    from open3dsot_amd import tracking
    model, _ = MT.make_model(mode, dev)
    frames, gt, gt_dev = scene
    T, K, E = gt.shape[0], gt.shape[1], 2
    kw = dict(sampling=sampling, seed=3, record_indices=True, use_graph=False, **MATCHING_KW)
    boxes0 = np.stack([gt[0, 0], gt[0, 1], far(gt[0, 2])])
    scn, plain = tracking.SceneTracker(model, K, **kw), tracking.SceneTracker(model, K, **kw)
    for trk in (scn, plain):
        trk.init(frames[0], boxes0)
    one = tracking.SequenceTracker(model, **kw)
    worst = 0.0
    for t in range(1, T):
        for k in (0, 1):
            for trk in (scn, plain):
                trk.set_box(k, gold["t%d.f%d.ref_box" % (k, t)])
        if t > E:
            teacher = gold["t2.f%d.ref_box" % t]
            scn.set_box(2, teacher)
            one.set_box(teacher)
        boxes, want = scn.update(frames[t]), plain.update(frames[t])
        same_inputs(scn, plain, (mode, t, "the other slots"), rows=slice(0, 2))
        assert torch.equal(scn.counts2[:2], plain.counts2[:2]) and torch.equal(scn.used_t[:2], plain.used_t[:2])
        assert torch.equal(scn.used_s[:2], plain.used_s[:2]) and torch.equal(scn.bank_state[t & 1, :2], plain.bank_state[t & 1, :2])
        assert torch.equal(tbits(boxes[:2]), tbits(want[:2])), (mode, t)
        if t <= E:
            assert int(scn.counts2[2, 0]) == 0 and not bool(scn.inputs["search_points"][2].any())      # the dummy: empty crops
        else:
            sbox = one.update(frames[t])
            worst = max(worst, assert_matching_row(scn, 2, one, boxes[2], sbox, (mode, t, "enrolled"), True))
            assert torch.equal(scn.bank_state[t & 1, 2], one.bank_state[(t - E) & 1]), (mode, t)
            if t == E + 1:                                     # the bank's `first` branch after an empty restart
                nm, total = int(scn.counts2[2, 1]), int(scn.bank_state[t & 1, 2, 1])
                assert nm > 2 and total == (2 * nm if mode == "bat_fap" else nm), (mode, nm, total)
        if t == E:
            box = gt_dev[E, 2] if sampling == "table" else gt[E, 2]                     # a device box, a host box
            scn.enroll(2, box)
            one.init(frames[E], gt[E, 2])
            assert torch.equal(tbits(scn.boxes[E, 2]), tbits(gt_dev[E, 2])) and torch.equal(tbits(scn.canon_wlh[2]), tbits(gt_dev[E, 2, 3:6]))
    print("enroll %s / %s: worst centre difference of the enrolled slot to its single tracker %.2e m" % (mode, sampling, worst))
    res, single = scn.results(), one.results()
    assert np.array_equal(bits(res[:, :2]), bits(plain.results()[:, :2]))
    # (row E of slot 2 was the enrolled box, asserted above, until the teacher's set_box before frame E + 1 replaced it)
    assert np.array_equal(bits(res[E, 2]), bits(single[0])) and np.abs(res[E + 1:, 2, :3] - single[1:, :3]).max() <= FEATURE_BOUND
    assert scn.counts()[E + 1:, 2].tolist() == one.counts()[1:].tolist()
    assert scn.overflow() == (0, 0, 0) and scn._start.tolist() == [0, 0, E]
    assert scn.lane_uploads == 4 and plain.lane_uploads == 2                              # t = 1, the frame after; enroll, the frame after


def test_enroll_motion_slot_takes_the_first_frame_prior(dev, motion_gold):
    from open3dsot_amd import tracking
    case, E = FR.MOTION, 2
    model, _ = motion_model(case, dev)
    frames, gt = motion_scene(motion_gold, case, dev)
    T, K = len(frames), 3
    kw = dict(sampling="device", seed=3, record_indices=True, use_graph=False, **MOTION_KW)
    scn, plain = tracking.MotionSceneTracker(model, K, **kw), tracking.MotionSceneTracker(model, K, **kw)
    for trk in (scn, plain):
        trk.init(frames[0], motion_targets(gt[0]))
    one = tracking.MotionSequenceTracker(model, **kw)
    N = int(scn.point_sample_size)
    for t in range(1, T):
        teacher = motion_targets(motion_gold["%s.f%d.ref_box" % (case, t)])
        for k in (0, 1):
            for trk in (scn, plain):
                trk.set_box(k, teacher[k])
        if t > E:
            scn.set_box(2, teacher[0])
            one.set_box(teacher[0])
        boxes, want = scn.update(frames[t]), plain.update(frames[t])
        same_inputs(scn, plain, (t, "the other slots"), rows=slice(0, 2))
        assert torch.equal(scn.counts2[:2], plain.counts2[:2]) and torch.equal(scn.used[:2], plain.used[:2])
        assert torch.equal(tbits(boxes[:2]), tbits(want[:2])), t
        prior = set(scn.inputs["points"][2, :N, 4].cpu().tolist())
        for k in (0, 1):
            assert set(scn.inputs["points"][k, :N, 4].cpu().tolist()) == ({0.0, 1.0} if t == 1 else {np.float32(0.8).item(), np.float32(0.2).item()}), (t, k)
        if t > E:
            assert_motion_row(scn, 2, one, boxes[2], one.update(frames[t]), (t, "enrolled"))
            assert prior == ({0.0, 1.0} if t == E + 1 else {np.float32(0.8).item(), np.float32(0.2).item()}), (t, prior)
        if t == E:
            scn.enroll(2, gt[E])
            one.init(frames[E], gt[E])
    assert np.array_equal(bits(scn.results()[:, :2]), bits(plain.results()[:, :2]))
    assert scn.counts()[E + 1:, 2].tolist() == one.counts()[1:].tolist()
    assert scn.overflow(per_target=True).tolist() == [[0, 0, 0]] * K and scn._start.tolist() == [0, 0, E]


# ---- 9. no host stop and no upload --------------------------------------------------------------------------------------------------
def count_uploads(monkeypatch, log, stamp):
    """every Tensor.copy_ whose source is a CPU tensor and whose destination is on the GPU appends stamp() to `log` (undone
    by host_stops' exit)"""
    real = torch.Tensor.copy_

    def counted(self, src, *a, **k):
        if torch.is_tensor(src) and not src.is_cuda and self.is_cuda:
            log.append(stamp())
        return real(self, src, *a, **k)
    monkeypatch.setattr(torch.Tensor, "copy_", counted)


@pytest.mark.parametrize("which", ["bat_fap", FR.MOTION])
def test_no_host_stop_and_no_upload_on_a_frame_without_an_event(dev, scene, motion_gold, which, monkeypatch):
    from open3dsot_amd import tracking
    if which == FR.MOTION:
        model, _ = motion_model(which, dev)
        frames, gt1 = motion_scene(motion_gold, which, dev)
        boxes0, K, kw = motion_targets(gt1[0]), 3, MOTION_KW
        new_box = torch.from_numpy(gt1[3]).to(dev)
    else:
        model, _ = MT.make_model(which, dev)
        frames, gt, gt_dev = scene
        boxes0, K, kw = gt[0], gt.shape[1], MATCHING_KW
        new_box = gt_dev[3, 2].clone()
    T = len(frames)
    trk = tracking.scene_tracker_for(model, K, sampling="table", use_graph=True, **kw)
    trk.init(frames[0], boxes0)
    trk.update(frames[1])                                  # the capture may synchronise
    uploads = []
    with host_stops(monkeypatch) as stops:
        count_uploads(monkeypatch, uploads, lambda: trk.t)
        for t in range(2, T):
            trk.update(frames[t])
            if t == 3:
                trk.retire(0)
                trk.enroll(2, new_box)                     # a device box: no copy at all
    assert stops.calls == [], stops.calls
    # frame 2 follows the first frame, frame 4 an enroll, frame 5 a slot's first frame: the lane table, once each; nothing else
    assert uploads == [2, 4, 5], uploads
    assert trk.graph is not None and trk.lane_uploads == 4 and np.isfinite(trk.results()).all()
    # the control: the reference K-target loop under the same harness stops once per frame at least
    ref = tracking.multi_tracker_for(model, K, use_graph=True)
    ref.init(frames[0], boxes0)
    ref.update(frames[1])
    with host_stops(monkeypatch) as stops:
        for t in range(2, T):
            ref.update(frames[t])
    assert len(stops.calls) >= T - 2 and "synchronize" in stops.calls


# ---- 10. fixed capacities cut and report --------------------------------------------------------------------------------------------
def test_a_cut_is_reported_for_its_slot_and_the_row_is_still_the_single_trackers(gold, dev, scene):
    from open3dsot_amd import tracking
    model, _ = MT.make_model("bat_fap", dev)
    frames, gt, _ = scene
    T, SMALL = gt.shape[0], 1000                           # frame 1 of target 0: 1419 search points, a model crop of 1270
    assert gold["t0.f1.counts"].tolist() == [1419, 2540]
    kw = dict(sampling="device", seed=1, record_indices=True, use_graph=False, search_capacity=SMALL, model_capacity=SMALL)
    scn, one = tracking.SceneTracker(model, 2, **kw), tracking.SequenceTracker(model, **kw)
    scn.init(frames[0], np.stack([gt[0, 0], far(gt[0, 0])]))
    one.init(frames[0], gt[0, 0])
    for t in range(1, T):
        teacher = gold["t0.f%d.ref_box" % t]
        scn.set_box(0, teacher)
        one.set_box(teacher)
        boxes = scn.update(frames[t])
        assert_matching_row(scn, 0, one, boxes[0], one.update(frames[t]), t, True)
        if t == 1:
            assert scn.bank_state[1, 0].cpu().tolist() == [SMALL, 2 * SMALL]               # the cut crop, twice
    counts, per = scn.counts(), scn.overflow(per_target=True)
    assert counts[1, 0].tolist() == [1419, 1270] and counts[1:, 1].max() == 0             # counted in full; the far slot stays empty
    assert per.shape == (2, 3) and per[0, 0] >= 1 and per[0, 1] >= 1 and per[1].tolist() == [0, 0, 0], per
    assert scn.overflow() == tuple(int(v) for v in per.sum(0)) == one.overflow()


# ---- 11. graph replay equals eager; two trackers on one model -----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bat_fap", FR.MOTION])
def test_graph_replay_equals_eager_and_a_second_tracker_does_not_disturb_the_first(dev, scene, motion_gold, which):
    from open3dsot_amd import tracking
    if which == FR.MOTION:
        model, _ = motion_model(which, dev)
        frames, gt1 = motion_scene(motion_gold, which, dev)
        boxes_a, kw = motion_targets(gt1[0]), MOTION_KW
    else:
        model, _ = MT.make_model(which, dev)
        frames, gt, _ = scene
        boxes_a, kw = gt[0], MATCHING_KW
    boxes_b = np.ascontiguousarray(boxes_a[[1, 2, 0]])
    T, K = len(frames), 3
    eager = tracking.track_scene(model, frames, boxes_a, use_graph=False, sampling="table", **kw)
    graph = tracking.track_scene(model, frames, boxes_a, use_graph=True, sampling="table", **kw)
    assert eager.shape == (T, K, 15) and np.array_equal(bits(graph), bits(eager))
    assert not np.array_equal(eager[1], eager[0])
    solo_b = tracking.track_scene(model, frames, boxes_b, use_graph=True, sampling="table", **kw)
    ta, tb = (tracking.scene_tracker_for(model, K, use_graph=True, sampling="table", **kw) for _ in range(2))
    ta.init(frames[0], boxes_a)
    tb.init(frames[0], boxes_b)
    for t in range(1, T):
        ta.update(frames[t])
        tb.update(frames[t])
    assert ta.graph is not None and tb.graph is not None
    assert np.array_equal(bits(ta.results()), bits(graph)) and np.array_equal(bits(tb.results()), bits(solo_b))
    assert not np.array_equal(solo_b, graph)


# ---- 12. K across a crop chunk ------------------------------------------------------------------------------------------------------
def test_33_targets_cross_a_crop_chunk(dev, scene):
    from open3dsot_amd import points_utils as PU, tracking
    model, _ = MT.make_model("bat_fap", dev)
    frames, gt, _ = scene
    K = PU.CROP_MULTI_CHUNK + 1
    assert K == 33
    boxes0 = np.stack([MT.turned(gt[0, j % 3], 0.05 * (j // 3), 0.0) for j in range(K)])
    scn = tracking.SceneTracker(model, K, sampling="table", use_graph=False, **MATCHING_KW)
    ref = tracking.MultiTargetTracker(model, K, use_graph=False)
    for trk in (scn, ref):
        trk.init(frames[0], boxes0)
    rows = [0, 31, 32]
    for t in (1, 2):
        a, b = scn.update(frames[t]), ref.update(frames[t])
        same_inputs(scn, ref, t, rows=rows)
        assert torch.equal(tbits(a[rows]), tbits(b[rows])), t
        assert scn.counts()[t, rows, 0].tolist() == [int(ref.log[-1][0][k]) for k in rows]
    assert np.array_equal(bits(scn.results()[:, rows]), bits(ref.results()[:, rows])) and scn.overflow() == (0, 0, 0)
    assert scn.counts()[1, 31].tolist() != scn.counts()[1, 32].tolist()                    # different rows on either side of the chunk


# ---- 13. evaluate_scene -------------------------------------------------------------------------------------------------------------
def test_evaluate_scene_returns_what_evaluate_targets_returns(dev, scene):
    from open3dsot_amd import metrics, tracking
    model, _ = MT.make_model("bat_fap", dev)
    frames, gt, _ = scene
    T, K = gt.shape[:2]
    valid = np.ones((T, K), np.int32)
    valid[4:, 1] = 0                                       # target 1 loses its annotation at frame 4: retired there
    ma, mb = metrics.SuccessPrecision(device=dev), metrics.SuccessPrecision(device=dev)
    got = tracking.evaluate_scene(model, frames, gt, valid=valid, metrics=ma, sampling="table", **MATCHING_KW)
    want = tracking.evaluate_targets(model, frames, gt, valid=valid, metrics=mb)
    for g, w, shape in zip(got, want, ((T, K), (T, K), (T, K, 15))):
        assert tuple(g.shape) == shape and torch.equal(tbits(g), tbits(w))
    a, b = ma.compute(), mb.compute()
    assert a == b and a["frames"] == T * K - (T - 4), (a, b)
    res = got[2].cpu().numpy()
    assert all(np.array_equal(bits(res[t, 1]), bits(res[3, 1])) for t in range(4, T))
