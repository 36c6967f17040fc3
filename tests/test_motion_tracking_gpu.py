"""The motion tracker's device-resident frame loop on the GPU: o3d_track_motion_input against its fp32 restatement
(tests/motion_oracle.py; xyz, time stamp and prior targetness bit for bit) and tracking.MotionSequenceTracker against the
reference's own run (tests/golden/ref_motion_tracking.npz), teacher-forced frame by frame and in closed loop."""
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

pytestmark = pytest.mark.gpu
COORD_BOUND, BC_BOUND = 2e-5, 1e-4        # tests/test_motion_tracking_cpu.py
FEATURE_BOUND = 1e-4                      # the project's bound on network outputs against the reference (relative to the largest entry)
CENTRE_BOUND = 1e-4 + 2e-5


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_motion_tracking.npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the kernel against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src", [3, 5000])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1024])
def test_motion_input_equals_the_oracle(dev, N, n_src):
    """both first_frame values, each zero flag, an index outside its source, candidate_bc NULL: xyz and the channels 3 and 4
    bit for bit, the BoxCloud within 1e-4 of its fp64 value"""
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng([N, n_src])
    wlh = (np.array([1.6, 3.9, 1.5]) * rng.uniform(0.9, 1.1, 3)).astype(np.float32)
    half = np.array([wlh[1], wlh[0], wlh[2]]) * 1.25 / 2
    prev = (rng.uniform(-1.6, 1.6, (n_src, 3)) * half).astype(np.float32)          # inside and outside the 1.25-scaled box
    cur = (rng.uniform(-1.6, 1.6, (n_src + 2, 3)) * half).astype(np.float32)
    prev[0] = [half[0], -half[1], half[2]]                                        # a row on the faces themselves (as fp32 rounds them)
    idx = np.concatenate([rng.integers(0, n_src, N), rng.integers(0, n_src + 2, N)]).astype(np.int32)
    idx[0] = 0
    bad = idx.copy()
    bad[N - 1], bad[2 * N - 1] = n_src, -1                                        # one past the end; negative
    tp, tc, tw = (torch.from_numpy(x).to(dev) for x in (prev, cur, wlh))
    seen = set()
    for first in (True, False):
        for zero in ((False, False), (True, False), (False, True), (True, True)):
            for ix in (idx, bad):
                for with_bc in (True, False):
                    pts = torch.full((2 * N, 5), -7.0, device=dev)
                    bc = torch.full((2 * N, 9), -7.0, device=dev)
                    got_p, got_b = PU.motion_input(None if zero[0] else tp, None if zero[1] else tc,
                                                   None if all(zero) else torch.from_numpy(ix).to(dev), tw, first, zero=zero,
                                                   out_points=pts, out_bc=bc if with_bc else False)
                    want_p, want_b = MO.motion_input(prev, cur, ix, N, wlh, first, zero=zero, with_bc=with_bc)
                    g = got_p.cpu().numpy()
                    assert got_p is pts and np.array_equal(bits(g), bits(want_p)), (first, zero, with_bc)
                    seen |= set(np.unique(g[:N, 4]).tolist())
                    if not with_bc:
                        assert got_b is None and bool((bc == -7.0).all())        # NULL: nothing written
                        continue
                    b = got_b.cpu().numpy()
                    assert np.abs(b[:N] - MO.boxcloud64(want_p[:N, :3], wlh)).max() <= BC_BOUND
                    assert np.abs(b - want_b).max() <= 2e-6 and not b[N:].any()
                    if zero[0]:                                                   # zero-filled: "inside", the BoxCloud of the origin
                        assert np.all(g[:N, 4] == np.float32(1.0 if first else 0.8)) and np.all(b[:N] == b[0])
    if N >= 255 and n_src == 5000:
        assert seen == {0.0, 1.0, np.float32(0.2).item(), np.float32(0.8).item()}
    a, _ = PU.motion_input(tp, tc, torch.from_numpy(idx).to(dev), tw, True)                    # the outputs allocated by the mirror
    assert a.shape == (2 * N, 5) and np.array_equal(bits(a.cpu().numpy()), bits(MO.motion_input(prev, cur, idx, N, wlh, True)[0]))


def test_points_in_box_and_transform_box_mirrors(dev):
    from open3dsot_amd import points_utils as PU, synth
    _, gt = synth.make_sequence(5, 2, 2000)
    rng = np.random.default_rng(1)
    b = gt[0].astype(np.float64)
    R = b[6:].reshape(3, 3)
    half = np.array([b[4], b[3], b[5]]) * 1.25 / 2
    q = rng.uniform(-1.5, 1.5, (3000, 3)) * half
    q = q[np.abs(MO.box_margin(q, half)) > 1e-4]
    pts = (q @ R.T + b[:3]).astype(np.float32)
    got = PU.points_in_box(torch.from_numpy(gt[0]).to(dev), torch.from_numpy(pts.T.copy()).to(dev), 1.25).cpu().numpy()
    want = MO.box_margin(q, half) > 0
    assert got.dtype == bool and 100 < want.sum() < want.size - 100 and np.array_equal(got, want)
    box = PU.unpack_box(torch.from_numpy(gt[0]).to(dev))
    c, s, r = PU.transform_box(box, box)                                           # the canonical box
    assert float(c.abs().max()) <= 1e-5 and torch.equal(s, box[1]) and float((r - torch.eye(3, device=dev)).abs().max()) <= 1e-6
    c, s, r = PU.transform_box(torch.from_numpy(gt[1]).to(dev), box)
    R1, c1 = gt[1][6:].reshape(3, 3).astype(np.float64), gt[1][:3].astype(np.float64)
    assert np.abs(c.cpu().numpy() - R.T @ (c1 - b[:3])).max() <= 1e-5 and np.abs(r.cpu().numpy() - R.T @ R1).max() <= 1e-6


# ---- the loop against the reference's run ------------------------------------------------------------------------------------
def make_model(case, dev):
    from open3dsot_amd import m2track
    cfg = MO.case_config(case)
    model = MO.init_weights(m2track.M2TRACK(**cfg))
    return model.to(dev).eval(), cfg


def sequence_of(gold, case, dev):
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(int(gold[case + ".seq_seed"]), MO.SEQ_FRAMES, MO.SEQ_POINTS)
    return [torch.from_numpy(f).to(dev) for f in frames], gt


class hard_masks:
    """The two hard-mask decisions of an M2-Track forward (torch.argmax of the segmentation logits per point and of the
    motion-state logits), recorded and -- with replay=True -- REPLACED by the reference's stored ones, under the rule of
    tests/test_golden_m2track.py::replay_hard_masks: a decision of the run under test may differ from the reference's only
    where the reference's stored margin is MO.TIE or less (asserted on exit).  `flipped`: the number of segmentation points
    that differed; `motion_flipped`: whether the motion-state decision did."""

    def __init__(self, gold, key, replay):
        self.g, self.k, self.replay, self.calls = gold, key, replay, 0
        self.flipped, self.motion_flipped, self.worst = 0, False, 0.0

    def __enter__(self):
        self.real = torch.argmax
        torch.argmax = self._hook
        return self

    def _hook(self, x, *a, **k):
        mine = self.real(x, *a, **k)
        which, self.calls = self.calls, self.calls + 1
        if which == 0:
            theirs = np.unpackbits(self.g[self.k + "seg_mask"])[:mine.numel()]
            margin = self.g[self.k + "seg_margin"]
        else:
            theirs, margin = np.atleast_1d(self.g[self.k + "motion_state"]), np.atleast_1d(self.g[self.k + "motion_margin"])
        t = torch.from_numpy(theirs.astype(np.int64)).reshape(mine.shape).to(mine.device)
        differ = (mine != t).reshape(-1).cpu().numpy()
        if differ.any():
            self.worst = max(self.worst, float(margin[differ].max()))
        if which == 0:
            self.flipped = int(differ.sum())
        else:
            self.motion_flipped = bool(differ.any())
        return t if self.replay else mine

    def __exit__(self, *exc):
        torch.argmax = self.real
        if exc[0] is None and self.replay:
            assert self.calls == 2, self.calls
            assert self.worst <= MO.TIE, ("a hard-mask decision differs from the reference's away from a tie", self.k, self.worst)
        return False


def frame_deviation(trk, est, box, gold, k, cfg):
    """-> the frame's deviations from the reference: points xyz, BoxCloud, estimation_boxes (relative), result centre"""
    N = cfg["point_sample_size"]
    pts, want = trk.inputs["points"][0].cpu().numpy(), gold[k + "points"]
    assert np.array_equal(pts[:, 3:], want[:, 3:]), k                               # time stamp and prior targetness: exact
    d = {"xyz": float(np.abs(pts[:, :3] - want[:, :3]).max())}
    if cfg["box_aware"]:
        bc = trk.inputs["candidate_bc"][0].cpu().numpy()
        assert not bc[N:].any()
        d["boxcloud"] = float(np.abs(bc[:N] - gold[k + "candidate_bc_prev"]).max())
    w = gold[k + "estimation_boxes"]
    d["estimation"] = float(np.abs(est.reshape(-1).cpu().numpy() - w).max() / max(1.0, np.abs(w).max()))
    d["centre"] = float(np.abs(box.cpu().numpy()[:3] - gold[k + "result_box"][:3]).max())
    return d


@pytest.mark.parametrize("case", list(MO.CASES))
def test_teacher_forced_frames_equal_the_reference(gold, dev, case):
    """every frame t starts from the reference's box t-1, the reference's hard masks replayed: counts equal, points <= 2e-5,
    BoxCloud <= 1e-4, estimation_boxes within the feature bound, the result centre within 1e-4 + 2e-5; over the case no more
    flipped segmentation points than the fixture's near-tie count"""
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    trk = tracking.MotionSequenceTracker(model, use_graph=False)
    trk.init(frames[0], gt[0])
    worst, flipped = {}, 0
    for t in range(1, MO.SEQ_FRAMES):
        k = "%s.f%d." % (case, t)
        trk.set_box(gold[k + "ref_box"])
        with hard_masks(gold, k, replay=True) as hm:
            box = trk.update(frames[t])
        flipped += hm.flipped
        assert list(trk.log[-1]) == gold[k + "counts"].tolist(), (case, t)
        d = frame_deviation(trk, trk.out, box, gold, k, cfg)
        print("%s frame %d:" % (case, t), {kk: "%.2e" % v for kk, v in d.items()}, "flipped", hm.flipped, hm.motion_flipped)
        assert d["xyz"] <= COORD_BOUND and d.get("boxcloud", 0.0) <= BC_BOUND, (case, t, d)
        assert d["estimation"] <= FEATURE_BOUND, (case, t, d)
        assert d["centre"] <= CENTRE_BOUND, (case, t, d)
        for kk, v in d.items():
            worst[kk] = max(worst.get(kk, 0.0), v)
    print("%s teacher-forced worst:" % case, {kk: "%.2e" % v for kk, v in worst.items()}, "flipped points", flipped)
    assert flipped <= int(gold[case + ".near_ties"]), (flipped, int(gold[case + ".near_ties"]))


def by_hand(model, cfg, frames, box0, dev):
    """the loop written with the public pieces, frame by frame"""
    from open3dsot_amd import points_utils as PU
    N = cfg["point_sample_size"]
    boxes = [PU.pack_box(box0, dev)]
    state = torch.cat([boxes[0][6:15], torch.zeros(1, device=dev)]).contiguous()
    idx = torch.arange(N, dtype=torch.int32, device=dev).repeat(2)
    for t in range(1, len(frames)):
        prev = PU.generate_subwindow(frames[t - 1], boxes[-1], cfg["bb_scale"], cfg["bb_offset"])
        this = PU.generate_subwindow(frames[t], boxes[-1], cfg["bb_scale"], cfg["bb_offset"])
        pp, _ = PU.regularize_pc(prev, N, seed=1)
        tp, _ = PU.regularize_pc(this, N, seed=1)
        pts, bc = PU.motion_input(pp.contiguous(), tp.contiguous(), idx, boxes[-1][3:6].contiguous(), t == 1,
                                  out_bc=None if cfg["box_aware"] else False)
        data = {"points": pts[None]}
        if cfg["box_aware"]:
            data["candidate_bc"] = bc[None]
        est = model.evaluate_one_sample(data)
        assert est.shape == (1, 4) and not est.requires_grad
        c, s, r = PU.getOffsetBB(PU.unpack_box(boxes[-1]), est[0], degrees=cfg["degrees"], use_z=cfg["use_z"],
                                 limit_box=cfg["limit_box"], frame=t, yaw_state=state)
        boxes.append(torch.cat([c, s, r.reshape(-1)]))
    return torch.stack(boxes).cpu().numpy()


@pytest.mark.parametrize("case", list(MO.CASES))
def test_track_sequence_equals_the_public_pieces_chained_by_hand(gold, dev, case):
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    eager = tracking.track_sequence(model, frames, gt[0], use_graph=False)
    hand = by_hand(model, cfg, frames, gt[0], dev)
    assert eager.shape == (MO.SEQ_FRAMES, 15) and np.array_equal(bits(eager), bits(hand))          # bit for bit
    graph = tracking.track_sequence(model, frames, gt[0], use_graph=True)
    assert np.array_equal(bits(graph), bits(eager))                                                 # replay == eager
    assert np.abs(eager[1:, :3] - eager[:-1, :3]).max() > 1e-3                                      # the box does move


@pytest.mark.parametrize("case", list(MO.CASES))
def test_closed_loop_follows_the_reference_trajectory(gold, dev, case):
    """No teacher, no replay: frame 1 under the teacher-forced bound when none of its decisions differs from the
    reference's; from frame 2 on the deviation compounds through the network and is MEASURED (printed;
    profiles/tracking_motion.txt holds a run's figures); the crop counts must equal the reference's up to the first frame whose
    hard masks differ from the reference's."""
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    trk = tracking.MotionSequenceTracker(model, use_graph=False)
    trk.init(frames[0], gt[0])
    dev_c, dev_r, first_flip = [], [], None
    for t in range(1, MO.SEQ_FRAMES):
        k = "%s.f%d." % (case, t)
        with hard_masks(gold, k, replay=False) as hm:
            box = trk.update(frames[t])
        if first_flip is None:
            assert list(trk.log[-1]) == gold[k + "counts"].tolist(), (case, t, dev_c)
            if hm.flipped or hm.motion_flipped:
                first_flip = t
        if t == 1 and first_flip is None:
            d = frame_deviation(trk, trk.out, box, gold, k, cfg)
            assert d["estimation"] <= FEATURE_BOUND and d["centre"] <= CENTRE_BOUND, d
        b, want = box.cpu().numpy(), gold[k + "result_box"]
        dev_c.append(float(np.abs(b[:3] - want[:3]).max()))
        dev_r.append(float(np.abs(b[6:] - want[6:]).max()))
    print("closed loop %s: centre deviation per frame 1..7 [m]: %s" % (case, " ".join("%.2e" % v for v in dev_c)))
    print("closed loop %s: rotation deviation per frame 1..7: %s" % (case, " ".join("%.2e" % v for v in dev_r)))
    print("closed loop %s: first frame with a hard-mask decision unlike the reference's: %s" % (case, first_flip))


def test_a_second_tracker_on_the_same_model_does_not_disturb_the_first(gold, dev):
    from open3dsot_amd import synth, tracking
    model, cfg = make_model("kitti", dev)
    fa, ga = sequence_of(gold, "kitti", dev)
    fb_np, gb = synth.make_sequence(77, MO.SEQ_FRAMES, MO.SEQ_POINTS)
    fb = [torch.from_numpy(f).to(dev) for f in fb_np]
    solo_a, solo_b = tracking.track_sequence(model, fa, ga[0]), tracking.track_sequence(model, fb, gb[0])
    ta, tb = tracking.MotionSequenceTracker(model), tracking.MotionSequenceTracker(model)
    ta.init(fa[0], ga[0])
    tb.init(fb[0], gb[0])
    for t in range(1, MO.SEQ_FRAMES):
        ta.update(fa[t])
        tb.update(fb[t])
    assert np.array_equal(bits(ta.results()), bits(solo_a)) and np.array_equal(bits(tb.results()), bits(solo_b))
    assert not np.array_equal(solo_a, solo_b)


def test_init_after_a_finished_sequence_starts_again_at_the_first_frame(gold, dev):
    from open3dsot_amd import tracking
    model, cfg = make_model("kitti", dev)
    frames, gt = sequence_of(gold, "kitti", dev)
    N = cfg["point_sample_size"]
    trk = tracking.MotionSequenceTracker(model, capacity=512)                     # smaller than the crops: the buffers grow
    trk.init(frames[0], gt[0])
    for t in range(1, 4):
        trk.update(frames[t])
    assert trk.crop_buf.shape[1] >= max(max(c) for c in trk.log)
    assert set(np.unique(trk.inputs["points"][0, :N, 4].cpu().numpy()).tolist()) <= {np.float32(0.2).item(), np.float32(0.8).item()}
    first = trk.results()
    trk.init(frames[0], gt[0])
    trk.update(frames[1])
    assert set(np.unique(trk.inputs["points"][0, :N, 4].cpu().numpy()).tolist()) <= {0.0, 1.0}      # first_frame again
    for t in range(2, 4):
        trk.update(frames[t])
    again = trk.results()
    assert again.shape == (4, 15) and np.array_equal(bits(again), bits(first))
    assert np.array_equal(bits(first), bits(tracking.track_sequence(model, frames[:4], gt[0])))
