"""The K-target loop of the motion tracker on the GPU: o3d_track_motion_input_multi bit for bit against K calls of
o3d_track_motion_input and against its fp32 restatement (tests/motion_oracle.py), and tracking.MultiMotionTracker against the
reference's own run (tests/golden/ref_motion_tracking.npz) and against K MotionSequenceTrackers.

The scene of the loop tests is the fixture's sequence with three targets: target 0 is the fixture's box, target 1 the same box
again, target 2 the box moved 500 m, where both crops are empty and the inputs are zero-filled."""
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
K3, FAR = 3, 500.0


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_motion_tracking.npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def tbits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- the kernel against K single launches and against the oracle -------------------------------------------------------------
def job_set(K, N, rng):
    """K jobs (prev | None, cur | None, idx, (zero_prev, zero_this)) as host arrays + wlh (K,3), the crop sizes mixed.  Target
    0 has an index equal to n_src in each half (a zero row).  From K = 3 on: target 1 has zero_prev set (its crop is still
    there, unread) and target 2 repeats target 0's job.  From K = 5 on: target 3 has zero_this set, target 4 both flags with
    NULL sources and no indices."""
    wlh = (np.array([1.6, 3.9, 1.5]) * rng.uniform(0.9, 1.1, (K, 3))).astype(np.float32)
    jobs = []
    for k in range(K):
        half = np.array([wlh[k, 1], wlh[k, 0], wlh[k, 2]]) * 1.25 / 2
        n_prev, n_this = 7 + 197 * k, 5000 - 911 * k
        prev = (rng.uniform(-1.6, 1.6, (n_prev, 3)) * half).astype(np.float32)    # inside and outside the 1.25-scaled box
        cur = (rng.uniform(-1.6, 1.6, (n_this, 3)) * half).astype(np.float32)
        prev[0] = [half[0], -half[1], half[2]]                                    # a row on the faces themselves
        idx = np.concatenate([rng.integers(0, n_prev, N), rng.integers(0, n_this, N)]).astype(np.int32)
        idx[0] = 0
        jobs.append([prev, cur, idx, (False, False)])
    jobs[0][2][N - 1], jobs[0][2][2 * N - 1] = jobs[0][0].shape[0], jobs[0][1].shape[0]       # one past the end of its source
    if K >= 3:
        jobs[1][3] = (True, False)
        jobs[2] = list(jobs[0])
        wlh[2] = wlh[0]
    if K >= 5:
        jobs[3][3] = (False, True)
        jobs[4] = [None, None, None, (True, True)]
    return [tuple(j) for j in jobs], wlh


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("N", [1, 128, 129, 256])
def test_motion_input_multi_equals_k_single_launches_and_the_oracle(dev, N, K):
    """2N = 256 fills exactly one workgroup, N = 129 puts the half boundary inside one.  Both first_frame values, with and
    without candidate_bc; the destinations are sentinel-filled with a guard row behind them"""
    from open3dsot_amd import points_utils as PU
    jobs, wlh = job_set(K, N, np.random.default_rng([N, K]))

    def up(x):
        return None if x is None else torch.from_numpy(x).to(dev)
    djobs = [(up(p), up(c), up(i), z) for p, c, i, z in jobs]
    table = PU.motion_job_table(djobs, dev)
    assert table.dtype == torch.uint8 and table.numel() == K * PU.MOTION_JOB.itemsize
    twlh = torch.from_numpy(wlh).to(dev)
    rows = 2 * N * K
    seen = set()
    for first in (True, False):
        for with_bc in (True, False):
            m_pts, s_pts = (torch.full((rows + 1, 5), -7.0, device=dev) for _ in range(2))
            m_bc, s_bc = (torch.full((rows + 1, 9), -7.0, device=dev) for _ in range(2))
            got_p, got_b = PU.motion_input_multi(table, K, N, twlh, first, m_pts[:rows], m_bc[:rows] if with_bc else False)
            assert got_p.data_ptr() == m_pts.data_ptr() and (got_b is None) == (not with_bc)
            for k, (p, c, i, z) in enumerate(djobs):
                at = slice(2 * N * k, 2 * N * (k + 1))
                PU.motion_input(p, c, i, twlh[k], first, zero=z, out_points=s_pts[at], out_bc=s_bc[at] if with_bc else False)
            torch.cuda.synchronize()
            assert torch.equal(tbits(m_pts), tbits(s_pts)), (first, with_bc)           # bit for bit, the guard row included
            assert torch.equal(tbits(m_bc), tbits(s_bc)), (first, with_bc)
            assert bool((m_pts[rows] == -7.0).all()) and bool((m_bc[rows] == -7.0).all())
            if not with_bc:
                assert bool((m_bc == -7.0).all())                                        # NULL: nothing written
            g, b = m_pts[:rows].cpu().numpy().reshape(K, 2 * N, 5), m_bc[:rows].cpu().numpy().reshape(K, 2 * N, 9)
            for k, (p, c, i, z) in enumerate(jobs):
                want_p, want_b = MO.motion_input(p, c, i, N, wlh[k], first, zero=z, with_bc=with_bc)
                assert np.array_equal(bits(g[k]), bits(want_p)), (first, with_bc, k)
                seen |= set(np.unique(g[k, :N, 4]).tolist())
                if with_bc:
                    assert np.abs(b[k, :N] - MO.boxcloud64(want_p[:N, :3], wlh[k])).max() <= BC_BOUND
                    assert np.abs(b[k] - want_b).max() <= 2e-6 and not b[k, N:].any()
                    if z[0]:                                                          # zero-filled: "inside", the BoxCloud of the origin
                        assert np.all(g[k, :N, 4] == np.float32(1.0 if first else 0.8)) and np.all(b[k, :N] == b[k, 0])
                if z[0]:
                    assert not g[k, :N, :3].any()
                if z[1]:
                    assert not g[k, N:, :3].any()
            assert not g[0, N - 1, :3].any() and not g[0, 2 * N - 1, :3].any()          # the index equal to n_src: a zero row
            if K >= 3:
                assert np.array_equal(bits(g[2]), bits(g[0])) and np.array_equal(bits(b[2]), bits(b[0]))       # identical jobs
    if N >= 128:
        assert seen == {0.0, 1.0, np.float32(0.2).item(), np.float32(0.8).item()}


# ---- the loop ----------------------------------------------------------------------------------------------------------------
_MODELS = {}


def make_model(case, dev):
    from open3dsot_amd import m2track
    if case not in _MODELS:
        cfg = MO.case_config(case)
        _MODELS[case] = (MO.init_weights(m2track.M2TRACK(**cfg)).to(dev).eval(), cfg)
    return _MODELS[case]


def sequence_of(gold, case, dev):
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(int(gold[case + ".seq_seed"]), MO.SEQ_FRAMES, MO.SEQ_POINTS)
    return [torch.from_numpy(f).to(dev) for f in frames], gt


def far(box):
    """the box moved 500 m along x: outside the scene, both of its windows are empty"""
    b = np.array(box, np.float32)
    b[0] += FAR
    return b


def targets(box):
    return np.stack([box, box, far(box)])


class hard_masks:
    """tests/test_motion_tracking_gpu.py::hard_masks restated per batch row.  Hooks torch.argmax for ONE forward of batch B:
    call 0 is the segmentation decision (B,2,n) -> (B,1,n), call 1 the motion-state decision (B,2) -> (B,1).  Recorded per
    call: `dec[call]` (B,n), the decisions of the run under test, and `margin[call]` (B,n), its own |l1 - l0|.  `keys` maps a
    batch row to a frame's prefix in the fixture; for those rows the decisions are compared with the reference's stored ones
    (`flipped[row]`: segmentation points that differ, `motion_flipped[row]`, `worst`: the largest stored margin at a differing
    decision) and, with replay=True, REPLACED by them under the rule of tests/test_golden_m2track.py::replay_hard_masks: a
    decision may differ from the reference's only where the reference's stored margin is MO.TIE or less (asserted on exit).
    Rows without a key keep their own decisions."""

    def __init__(self, gold=None, keys=None, replay=False):
        self.g, self.keys, self.replay, self.calls = gold, dict(keys or {}), replay, 0
        self.dec, self.margin = [], []
        self.flipped, self.motion_flipped, self.worst = {r: 0 for r in self.keys}, {r: False for r in self.keys}, 0.0

    def __enter__(self):
        self.real = torch.argmax
        torch.argmax = self._hook
        return self

    def _hook(self, x, *a, **k):
        mine = self.real(x, *a, **k)
        which, self.calls = self.calls, self.calls + 1
        B = x.shape[0]
        self.dec.append(mine.reshape(B, -1).cpu().numpy())
        self.margin.append((x[:, 1] - x[:, 0]).abs().reshape(B, -1).cpu().numpy())
        out = mine.clone()
        for row, key in self.keys.items():
            if which == 0:
                theirs = np.unpackbits(self.g[key + "seg_mask"])[:self.dec[-1].shape[1]]
                margin = self.g[key + "seg_margin"]
            else:
                theirs, margin = np.atleast_1d(self.g[key + "motion_state"]), np.atleast_1d(self.g[key + "motion_margin"])
            differ = self.dec[-1][row] != theirs.astype(np.int64)
            if differ.any():
                self.worst = max(self.worst, float(margin[differ].max()))
            if which == 0:
                self.flipped[row] = int(differ.sum())
            else:
                self.motion_flipped[row] = bool(differ.any())
            out[row] = torch.from_numpy(theirs.astype(np.int64)).reshape(mine[row].shape).to(mine.device)
        return out if self.replay else mine

    def __exit__(self, *exc):
        torch.argmax = self.real
        if exc[0] is None:
            assert self.calls == 2, self.calls
            if self.replay:
                assert self.worst <= MO.TIE, ("a hard-mask decision differs from the reference's away from a tie", self.keys, self.worst)
        return False

    def differs_from_reference(self, row):
        return bool(self.flipped[row] or self.motion_flipped[row])


def row_deviation(trk, row, box, gold, k, cfg):
    """tests/test_motion_tracking_gpu.py::frame_deviation for batch row `row`: the row's deviations from the reference's
    frame k: points xyz, BoxCloud, estimation_boxes (relative), result centre"""
    N = cfg["point_sample_size"]
    pts, want = trk.inputs["points"][row].cpu().numpy(), gold[k + "points"]
    assert np.array_equal(pts[:, 3:], want[:, 3:]), (k, row)                        # time stamp and prior targetness: exact
    d = {"xyz": float(np.abs(pts[:, :3] - want[:, :3]).max())}
    if cfg["box_aware"]:
        bc = trk.inputs["candidate_bc"][row].cpu().numpy()
        assert not bc[N:].any()
        d["boxcloud"] = float(np.abs(bc[:N] - gold[k + "candidate_bc_prev"]).max())
    w = gold[k + "estimation_boxes"]
    d["estimation"] = float(np.abs(trk.out[row].reshape(-1).cpu().numpy() - w).max() / max(1.0, np.abs(w).max()))
    d["centre"] = float(np.abs(box[row].cpu().numpy()[:3] - gold[k + "result_box"][:3]).max())
    return d


@pytest.mark.parametrize("case", list(MO.CASES))
def test_teacher_forced_rows_equal_the_reference(gold, dev, case):
    """K = 3, every frame started from the reference's box t-1, the reference's hard masks replayed on rows 0 and 1: counts
    equal, points <= 2e-5 with channels 3 and 4 exact, BoxCloud <= 1e-4, estimation_boxes within the feature bound, the
    result centre within 1e-4 + 2e-5; per row no more flipped segmentation points over the case than the fixture's near-tie
    count.  Row 2 (both crops empty): counts (0, 0) and the inputs of a MotionSequenceTracker on the same box, bit for bit; its
    network output is not compared (every point is the origin, so every margin is one number and may sit on a tie)"""
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    trk = tracking.MultiMotionTracker(model, K3, use_graph=False)
    assert trk.init(frames[0], targets(gt[0])).shape == (K3, 15)
    lone = tracking.MotionSequenceTracker(model, use_graph=False)
    lone.init(frames[0], far(gt[0]))
    worst, flipped = {}, [0, 0]
    for t in range(1, MO.SEQ_FRAMES):
        k = "%s.f%d." % (case, t)
        for row, box in enumerate(targets(gold[k + "ref_box"])):
            trk.set_box(row, box)
        with hard_masks(gold, {0: k, 1: k}, replay=True) as hm:
            boxes = trk.update(frames[t])
        assert boxes.shape == (K3, 15)
        n_prev, n_this = trk.log[-1]
        for row in (0, 1):
            flipped[row] += hm.flipped[row]
            assert [int(n_prev[row]), int(n_this[row])] == gold[k + "counts"].tolist(), (case, t, row)
            d = row_deviation(trk, row, boxes, gold, k, cfg)
            print("%s frame %d row %d:" % (case, t, row), {kk: "%.2e" % v for kk, v in d.items()}, "flipped", hm.flipped[row],
                  hm.motion_flipped[row])
            assert d["xyz"] <= COORD_BOUND and d.get("boxcloud", 0.0) <= BC_BOUND, (case, t, row, d)
            assert d["estimation"] <= FEATURE_BOUND, (case, t, row, d)
            assert d["centre"] <= CENTRE_BOUND, (case, t, row, d)
            for kk, v in d.items():
                worst[kk] = max(worst.get(kk, 0.0), v)
        lone.set_box(far(gold[k + "ref_box"]))
        lone.update(frames[t])
        assert (int(n_prev[2]), int(n_this[2])) == (0, 0) == tuple(lone.log[-1]), (case, t)
        for name in lone.inputs:
            assert torch.equal(tbits(trk.inputs[name][2]), tbits(lone.inputs[name][0])), (case, t, name)
        assert not trk.inputs["points"][2, :, :3].any()
    print("%s K = 3 teacher-forced worst:" % case, {kk: "%.2e" % v for kk, v in worst.items()}, "flipped points per row", flipped)
    assert max(flipped) <= int(gold[case + ".near_ties"]), (flipped, int(gold[case + ".near_ties"]))
    assert trk.results().shape == (MO.SEQ_FRAMES, K3, 15)


def compare_with_singles(multi, singles, frames, teacher, what):
    """One teacher-forced pass of a batched tracker and its K single trackers over the frames; teacher(t) -> the K boxes
    every tracker starts frame t from.  Inputs of every row bit for bit, counts equal; on the rows `checked` the hard-mask
    decisions of the batched forward differ from the single forward's only where the single run's own margin is MO.TIE or
    less; where no decision of a (row, frame) differs, the centre within the feature bound and wlh bit-equal.
    -> (largest centre difference among those, number of differing decisions)"""
    K = len(singles)
    checked = range(min(K, 2))                  # row 2 is all origin: every margin one number, perhaps on a tie
    worst, near = 0.0, 0
    for t in range(1, len(frames)):
        start = teacher(t)
        for k in range(K):
            multi.set_box(k, start[k])
            singles[k].set_box(start[k])
        with hard_masks() as hm:
            boxes = multi.update(frames[t])
        n_prev, n_this = multi.log[-1]
        for k, s in enumerate(singles):
            with hard_masks() as hs:
                sbox = s.update(frames[t])
            assert (int(n_prev[k]), int(n_this[k])) == tuple(s.log[-1]), (what, k, t)
            assert set(s.inputs) == set(multi.inputs)
            for name in s.inputs:
                assert torch.equal(tbits(multi.inputs[name][k]), tbits(s.inputs[name][0])), (what, k, t, name)
            if k not in checked:
                continue
            differing = 0
            for call in (0, 1):
                differ = hm.dec[call][k] != hs.dec[call][0]
                differing += int(differ.sum())
                assert not differ.any() or float(hs.margin[call][0][differ].max()) <= MO.TIE, (what, k, t, call)
            near += differing
            if differing == 0:
                d = float((boxes[k, :3] - sbox[:3]).abs().max())
                worst = max(worst, d)
                assert d <= FEATURE_BOUND, (what, k, t, d)
                assert torch.equal(tbits(boxes[k, 3:6]), tbits(sbox[3:6]))
    print("%s: largest |batched - single| centre %.3e, decisions that differ (all within a tie) %d" % (what, worst, near))
    return worst, near


@pytest.mark.parametrize("case", list(MO.CASES))
def test_batched_equals_k_single_trackers_teacher_forced(gold, dev, case):
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    multi = tracking.MultiMotionTracker(model, K3, use_graph=False)
    multi.init(frames[0], targets(gt[0]))
    singles = [tracking.MotionSequenceTracker(model, use_graph=False) for _ in range(K3)]
    for s, box in zip(singles, targets(gt[0])):
        s.init(frames[0], box)
    _, near = compare_with_singles(multi, singles, frames, lambda t: targets(gold["%s.f%d.ref_box" % (case, t)]), case)
    assert near <= MO.MAX_NEAR_TIES, near
    assert multi.box_aware == cfg["box_aware"] and ("candidate_bc" in multi.inputs) == cfg["box_aware"]


@pytest.mark.parametrize("case", list(MO.CASES))
def test_one_target_reproduces_the_single_tracker(gold, dev, case):
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    multi, single = tracking.MultiMotionTracker(model, 1, use_graph=False), tracking.MotionSequenceTracker(model, use_graph=False)
    assert multi.init(frames[0], [gt[0]]).shape == (1, 15)
    single.init(frames[0], gt[0])
    _, near = compare_with_singles(multi, [single], frames, lambda t: gold["%s.f%d.ref_box" % (case, t)][None], case + " K = 1")
    assert near <= MO.MAX_NEAR_TIES, near
    assert multi.results().shape == (MO.SEQ_FRAMES, 1, 15)


@pytest.mark.parametrize("case", list(MO.CASES))
def test_graph_replay_equals_the_eager_loop(gold, dev, case):
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    eager = tracking.track_targets(model, frames, targets(gt[0]), use_graph=False)
    graph = tracking.track_targets(model, frames, targets(gt[0]), use_graph=True)
    assert eager.shape == (MO.SEQ_FRAMES, K3, 15) and np.array_equal(bits(graph), bits(eager))      # replay == eager
    assert np.array_equal(bits(eager[0]), bits(targets(gt[0])))
    assert np.abs(eager[1:, :2, :3] - eager[:-1, :2, :3]).max() > 1e-3                               # the boxes do move
    with pytest.raises(ValueError, match="ref_boxes"):
        tracking.track_targets(model, frames, targets(gt[0]), ref_boxes=[targets(gt[0])] * len(frames))


def run(trk, frames, boxes0, before=None):
    trk.init(frames[0], boxes0)
    for t in range(1, len(frames)):
        if before is not None:
            before(t)
        trk.update(frames[t])
    return trk.results()


def test_small_capacities_grow_and_change_nothing(gold, dev):
    from open3dsot_amd import tracking
    model, cfg = make_model("kitti", dev)
    frames, gt = sequence_of(gold, "kitti", dev)
    big, small = tracking.MultiMotionTracker(model, K3), tracking.MultiMotionTracker(model, K3, capacity=64)
    want, got = run(big, frames, targets(gt[0])), run(small, frames, targets(gt[0]))
    assert np.array_equal(bits(got), bits(want))
    for a, b in zip(small.log, big.log):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the log shows the re-crop: counts beyond the 64 rows the buffer started with, and more crop calls than frames
    assert max(int(max(e[0].max(), e[1].max())) for e in small.log) > 64
    assert small.crop_calls > MO.SEQ_FRAMES - 1 and big.crop_calls == MO.SEQ_FRAMES - 1
    assert small.crop_buf.shape[2] >= max(int(max(e[0].max(), e[1].max())) for e in small.log) > 64


def test_retire_repeats_the_box_and_leaves_the_others_alone(gold, dev):
    from open3dsot_amd import tracking
    model, cfg = make_model("kitti", dev)
    frames, gt = sequence_of(gold, "kitti", dev)
    full = tracking.track_targets(model, frames, targets(gt[0]))
    trk = tracking.MultiMotionTracker(model, K3)
    state = {}

    def before(t):
        if t == 3:
            trk.retire(1)
            state["yaw"] = trk.yaw_state[1].clone()
    res = run(trk, frames, targets(gt[0]), before)
    assert np.array_equal(bits(res[:3]), bits(full[:3]))
    assert all(np.array_equal(bits(res[t, 1]), bits(res[2, 1])) for t in range(3, MO.SEQ_FRAMES))     # its last box, repeated
    assert not np.array_equal(full[3, 1], full[2, 1]) and torch.equal(tbits(trk.yaw_state[1]), tbits(state["yaw"]))
    assert np.array_equal(bits(res[:, [0, 2]]), bits(full[:, [0, 2]]))                                # the others: as without it
    assert not np.array_equal(res[3, 0], res[2, 0])
    trk.init(frames[0], targets(gt[0]))                                                               # init follows all K again
    trk.update(frames[1])
    assert np.array_equal(bits(trk.results()), bits(full[:2]))


def test_a_second_tracker_on_the_same_model_does_not_disturb_the_first(gold, dev):
    from open3dsot_amd import synth, tracking
    model, cfg = make_model("kitti", dev)
    fa, ga = sequence_of(gold, "kitti", dev)
    fb_np, gb = synth.make_sequence(77, MO.SEQ_FRAMES, MO.SEQ_POINTS)
    fb = [torch.from_numpy(f).to(dev) for f in fb_np]
    solo_a, solo_b = tracking.track_targets(model, fa, targets(ga[0])), tracking.track_targets(model, fb, targets(gb[0]))
    ta, tb = tracking.MultiMotionTracker(model, K3), tracking.MultiMotionTracker(model, K3)
    ta.init(fa[0], targets(ga[0]))
    tb.init(fb[0], targets(gb[0]))
    for t in range(1, MO.SEQ_FRAMES):
        ta.update(fa[t])
        tb.update(fb[t])
    assert np.array_equal(bits(ta.results()), bits(solo_a)) and np.array_equal(bits(tb.results()), bits(solo_b))
    assert not np.array_equal(solo_a, solo_b)


@pytest.mark.parametrize("case", list(MO.CASES))
def test_closed_loop_follows_the_reference_trajectory(gold, dev, case):
    """No teacher, no replay: on rows 0 and 1, frame 1 under the teacher-forced bound when none of its decisions differs from
    the reference's; from frame 2 on the deviation compounds through the network and is MEASURED (printed), as
    tests/test_motion_tracking_gpu.py::test_closed_loop_follows_the_reference_trajectory does; the crop counts must equal the
    reference's up to the first frame whose hard masks differ from the reference's"""
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    trk = tracking.MultiMotionTracker(model, K3, use_graph=False)
    trk.init(frames[0], targets(gt[0]))
    dev_c, dev_r, first_flip = [[], []], [[], []], [None, None]
    for t in range(1, MO.SEQ_FRAMES):
        k = "%s.f%d." % (case, t)
        with hard_masks(gold, {0: k, 1: k}, replay=False) as hm:
            boxes = trk.update(frames[t])
        n_prev, n_this = trk.log[-1]
        for row in (0, 1):
            if first_flip[row] is None:
                assert [int(n_prev[row]), int(n_this[row])] == gold[k + "counts"].tolist(), (case, t, row, dev_c)
                if hm.differs_from_reference(row):
                    first_flip[row] = t
            if t == 1 and first_flip[row] is None:
                d = row_deviation(trk, row, boxes, gold, k, cfg)
                assert d["estimation"] <= FEATURE_BOUND and d["centre"] <= CENTRE_BOUND, (row, d)
            b, want = boxes[row].cpu().numpy(), gold[k + "result_box"]
            dev_c[row].append(float(np.abs(b[:3] - want[:3]).max()))
            dev_r[row].append(float(np.abs(b[6:] - want[6:]).max()))
    for row in (0, 1):
        print("closed loop %s row %d: centre deviation per frame 1..7 [m]: %s" % (case, row, " ".join("%.2e" % v for v in dev_c[row])))
        print("closed loop %s row %d: rotation deviation per frame 1..7: %s" % (case, row, " ".join("%.2e" % v for v in dev_r[row])))
        print("closed loop %s row %d: first frame with a hard-mask decision unlike the reference's: %s" % (case, row, first_flip[row]))
