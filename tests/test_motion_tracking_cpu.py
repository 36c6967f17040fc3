"""The motion tracker's front end without a GPU: the fp32 restatement of o3d_track_motion_input (tests/motion_oracle.py)
against the reference's own build_input_dict and frame loop (tests/golden/ref_motion_tracking.npz, made by
tests/golden/make_golden_motion_tracking.py), the new entry point's argument validation and ctypes signature, the device
mirrors' refusal of CPU tensors and the points_in_box stand-in against a brute-force box test."""
import ctypes
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
from test_capi_symbols import header_prototypes  # noqa: E402

COORD_BOUND = 2e-5            # the project's bound on a cropped coordinate (tests/test_tracking_cpu.py)
BC_BOUND = 1e-4               # BoxCloud distances (tests/test_tracking_gpu.py)


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_motion_tracking.npz"))


def check_input(got_pts, got_bc, gold, k, where):
    """the oracle's (points, candidate_bc) against the fixture's: channels 3 and 4 equal, xyz and BoxCloud within bounds"""
    want = gold[k + "points"]
    N = want.shape[0] // 2
    assert got_pts.shape == want.shape and got_pts.dtype == np.float32
    assert np.array_equal(got_pts[:, 3:], want[:, 3:]), where                     # time stamp and prior targetness: exact
    d = float(np.abs(got_pts[:, :3].astype(np.float64) - want[:, :3]).max())
    assert d <= COORD_BOUND, (where, d)
    dbc = 0.0
    if k + "candidate_bc_prev" in gold:
        dbc = float(np.abs(got_bc[:N].astype(np.float64) - gold[k + "candidate_bc_prev"]).max())
        assert dbc <= BC_BOUND, (where, dbc)
        assert not got_bc[N:].any(), where
    return d, dbc


@pytest.mark.parametrize("case", list(MO.CASES))
def test_oracle_input_equals_the_reference_on_the_sequences(gold, case):
    """every frame, from the reference's box: the crop counts equal, `points` and `candidate_bc` as check_input states"""
    from open3dsot_amd import synth
    cfg = MO.case_config(case)
    frames, gt = synth.make_sequence(int(gold[case + ".seq_seed"]), MO.SEQ_FRAMES, MO.SEQ_POINTS)
    worst = [0.0, 0.0]
    for t in range(1, MO.SEQ_FRAMES):
        k = "%s.f%d." % (case, t)
        pts, bc, counts = MO.host_input(frames[t - 1], frames[t], gold[k + "ref_box"], cfg, t == 1, with_bc=cfg["box_aware"])
        assert list(counts) == gold[k + "counts"].tolist(), (case, t)
        assert min(counts) >= 3
        assert (k + "candidate_bc_prev" in gold) == bool(cfg["box_aware"])
        d = check_input(pts, bc, gold, k, (case, t))
        worst = [max(a, b) for a, b in zip(worst, d)]
    assert int(gold[case + ".near_ties"]) <= MO.MAX_NEAR_TIES
    print("%s: largest |oracle - reference| coordinate %.3e (bound %.1e), BoxCloud %.3e (bound %.1e)"
          % (case, worst[0], COORD_BOUND, worst[1], BC_BOUND))


@pytest.mark.parametrize("name", list(MO.INPUT_CASES))
def test_oracle_input_equals_the_reference_on_the_input_cases(gold, name):
    """zero fill (mask "inside", BoxCloud of the origin), a draw with replacement, the arange path"""
    cfg = dict(MO.case_config("kitti"), point_sample_size=MO.INPUT_N)
    n_prev, n_this, frame_id = MO.INPUT_CASES[name]
    prev, this, box = MO.input_case_frames(name)
    pts, bc, counts = MO.host_input(prev, this, box, cfg, frame_id == 1)
    k = "in.%s." % name
    assert list(counts) == [n_prev, n_this] == gold[k + "counts"].tolist()
    check_input(pts, bc, gold, k, name)
    N = MO.INPUT_N
    if name == "zero_fill":
        assert not pts[:N, :3].any() and np.all(pts[:N, 4] == np.float32(0.8))
        assert np.abs(bc[:N] - MO.boxcloud64(np.zeros((1, 3)), box[3:6])).max() <= BC_BOUND       # the BoxCloud of the origin
    if name == "with_replacement":
        assert len(np.unique(pts[:N, :3], axis=0)) < N and set(np.unique(pts[:N, 4])) == {0.0, 1.0}
    if name == "exact":
        assert np.array_equal(pts[:N, :3], TO.crop(prev, box, cfg["bb_scale"], cfg["bb_offset"], TO.SUBWINDOW)[1])


def test_oracle_offset_box_equals_the_reference(gold):
    """getOffsetBB in radians: the oracle's box from (reference box, estimation_boxes) against the reference's result box"""
    for case in MO.CASES:
        cfg = MO.case_config(case)
        for t in range(1, MO.SEQ_FRAMES):
            k = "%s.f%d." % (case, t)
            box, _ = TO.offset_box(gold[k + "ref_box"], gold[k + "estimation_boxes"], cfg["degrees"], cfg["use_z"], cfg["limit_box"])
            want = gold[k + "result_box"]
            assert np.abs(box[:3] - want[:3]).max() <= 1e-5 and np.abs(box[6:] - want[6:]).max() <= 1e-6, (case, t)
            assert np.array_equal(box[3:6], want[3:6].astype(np.float32))
            if t > 1:                                                       # the loop is closed: a frame starts where the last ended
                assert np.array_equal(gold[k + "ref_box"], gold["%s.f%d.result_box" % (case, t - 1)])


def test_motion_input_validates_before_any_launch():
    from open3dsot_amd import capi, points_utils  # noqa: F401  (registers)
    lib = capi.load()
    EINVAL = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.o3d_track_motion_input
    assert f(None, 0, None, 0, None, 4, 0, 0, None, 1, None, None, None) == EINVAL        # NULL operands
    assert f(p, 8, p, 8, p, 4, 0, 0, None, 1, p, p, None) == EINVAL                       # no wlh
    assert f(p, 8, p, 8, p, 4, 0, 0, p, 1, None, p, None) == EINVAL                       # nowhere to write the points
    assert f(p, 8, p, 8, p, -1, 0, 0, p, 1, p, p, None) == EINVAL                         # negative sizes
    assert f(p, -8, p, 8, p, 4, 0, 0, p, 1, p, p, None) == EINVAL
    assert f(p, 8, p, -8, p, 4, 0, 0, p, 1, p, p, None) == EINVAL
    assert f(None, 0, p, 8, p, 4, 0, 0, p, 1, p, p, None) == EINVAL                       # a gather without a source
    assert f(p, 8, None, 8, p, 4, 0, 0, p, 1, p, p, None) == EINVAL
    assert f(p, 0, p, 8, p, 4, 0, 0, p, 1, p, p, None) == EINVAL                          # ... or from an empty one
    assert f(p, 8, p, 8, None, 4, 0, 0, p, 1, p, p, None) == EINVAL                       # ... or without indices
    assert f(None, 0, None, 0, None, 4, 1, 0, p, 1, p, p, None) == EINVAL                 # one half zero-filled: the other still gathers
    assert f(None, 0, None, 0, None, 0, 1, 1, p, 1, p, None, None) == 0                   # nothing to do, candidate_bc NULL: fine


def test_new_ctypes_signature_matches_the_header():
    from open3dsot_amd import capi, points_utils  # noqa: F401  (registers)
    protos = header_prototypes()
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_float: "f", ctypes.c_double: "d"}
    name = "o3d_track_motion_input"
    assert name in protos and name in capi.SIGNATURES
    assert [kind[a] for a in capi.SIGNATURES[name]] == protos[name]


def test_mirrors_and_tracker_refuse_cpu_tensors():
    from open3dsot_amd import m2track, points_utils as PU, tracking
    box = (torch.zeros(3), torch.ones(3), torch.eye(3))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.motion_input(torch.zeros(8, 3), torch.zeros(8, 3), torch.zeros(8, dtype=torch.int32), torch.ones(3), True)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.points_in_box(box, torch.zeros(3, 8), 1.25)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.transform_box(box, box)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        tracking.MotionSequenceTracker(m2track.M2TRACK())
    with pytest.raises(RuntimeError, match="CPU not supported"):
        tracking.track_sequence(m2track.M2TRACK(), [torch.zeros(8, 3)], np.zeros(15))
    assert hasattr(m2track.M2TRACK, "evaluate_one_sample")


def test_points_in_box_standin_equals_a_brute_force_box_test():
    """random oriented boxes and points, fp64: inside iff the box-frame coordinates are within the scaled half extents; points
    within 1e-9 of a face are left out"""
    import points_in_box_standin
    import quat_standin

    class Box:
        def __init__(self, c, wlh, R):
            self.center, self.wlh, self.R = c, wlh, R

        def corners(self, wlh_factor=1.0):          # (3,8), the corner order of motion_oracle's sign tables
            w, l, h = self.wlh * wlh_factor
            local = np.stack([MO.SX * (l / 2), MO.SY * (w / 2), MO.SZ * (h / 2)]).astype(np.float64)
            return self.R @ local + self.center[:, None]
    rng = np.random.default_rng(0)
    seen = [0, 0]
    for trial in range(20):
        axis = rng.normal(size=3)
        R = quat_standin.Quaternion(axis=axis / np.linalg.norm(axis), radians=rng.uniform(-np.pi, np.pi)).rotation_matrix
        c, wlh, factor = rng.uniform(-20, 20, 3), rng.uniform(0.5, 5, 3), rng.uniform(0.8, 1.5)
        pts = c[:, None] + R @ (rng.uniform(-1.2, 1.2, (3, 4000)) * (np.array([wlh[1], wlh[0], wlh[2]]) * factor / 2)[:, None])
        q = R.T @ (pts - c[:, None])
        m = (np.array([wlh[1], wlh[0], wlh[2]]) * factor / 2)[:, None] - np.abs(q)
        use = np.abs(m).min(0) > 1e-9
        want = (m > 0).all(0)
        got = points_in_box_standin.points_in_box(Box(c, wlh, R), pts, wlh_factor=factor)
        assert np.array_equal(got[use], want[use]), trial
        seen[0] += int(want[use].sum())
        seen[1] += int((~want[use]).sum())
    assert min(seen) > 10000
