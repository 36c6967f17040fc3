"""The tracking front end without a GPU: the fp32 restatement of csrc/track.hip (tests/tracking_oracle.py) against the
reference's own crops (tests/golden/ref_tracking.npz, made by tests/golden/make_golden_tracking.py from the reference's
datasets/points_utils.py and evaluate_one_sequence), the new entry points' argument validation and ctypes signatures, the
device mirrors' refusal of CPU tensors and the determinism of synth.make_sequence."""
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
import tracking_oracle as TO  # noqa: E402
from test_capi_symbols import header_prototypes  # noqa: E402

# |oracle coordinate - reference coordinate|: the oracle rounds the centre to fp32 (<= ulp/2), then one subtraction and
# three products with two additions, each <= ulp/2 of a value below 128 m: ulp(64..128 m) = 7.6e-6 -> 2e-5
COORD_BOUND = 2e-5


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_tracking.npz"))


def _template_from_bank(case, t, crops):
    agg = TO.case_config(case)[1]["shape_aggregation"]
    if agg == "first":
        return crops[0]
    if agg == "firstandprevious":
        return np.concatenate([crops[0], crops[t - 1]], 0)
    return np.concatenate(crops[:t], 0)


def replay_case(gold, case, boxes_from_reference=True):
    """The oracle's crops along the reference's trajectory: frame t's search window by the reference box, the model crops by
    the reference's result boxes -> per frame (search crop, template cloud)"""
    from open3dsot_amd import synth
    _, cfg = TO.case_config(case)
    frames, gt = synth.make_sequence(int(gold[case + ".seq_seed"]), TO.SEQ_FRAMES, TO.SEQ_POINTS)
    results = [gt[0].astype(np.float64)] + [gold["%s.f%d.result_box" % (case, t)] for t in range(1, TO.SEQ_FRAMES)]
    crops, out = [], []
    for t in range(1, TO.SEQ_FRAMES):
        ref = gold["%s.f%d.ref_box" % (case, t)]
        ns, search = TO.crop(frames[t], ref, cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)
        crops.append(TO.crop(frames[t - 1], results[t - 1], cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)[1])
        out.append((search, _template_from_bank(case, t, crops)))
    return out


@pytest.mark.parametrize("case", list(TO.CASES))
def test_oracle_crops_equal_the_reference_on_the_sequences(gold, case):
    """counts (hence masks: the generator asserts a 1e-3 m margin at every crop plane) equal, and the regularised clouds --
    the reference's own index draw applied to the oracle's crop -- within COORD_BOUND of the reference's"""
    from open3dsot_amd import tracking
    _, cfg = TO.case_config(case)
    worst = 0.0
    for t, (search, template) in enumerate(replay_case(gold, case), start=1):
        k = "%s.f%d." % (case, t)
        assert [search.shape[0], template.shape[0]] == gold[k + "counts"].tolist(), (case, t)
        for cloud, size, key in ((template, cfg["template_size"], "template_points"), (search, cfg["search_size"], "search_points")):
            idx = tracking.draw_indices(cloud.shape[0], size)
            got = np.zeros((size, 3), np.float32) if idx is None else cloud[idx]
            d = float(np.abs(got.astype(np.float64) - gold[k + key]).max())
            worst = max(worst, d)
            assert d <= COORD_BOUND, (case, t, key, d)
    print("%s: largest |oracle - reference| coordinate %.3e (bound %.1e)" % (case, worst, COORD_BOUND))


def test_oracle_masks_equal_the_reference_on_the_full_size_frame(gold):
    """a 120 000-point frame: both masks equal outside the band of points within 1e-4 m of a crop plane (<= 8 per crop)"""
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(int(gold["full.seq_seed"]), 1, TO.FULL_POINTS)
    n = int(gold["full.n"])
    assert frames[0].shape[0] == n
    k = TO.TEST_KEYS
    for key, scale, offset, mode in (("search", k["search_bb_scale"], k["search_bb_offset"], TO.SUBWINDOW),
                                     ("model", k["model_bb_scale"], k["model_bb_offset"], TO.MODEL)):
        want = np.unpackbits(gold["full.%s_mask" % key])[:n].astype(bool)
        near = gold["full.%s_near" % key]
        assert near.size <= 8
        got, _ = TO.crop_mask(frames[0], gt[0], scale, offset, mode)
        cmp = np.ones(n, bool)
        cmp[near] = False
        assert want.sum() > 100 and np.array_equal(got[cmp], want[cmp]), key


def test_oracle_offset_box_equals_the_reference(gold):
    """getOffsetBB: the oracle's box from (reference box, chosen offset) against the reference's result box"""
    for case in TO.CASES:
        _, cfg = TO.case_config(case)
        for t in range(1, TO.SEQ_FRAMES):
            k = "%s.f%d." % (case, t)
            box, _ = TO.offset_box(gold[k + "ref_box"], gold[k + "offset"], cfg["degrees"], cfg["use_z"], cfg["limit_box"])
            want = gold[k + "result_box"]
            assert np.abs(box[:3] - want[:3]).max() <= 1e-5 and np.abs(box[6:] - want[6:]).max() <= 1e-6, (case, t)
            assert np.array_equal(box[3:6], want[3:6].astype(np.float32))


def test_new_entry_points_validate_before_any_launch():
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.o3d_track_crop(None, 1, None, 0, None) == EINVAL
    jobs = (PU._CropJob * 1)()                                   # a zeroed job: NULL operands
    assert lib.o3d_track_crop(ctypes.addressof(jobs), 1, p, 64, None) == EINVAL
    assert lib.o3d_track_crop(ctypes.addressof(jobs), 0, p, 64, None) == EINVAL
    assert lib.o3d_track_crop(ctypes.addressof(jobs), 5, p, 64, None) == EINVAL           # more than 4 jobs
    jobs[0] = PU._CropJob(p.value, 8, p.value, 1.0, 0.0, 7, p.value, 8, p.value)
    assert lib.o3d_track_crop(ctypes.addressof(jobs), 1, p, 64, None) == EINVAL           # unknown mode
    jobs[0] = PU._CropJob(p.value, -1, p.value, 1.0, 0.0, 0, p.value, 8, p.value)
    assert lib.o3d_track_crop(ctypes.addressof(jobs), 1, p, 64, None) == EINVAL           # negative size
    assert lib.o3d_track_crop_scratch(ctypes.addressof(jobs), 1) == -1
    jobs[0] = PU._CropJob(p.value, 120000, p.value, 1.0, 0.0, 0, p.value, 8, p.value)
    assert lib.o3d_track_crop_scratch(ctypes.addressof(jobs), 1) == 469                   # one per workgroup of 256 points
    assert lib.o3d_track_crop(ctypes.addressof(jobs), 1, p, 468, None) == EINVAL          # scratch too small
    assert lib.o3d_track_resample(None, 1, None) == EINVAL
    rj = (PU._ResampleJob * 2)()
    rj[0] = PU._ResampleJob(None, 0, None, p.value, 8, 0)                                 # a gather without a source
    assert lib.o3d_track_resample(ctypes.addressof(rj), 1, None) == EINVAL
    assert lib.o3d_track_resample(ctypes.addressof(rj), 3, None) == EINVAL
    assert lib.o3d_track_offset_box(None, None, None, 0, 1, 1, 0, 0, None, None, 0, None, None) == EINVAL
    assert lib.o3d_track_offset_box(p, p, None, 0, 1, 1, 0, 0, None, None, 0, None, None) == EINVAL     # nowhere to write
    assert lib.o3d_track_offset_box(p, p, None, 0, 1, 1, 0, 0, None, p, 4, None, None) == EINVAL        # results without a counter


def test_new_ctypes_signatures_match_the_header():
    from open3dsot_amd import capi, points_utils  # noqa: F401  (registers)
    protos = header_prototypes()
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_float: "f", ctypes.c_double: "d"}
    for name in ("o3d_track_crop", "o3d_track_crop_scratch", "o3d_track_resample", "o3d_track_offset_box"):
        assert name in protos and name in capi.SIGNATURES, name
        assert [kind[a] for a in capi.SIGNATURES[name]] == protos[name], name


def test_job_structs_match_the_header_layout():
    import re
    from open3dsot_amd import points_utils as PU
    src = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    for name, cls in (("o3d_crop_job", PU._CropJob), ("o3d_resample_job", PU._ResampleJob)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, src).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [n.strip().lstrip("*").strip() for n in re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl).group(2).split(",")]
        assert fields == [f[0] for f in cls._fields_], (name, fields)


def test_device_mirrors_refuse_cpu_tensors():
    from open3dsot_amd import points_utils as PU, tracking, trackers
    pts = torch.zeros(8, 3)
    box = (np.zeros(3), np.ones(3), np.eye(3))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.generate_subwindow(pts, box, 1.25)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.cropAndCenterPC(pts, box)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.getModel([pts], [box])
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.getOffsetBB(box, torch.zeros(4))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        tracking.SequenceTracker(trackers.P2B())


def test_make_sequence_is_deterministic_and_leaves_the_other_generators_alone():
    from open3dsot_amd import synth
    a, ga = synth.make_sequence(3, 4, 5000)
    b, gb = synth.make_sequence(3, 4, 5000)
    assert len(a) == 4 and all(x.shape == (5000, 3) and x.dtype == np.float32 for x in a) and ga.shape == (4, 15)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(ga, gb)
    c, _ = synth.make_sequence(4, 4, 5000)
    assert not np.array_equal(a[0], c[0])
    for t in range(4):                       # the target is in the cloud: its box keeps at least its own surface points
        n, _ = TO.crop(a[t], ga[t], 1.25, 0.0, TO.MODEL)
        assert n >= 64
        R = ga[t, 6:].reshape(3, 3).astype(np.float64)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6
    assert np.abs(np.linalg.norm(ga[1:, :2] - ga[:-1, :2], axis=1) - np.linalg.norm(ga[1, :2] - ga[0, :2])).max() < 1e-4   # smooth path


def test_aggregation_follows_the_reference_order_of_tests():
    from open3dsot_amd import tracking
    assert [tracking._aggregation(n) for n in ("first", "previous", "firstandprevious", "all", "FirstAndPrevious")] == \
        ["first", "previous", "firstandprevious", "all", "firstandprevious"]
    with pytest.raises(ValueError):
        tracking._aggregation("mean")
