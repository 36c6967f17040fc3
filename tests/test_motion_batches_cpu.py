"""M2-Track training batches built on the device, the part that needs no GPU: the numpy restatement
(tests/motion_sampler_oracle.py) against the reference's own motion_processing with apply_augmentation
(tests/golden/ref_motion_batches.npz), the selection rule, and the host side of the library (the declared and exported
entries, struct sizes, argument validation)."""
import ctypes
import os
import re

import numpy as np
import pytest

import fixture_io
import motion_sampler_oracle as MSO
import tracking_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# case -> the overrides of sampler.MOTION_DATA_KEYS (tests/golden/make_golden_motion_batches.py::CASES)
CASES = {"plain": dict(use_augmentation=False, point_sample_size=512), "aug": dict(point_sample_size=512), "sparse": {},
         "deg": dict(degrees=True, box_aware=False, point_sample_size=256)}
BIG = (1 << 20,) * 2                                      # capacities that truncate nothing
NEW_ENTRIES = ("o3d_train_augment", "o3d_track_crop_groups_aug", "o3d_train_inside_box", "o3d_train_motion_labels",
               "o3d_train_select_motion", "o3d_train_motion_sample")


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_motion_batches.npz"))


def case_inputs(ref, case):
    from open3dsot_amd import sampler, synth
    cfg = dict(sampler.MOTION_DATA_KEYS, **CASES[case])
    frames, gt = synth.make_sequence(int(ref[case + ".seq_seed"]), 8, int(ref[case + ".n_points"]))
    return cfg, frames, gt, [tuple(int(v) for v in s) for s in ref[case + ".samples"]]


def case_draws(ref, cfg, keys):
    """the reference's recorded draws of the samples `keys` (None: a candidate outside the fixture, zeros) as build() takes them"""
    J, N = len(keys), cfg["point_sample_size"]
    draws = {"offset": np.zeros((J, 3)), "aug_prev": np.zeros((J, 6)), "aug_this": np.zeros((J, 6)),
             "idx_prev": np.zeros((J, N), np.int32), "idx_this": np.zeros((J, N), np.int32)}
    for j, k in enumerate(keys):
        if k is not None:
            for name in draws:
                if k + name in ref:
                    draws[name][j] = ref[k + name]
    return draws


@pytest.fixture(scope="module")
def oracle_builds(ref):
    """the oracle's build, teacher-forced with the reference's draws, one batch per case (B = J = the case's samples):
    computed once"""
    builds = {}
    for case in CASES:
        cfg, frames, gt, samples = case_inputs(ref, case)
        keys = ["%s.s%d." % (case, s) for s in range(len(samples))]
        d = case_draws(ref, cfg, keys)
        builds[case] = MSO.build({"t": (frames, gt)}, [("t",) + s for s in samples], cfg, len(samples), d["offset"], d["aug_prev"],
                                 d["aug_this"], BIG, d["idx_prev"], d["idx_this"]) + (cfg, keys)
    return builds


# ---- the host side of the library ----------------------------------------------------------------------------------------------------
def test_header_declares_the_six_entries_and_the_library_exports_them():
    from open3dsot_amd import build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "o3dsot.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(o3d_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(build.build())
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_struct_sizes_match_the_library():
    from open3dsot_amd import points_utils as PU
    assert PU.CROP_AUG.itemsize == 112 and ctypes.sizeof(PU._TrainMotionSampleArgs) == 248
    assert [PU.CROP_AUG.fields[n][1] for n in ("enabled", "box", "A", "c")] == [0, 4, 64, 100]
    for name, size, where in (("o3d_crop_aug", 112, "train_batch.hip"), ("o3d_train_motion_sample_args", 248, "track.hip")):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in open(os.path.join(ROOT, "open3dsot_amd", "csrc", where)).read()
    hdr = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*o3d_train_motion_sample_args;", hdr).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = re.match(r"(?:const\s+)?\w+\s*\**\s*(.*)", decl).group(1)
            fields += [n.strip().lstrip("*").strip() for n in names.split(",")]
    assert fields == [f[0] for f in PU._TrainMotionSampleArgs._fields_]


def test_entries_validate_before_any_launch():
    """NULL operands and sizes out of range return O3D_EINVAL (-1) before any HIP call (host buffers stand in for device
    pointers: nothing dereferences them)"""
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert lib.o3d_train_augment(None, p, None, 4, 4, p, p, None) == -1
    assert lib.o3d_train_augment(p, p, None, 4, 5, p, p, None) == -1                              # no slot table: n_slots == K
    assert lib.o3d_train_augment(p, p, p, 0, 4, p, p, None) == -1
    assert lib.o3d_train_augment(p, p, p, 4, 3 * 1024 + 1, p, p, None) == -1
    assert lib.o3d_train_augment(p, p, p, 4, 4, p, None, None) == -1
    plan = np.zeros(2, PU.CROP_PLAN)
    plan["points"], plan["targets"], plan["n"], plan["n_targets"] = p, p, [300, 10], [2, 3]
    need = PU.crop_groups_plan(plan)[0]
    assert lib.o3d_track_crop_groups_aug(None, p, p, 2, p, need, None) == -1
    assert lib.o3d_track_crop_groups_aug(plan.ctypes.data, None, p, 2, p, need, None) == -1
    assert lib.o3d_track_crop_groups_aug(plan.ctypes.data, p, p, 2, None, need, None) == -1
    assert lib.o3d_track_crop_groups_aug(plan.ctypes.data, p, p, 2, p, need - 1, None) == -1      # scratch too short
    bad = plan.copy()
    bad["sbase"][1] += 1                                                                          # a plan that was not planned
    assert lib.o3d_track_crop_groups_aug(bad.ctypes.data, p, p, 2, p, need + 8, None) == -1
    assert lib.o3d_train_inside_box(None, 4, p, 1.0, p, None) == -1
    assert lib.o3d_train_inside_box(p, 4, None, 1.0, p, None) == -1
    assert lib.o3d_train_inside_box(p, -1, p, 1.0, p, None) == -1
    assert lib.o3d_train_inside_box(None, 0, p, 1.0, None, None) == 0                             # nothing to test
    assert lib.o3d_train_motion_labels(p, p, None, 4, 0, 0.15, *([p] * 8), None) == -1
    assert lib.o3d_train_motion_labels(p, p, p, 0, 0, 0.15, *([p] * 8), None) == -1
    assert lib.o3d_train_motion_labels(p, p, p, 1025, 0, 0.15, *([p] * 8), None) == -1
    assert lib.o3d_train_motion_labels(p, p, p, 4, 0, 0.15, *([p] * 7), None, None) == -1
    assert lib.o3d_train_select_motion(None, 4, 2, 8, 8, p, p, p, None) == -1
    assert lib.o3d_train_select_motion(p, 4, 5, 8, 8, p, p, p, None) == -1                        # B > J
    assert lib.o3d_train_select_motion(p, 1025, 2, 8, 8, p, p, p, None) == -1
    assert lib.o3d_train_select_motion(p, 4, 2, -1, 8, p, p, p, None) == -1
    assert lib.o3d_train_motion_sample(None, None) == -1

    def args(**over):
        a = PU._TrainMotionSampleArgs(p, p, p, p, 8, 8, 4, 2, 16, None, None, p, 0, 0, p, p, p, p, p, p, p, p, p, None, p, p, p, p, p, p,
                                      None, None, None, None)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    for over in (dict(sel=None), dict(crop_this=None), dict(B=5), dict(J=0), dict(N=0), dict(N=(1 << 20) + 1), dict(cap_prev=-1),
                 dict(idx_prev=p), dict(idx_this=p), dict(seg_label=None), dict(candidate_id=None), dict(canon_box=None),
                 dict(motion_state_label=None), dict(bc_boxes=p), dict(xyz_halves=p)):
        a = args(**over)
        assert lib.o3d_train_motion_sample(ctypes.addressof(a), None) == -1, over


# ---- the oracle against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_build_matches_the_reference(ref, oracle_builds, case):
    batch, cands, cfg, keys = oracle_builds[case]
    J, N = len(keys), cfg["point_sample_size"]
    assert J == {"plain": 8, "aug": 8, "sparse": 2, "deg": 2}[case]
    assert batch["sel"].tolist() == list(range(J)) and batch["n_valid"] == J and batch["overflow"] == 0
    for r, k in enumerate(keys):
        assert np.array_equal(cands[r]["counts"][1:], ref[k + "counts"]), k
        assert abs(int(cands[r]["counts"][0]) - int(ref[k + "inbox_count"])) <= int(ref[k + "inbox_slack"]), k
        assert int(ref[k + "inbox_count"]) >= 50 or int(ref[k + "inbox_count"]) <= 5
        MSO.check_against_reference({name: v[r] for name, v in batch.items() if isinstance(v, np.ndarray) and v.ndim >= 1 and name != "sel"},
                                    ref, k, cfg)
        assert ("candidate_bc" in batch) == cfg["box_aware"] == (k + "candidate_bc" in ref)
        if cfg["use_augmentation"]:                        # the augmented boxes themselves, against apply_transform's
            for got, want in ((cands[r]["prev_gt"], ref[k + "prev_gt_aug"]), (cands[r]["this_gt"], ref[k + "this_gt_aug"])):
                assert np.abs(got - want).max() <= 2e-6
        assert np.abs(cands[r]["ref_box"] - ref[k + "ref_box"]).max() <= 2e-6
    if case == "sparse":                                   # the with-replacement route: both halves shorter than the sample
        assert (ref["sparse.s1.counts"] < N).all() and (ref["sparse.s1.counts"] > 2).all()
    if case == "aug":                                      # a flip on one frame only: the relative yaw is near +-pi
        assert max(abs(float(ref["aug.s%d.motion_label" % s][3])) for s in range(8)) > 3.0
    assert batch["seg_label"].dtype == np.int64 and 0 < batch["seg_label"].mean() < 1
    assert set(np.unique(batch["points"][:, :N, 4])) <= {np.float32(0), np.float32(1), np.float32(0.2), np.float32(0.8)}


def test_far_candidate_is_invalid(ref):
    """the reference raises its AssertionError for the candidate moved 500 m; the oracle's counts make it invalid"""
    assert bool(ref["far.raises"])
    cfg, frames, gt, _ = case_inputs(ref, "plain")
    gt = gt.copy()
    gt[:, 0] += float(ref["far.shift"])
    got = MSO.candidate(frames, gt, tuple(int(v) for v in ref["far.sample"]), cfg, np.zeros(3), None, None, BIG)
    sel, n_valid, _ = MSO.select(got["counts"][None], 1, BIG)
    assert n_valid == 0 and sel[0] == -1 and got["counts"].tolist() == [0, 0, 0]
    assert not got["points"][:, :3].any()


def test_oracle_augmented_crop_with_disabled_records_is_the_plain_crop():
    rng = np.random.default_rng(7)
    pts = rng.uniform(-4, 4, (3000, 3)).astype(np.float32)
    box = np.concatenate([rng.uniform(-1, 1, 3), [1.6, 3.9, 1.5], MSO.rz(0.7).reshape(-1)]).astype(np.float32)
    off = {"enabled": 0, "box": box, "A": rng.normal(size=9).astype(np.float32), "c": rng.normal(size=3).astype(np.float32)}
    for mode, offset in ((TO.SUBWINDOW, 2.0), (TO.MODEL, 0.0)):
        want = TO.crop(pts, box, 1.25, offset, mode, 500)
        for rec in (None, off):
            got = MSO.crop_aug(pts, box, 1.25, offset, mode, rec, 500)
            assert got[0] == want[0] > 0 and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
    on = dict(off, enabled=1)
    moved = MSO.aug_points(pts, on)
    inside = MSO.inside_box(pts, box, 1.25)[0]
    assert 0 < inside.sum() < 3000 and np.array_equal(moved[~inside], pts[~inside]) and not np.array_equal(moved[inside], pts[inside])


def test_oracle_augment_is_apply_transform():
    """A and c' move a point exactly as apply_transform does: to the box frame, flip, rotate, translate, back (fp64 here;
    the fixture cases pin it on the reference's own code)"""
    rng = np.random.default_rng(9)
    for flip_x, flip_y in ((0, 0), (1, 0), (0, 1), (1, 1)):
        gt = np.concatenate([rng.uniform(-20, 20, 3), [1.6, 3.9, 1.5], MSO.rz(rng.uniform(-3, 3)).reshape(-1)]).astype(np.float32)
        draw = np.array([0.1, -0.2, 0.3, 7.0, flip_x, flip_y], np.float32)
        c, R2, A = MSO.augment64(gt, draw)
        R, c0 = gt[6:].astype(np.float64).reshape(3, 3), gt[:3].astype(np.float64)
        p = rng.uniform(-1, 1, (50, 3)) + c0
        q = (p - c0) @ R
        q = q * np.array([-1.0 if flip_x else 1.0, -1.0 if flip_y else 1.0, 1.0])
        q = q @ MSO.rz(np.deg2rad(7.0)).T + draw[:3].astype(np.float64)
        want = q @ R.T + c0
        assert np.abs((p - c0) @ A.reshape(3, 3).T + c - want).max() < 1e-12
        assert np.abs(R2.reshape(3, 3) - R @ MSO.rz(np.deg2rad(7.0)) @ (MSO.rz(np.pi) if flip_x else np.eye(3))).max() < 1e-12
        box, rec = MSO.augment(gt, draw)
        assert np.array_equal(box[3:6], gt[3:6]) and np.array_equal(rec["box"], gt) and np.array_equal(rec["c"], box[:3])


# ---- the selection -------------------------------------------------------------------------------------------------------------------
OK_ROW, FEW_IN_BOX, FEW_THIS = (11, 0, 21), (10, 500, 500), (500, 500, 20)
SELECT_PATTERNS = {
    "all": ([OK_ROW] * 6, 4, [0, 1, 2, 3], 6),
    "none": ([FEW_IN_BOX, FEW_THIS, FEW_IN_BOX], 2, [-1, -1], 0),
    "alternating": ([FEW_IN_BOX, OK_ROW, FEW_THIS, OK_ROW, FEW_IN_BOX, OK_ROW], 4, [1, 3, 5, 1], 3),
    "fewer_than_B": ([OK_ROW, FEW_IN_BOX, OK_ROW, FEW_THIS, FEW_IN_BOX], 5, [0, 2, 0, 2, 0], 2),
}


@pytest.mark.parametrize("name", list(SELECT_PATTERNS))
def test_selection_rule(name):
    counts, B, want, n_valid = SELECT_PATTERNS[name]
    sel, nv, over = MSO.select(np.array(counts, np.int32), B, BIG)
    assert sel.tolist() == want and nv == n_valid and over == 0


def test_selection_overflow_counts_the_chosen_crops():
    counts = np.array([(30, 40, 50), (5, 50, 50), (11, 100, 25)], np.int32)
    sel, nv, over = MSO.select(counts, 3, (32, 32))
    assert sel.tolist() == [0, 2, 0] and nv == 2
    assert over == 2 + 1 + 2                           # the in-box count is no crop: it never overflows


# ---- the builder's host side ---------------------------------------------------------------------------------------------------------
def test_builder_sizes_draws_and_the_sampler_refusal():
    from open3dsot_amd import sampler
    assert sampler.MOTION_DATA_KEYS == dict(bb_scale=1.25, bb_offset=2, point_sample_size=1024, degrees=False, data_limit_box=True,
                                            num_candidates=4, motion_threshold=0.15, use_augmentation=True, box_aware=True)
    with pytest.raises(ValueError):
        sampler.MotionBatchBuilder({}, 8, candidates=4)
    b = sampler.MotionBatchBuilder({}, 48)
    assert b.J == 60 and b.N == 1024 and b.box_aware and b.augment and not b.degrees and b.motion_threshold == 0.15
    off = b.draw_offsets([0, 1, 2, 3])
    assert not off[0].any() and off[1:].all() and np.abs(off[:, :2]).max() <= 0.3 and np.abs(off[:, 2]).max() <= 0.3 * np.deg2rad(5)
    a_prev, a_this = b.draw_augmentation(500)
    assert a_prev.shape == a_this.shape == (500, 6) and not np.array_equal(a_prev, a_this)
    assert np.abs(a_prev[:, :3]).max() <= 0.3 and 9 < np.abs(a_prev[:, 3]).max() <= 10
    assert set(np.unique(a_prev[:, 4:])) == {0.0, 1.0} and 0.4 < a_this[:, 4:].mean() < 0.6
    with pytest.raises(ValueError, match="random_sample"):
        sampler.DeviceBatchSampler([], b, random_sample=True)
    with pytest.raises(NotImplementedError):                # the siamese builder's augmentation stays out of scope
        sampler.SiameseBatchBuilder(dict(use_augmentation=True), 4)
