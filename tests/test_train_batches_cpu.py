"""Training batches built on the device, the part that needs no GPU: the numpy restatement (tests/sampler_oracle.py) against
the reference's own siamese_processing (tests/golden/ref_train_batches.npz), the index draw's properties, the selection rule,
and the host side of the library (the crop planner, struct sizes, argument validation)."""
import ctypes
import os
import re

import numpy as np
import pytest

import fixture_io
import sampler_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"bat": True, "p2b": False, "sparse": True}       # case -> box_aware
BIG = (1 << 20,) * 3                                      # capacities that truncate nothing


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_train_batches.npz"))


def case_inputs(ref, case):
    from open3dsot_amd import sampler, synth
    cfg = dict(sampler.DATA_KEYS, box_aware=CASES[case])
    frames, gt = synth.make_sequence(int(ref[case + ".seq_seed"]), 8, int(ref[case + ".n_points"]))
    return cfg, frames, gt, [tuple(int(v) for v in s) for s in ref[case + ".samples"]]


@pytest.fixture(scope="module")
def oracle_runs(ref):
    """the oracle, teacher-forced with the reference's draws, on every sample of the fixture: computed once"""
    runs = {}
    for case in CASES:
        cfg, frames, gt, samples = case_inputs(ref, case)
        for s, sample in enumerate(samples):
            k = "%s.s%d." % (case, s)
            runs[k] = SO.candidate(frames, gt, sample, cfg, ref[k + "offset_t"], ref[k + "offset_s"], BIG, ref[k + "idx_t"],
                                   ref[k + "idx_s"])
    return runs


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_matches_the_reference(ref, oracle_runs, case):
    n = ref[case + ".samples"].shape[0]
    assert n == 8
    for s in range(n):
        k = "%s.s%d." % (case, s)
        got = oracle_runs[k]
        assert np.array_equal(got["counts"], ref[k + "counts"]), k
        SO.check_against_reference(got, ref, k, CASES[case])
        assert (k + "points2cc_dist_t" in ref) == CASES[case]
    if case == "sparse":                                   # the with-replacement route: both clouds shorter than their sample
        c = ref["sparse.s1.counts"]
        assert c[0] + c[1] < 512 and c[2] < 1024


def test_far_candidate_is_invalid(ref):
    """the reference raises its AssertionError for the candidate moved 500 m; the oracle's counts make it invalid"""
    assert bool(ref["far.raises"])
    cfg, frames, gt, _ = case_inputs(ref, "bat")
    gt = gt.copy()
    gt[:, 0] += float(ref["far.shift"])
    got = SO.candidate(frames, gt, tuple(int(v) for v in ref["far.sample"]), cfg, np.zeros(3), np.zeros(3), BIG)
    sel, n_valid, _ = SO.select(got["counts"][None], 1, BIG)
    assert n_valid == 0 and sel[0] == -1
    assert not got["template_points"].any() and not got["seg_label"].any()


# ---- the index draw ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 5, 20, 21, 511, 512, 513, 1025, 5000])
@pytest.mark.parametrize("S", [1, 64, 512])
def test_draw_properties(n, S):
    for key in (0, 1, 0xDEADBEEF, SO.draw_key(3, 7, 11, 1)):
        idx = SO.sample_indices(key, n, S)
        assert idx.shape == (S,) and idx.min() >= 0 and idx.max() < n
        if S < n:
            assert np.unique(idx).size == S            # a bijection's first S values: pairwise distinct
        if S == n:
            assert np.array_equal(idx, np.arange(n))


def test_draw_is_a_bijection_and_short_clouds_have_none():
    for n in (3, 4, 17, 1000):
        full = np.concatenate([SO.sample_indices(99, n, n - 1), []]).astype(np.int64)
        assert np.unique(full).size == n - 1
    assert SO.sample_indices(5, 2, 8) is None and SO.sample_indices(5, 0, 8) is None
    a, b = SO.sample_indices(SO.draw_key(0, 0, 0, 0), 1000, 100), SO.sample_indices(SO.draw_key(0, 1, 0, 0), 1000, 100)
    assert not np.array_equal(a, b)                    # the batch counter is part of the key


def test_draw_inclusion_frequency():
    """n = 1 000, S = 100 over 2 000 keys: every index is included 200 times in the mean, binomial sigma 13.4; within 6 sigma"""
    hits = np.zeros(1000, np.int64)
    for c in range(2000):
        hits[SO.sample_indices(SO.draw_key(1, c, 0, 0), 1000, 100)] += 1
    assert hits.sum() == 200000
    assert np.abs(hits - 200).max() <= 80, (hits.min(), hits.max())


# ---- the selection -------------------------------------------------------------------------------------------------------------------
OK_ROW, BAD_T, BAD_S = (15, 6, 21), (10, 10, 500), (500, 500, 20)
SELECT_PATTERNS = {
    "all": ([OK_ROW] * 6, 4, [0, 1, 2, 3], 6),
    "none": ([BAD_T, BAD_S, BAD_T], 2, [-1, -1], 0),
    "one": ([BAD_T, BAD_S, OK_ROW, BAD_S], 3, [2, 2, 2], 1),
    "first_invalid": ([BAD_S, OK_ROW, OK_ROW, OK_ROW], 3, [1, 2, 3], 3),
    "fewer_than_B": ([OK_ROW, BAD_T, OK_ROW, BAD_S, BAD_T], 5, [0, 2, 0, 2, 0], 2),
}


@pytest.mark.parametrize("name", list(SELECT_PATTERNS))
def test_selection_rule(name):
    counts, B, want, n_valid = SELECT_PATTERNS[name]
    sel, nv, over = SO.select(np.array(counts, np.int32), B, BIG)
    assert sel.tolist() == want and nv == n_valid and over == 0


def test_selection_overflow_counts_the_chosen_crops():
    counts = np.array([(30, 40, 50), (5, 5, 5), (10, 100, 25)], np.int32)
    sel, nv, over = SO.select(counts, 3, (32, 32, 32))
    assert sel.tolist() == [0, 2, 0] and nv == 2
    assert over == 2 + 1 + 2                           # rows 0 and 2 are candidate 0 (two crops over), row 1 candidate 2 (one)


# ---- the host side of the library ----------------------------------------------------------------------------------------------------
def test_struct_sizes_match_the_library():
    from open3dsot_amd import points_utils as PU
    assert PU.CROP_PLAN.itemsize == 48 and PU.CROP_TARGET.itemsize == 48 and ctypes.sizeof(PU._TrainSampleArgs) == 192
    src = open(os.path.join(ROOT, "open3dsot_amd", "csrc", "train_batch.hip")).read()
    for name, size in (("o3d_crop_target", 48), ("o3d_crop_plan", 48), ("o3d_train_sample_args", 192)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in src
    hdr = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*o3d_train_sample_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = re.match(r"(?:const\s+)?\w+\s*\**\s*(.*)", decl).group(1)
            fields += [n.strip().lstrip("*").strip() for n in names.split(",")]
    assert fields == [f[0] for f in PU._TrainSampleArgs._fields_]
    assert [n for n in PU.CROP_PLAN.names] == ["points", "n", "targets", "n_targets", "wg_start", "row_start", "sbase"]


def test_crop_planner():
    """o3d_track_crop_groups_scratch is host code: first workgroup, first row and first scratch word of every group"""
    from open3dsot_amd import points_utils as PU
    ns, ks = [0, 1, 255, 256, 257, 1000, 120000], [1, 4, 33, 1, 2, 1024, 3]
    plan = np.zeros(len(ns), PU.CROP_PLAN)
    plan["points"], plan["targets"], plan["n"], plan["n_targets"] = 4096, 8192, ns, ks
    need, wgs, rows = PU.crop_groups_plan(plan)
    W = [max(1, -(-n // 256)) for n in ns]
    assert W == [1, 1, 1, 1, 2, 4, 469]
    assert plan["wg_start"].tolist() == np.concatenate([[0], np.cumsum(W)[:-1]]).tolist() and wgs == sum(W)
    assert plan["row_start"].tolist() == np.concatenate([[0], np.cumsum(ks)[:-1]]).tolist() and rows == sum(ks)
    words = [w * k for w, k in zip(W, ks)]
    assert plan["sbase"].tolist() == np.concatenate([[0], np.cumsum(words)[:-1]]).tolist() and need == sum(words)
    for field, bad in (("n", -1), ("n_targets", 0), ("n_targets", 1025), ("targets", 0), ("points", 0)):
        p = plan.copy()
        p[field][5] = bad
        with pytest.raises(Exception, match="bad table"):
            PU.crop_groups_plan(p)
    lib = __import__("open3dsot_amd.capi", fromlist=["x"]).load()
    assert lib.o3d_track_crop_groups_scratch(None, 1, None) == -1
    assert lib.o3d_track_crop_groups_scratch(plan.ctypes.data, 0, None) == -1
    big = np.zeros(PU.CROP_MAX_GROUPS + 1, PU.CROP_PLAN)
    big["targets"], big["n_targets"] = 8192, 1
    assert lib.o3d_track_crop_groups_scratch(big.ctypes.data, PU.CROP_MAX_GROUPS + 1, None) == -1
    assert lib.o3d_track_crop_groups_scratch(big.ctypes.data, PU.CROP_MAX_GROUPS, None) == PU.CROP_MAX_GROUPS


def test_entries_validate_before_any_launch():
    """the four entries return O3D_EINVAL (-1) for NULL operands, sizes out of range and a table whose plan is wrong, before
    any HIP call (host buffers stand in for device pointers: nothing dereferences them)"""
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    plan = np.zeros(2, PU.CROP_PLAN)
    plan["points"], plan["targets"], plan["n"], plan["n_targets"] = p, p, [300, 10], [2, 3]
    need = PU.crop_groups_plan(plan)[0]
    assert need == 2 * 2 + 3
    assert lib.o3d_track_crop_groups(None, p, 2, p, need, None) == -1
    assert lib.o3d_track_crop_groups(plan.ctypes.data, None, 2, p, need, None) == -1
    assert lib.o3d_track_crop_groups(plan.ctypes.data, p, 2, None, need, None) == -1
    assert lib.o3d_track_crop_groups(plan.ctypes.data, p, 2, p, need - 1, None) == -1          # scratch too short
    assert lib.o3d_track_crop_groups(plan.ctypes.data, p, 0, p, need, None) == -1
    assert lib.o3d_track_crop_groups(plan.ctypes.data, p, PU.CROP_MAX_GROUPS + 1, p, need, None) == -1
    for field in ("wg_start", "row_start", "sbase"):                                            # a plan that was not planned
        bad = plan.copy()
        bad[field][1] += 1
        assert lib.o3d_track_crop_groups(bad.ctypes.data, p, 2, p, need + 8, None) == -1
    assert lib.o3d_train_select(None, 4, 2, 8, 8, 8, p, p, p, None) == -1
    assert lib.o3d_train_select(p, 4, 5, 8, 8, 8, p, p, p, None) == -1                          # B > J
    assert lib.o3d_train_select(p, 1025, 2, 8, 8, 8, p, p, p, None) == -1
    assert lib.o3d_train_select(p, 4, 0, 8, 8, 8, p, p, p, None) == -1
    assert lib.o3d_train_select(p, 4, 2, 8, -1, 8, p, p, p, None) == -1
    assert lib.o3d_train_select(p, 4, 2, 8, 8, 8, p, p, None, None) == -1
    assert lib.o3d_train_labels(p, p, p, p, 0, p, p, p, p, None) == -1
    assert lib.o3d_train_labels(p, p, None, p, 4, p, p, p, p, None) == -1
    assert lib.o3d_train_labels(p, p, p, p, 4, p, p, p, None, None) == -1
    assert lib.o3d_train_sample(None, None) == -1

    def args(**over):
        a = PU._TrainSampleArgs(p, p, p, p, p, 8, 8, 8, 4, 2, 16, 16, None, None, 0, 0, p, p, p, p, p, p, p, p, p, None, None, None)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    for over in (dict(sel=None), dict(crop_search=None), dict(B=5), dict(J=0), dict(M=0), dict(N=(1 << 20) + 1), dict(cap_first=-1),
                 dict(idx_t=p), dict(idx_s=p), dict(seg_label=None), dict(search_box=None), dict(bbox_size=None)):
        a = args(**over)
        assert lib.o3d_train_sample(ctypes.addressof(a), None) == -1, over


def test_builder_refuses_augmentation_and_bad_sizes():
    from open3dsot_amd import sampler
    with pytest.raises(NotImplementedError):
        sampler.SiameseBatchBuilder(dict(use_augmentation=True), 4)
    with pytest.raises(ValueError):
        sampler.SiameseBatchBuilder({}, 8, candidates=4)
    b = sampler.SiameseBatchBuilder({}, 48)
    assert b.J == 60 and (b.M, b.N) == (512, 1024) and b.box_aware and b.degrees
    off_t, off_s = b.draw_offsets([0, 1, 2, 3])
    assert not off_t[0].any() and not off_s[0].any() and off_t[1:].all() and off_s[1:].all()
    assert np.abs(off_t[:, :2]).max() <= 0.3 and np.abs(off_t[:, 2]).max() <= 1.5
