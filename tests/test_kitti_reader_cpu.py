"""The KITTI reader (open3dsot_amd/datasets.py, csrc/preload.hip) without a GPU: the host parser against the reference's own
kittiDataset (tests/golden/ref_kitti.npz, made on the tree of tests/kitti_tree.py), the numpy restatement of the device rule
(tests/kitti_oracle.py) against every cloud of that fixture bit for bit, the argument checks of the three entry points and
the refusal of a CPU device."""
import ctypes
import os

import numpy as np
import pytest

import fixture_io
import kitti_oracle as KO
import kitti_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_kitti.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return kitti_tree.build(str(tmp_path_factory.mktemp("kitti") / "tree"))


def cases(ref):
    """(name, mode, offset, category, split) of every case of the fixture"""
    out = []
    for k in ref.files:
        if k.endswith(".lengths"):
            mode, offset, category, split = k[:-len(".lengths")].split(".")
            out.append((k[:-len(".lengths")], mode, int(offset), category, split))
    return out


def ref_clouds(ref, name):
    """the fixture's clouds of a case, cut into tracklets"""
    flat = [ref["cloud.%d" % i] for i in ref[name + ".cloud_ids"]]
    ends = np.cumsum(ref[name + ".lengths"])
    return [flat[a:b] for a, b in zip(np.concatenate([[0], ends[:-1]]), ends)]


def read_bin(tree):
    def read(scene, frame):
        file = os.path.join(tree, "velodyne", scene, "%06d.bin" % frame)
        return np.fromfile(file, np.float32).reshape(-1, 4) if os.path.exists(file) else None
    return read


def test_the_fixture_covers_the_issue_cases(ref):
    got = {(m, o, c) for _, m, o, c, s in cases(ref) if s == "traintiny"}
    assert got == {(m, o, c) for m in ("velodyne", "camera") for o in (10, -1) for c in ("Car", "All", "Other")}
    assert any(s == "testtiny" for *_, s in cases(ref))
    car = ref["velodyne.10.Car.traintiny.lengths"]
    clouds = sum(ref_clouds(ref, "velodyne.10.Car.traintiny"), [])
    sizes = [c.shape[0] for c in clouds]
    assert list(car) == [6, 4, 2]                                   # tracks 0, 3 (with its gap), 4 (the far box)
    assert 0 in sizes and 1 in sizes and max(sizes) > 256           # an empty crop, the missing file's one point, several blocks
    assert list(ref["velodyne.10.Car.traintiny.frames"][6:10]) == [0, 1, 4, 5]


def test_scene_lists_per_split_string(ref):
    from open3dsot_amd import datasets as D
    splits = [k[len("scenes."):] for k in ref.files if k.startswith("scenes.")]
    assert len(splits) >= 10
    for s in splits:
        assert D.kitti_scene_list(s) == [str(x) for x in ref["scenes." + s]], s
    assert D.kitti_scene_list("traintiny") == ["0000"] and D.kitti_scene_list("testtiny") == ["0019"]
    assert len(D.kitti_scene_list("whatever")) == 21


def test_parser_equals_the_reference(ref, tree):
    """tracklet order and lengths, frame numbers, and boxes to 1e-9 absolute in fp64: a box is a dozen fp64 operations on
    magnitudes <= 100 m (error <= 1e-13), so 1e-9 is margin; the packed float32 boxes equal the float32 cast of the fixture's"""
    from open3dsot_amd import datasets as D
    for name, mode, offset, category, split in cases(ref):
        annos, calibs = D.kitti_annotations(tree, split, category, mode)
        assert [len(a["frames"]) for a in annos] == list(ref[name + ".lengths"]), name
        assert [a["scene"] for a in annos] == [str(s) for s in ref[name + ".scenes"]], name
        assert [a["track_id"] for a in annos] == list(ref[name + ".track_ids"]), name
        assert np.array_equal(np.concatenate([a["frames"] for a in annos]), ref[name + ".frames"]), name
        boxes = np.concatenate([a["boxes"] for a in annos])
        assert boxes.dtype == np.float64 and boxes.shape == ref[name + ".boxes"].shape
        err = np.abs(boxes - ref[name + ".boxes"]).max()
        assert err <= 1e-9, (name, err)
        assert np.array_equal(boxes.astype(np.float32), ref[name + ".boxes"].astype(np.float32)), name
    other = [a["track_id"] for a in D.kitti_annotations(tree, "traintiny", "Other")[0]]
    assert other == [0, 1, 3, 2, 4, 5]                              # first appearance in the file, DontCare dropped, Misc kept
    assert [a["track_id"] for a in D.kitti_annotations(tree, "traintiny", "All")[0]] == [0, 1, 3, 2, 4]


def test_calibration_lines_that_do_not_reshape_are_skipped(tree):
    from open3dsot_amd import datasets as D
    calib = D.read_kitti_calib(os.path.join(tree, "calib", "0000.txt"))
    assert set(calib) == {"P0:", "Tr_velo_cam", "Tr_imu_velo"}      # the 9-value R_rect line is gone
    assert np.allclose(calib["Tr_velo_cam"], kitti_tree.velo_to_cam("0000"), atol=1e-12, rtol=0)


def test_directional_rounding():
    from open3dsot_amd import datasets as D
    rng = np.random.default_rng(0)
    m = np.concatenate([rng.normal(scale=50.0, size=2000), np.float32(rng.normal(size=50)).astype(np.float64),
                        [0.0, -0.0, 1e-50, -1e-50, 1e39, -1e39, np.inf, -np.inf, 3.4028234663852886e38]])
    up, down = D.round_up_f32(m), D.round_down_f32(m)
    assert up.dtype == down.dtype == np.float32
    assert (up.astype(np.float64) >= m).all() and (down.astype(np.float64) <= m).all()
    with np.errstate(over="ignore"):
        exact = m.astype(np.float32).astype(np.float64) == m
    assert np.array_equal(up[exact], down[exact])
    with np.errstate(over="ignore"):
        assert np.array_equal(np.nextafter(down[~exact], np.float32(np.inf)), up[~exact])  # neighbours: nothing lies between
    for i, v in enumerate(m):
        assert KO.f32_at_least(v) == up[i] and KO.f32_at_most(v) == down[i]
    box = np.concatenate([[1.0, 2.0, 3.0], [2.0, 4.0, 1.5], np.eye(3).reshape(-1)])
    assert np.array_equal(D.preload_bounds(box[None], 10)[0], np.array([-11, -9, -7.75, 13, 13, 13.75], np.float32))
    assert np.array_equal(D.preload_bounds(box[None], 10)[0], KO.bounds(box, 10))
    assert np.array_equal(D.preload_bounds(box[None], -1)[0], np.array([-np.inf] * 3 + [np.inf] * 3, np.float32))


def test_oracle_equals_every_reference_cloud_bit_for_bit(ref, tree):
    """the device rule -- directional float32 bounds, ordered fp64 transform, strict compares, order kept -- restated in numpy
    reproduces the reference's preload on every case: this pins the specification without a GPU"""
    from open3dsot_amd import datasets as D
    n = 0
    for name, mode, offset, category, split in cases(ref):
        annos, calibs = D.kitti_annotations(tree, split, category, mode)
        got = KO.reader(annos, calibs, mode, offset, read_bin(tree))
        want = ref_clouds(ref, name)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert len(g) == len(w)
            for t, (a, b) in enumerate(zip(g, w)):
                assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), (name, k, t)
                n += 1
    assert n > 200


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------
HAND_N = [0, 1, 256, 257, 1000, 5]
HAND_BOXES = [2, 0, 1, 33, 3, 0]


def hand_table():
    t = np.zeros((6, 6), np.int32)
    t[:, 0] = [0, 0, 1, 257, 514, 1514]
    t[:, 1] = HAND_N
    t[:, 3] = HAND_BOXES
    return t, 1519


def test_preload_scratch_against_a_hand_computed_plan():
    from open3dsot_amd import capi, points_utils as PU
    t, rows = hand_table()
    need, wgs, B = PU.preload_plan(t, rows)
    # W = 1 (empty, boxes), 0 (no box), 1, 2, 4, 0: scratch 1*2 + 1*1 + 2*33 + 4*3
    assert (need, wgs, B) == (81, 8, 39)
    assert list(t[:, 2]) == [0, 2, 2, 3, 36, 39] and list(t[:, 4]) == [0, 1, 1, 2, 4, 8] and list(t[:, 5]) == [0, 2, 2, 3, 69, 81]
    assert KO.plan(HAND_N, HAND_BOXES) == (list(t[:, 2]), list(t[:, 4]), list(t[:, 5]), 81, 8, 39)
    lib = capi.load()
    assert lib.o3d_preload_scratch(None, 0, 0, None) == 0                                   # no frame: nothing to plan
    assert lib.o3d_preload_scratch(None, 1, 0, None) == -1
    for col, bad in ((0, -1), (1, -1), (3, -1), (3, PU.PRELOAD_MAX_BOXES + 1), (0, 1515), (1, 6)):
        u = t.copy()
        u[5, col] = bad
        assert lib.o3d_preload_scratch(u.ctypes.data, 6, rows, None) == -1, (col, bad)
    assert lib.o3d_preload_scratch(t.ctypes.data, PU.PRELOAD_MAX_FRAMES + 1, rows, None) == -1
    assert lib.o3d_preload_scratch(t.ctypes.data, 6, PU.PRELOAD_MAX_ROWS + 1, None) == -1
    assert lib.o3d_preload_scratch(t.ctypes.data, 6, rows - 1, None) == -1
    big = np.zeros((3, 6), np.int32)                                                        # 2^31 words of scratch
    big[:, 1], big[:, 3] = 2 ** 28, 1024
    big[:, 0] = 0
    assert lib.o3d_preload_scratch(big.ctypes.data, 3, 2 ** 28, None) == -1
    assert (PU.PRELOAD_MAX_FRAMES, PU.PRELOAD_MAX_BOXES, PU.PRELOAD_MAX_ROWS) == (4096, 1024, 2 ** 29 - 1)


def test_preload_entries_refuse_bad_arguments_before_any_hip_call():
    """every bad argument gives O3D_EINVAL with a NULL stream and no device; the empty calls succeed without a launch"""
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL = capi.CONSTANTS["O3D_EINVAL"]
    t, rows = hand_table()
    need, wgs, B = PU.preload_plan(t, rows)
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                                              # never dereferenced: every call returns first
    tp = t.ctypes.data

    def count(raw=p, raw_rows=rows, frames=tp, dev_frames=p, F=6, bounds=p, B=B, transform=None, scratch=p, scratch_len=need, counts=p):
        return lib.o3d_preload_count(raw, raw_rows, frames, dev_frames, F, bounds, B, transform, scratch, scratch_len, counts, None)

    def scatter(raw=p, raw_rows=rows, frames=tp, dev_frames=p, F=6, bounds=p, B=B, transform=None, scratch=p, scratch_len=need,
                out_row=p, pool=p, pool_rows=100):
        return lib.o3d_preload_scatter(raw, raw_rows, frames, dev_frames, F, bounds, B, transform, scratch, scratch_len, out_row, pool,
                                       pool_rows, None)

    bad = [dict(raw=None), dict(raw=p + 4), dict(raw_rows=rows - 1), dict(raw_rows=-1), dict(raw_rows=PU.PRELOAD_MAX_ROWS + 1),
           dict(frames=None), dict(dev_frames=None), dict(F=4), dict(F=-1), dict(F=PU.PRELOAD_MAX_FRAMES + 1), dict(bounds=None),
           dict(B=B - 1), dict(B=B + 1), dict(B=-1), dict(scratch=None), dict(scratch_len=need - 1)]
    for kw in bad:
        assert count(**kw) == EINVAL, kw
        assert scatter(**kw) == EINVAL, kw
    assert count(counts=None) == EINVAL
    assert scatter(out_row=None) == EINVAL and scatter(pool=None) == EINVAL and scatter(pool_rows=-1) == EINVAL
    for col, v in ((2, 1), (4, 1), (5, 1), (3, PU.PRELOAD_MAX_BOXES + 1), (1, -1), (0, -1)):      # a table that is not the plan
        u = t.copy()
        u[3, col] = v
        assert count(frames=u.ctypes.data) == EINVAL and scatter(frames=u.ctypes.data) == EINVAL, (col, v)
    # the empty calls: no frame; frames without a box (whatever their n) -- nothing to launch, no pointer needed
    assert count(raw=None, raw_rows=0, frames=None, dev_frames=None, F=0, bounds=None, B=0, scratch=None, scratch_len=0, counts=None) == 0
    assert scatter(raw=None, raw_rows=0, frames=None, dev_frames=None, F=0, bounds=None, B=0, scratch=None, scratch_len=0, out_row=None,
                   pool=None, pool_rows=0) == 0
    e = np.zeros((2, 6), np.int32)
    e[:, 1] = [0, 7]
    assert PU.preload_plan(e, 7) == (0, 0, 0)
    assert count(raw=None, raw_rows=7, frames=e.ctypes.data, dev_frames=None, F=2, bounds=None, B=0, scratch=None, scratch_len=0,
                 counts=None) == 0
    assert scatter(raw=None, raw_rows=7, frames=e.ctypes.data, dev_frames=None, F=2, bounds=None, B=0, scratch=None, scratch_len=0,
                   out_row=None, pool=None, pool_rows=0) == 0
    assert count(F=0, B=1) == EINVAL                                                         # boxes without a frame


def test_the_wrappers_and_the_reader_refuse_the_cpu(tree):
    import torch
    from open3dsot_amd import datasets as D, points_utils as PU
    with pytest.raises(RuntimeError, match="CPU not supported"):
        D.KittiTracklets(tree, "traintiny", device="cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        D.KittiTracklets.load(os.path.join(tree, "nothing.npz"), device="cpu")
    t, rows = hand_table()
    PU.preload_plan(t, rows)
    z = torch.zeros((4, 4))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.preload_count(z, t, z, z, None, z, z)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.preload_scatter(z, t, z, z, None, z, z, z)


def test_no_pandas_in_the_product():
    src = open(os.path.join(ROOT, "open3dsot_amd", "datasets.py")).read()
    assert "pandas" not in src
