"""The Waymo reader (open3dsot_amd/datasets.py, csrc/preload.hip) without a GPU: the host half against the reference's own
WaymoDataset (tests/golden/ref_waymo.npz, made on the tree of tests/waymo_tree.py, sot_infos by the reference's
generate_waymo_data), the numpy restatement of the device rule (tests/waymo_oracle.py) against every cloud of that fixture
bit for bit, the argument checks of the two posed entry points and the refusal of a CPU device.  Every comparison is exact."""
import ctypes
import os
import pickle

import numpy as np
import pytest

import fixture_io
import waymo_oracle as WO
import waymo_tree
from waymo_oracle import cases, ref_clouds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_waymo.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the tree with sot_infos written by the package's generate_waymo_sot_infos"""
    from open3dsot_amd import datasets as D
    return waymo_tree.build(str(tmp_path_factory.mktemp("waymo") / "tree"), D.generate_waymo_sot_infos)


def rel_files(tree, annos):
    return [os.path.relpath(f, tree) for a in annos for f in a["files"]]


def test_the_fixture_covers_the_issue_cases(ref):
    got = {(c, o) for _, c, o, s, t in cases(ref) if s == "train" and not t}
    assert got == {(c, o) for c in waymo_tree.CLASSES for o in (10, -1)}
    assert sum(t for *_, t in cases(ref)) == 1 and any(s == "val" for _, _, _, s, _ in cases(ref))
    name = "VEHICLE.10.train"
    assert list(ref[name + ".keys"]) == ["s0_veh_a", "s0_veh_b", "s0_veh_far", "s1_veh_a", "s1_veh_b", "s1_veh_far"]
    assert list(ref[name + ".lengths"]) == [6, 4, 2, 5, 3, 2]       # every frame; the gap; the far box, per sequence
    sizes = [c.shape[0] for t in ref_clouds(ref, name) for c in t]
    assert sizes[4] == 0 and sizes[10] == sizes[11] == 0 and max(sizes) > 256       # the empty frame, the far box, several blocks
    files = list(ref[name + ".files"])
    assert files[0] == os.path.join("train", "lidar", "seq_0_frame_0.pkl") and files[6:10] == [files[0], files[1], files[4], files[5]]
    assert list(ref["VEHICLE.10.val.lengths"]) == [1] * 102 and list(ref["VEHICLE.10.val.tiny.lengths"]) == [1] * 100
    shared = [c.shape[0] for t in ref_clouds(ref, "VEHICLE.-1.train") for c in t]
    assert shared[0] == shared[6] and 300 <= shared[0] <= 2000      # uncropped: whole frames
    centre = ref[name + ".boxes"][:, :3]
    assert 1e3 < np.abs(centre[:, :2]).min() and np.abs(centre).max() < 3e4         # the global frame: kilometres


def test_names_are_handled_as_the_reference_handles_them(tree):
    from open3dsot_amd import datasets as D
    assert D.waymo_names("TEST", "Vehicle") == ("val", "vehicle") and D.waymo_names("Train", "CYCLIST") == ("train", "cyclist")
    assert D.waymo_names("val", "pedestrian") == ("val", "pedestrian")
    for split, category in (("valid", "VEHICLE"), ("traintiny", "VEHICLE"), ("", "VEHICLE"), ("train", "Car"), ("train", "SIGN")):
        with pytest.raises(ValueError):
            D.waymo_names(split, category)
        with pytest.raises(ValueError):
            D.waymo_annotations(tree, split, category)
    a = D.waymo_annotations(tree, "test", "VEHICLE")[0]
    b = D.waymo_annotations(tree, "VAL", "vehicle")[0]
    assert [t["key"] for t in a] == [t["key"] for t in b] and len(a) == 102


def test_host_half_equals_the_reference(ref, tree):
    """tracklet order, lengths, file names and the fp64 boxes byte for byte: the host half does the reference's operations in
    the reference's order on the same numpy"""
    from open3dsot_amd import datasets as D
    for name, category, offset, split, tiny in cases(ref):
        annos, files, poses = D.waymo_annotations(tree, split, category, tiny)
        assert [a["key"] for a in annos] == [str(k) for k in ref[name + ".keys"]], name
        assert [len(a["frames"]) for a in annos] == list(ref[name + ".lengths"]), name
        assert rel_files(tree, annos) == [str(f) for f in ref[name + ".files"]], name
        boxes = np.concatenate([a["boxes"] for a in annos])
        assert boxes.dtype == np.float64 and boxes.tobytes() == ref[name + ".boxes"].tobytes(), name
        assert poses.dtype == np.float64 and poses.shape == (len(files), 3, 4) and len(set(files)) == len(files)
        assert [files[f] for a in annos for f in a["frames"]] == [f for a in annos for f in a["files"]]
        rot = poses[:, :, :3]
        assert np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
        assert 1e3 < np.abs(poses[:, :, 3]).min() and np.abs(poses[:, :, 3]).max() < 2e4


def test_tiny_keeps_100_of_102(tree):
    from open3dsot_amd import datasets as D
    full = D.waymo_annotations(tree, "val", "VEHICLE")[0]
    tiny = D.waymo_annotations(tree, "val", "VEHICLE", tiny=True)[0]
    assert len(full) == 102 and len(tiny) == 100 and [a["key"] for a in tiny] == [a["key"] for a in full[:100]]
    assert len(D.waymo_annotations(tree, "val", "VEHICLE", tiny=True)[1]) == 2          # two frame files serve them all


def test_every_annotation_file_is_read_once(tree, monkeypatch):
    from open3dsot_amd import datasets as D
    opened = []
    real = D._unpickle
    monkeypatch.setattr(D, "_unpickle", lambda f: (opened.append(f), real(f))[1])
    annos, files, poses = D.waymo_annotations(tree, "train", "VEHICLE")
    assert len(files) == 11 and sum(len(a["frames"]) for a in annos) == 22
    assert sorted(opened[1:]) == sorted(f.replace("lidar", "annos") for f in files) and opened[0].endswith("sot_infos_vehicle_train.pkl")


def test_generate_waymo_sot_infos_reproduces_the_reference(ref, tree):
    """the sot_infos dicts written by datasets.generate_waymo_sot_infos (the tree fixture) against those the reference's
    generate_waymo_data wrote when the fixture was made: keys, order, files, boxes, class"""
    for split in ("train", "val"):
        for cls in waymo_tree.CLASSES:
            with open(os.path.join(tree, "sot_infos_%s_%s.pkl" % (cls.lower(), split)), "rb") as f:
                sot = pickle.load(f)
            k = "sot.%s.%s." % (cls, split)
            assert type(sot) is dict and list(sot) == [str(x) for x in ref[k + "keys"]], k
            assert [len(v) for v in sot.values()] == list(ref[k + "lengths"])
            assert [os.path.relpath(a["PC"], tree) for v in sot.values() for a in v] == [str(f) for f in ref[k + "files"]]
            boxes = np.array([a["Box"] for v in sot.values() for a in v], np.float32).reshape(-1, 9)
            assert all(a["Box"].dtype == np.float32 for v in sot.values() for a in v)
            assert boxes.tobytes() == ref[k + "boxes"].tobytes()
            assert all(a["Class"] == cls and set(a) == {"PC", "Box", "Class"} for v in sot.values() for a in v)
    assert len(ref["sot.VEHICLE.train.keys"]) == 6 and len(ref["sot.CYCLIST.val.keys"]) == 1


def test_a_missing_sot_infos_file_is_named(tree, tmp_path):
    from open3dsot_amd import datasets as D
    with pytest.raises(FileNotFoundError, match="generate_waymo_sot_infos"):
        D.waymo_annotations(str(tmp_path), "train", "VEHICLE")


def test_relative_paths_resolve_against_root(ref, tmp_path):
    """root=None opens the 'PC' strings as they stand; a tree with relative strings needs root"""
    from open3dsot_amd import datasets as D
    rel = waymo_tree.build(str(tmp_path / "rel"), D.generate_waymo_sot_infos, absolute=False)
    annos, files, poses = D.waymo_annotations(rel, "train", "PEDESTRIAN", root=rel)
    assert files[0] == os.path.join("train", "lidar", "seq_0_frame_1.pkl")
    boxes = np.concatenate([a["boxes"] for a in annos])
    assert boxes.tobytes() == ref["PEDESTRIAN.10.train.boxes"].tobytes()
    with pytest.raises(FileNotFoundError):
        D.waymo_annotations(rel, "train", "PEDESTRIAN")


def test_oracle_equals_every_reference_cloud_bit_for_bit(ref, tree):
    """the device rule -- ordered fp64 pose transform rounded once, directional float32 bounds, strict compares, order kept --
    restated in numpy reproduces the reference's preload on every case: this pins the specification without a GPU"""
    from open3dsot_amd import datasets as D
    n = 0
    for name, category, offset, split, tiny in cases(ref):
        annos, files, poses = D.waymo_annotations(tree, split, category, tiny)
        got = WO.reader(annos, files, poses, offset, D.waymo_points)
        want = ref_clouds(ref, name)
        assert [len(g) for g in got] == [len(w) for w in want] == list(ref[name + ".lengths"]), name
        for k, (g, w) in enumerate(zip(got, want)):
            for t, (a, b) in enumerate(zip(g, w)):
                assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (name, k, t)
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, k, t)
                n += 1
    assert n > 300


def test_points_must_be_float32(tree, tmp_path):
    from open3dsot_amd import datasets as D
    good = os.path.join(tree, "train", "lidar", "seq_0_frame_0.pkl")
    pts = D.waymo_points(good)
    assert pts.dtype == np.float32 and pts.ndim == 2 and pts.shape[1] == 3 and pts.flags.c_contiguous
    assert D.waymo_points(os.path.join(tree, "train", "lidar", "seq_0_frame_4.pkl")).shape == (0, 3)
    for bad in (pts.astype(np.float64), pts.astype(np.float16), np.zeros((5, 4), np.float32)):
        file = str(tmp_path / "bad.pkl")
        with open(file, "wb") as f:
            pickle.dump({"lidars": {"points_xyz": bad}}, f)
        with pytest.raises(ValueError, match="float32"):
            D.waymo_points(file)


def test_the_reader_refuses_the_cpu(tree):
    import torch
    from open3dsot_amd import datasets as D, points_utils as PU
    with pytest.raises(RuntimeError, match="CPU not supported"):
        D.WaymoTracklets(tree, "train", device="cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        D.WaymoTracklets.load(os.path.join(tree, "nothing.npz"), device="cpu")
    t = np.zeros((1, 6), np.int32)
    t[0, 1], t[0, 3] = 4, 1
    PU.preload_plan(t, 4)
    z = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.preload_count(z, t, z, z, None, z, z, poses=z)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.preload_scatter(z, t, z, z, None, z, z, z, poses=z)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------
def hand_table():
    t = np.zeros((6, 6), np.int32)
    t[:, 0] = [0, 0, 1, 257, 514, 1514]
    t[:, 1] = [0, 1, 256, 257, 1000, 5]
    t[:, 3] = [2, 0, 1, 33, 3, 0]
    return t, 1519


def test_posed_entries_refuse_bad_arguments_before_any_hip_call():
    """every bad argument gives O3D_EINVAL with a NULL stream and no device; the empty calls succeed without a launch"""
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL = capi.CONSTANTS["O3D_EINVAL"]
    t, rows = hand_table()
    need, wgs, B = PU.preload_plan(t, rows)
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                                              # never dereferenced: every call returns first
    tp = t.ctypes.data

    def count(raw=p, raw_rows=rows, row_floats=3, frames=tp, dev_frames=p, F=6, bounds=p, B=B, poses=p, scratch=p, scratch_len=need,
              counts=p):
        return lib.o3d_preload_posed_count(raw, raw_rows, row_floats, frames, dev_frames, F, bounds, B, poses, scratch, scratch_len, counts,
                                           None)

    def scatter(raw=p, raw_rows=rows, row_floats=3, frames=tp, dev_frames=p, F=6, bounds=p, B=B, poses=p, scratch=p, scratch_len=need,
                out_row=p, pool=p, pool_rows=100):
        return lib.o3d_preload_posed_scatter(raw, raw_rows, row_floats, frames, dev_frames, F, bounds, B, poses, scratch, scratch_len,
                                             out_row, pool, pool_rows, None)

    bad = [dict(row_floats=2), dict(row_floats=5), dict(row_floats=0), dict(row_floats=-3), dict(poses=None), dict(poses=p + 4),
           dict(poses=p + 1), dict(raw=p + 4, row_floats=4), dict(raw=p + 2), dict(raw=p + 1, row_floats=4),
           # what the existing pair refuses
           dict(raw=None), dict(raw_rows=rows - 1), dict(raw_rows=-1), dict(raw_rows=PU.PRELOAD_MAX_ROWS + 1),
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
    # the empty calls: no frame (no pose is needed); frames without a box -- nothing to launch
    for rf in (3, 4):
        assert count(raw=None, raw_rows=0, row_floats=rf, frames=None, dev_frames=None, F=0, bounds=None, B=0, poses=None, scratch=None,
                     scratch_len=0, counts=None) == 0
        assert scatter(raw=None, raw_rows=0, row_floats=rf, frames=None, dev_frames=None, F=0, bounds=None, B=0, poses=None, scratch=None,
                       scratch_len=0, out_row=None, pool=None, pool_rows=0) == 0
    e = np.zeros((2, 6), np.int32)
    e[:, 1] = [0, 7]
    assert PU.preload_plan(e, 7) == (0, 0, 0)
    kw = dict(raw=None, raw_rows=7, frames=e.ctypes.data, dev_frames=None, F=2, bounds=None, B=0, scratch=None, scratch_len=0)
    assert count(counts=None, **kw) == 0 and scatter(out_row=None, pool=None, pool_rows=0, **kw) == 0
    assert count(counts=None, poses=None, **kw) == EINVAL                                    # F = 2: the poses are asked for
    assert count(F=0, B=1) == EINVAL                                                         # boxes without a frame
    assert count(F=0, row_floats=2, B=0) == EINVAL
    # a raw table of four floats a row needs 16-byte alignment (that three floats a row need only 4 is shown on the GPU: a
    # call that passes every check launches)
    assert scatter(raw=p + 4, row_floats=4) == EINVAL
