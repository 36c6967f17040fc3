"""The NuScenes reader (open3dsot_amd/datasets.py, csrc/preload.hip) without a GPU: the host half against the reference's own
NuScenesDataset (tests/golden/ref_nuscenes.npz, made on the tree of tests/nuscenes_tree.py over the stand-in devkit of
tests/golden/nuscenes_standin.py, under numpy >= 2), the numpy restatement of the steps rule (tests/nuscenes_oracle.py) against
every cloud of that fixture bit for bit, the two translate modes against each other, the argument checks of the two steps
entry points and the refusal of a CPU device.  Every comparison is exact."""
import ctypes
import os
import sys

import numpy as np
import pytest

import fixture_io
import nuscenes_oracle as NO
import nuscenes_tree
from nuscenes_oracle import cases, ref_clouds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = nuscenes_tree.VERSION


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_nuscenes.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return nuscenes_tree.build(str(tmp_path_factory.mktemp("nuscenes") / "tree"))


def annotations(tree, category, split, key_only=False, min_points=0, scenes=nuscenes_tree.SPLITS):
    from open3dsot_amd import datasets as D
    return D.nuscenes_annotations(tree, split, category, V, key_only, min_points, scenes)


def test_the_fixture_covers_the_issue_cases(ref):
    got = {c[1:] for c in cases(ref)}
    for category in ("car", "pedestrian", "bus"):
        for offset in (10, -1):
            assert (category, offset, "train", False, 0) in got
    assert ("truck", 10, "train", False, 0) in got and ("car", 10, "val", False, 0) in got and ("car", -1, "val", False, 0) in got
    assert {(k, m) for c, o, s, k, m in got if (c, o, s) == ("car", 10, "train")} == {(False, 0), (True, 0), (False, 1), (False, 5)}
    T = nuscenes_tree.token
    name = "car.10.train.k0.m0"
    want = [T("instance", s, n) for s in ("scene-0001", "scene-0002") for n in ("car_a", "car_b", "car_none", "car_few", "car_one")]
    assert [str(k) for k in ref[name + ".keys"]] == want
    assert list(ref[name + ".lengths"]) == [5, 4, 5, 5, 1, 4, 3, 4, 4, 1]       # instances sharing sweeps; the one-annotation tracklet
    files = [str(f) for f in ref[name + ".files"]]
    assert files[:5] == nuscenes_tree.sweeps()[:5] and files[5:9] == files[1:5]      # the KEY-FRAME LIDAR_TOP record of every sample
    assert all(f.startswith("samples/LIDAR_TOP/") for c in cases(ref) for f in ref[c[0] + ".files"])
    # min_points against the FIRST annotation only: 1 drops car_none (0 points), 5 drops car_few (3 points) as well
    assert [str(k) for k in ref["car.10.train.k0.m1.keys"]] == [k for k in want if k not in {T("instance", s, "car_none") for s in ("scene-0001", "scene-0002")}]
    assert len(ref["car.10.train.k0.m5.keys"]) == 6
    # key_frame_only drops nothing on a well-formed set
    for k in ("keys", "lengths", "files", "boxes", "cloud_ids"):
        assert ref["car.10.train.k1.m0." + k].tobytes() == ref[name + "." + k].tobytes()
    # two general classes under `pedestrian`; the ignored class is in no case; the class with no instance; the other split;
    # the scene in no split
    assert [str(k) for k in ref["pedestrian.10.train.k0.m0.keys"]] == [T("instance", s, n) for s in ("scene-0001", "scene-0002") for n in ("ped_a", "ped_c")]
    assert list(ref["bus.10.train.k0.m0.lengths"]) == [5, 4]
    assert len(ref["truck.10.train.k0.m0.keys"]) == 0 and ref["truck.10.train.k0.m0.boxes"].shape == (0, 15)
    assert list(ref["car.10.val.k0.m0.lengths"]) == [3, 2, 3, 3, 1]
    every = {str(k) for c in cases(ref) for k in ref[c[0] + ".keys"]}
    assert not any(T("instance", "scene-0004", n[0]) in every or T("instance", s, "barrier") in every
                   for n in nuscenes_tree.TRACKS for s, _ in nuscenes_tree.SCENES)
    shared = [c.shape[0] for t in ref_clouds(ref, "car.-1.train.k0.m0") for c in t]
    assert shared[1] == shared[5] and all(200 <= n <= 600 for n in shared)             # uncropped: whole sweeps
    cropped = [c.shape[0] for t in ref_clouds(ref, name) for c in t]
    assert 0 < min(cropped) and max(cropped) < 600 and sum(cropped) < sum(shared)
    centre = ref[name + ".boxes"][:, :3]
    assert 350 <= np.abs(centre[:, :2]).min() and np.abs(centre).max() <= 2000          # the global frame: hundreds of metres


def test_host_half_equals_the_reference(ref, tree):
    """tracklet order, lengths, instance tokens, file names and the fp64 boxes byte for byte"""
    for name, category, offset, split, key_only, min_points in cases(ref):
        annos, files, steps = annotations(tree, category.capitalize(), split, key_only, min_points)
        assert [a["key"] for a in annos] == [str(k) for k in ref[name + ".keys"]], name
        assert [len(a["frames"]) for a in annos] == list(ref[name + ".lengths"]), name
        assert [f for a in annos for f in a["files"]] == [str(f) for f in ref[name + ".files"]], name
        boxes = np.concatenate([a["boxes"] for a in annos] + [np.zeros((0, 15))])
        assert boxes.dtype == np.float64 and boxes.tobytes() == ref[name + ".boxes"].tobytes(), name
        assert steps.dtype == np.float64 and steps.shape == (len(files), 2, 12) and len(set(files)) == len(files)
        assert [files[f] for a in annos for f in a["frames"]] == [f for a in annos for f in a["files"]]
        if len(files):
            M = steps.reshape(-1, 2, 3, 4)
            assert np.abs(M[..., :3] @ M[..., :3].transpose(0, 1, 3, 2) - np.eye(3)).max() < 1e-12
            assert np.abs(M[:, 0, :, 3]).max() < 3 and 400 <= np.abs(M[:, 1, :2, 3]).min() and np.abs(M[:, 1, :, 3]).max() <= 2000


def test_min_points_false_is_the_reference_default(tree):
    """the reference's kwargs default is min_points=False, which compares as 0"""
    a = annotations(tree, "Car", "train", min_points=False)[0]
    b = annotations(tree, "Car", "train", min_points=0)[0]
    assert [t["key"] for t in a] == [t["key"] for t in b] and len(a) == 10


def test_every_json_table_is_read_once(tree, monkeypatch):
    from open3dsot_amd import datasets as D
    opened = []
    real = D._read_json
    monkeypatch.setattr(D, "_read_json", lambda f: (opened.append(f), real(f))[1])
    annotations(tree, "Car", "train")
    tables = ("category", "instance", "sample_annotation", "sample", "sample_data", "scene", "sensor", "calibrated_sensor", "ego_pose")
    assert sorted(opened) == sorted(os.path.join(tree, V, t + ".json") for t in tables)
    opened.clear()
    annotations(tree, "Car", "train", scenes=os.path.join(tree, "splits.json"))
    assert len(opened) == 10 and opened[0] == os.path.join(tree, "splits.json")


def test_the_scenes_argument_takes_a_dict_a_file_or_names(ref, tree):
    want = [str(k) for k in ref["car.10.val.k0.m0.keys"]]
    for scenes in (nuscenes_tree.SPLITS, os.path.join(tree, "splits.json"), ["scene-0003"], iter(("scene-0003",))):
        assert [a["key"] for a in annotations(tree, "Car", "val", scenes=scenes)[0]] == want
    assert annotations(tree, "Car", "test")[0] == []
    with pytest.raises(ValueError, match="mini_train"):
        annotations(tree, "Car", "mini_train")
    with pytest.raises(ValueError, match="mini_train"):
        annotations(tree, "Car", "mini_train", scenes=os.path.join(tree, "splits.json"))


def test_without_the_devkit_scenes_must_be_given(tree, monkeypatch):
    """scenes=None imports nuscenes.utils.splits lazily; where that fails the error says to pass scenes.  Where the import
    works (a stand-in here) its create_splits_scenes() is what is used"""
    import types
    for name in ("nuscenes", "nuscenes.utils", "nuscenes.utils.splits"):
        monkeypatch.setitem(sys.modules, name, None)              # the import fails, whether or not a devkit is installed
    with pytest.raises(ValueError, match="scenes="):
        annotations(tree, "Car", "train", scenes=None)
    mods = {n: types.ModuleType(n) for n in ("nuscenes", "nuscenes.utils", "nuscenes.utils.splits")}
    mods["nuscenes.utils.splits"].create_splits_scenes = lambda: dict(nuscenes_tree.SPLITS)
    mods["nuscenes"].utils, mods["nuscenes.utils"].splits = mods["nuscenes.utils"], mods["nuscenes.utils.splits"]
    for name, m in mods.items():
        monkeypatch.setitem(sys.modules, name, m)
    assert len(annotations(tree, "Car", "train", scenes=None)[0]) == 10


def test_an_unknown_class_lists_the_known_ones(tree):
    from open3dsot_amd import datasets as D
    with pytest.raises(ValueError, match="bicycle, bus, car, motorcycle, pedestrian, trailer, truck"):
        annotations(tree, "Van", "train")
    assert len(annotations(tree, "PEDESTRIAN", "train")[0]) == 4          # any case: the reference lower-cases
    assert sum(len(v) for v in D.NUSCENES_TRACKING_CLASSES.values()) == len(nuscenes_tree.CATEGORIES) == 23
    assert sorted(c for v in D.NUSCENES_TRACKING_CLASSES.values() for c in v) == sorted(nuscenes_tree.CATEGORIES)


def test_sweep_lengths(tree, tmp_path):
    from open3dsot_amd import datasets as D
    good = os.path.join(tree, nuscenes_tree.sweeps()[0])
    assert D.nuscenes_rows(good) == os.path.getsize(good) // 20 == NO.read_sweep(good).shape[0]
    bad = tmp_path / "bad.pcd.bin"
    bad.write_bytes(b"\0" * 50)
    with pytest.raises(ValueError, match="bad.pcd.bin"):
        D.nuscenes_rows(str(bad))
    bad.write_bytes(b"\0" * 16)                                      # a row of four floats is no row of this set
    with pytest.raises(ValueError, match="bad.pcd.bin"):
        D.nuscenes_rows(str(bad))
    bad.write_bytes(b"")
    assert D.nuscenes_rows(str(bad)) == 0
    with pytest.raises(FileNotFoundError):
        D.nuscenes_rows(str(tmp_path / "missing.pcd.bin"))


def test_oracle_equals_every_reference_cloud_bit_for_bit(ref, tree):
    """the device rule -- two rounded rigid steps in float64 mode, directional float32 bounds, strict compares, order kept --
    restated in numpy reproduces the reference's preload on every case: this pins the specification without a GPU"""
    n = 0
    for name, category, offset, split, key_only, min_points in cases(ref):
        annos, files, steps = annotations(tree, category, split, key_only, min_points)
        got = NO.reader(annos, files, steps, offset, lambda f: NO.read_sweep(os.path.join(tree, f)), 0)
        want = ref_clouds(ref, name)
        assert [len(g) for g in got] == [len(w) for w in want] == list(ref[name + ".lengths"]), name
        for k, (g, w) in enumerate(zip(got, want)):
            for t, (a, b) in enumerate(zip(g, w)):
                assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (name, k, t)
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, k, t)
                n += 1
    assert n == sum(int(ref[c[0] + ".lengths"].sum()) for c in cases(ref)) and n > 200       # every frame of every case


def test_the_two_translate_modes_differ_on_every_sweep(ref, tree):
    """the float32 mode (numpy < 2) against the float64 mode (numpy >= 2) on the tree's own uncropped sweeps: at least one
    coordinate differs in every sweep, so the wrong mode cannot pass the comparisons with the fixture; and the oracle's float32
    mode is r + np.float32(t), written out here once more, independently"""
    seen = 0
    for split in ("train", "val"):
        annos, files, steps = annotations(tree, "Car", split)
        for f, S in zip(files, steps):
            raw = NO.read_sweep(os.path.join(tree, f))
            p64, p32 = NO.chain(raw, S, 0), NO.chain(raw, S, 1)
            assert p64.dtype == p32.dtype == np.float32 and p64.shape == p32.shape == (raw.shape[0], 3)
            assert (p64.view(np.int32) != p32.view(np.int32)).sum() >= 1, f
            p = raw[:, :3].copy()
            for M in S.reshape(2, 3, 4):
                r = np.empty_like(p)
                for i in range(3):
                    acc = np.float64(M[i, 0]) * p[:, 0].astype(np.float64)
                    acc = acc + np.float64(M[i, 1]) * p[:, 1].astype(np.float64)
                    acc = acc + np.float64(M[i, 2]) * p[:, 2].astype(np.float64)
                    r[:, i] = acc.astype(np.float32)
                t32 = M[:, 3].astype(np.float32)
                p = r + t32[None, :]
                assert p.dtype == np.float32
            assert np.array_equal(p.view(np.int32), p32.view(np.int32)), f
            seen += 1
    assert seen == 12
    # the uncropped fixture clouds are the float64 mode's
    clouds = ref_clouds(ref, "car.-1.train.k0.m0")
    annos, files, steps = annotations(tree, "Car", "train")
    raw = NO.read_sweep(os.path.join(tree, files[0]))
    assert np.array_equal(NO.chain(raw, steps[0], 0).view(np.int32), clouds[0][0].view(np.int32))
    assert not np.array_equal(NO.chain(raw, steps[0], 1).view(np.int32), clouds[0][0].view(np.int32))


def test_the_reader_refuses_the_cpu(tree):
    import torch
    from open3dsot_amd import datasets as D, points_utils as PU
    with pytest.raises(RuntimeError, match="CPU not supported"):
        D.NuScenesTracklets(tree, "train", version=V, scenes=nuscenes_tree.SPLITS, device="cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        D.NuScenesTracklets.load(os.path.join(tree, "nothing.npz"), device="cpu")
    t = np.zeros((1, 6), np.int32)
    t[0, 1], t[0, 3] = 4, 1
    PU.preload_plan(t, 4)
    z = torch.zeros((4, 5))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.preload_count(z, t, z, z, None, z, z, steps=z, translate32=0)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.preload_scatter(z, t, z, z, None, z, z, z, steps=z, translate32=1)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------
def hand_table():
    t = np.zeros((6, 6), np.int32)
    t[:, 0] = [0, 0, 1, 257, 514, 1514]
    t[:, 1] = [0, 1, 256, 257, 1000, 5]
    t[:, 3] = [2, 0, 1, 33, 3, 0]
    return t, 1519


def test_steps_entries_refuse_bad_arguments_before_any_hip_call():
    """every bad argument gives O3D_EINVAL with a NULL stream and no device; the empty calls succeed without a launch"""
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL = capi.CONSTANTS["O3D_EINVAL"]
    assert PU.PRELOAD_MAX_STEPS == capi.CONSTANTS["O3D_PRELOAD_MAX_STEPS"] == 4
    t, rows = hand_table()
    need, wgs, B = PU.preload_plan(t, rows)
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                                              # never dereferenced: every call returns first
    tp = t.ctypes.data

    def count(raw=p, raw_rows=rows, row_floats=5, frames=tp, dev_frames=p, F=6, bounds=p, B=B, steps=p, n_steps=2, translate32=0,
              scratch=p, scratch_len=need, counts=p):
        return lib.o3d_preload_steps_count(raw, raw_rows, row_floats, frames, dev_frames, F, bounds, B, steps, n_steps, translate32,
                                           scratch, scratch_len, counts, None)

    def scatter(raw=p, raw_rows=rows, row_floats=5, frames=tp, dev_frames=p, F=6, bounds=p, B=B, steps=p, n_steps=2, translate32=0,
                scratch=p, scratch_len=need, out_row=p, pool=p, pool_rows=100):
        return lib.o3d_preload_steps_scatter(raw, raw_rows, row_floats, frames, dev_frames, F, bounds, B, steps, n_steps, translate32,
                                             scratch, scratch_len, out_row, pool, pool_rows, None)

    bad = [dict(row_floats=2), dict(row_floats=6), dict(row_floats=0), dict(row_floats=-3), dict(n_steps=0), dict(n_steps=5),
           dict(n_steps=-1), dict(translate32=2), dict(translate32=-1), dict(steps=None), dict(steps=p + 4), dict(steps=p + 1),
           dict(raw=p + 4, row_floats=4), dict(raw=p + 2), dict(raw=p + 2, row_floats=3), dict(raw=p + 1, row_floats=4),
           # what the existing pairs refuse
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
    # the empty calls: no frame (no steps are needed); frames without a box -- nothing to launch
    for rf in (3, 4, 5):
        for ns in (1, 4):
            for t32 in (0, 1):
                assert count(raw=None, raw_rows=0, row_floats=rf, frames=None, dev_frames=None, F=0, bounds=None, B=0, steps=None,
                             n_steps=ns, translate32=t32, scratch=None, scratch_len=0, counts=None) == 0
                assert scatter(raw=None, raw_rows=0, row_floats=rf, frames=None, dev_frames=None, F=0, bounds=None, B=0, steps=None,
                               n_steps=ns, translate32=t32, scratch=None, scratch_len=0, out_row=None, pool=None, pool_rows=0) == 0
    e = np.zeros((2, 6), np.int32)
    e[:, 1] = [0, 7]
    assert PU.preload_plan(e, 7) == (0, 0, 0)
    kw = dict(raw=None, raw_rows=7, frames=e.ctypes.data, dev_frames=None, F=2, bounds=None, B=0, scratch=None, scratch_len=0)
    assert count(counts=None, **kw) == 0 and scatter(out_row=None, pool=None, pool_rows=0, **kw) == 0
    assert count(counts=None, steps=None, **kw) == EINVAL                                    # F = 2: the steps are asked for
    assert count(F=0, B=1) == EINVAL                                                         # boxes without a frame
    assert count(F=0, row_floats=2, B=0) == EINVAL and count(F=0, n_steps=0, B=0) == EINVAL
    # rows of four floats need 16-byte alignment; rows of five need only 4 (a call that passes every check launches: shown on
    # the GPU)
    assert scatter(raw=p + 4, row_floats=4) == EINVAL
    # the posed pair still refuses rows of five floats
    assert lib.o3d_preload_posed_count(p, rows, 5, tp, p, 6, p, B, p, p, need, p, None) == EINVAL
