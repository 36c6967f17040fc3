"""The multi-target tracking loop without a GPU: the three o3d_track_*_multi exports (header, ctypes signatures, struct
layouts, argument validation), synth.make_scene, the memoised index draw, the reference fixture
(tests/golden/ref_multi_tracking.npz, made by tests/golden/make_golden_multi_tracking.py) and the constructor's refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fixture_io  # noqa: E402
import tracking_oracle as TO  # noqa: E402
from test_capi_symbols import declared_symbols, header_prototypes  # noqa: E402

NEW = ("o3d_track_crop_multi", "o3d_track_resample_multi", "o3d_track_offset_box_multi")


def test_the_three_exports_are_declared_bound_and_exported():
    from open3dsot_amd import capi, points_utils  # noqa: F401  (registers)
    protos, declared = header_prototypes(), declared_symbols()
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_float: "f", ctypes.c_double: "d"}
    lib = capi.load()
    for name in NEW + ("o3d_track_crop_multi_scratch",):
        assert name in declared and name in protos and name in capi.SIGNATURES, name
        assert [kind[a] for a in capi.SIGNATURES[name]] == protos[name], name
        assert hasattr(lib, name), name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "%d exports" % len(declared) in readme and "MultiTargetTracker" in readme      # the count README.md states


def test_table_records_match_the_header_layout():
    """the numpy record types the tracker fills its device tables with: the header's fields, in its order, at C's offsets"""
    from open3dsot_amd import points_utils as PU
    src = open(os.path.join(ROOT, "include", "o3dsot.h")).read()

    def fields_of(name):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, src).group(1)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                out += [n.strip().lstrip("*").strip() for n in re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl).group(2).split(",")]
        return out
    assert fields_of("o3d_crop_target") == list(PU.CROP_TARGET.names)
    assert fields_of("o3d_resample_job") == list(PU.RESAMPLE_JOB.names)
    assert fields_of("o3d_crop_group") == [f[0] for f in PU._CropGroup._fields_]

    class CTarget(ctypes.Structure):
        _fields_ = [("box", ctypes.c_void_p), ("scale", ctypes.c_float), ("offset", ctypes.c_float), ("mode", ctypes.c_int),
                    ("out", ctypes.c_void_p), ("capacity", ctypes.c_int), ("count", ctypes.c_void_p)]
    assert ctypes.sizeof(CTarget) == PU.CROP_TARGET.itemsize
    assert [getattr(CTarget, n).offset for n in PU.CROP_TARGET.names] == [PU.CROP_TARGET.fields[n][1] for n in PU.CROP_TARGET.names]
    assert ctypes.sizeof(PU._ResampleJob) == PU.RESAMPLE_JOB.itemsize
    assert [getattr(PU._ResampleJob, n).offset for n in PU.RESAMPLE_JOB.names] == [PU.RESAMPLE_JOB.fields[n][1] for n in PU.RESAMPLE_JOB.names]
    m = re.search(r"#define O3D_CROP_MULTI_CHUNK (\d+)", src)
    assert int(m.group(1)) == PU.CROP_MULTI_CHUNK
    assert int(re.search(r"#define O3D_CROP_MULTI_MAX_TARGETS (\d+)", src).group(1)) == PU.CROP_MULTI_MAX_TARGETS >= 256


def test_multi_entry_points_validate_before_any_launch():
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    g = (PU._CropGroup * 2)()
    assert lib.o3d_track_crop_multi(None, 1, p, 64, None) == EINVAL
    assert lib.o3d_track_crop_multi(ctypes.addressof(g), 1, p, 64, None) == EINVAL              # a zeroed group: no targets
    g[0] = PU._CropGroup(p.value, 120000, p.value, 3)
    assert lib.o3d_track_crop_multi_scratch(ctypes.addressof(g), 1) == 3 * 469                   # one per (target, workgroup)
    assert lib.o3d_track_crop_multi(ctypes.addressof(g), 1, p, 3 * 469 - 1, None) == EINVAL     # scratch too small
    assert lib.o3d_track_crop_multi(ctypes.addressof(g), 1, None, 3 * 469, None) == EINVAL
    assert lib.o3d_track_crop_multi(ctypes.addressof(g), 0, p, 1 << 20, None) == EINVAL
    assert lib.o3d_track_crop_multi(ctypes.addressof(g), 3, p, 1 << 20, None) == EINVAL         # more than two groups
    g[1] = PU._CropGroup(p.value, 257, p.value, 256)
    assert lib.o3d_track_crop_multi_scratch(ctypes.addressof(g), 2) == 3 * 469 + 256 * 2
    g[1] = PU._CropGroup(p.value, 257, p.value, PU.CROP_MULTI_MAX_TARGETS + 1)
    assert lib.o3d_track_crop_multi_scratch(ctypes.addressof(g), 2) == -1                        # beyond the limit
    assert lib.o3d_track_crop_multi(ctypes.addressof(g), 2, p, 1 << 30, None) == EINVAL
    g[1] = PU._CropGroup(None, 8, p.value, 1)
    assert lib.o3d_track_crop_multi(ctypes.addressof(g), 2, p, 1 << 20, None) == EINVAL         # points without a cloud
    g[1] = PU._CropGroup(p.value, -1, p.value, 1)
    assert lib.o3d_track_crop_multi(ctypes.addressof(g), 2, p, 1 << 20, None) == EINVAL
    assert lib.o3d_track_resample_multi(None, 2, None) == EINVAL
    assert lib.o3d_track_resample_multi(p, -1, None) == EINVAL
    assert lib.o3d_track_resample_multi(None, 0, None) == 0                                      # nothing to do
    assert lib.o3d_track_offset_box_multi(None, None, None, None, None, 1, 1, 1, 0, 0, None, None, 0, None, None) == EINVAL
    assert lib.o3d_track_offset_box_multi(p, p, None, None, None, 0, 1, 1, 0, 0, p, None, 0, None, None) == EINVAL   # K = 0
    assert lib.o3d_track_offset_box_multi(p, p, None, None, None, 2, 1, 1, 0, 0, None, None, 0, None, None) == EINVAL  # nowhere to write
    assert lib.o3d_track_offset_box_multi(p, p, None, None, None, 2, 1, 1, 0, 0, None, p, 4, None, None) == EINVAL   # no counter
    assert lib.o3d_track_offset_box_multi(p, p, None, None, None, 2, 1, 1, 0, -1, p, None, 0, None, None) == EINVAL  # seed


def test_make_scene_is_deterministic_and_holds_make_sequence():
    from open3dsot_amd import synth
    a, ga = synth.make_scene(3, 4, 3000, 3)
    b, gb = synth.make_scene(3, 4, 3000, 3)
    assert len(a) == 4 and all(x.shape == (9000, 3) and x.dtype == np.float32 for x in a)
    assert ga.shape == (4, 3, 15) and ga.dtype == np.float32
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(ga, gb)
    c, _ = synth.make_scene(4, 4, 3000, 3)
    assert not np.array_equal(a[0], c[0])
    # sub-scene 0 is make_sequence of the derived seed, bit for bit
    s0, g0 = synth.make_sequence(synth.scene_subseed(3, 0), 4, 3000)
    assert all(np.array_equal(x[:3000].view(np.int32), y.view(np.int32)) for x, y in zip(a, s0))
    assert np.array_equal(ga[:, 0].view(np.int32), g0.view(np.int32))
    # sub-scene j is make_sequence(derived seed) turned by 2 pi j / 3 about z: every target is in the merged cloud, its box
    # orthonormal, its height unchanged, its bearing advanced by the sector
    for j in range(3):
        sj, gj = synth.make_sequence(synth.scene_subseed(3, j), 4, 3000)
        assert np.array_equal(a[2][3000 * j:3000 * (j + 1), 2], sj[2][:, 2])
        assert np.abs(np.linalg.norm(ga[:, j, :2], axis=1) - np.linalg.norm(gj[:, :2], axis=1)).max() < 1e-5
        turn = np.arctan2(ga[0, j, 1], ga[0, j, 0]) - np.arctan2(gj[0, 1], gj[0, 0])
        assert abs((turn - 2 * np.pi * j / 3 + np.pi) % (2 * np.pi) - np.pi) < 1e-6
        for t in range(4):
            R = ga[t, j, 6:].reshape(3, 3).astype(np.float64)
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6
            assert TO.crop(a[t], ga[t, j], 1.25, 0.0, TO.MODEL)[0] >= 64
    one, g1 = synth.make_scene(3, 2, 3000, 1)
    assert np.array_equal(one[1], synth.make_sequence(synth.scene_subseed(3, 0), 2, 3000)[0][1]) and g1.shape == (2, 1, 15)


def test_memoised_draw_equals_draw_indices():
    from open3dsot_amd import tracking
    cache = tracking.DrawCache(maxsize=4)
    sizes = (0, 2, 3, 511, 512, 513, 5000)
    for n in sizes:
        want = tracking.draw_indices(n, 512)
        got = cache.get(n, 512)
        assert (got is None) == (want is None), n
        if want is not None:
            assert got.dtype == np.int32 and got.shape == (512,) and np.array_equal(got, want), n
    assert cache.misses == len(sizes) and cache.hits == 0 and len(cache) == 4            # bounded
    again = cache.get(5000, 512)
    assert cache.hits == 1 and cache.misses == len(sizes) and again is cache.get(5000, 512)   # a hit returns the held array
    assert np.array_equal(again, tracking.draw_indices(5000, 512))
    with pytest.raises(ValueError):
        again[0] = 0                                                                    # shared between callers: read-only
    cache.get(0, 512)                                                                   # evicted long ago: drawn again
    assert cache.misses == len(sizes) + 1
    assert np.array_equal(cache.get(5000, 1024), tracking.draw_indices(5000, 1024))      # the size is part of the key


def test_fixture_records_its_margins():
    gold = fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_multi_tracking.npz"))
    assert int(gold["n_targets"]) == 3 and int(gold["n_frames"]) == 6 and int(gold["n_points"]) == 20000
    assert int(gold["scene_seed"]) >= 0
    for k in range(3):
        assert float(gold["t%d.worst_margin" % k]) > 1e-3 and float(gold["t%d.worst_gap" % k]) > 1e-3
        for t in range(1, 6):
            key = "t%d.f%d." % (k, t)
            assert gold[key + "template_points"].shape == (512, 3) and gold[key + "search_points"].shape == (1024, 3)
            assert gold[key + "points2cc_dist_t"].shape == (512, 9) and gold[key + "proposals"].shape == (64, 5)
            s = np.sort(gold[key + "proposals"][:, 4])
            assert s[-1] - s[-2] > 1e-3
            assert gold[key + "ref_box"].shape == (15,) and gold[key + "result_box"].shape == (15,)
    for f in os.listdir(os.path.join(ROOT, "tests", "golden")):
        if f.startswith("ref_multi_tracking"):
            assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) <= 1024 * 1024


def test_fixture_crops_equal_the_oracle_on_the_scene():
    """the fp32 restatement of the crop along the reference's trajectories of the three targets: counts equal, regularised
    clouds within the bound of test_tracking_cpu.py"""
    from open3dsot_amd import synth, tracking
    gold = fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_multi_tracking.npz"))
    _, cfg = TO.case_config("bat_fap")
    frames, gt = synth.make_scene(int(gold["scene_seed"]), 6, 20000, 3)
    for k in range(3):
        first = TO.crop(frames[0], gt[0, k], cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)[1]
        for t in range(1, 6):
            key = "t%d.f%d." % (k, t)
            ref = gold[key + "ref_box"]
            search = TO.crop(frames[t], ref, cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)[1]
            prev = TO.crop(frames[t - 1], ref, cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)[1]
            template = np.concatenate([first, prev], 0)
            assert [search.shape[0], template.shape[0]] == gold[key + "counts"].tolist(), (k, t)
            for cloud, size, name in ((template, 512, "template_points"), (search, 1024, "search_points")):
                idx = tracking.draw_indices(cloud.shape[0], size)
                assert np.abs(cloud[idx].astype(np.float64) - gold[key + name]).max() <= 2e-5, (k, t, name)


def test_multi_target_tracker_refuses_cpu_models_and_the_motion_tracker():
    from open3dsot_amd import m2track, tracking, trackers
    import motion_oracle as MO
    with pytest.raises(RuntimeError, match="CPU not supported"):
        tracking.MultiTargetTracker(trackers.P2B(), 3)
    with pytest.raises(TypeError, match="MotionSequenceTracker"):
        tracking.MultiTargetTracker(m2track.M2TRACK(**MO.case_config("kitti")), 3)
    assert callable(tracking.track_targets)
