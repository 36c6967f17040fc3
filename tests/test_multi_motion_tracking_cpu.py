"""The K-target loop of the motion tracker without a GPU: the o3d_track_motion_input_multi export (header, ctypes signature,
record layout, argument validation before any launch), the refusals of tracking.MultiMotionTracker and the dispatch of
tracking.track_targets by the model's type."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import motion_oracle as MO  # noqa: E402
from test_capi_symbols import declared_symbols, header_prototypes  # noqa: E402

NAME = "o3d_track_motion_input_multi"


def test_the_export_is_declared_bound_and_exported():
    from open3dsot_amd import capi, points_utils  # noqa: F401  (registers)
    protos, declared = header_prototypes(), declared_symbols()
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_float: "f", ctypes.c_double: "d"}
    assert NAME in declared and NAME in protos and NAME in capi.SIGNATURES
    assert [kind[a] for a in capi.SIGNATURES[NAME]] == protos[NAME] == list("piipippp")
    assert hasattr(capi.load(), NAME)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "%d exports" % len(declared) in readme and "MultiMotionTracker" in readme          # the count README.md states


def test_motion_job_record_matches_the_header_and_the_static_assert():
    """the numpy record the tracker fills its device table with: the header's fields, in its order, at C's offsets, and the
    size that csrc/track.hip asserts"""
    from open3dsot_amd import points_utils as PU
    src = open(os.path.join(ROOT, "include", "o3dsot.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*o3d_motion_job;", src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip().lstrip("*").strip() for n in re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl).group(2).split(",")]
    assert fields == list(PU.MOTION_JOB.names) == ["prev", "n_prev", "cur", "n_this", "idx", "zero_prev", "zero_this"]

    class CJob(ctypes.Structure):
        _fields_ = [("prev", ctypes.c_void_p), ("n_prev", ctypes.c_int), ("cur", ctypes.c_void_p), ("n_this", ctypes.c_int),
                    ("idx", ctypes.c_void_p), ("zero_prev", ctypes.c_int), ("zero_this", ctypes.c_int)]
    assert ctypes.sizeof(CJob) == PU.MOTION_JOB.itemsize
    assert [getattr(CJob, n).offset for n in PU.MOTION_JOB.names] == [PU.MOTION_JOB.fields[n][1] for n in PU.MOTION_JOB.names]
    hip = open(os.path.join(ROOT, "open3dsot_amd", "csrc", "track.hip")).read()
    m = re.search(r"static_assert\(sizeof\(o3d_motion_job\) == (\d+)", hip)
    assert m and int(m.group(1)) == PU.MOTION_JOB.itemsize


def test_one_definition_of_the_row_arithmetic():
    """the channels, the inside test and the BoxCloud are written once in csrc/track.hip and called by both kernels"""
    hip = open(os.path.join(ROOT, "open3dsot_amd", "csrc", "track.hip")).read()
    assert hip.count("void motion_row(") == 1 and len(re.findall(r"\bmotion_row\(x, y, z,", hip)) == 2
    assert hip.count("hx = (l * 1.25f) * 0.5f") == 1 and hip.count("0.8f : 0.2f") == 1 and hip.count("bc[1 + k] = sqrtf(") == 1
    from open3dsot_amd import build
    assert ("track.hip", ["-ffp-contract=off"]) in build.SOURCES


def test_the_entry_validates_before_any_launch():
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.o3d_track_motion_input_multi
    assert f(None, 1, 4, None, 1, None, None, None) == EINVAL               # NULL operands
    assert f(None, 1, 4, p, 1, p, p, None) == EINVAL                        # no job table
    assert f(p, 1, 4, None, 1, p, p, None) == EINVAL                        # no wlh
    assert f(p, 1, 4, p, 1, None, p, None) == EINVAL                        # nowhere to write the points
    assert f(p, 0, 4, p, 1, p, p, None) == EINVAL                           # K = 0
    assert f(p, -1, 4, p, 1, p, p, None) == EINVAL
    assert f(p, PU.CROP_MULTI_MAX_TARGETS + 1, 4, p, 1, p, p, None) == EINVAL
    assert f(p, 1, 0, p, 1, p, p, None) == EINVAL                           # N = 0
    assert f(p, 1, -4, p, 1, p, None, None) == EINVAL


def test_multi_motion_tracker_makes_its_three_refusals():
    from open3dsot_amd import m2track, points_utils as PU, tracking, trackers
    cfg = MO.case_config("kitti")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        tracking.MultiMotionTracker(m2track.M2TRACK(**cfg), 3)
    with pytest.raises(TypeError, match="MultiTargetTracker"):
        tracking.MultiMotionTracker(trackers.P2B(), 3)
    for bad in (0, -1, PU.CROP_MULTI_MAX_TARGETS + 1):
        with pytest.raises(ValueError, match="n_targets"):
            tracking.MultiMotionTracker(m2track.M2TRACK(**cfg), bad)
    # the matching trackers' class still sends the motion tracker away, now with a pointer to the new class
    with pytest.raises(TypeError, match="MotionSequenceTracker.*MultiMotionTracker"):
        tracking.MultiTargetTracker(m2track.M2TRACK(**cfg), 3)
    for name in ("init", "update", "set_box", "retire", "results"):
        assert callable(getattr(tracking.MultiMotionTracker, name)), name
    # the code the two K-target classes share has one home
    for name in ("_pack", "init", "set_box", "retire", "_crop_group", "_crop_multi"):
        assert getattr(tracking.MultiMotionTracker, name) is getattr(tracking.MultiTargetTracker, name), name


def test_track_targets_picks_the_class_by_the_models_type():
    from open3dsot_amd import m2track, tracking, trackers
    model = m2track.M2TRACK(**MO.case_config("kitti"))
    boxes = np.zeros((2, 15), np.float32)
    with pytest.raises(RuntimeError, match="MultiMotionTracker: CPU not supported"):
        tracking.track_targets(model, [torch.zeros(8, 3)], boxes)
    with pytest.raises(RuntimeError, match="MultiTargetTracker: CPU not supported"):
        tracking.track_targets(trackers.P2B(), [torch.zeros(8, 3)], boxes)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        tracking.multi_tracker_for(model, 2)


def test_binding_refuses_cpu_tensors():
    from open3dsot_amd import points_utils as PU
    tab = torch.zeros(PU.MOTION_JOB.itemsize, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.motion_input_multi(tab, 1, 4, torch.ones(1, 3), True, torch.zeros(1, 8, 5), torch.zeros(1, 8, 9))
