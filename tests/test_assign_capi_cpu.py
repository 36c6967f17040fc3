"""o3d_scene_assign, o3d_scene_manage_assign and o3d_scene_mot_walk_assign are declared in include/o3dsot.h, exported by the
library, and refuse bad arguments with O3D_EINVAL before any HIP call: checked on the built library without a GPU, like
test_mot_capi_cpu."""
import ctypes

import pytest

ENTRIES = ("o3d_scene_assign", "o3d_scene_manage_assign", "o3d_scene_mot_walk_assign")


def test_the_three_entries_are_declared_and_exported():
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f"}
    want = {"o3d_scene_assign": "ppppiiffiipppp",
            "o3d_scene_manage_assign": "ppppiippppipppppippippp" + "ffiiiiiiip",
            "o3d_scene_mot_walk_assign": "ppppiiiffpppppppp" + "iip"}
    for name in ENTRIES:
        assert "".join(kinds[a] for a in capi.SIGNATURES[name]) == want[name], name
        assert hasattr(lib, name) and capi.RESTYPES[name] is ctypes.c_int
    # the two older entries are the new ones without the rule
    assert capi.SIGNATURES["o3d_scene_manage"] == capi.SIGNATURES["o3d_scene_manage_assign"][:-3] + [ctypes.c_void_p]
    assert capi.SIGNATURES["o3d_scene_mot_walk"] == capi.SIGNATURES["o3d_scene_mot_walk_assign"][:-3] + [ctypes.c_void_p]
    c = capi.CONSTANTS
    assert (c["O3D_ASSIGN_GREEDY"], c["O3D_ASSIGN_OPTIMAL"], c["O3D_COST_DISTANCE"], c["O3D_COST_OVERLAP"]) == (0, 1, 0, 1)
    assert PU.ASSIGNMENTS == dict(greedy=0, optimal=1) and PU.ASSIGN_COSTS == dict(distance=0, overlap=1)


def test_assign_entry_points_reject_bad_arguments_before_touching_the_device():
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL = capi.CONSTANTS["O3D_EINVAL"]
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = PU.CROP_MULTI_MAX_TARGETS + 1
    rules = ((-1, 0), (2, 0), (0, -1), (0, 2), (1, 2), (7, 7))

    assign = lib.o3d_scene_assign
    good = [p, p, p, p, 2, 3, 0.0, 2.0, 1, 0, p, p, p, None]
    for i in (0, 1, 10, 11, 12):                                    # every operand (row_active and n_col may be NULL)
        bad = list(good)
        bad[i] = None
        assert assign(*bad) == EINVAL, i
    for i, v in ((4, 0), (4, big), (5, 0), (5, PU.SCENE_MAX_DETECTIONS + 1), (4, -1), (5, -1)):
        bad = list(good)
        bad[i] = v
        assert assign(*bad) == EINVAL, (i, v)
    for a, c in rules:
        bad = list(good)
        bad[8], bad[9] = a, c
        assert assign(*bad) == EINVAL, (a, c)

    walk = lib.o3d_scene_mot_walk_assign
    good = [p, p, p, p, 0, 2, 3, 0.0, 2.0, p, p, p, p, p, p, p, p, 1, 1, None]
    assert walk(*good) == 0                                          # F = 0: nothing to do, no launch
    for i in (0, 1, 2, 3, 9, 10, 11, 12, 13, 14, 15, 16):
        bad = list(good)
        bad[i] = None
        assert walk(*bad) == EINVAL, i
    for i, v in ((4, -1), (4, PU.SCENE_MOT_MAX_FRAMES + 1), (5, 0), (5, big), (6, 0), (6, big)):
        bad = list(good)
        bad[i] = v
        assert walk(*bad) == EINVAL, (i, v)
    for a, c in rules:
        bad = list(good)
        bad[17], bad[18] = a, c
        assert walk(*bad) == EINVAL, (a, c)

    manage = lib.o3d_scene_manage_assign
    #       ov di dets n  K  D  cur yaw wlh res T  frame act slot next counts col bank lanes rule ids match drop
    good = [p, p, p, p, 2, 3, p, p, p, p, 4, p, p, p, p, p, 0, p, p, 2, p, p, p, 0.0, 2.0, 2, 0, 0, 1, 1, 1, 0, None]
    for i in (0, 1, 2, 3, 6, 7, 8, 9, 11, 12, 13, 14, 15, 18, 20, 21, 22):      # every operand but bank_state_next
        bad = list(good)
        bad[i] = None
        assert manage(*bad) == EINVAL, i
    for i, v in ((4, 0), (4, big), (5, -1), (5, PU.SCENE_MAX_DETECTIONS + 1), (10, 0), (16, 2), (19, -2), (19, 4)):
        bad = list(good)
        bad[i] = v
        assert manage(*bad) == EINVAL, (i, v)
    for a, c in rules:
        bad = list(good)
        bad[30], bad[31] = a, c
        assert manage(*bad) == EINVAL, (a, c)


def test_the_python_layers_refuse_unknown_names_before_any_launch():
    from open3dsot_amd import metrics, points_utils as PU
    with pytest.raises(ValueError, match="assignment"):
        PU._assign_args("hungarian", "distance", "x")
    with pytest.raises(ValueError, match="cost"):
        PU._assign_args("optimal", "iou", "x")
    assert PU._assign_args("optimal", "overlap", "x") == (1, 1)
    with pytest.raises(ValueError, match="assignment"):
        metrics.ClearMOT(2, device="cuda", assignment="hungarian")
