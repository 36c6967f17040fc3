"""o3d_scene_pair_scores_frames and o3d_scene_mot_walk refuse bad arguments with O3D_EINVAL before any HIP call: checked on the
built library without a GPU, like test_capi_symbols.test_entry_points_reject_bad_arguments_before_touching_the_device."""
import ctypes


def test_mot_entry_points_reject_bad_arguments_before_touching_the_device():
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL = capi.CONSTANTS["O3D_EINVAL"]
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = PU.CROP_MULTI_MAX_TARGETS + 1
    assert PU.SCENE_MOT_MAX_FRAMES == capi.CONSTANTS["O3D_SCENE_MOT_MAX_FRAMES"] >= 1

    score = lib.o3d_scene_pair_scores_frames
    good = [p, p, p, p, 0, 2, 3, 3, 2, p, p, None]                # F = 0: nothing to do, no launch
    assert score(*good) == 0
    for i in (0, 1, 2, 3, 9, 10):                                  # every operand
        bad = list(good)
        bad[i] = None
        assert score(*bad) == EINVAL, i
    for i, v in ((4, -1), (5, 0), (5, big), (6, 0), (6, big), (7, 1), (7, 4), (8, 0), (8, 3)):
        bad = list(good)
        bad[i] = v
        assert score(*bad) == EINVAL, (i, v)
    assert score(p, p, p, p, 2 ** 31 - 1, 1024, 1024, 3, 2, p, p, None) == EINVAL          # more workgroups than a launch takes

    walk = lib.o3d_scene_mot_walk
    good = [p, p, p, p, 0, 2, 3, 0.0, 2.0, p, p, p, p, p, p, p, p, None]
    assert walk(*good) == 0
    for i in (0, 1, 2, 3, 9, 10, 11, 12, 13, 14, 15, 16):
        bad = list(good)
        bad[i] = None
        assert walk(*bad) == EINVAL, i
    for i, v in ((4, -1), (4, PU.SCENE_MOT_MAX_FRAMES + 1), (5, 0), (5, big), (6, 0), (6, big)):
        bad = list(good)
        bad[i] = v
        assert walk(*bad) == EINVAL, (i, v)


def test_the_wrappers_refuse_cpu_tensors():
    import pytest
    import torch
    from open3dsot_amd import metrics, points_utils as PU
    z = torch.zeros
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.scene_pair_scores_frames(z(1, 2, 15), z(1, 2, dtype=torch.int32), z(1, 3, 15), z(1, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.scene_mot_walk(z(1, 2, 3), z(1, 2, 3), z(1, 2, dtype=torch.int32), z(1, 3, dtype=torch.int32), *[z(2, dtype=torch.int32)] * 3)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        metrics.ClearMOT(2, device="cpu")
