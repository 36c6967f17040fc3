"""The free-running tracking loop (tracking.py, sampling="device") without a GPU: the bank oracle against plain Python lists,
the index properties of the draw, the validation of the three new entry points and the `sampling` keyword."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import free_running_oracle as FO  # noqa: E402
import sampler_oracle as SO  # noqa: E402

MODEL_COUNTS = [1257, 4, 0, 1, 300, 3]            # the model crop of frames 1..6
SMALL_BANK = 1400                                 # `all` holds 1262 rows after frame 4 and would hold 1562 after frame 5


def crops_of(counts, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(n, 3)).astype(np.float32) for n in counts]


def template_by_lists(crops, rule, t):
    """the template cloud of frame t (1-based) as getModel / cropAndCenterPC concatenate it: crops[f - 1] is the crop of frame
    f - 1 by its own result box, made at frame f"""
    if rule == "first":
        parts = [crops[0]]
    elif rule == "previous":
        parts = [crops[t - 1]]
    elif rule == "firstandprevious":
        parts = [crops[0], crops[t - 1]]
    else:
        parts = crops[:t]
    return np.concatenate(parts, 0)


@pytest.mark.parametrize("bank_cap", [8 * 1300, SMALL_BANK])
@pytest.mark.parametrize("rule", FO.RULES)
def test_bank_oracle_equals_the_concatenation_of_python_lists(rule, bank_cap):
    crops = crops_of(MODEL_COUNTS)
    bank = np.full((bank_cap, 3), np.nan, np.float32)
    state, full = (0, 0), []
    for t in range(1, len(crops) + 1):
        has_crop = t == 1 or rule != "first"
        state = FO.bank_update(state, crops[t - 1], rule, t == 1, has_crop, bank, bank_cap)
        want = template_by_lists(crops, rule, t)
        full.append(want.shape[0] > bank_cap)
        assert state[1] == min(want.shape[0], bank_cap), (rule, t)
        assert state[0] == MODEL_COUNTS[0]
        assert np.array_equal(bank[:state[1]].view(np.int32), want[:bank_cap].view(np.int32)), (rule, t)
    if bank_cap == SMALL_BANK:
        # `all` overflows at frame 5 and stays full; firstandprevious holds 2 x 1257 rows at frame 1 and 1257 + 300 at frame 5
        want_full = {"all": [0, 0, 0, 0, 1, 1], "firstandprevious": [1, 0, 0, 0, 1, 0]}.get(rule, [0] * 6)
        assert full == [bool(v) for v in want_full]
    else:
        assert not any(full)


@pytest.mark.parametrize("n,S", [(3, 64), (63, 64), (64, 64), (65, 64), (1313, 1024), (2514, 512), (13, 1024)])
def test_index_properties_of_the_draw(n, S):
    src = np.arange(3 * (n + 5), dtype=np.float32).reshape(-1, 3)
    for key in FO.keys(0) + FO.keys(7):
        dst, used = FO.resample_drawn(src, n, n + 5, key, S)
        assert used.shape == (S,) and used.dtype == np.int32
        assert used.min() >= 0 and used.max() < n                                  # in range: every index < n
        if n == S:
            assert np.array_equal(used, np.arange(S))                               # the identity
        if S < n:
            assert np.unique(used).size == S                                        # without replacement: all distinct
        assert np.array_equal(dst, src[used])
        cut, used_cut = FO.resample_drawn(src, n + 100, n, key, S)                  # a count beyond the buffer draws from `cap` rows
        assert np.array_equal(used_cut, used) and np.array_equal(cut, dst)
    for few in (0, 1, 2):
        dst, used = FO.resample_drawn(src, few, n, FO.keys(0)[0], S)
        assert not dst.any() and np.all(used == -1)
    assert FO.keys(0)[0] != FO.keys(0)[1] and FO.keys(0) != FO.keys(1)


def test_the_python_port_of_draw_key_equals_the_oracle():
    from open3dsot_amd import points_utils as PU, tracking
    for seed in (0, 1, 7, 123456789, 2 ** 31 - 1):
        for cloud in (0, 1):
            assert PU.draw_key(seed, 0, 0, cloud) == SO.draw_key(seed, 0, 0, cloud)
        assert tracking.draw_keys(seed) == FO.keys(seed)
    assert PU.draw_key(3, 7, 11, 1) == SO.draw_key(3, 7, 11, 1)
    for key in (0, 1, 0x7FFFFFFF, 0x80000000, 0xDEADBEEF, 0xFFFFFFFF):
        assert ctypes.c_uint32(PU._key_bits(key)).value == key and -2 ** 31 <= PU._key_bits(key) < 2 ** 31


def test_new_entry_points_reject_bad_arguments_before_touching_the_device():
    from open3dsot_amd import capi, points_utils  # noqa: F401  (registers argtypes)
    lib = capi.load()
    EINVAL = capi.CONSTANTS["O3D_EINVAL"]
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.cast(ctypes.addressof(buf) + 64, ctypes.c_void_p)
    job, none = [p, p, 8, 1, p, 8, None], [None, None, 0, 0, None, 0, None]
    assert lib.o3d_track_resample_drawn(*none, *none, 1, None) == EINVAL
    for field, bad in ((0, None), (1, None), (4, None), (2, 0), (2, -1), (5, 0), (5, -3)):      # src, n_dev, dst, cap, S
        broken = list(job)
        broken[field] = bad
        assert lib.o3d_track_resample_drawn(*broken, *none, 1, None) == EINVAL, (field, bad)
        assert lib.o3d_track_resample_drawn(*job, *broken, 2, None) == EINVAL, (field, bad)
    assert lib.o3d_track_resample_drawn(*job, *job, 0, None) == EINVAL and lib.o3d_track_resample_drawn(*job, *job, 3, None) == EINVAL
    good = [p, p, 8, p, 16, 0, 1, 1, p, q]             # crop, count, crop_cap, bank, bank_cap, rule, first, has_crop, state_in, state_out
    for field, bad in ((0, None), (1, None), (3, None), (8, None), (9, None), (9, p), (2, 0), (4, 0), (4, -1), (5, -1), (5, 4)):
        broken = list(good)
        broken[field] = bad
        assert lib.o3d_track_bank_update(*broken, None) == EINVAL, (field, bad)
    good = [p, p, p, 8, 1, 2, 4, p, 1, p, None, None]      # prev, cur, counts, capacity, keys, N, wlh, first_frame, points, bc, used
    for field, bad in ((0, None), (1, None), (2, None), (7, None), (9, None), (3, 0), (3, -2), (6, 0), (6, -1)):
        broken = list(good)
        broken[field] = bad
        assert lib.o3d_track_motion_input_drawn(*broken, None) == EINVAL, (field, bad)


class _NoModel:
    """enough of a model for the keyword checks, which come before anything touches it"""


@pytest.mark.parametrize("name", ["SequenceTracker", "MotionSequenceTracker"])
def test_sampling_keyword_of_the_single_trackers(name):
    from open3dsot_amd import tracking
    with pytest.raises(ValueError, match="sampling"):
        getattr(tracking, name)(_NoModel(), sampling="nonsense")
    with pytest.raises(ValueError, match="sampling"):
        tracking.tracker_for(_NoModel(), sampling="nonsense")
    with pytest.raises(ValueError, match="sampling"):
        tracking.track_sequence(_NoModel(), [None], None, sampling="nonsense")
    with pytest.raises(ValueError, match="sampling"):
        tracking.evaluate_sequence(_NoModel(), [None], None, sampling="nonsense")
    with pytest.raises(ValueError, match="sampling"):
        tracking.evaluate(_NoModel(), [], sampling="nonsense")


@pytest.mark.parametrize("name", ["MultiTargetTracker", "MultiMotionTracker"])
def test_the_multi_trackers_refuse_device_sampling(name):
    from open3dsot_amd import tracking
    for sampling, match in (("device", "follow-up"), ("nonsense", "sampling")):
        with pytest.raises(ValueError, match=match):
            getattr(tracking, name)(_NoModel(), 2, sampling=sampling)
        with pytest.raises(ValueError, match=match):
            tracking.multi_tracker_for(_NoModel(), 2, sampling=sampling)
        with pytest.raises(ValueError, match=match):
            tracking.track_targets(_NoModel(), [None], [None, None], sampling=sampling)
        with pytest.raises(ValueError, match=match):
            tracking.evaluate_targets(_NoModel(), [None], np.zeros((1, 2, 15), np.float32), sampling=sampling)
