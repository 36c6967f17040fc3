"""sampling="table" without a GPU: the host builder of the draw tables against tracking.draw_indices row by row, the `sampling`
keyword (accepted by the single and lane loops, refused by the K-target loops), and the argument validation of the four
o3d_track_*_tabled entry points, which returns before any HIP call."""
import ctypes

import numpy as np
import pytest

TABLES = [(40, 8), (300, 257), (600, 512)]         # (600, 512): rows above 512 are drawn without replacement


@pytest.mark.parametrize("capacity,S", TABLES)
def test_the_host_table_is_draw_indices_row_by_row(capacity, S):
    from open3dsot_amd import tracking
    table = tracking.draw_table_host(capacity, S)
    assert table.shape == (capacity + 1, S) and table.dtype == np.int32 and table.flags.c_contiguous
    assert np.all(table[:3] == -1)                                                      # the zero-fill case
    assert np.array_equal(table[S], np.arange(S))                                       # n == S: the identity
    for n in range(3, capacity + 1):
        want = tracking.draw_indices(n, S)
        assert np.array_equal(table[n], want), n
        assert table[n].min() >= 0 and table[n].max() < n, n
        if n > S:                                                                       # drawn without replacement
            assert np.unique(table[n]).size == S, n
    assert any(np.unique(table[n]).size < S for n in range(3, min(S, capacity + 1)))    # n < S does repeat rows
    for n in (0, 1, 2):
        assert tracking.draw_indices(n, S) is None


def test_the_host_table_refuses_impossible_sizes():
    from open3dsot_amd import tracking
    for capacity, S in ((0, 8), (-1, 8), (8, 0)):
        with pytest.raises(ValueError, match="capacity"):
            tracking.draw_table_host(capacity, S)


def test_the_cache_starts_empty_and_clears():
    from open3dsot_amd import tracking
    tracking.clear_draw_tables()
    assert tracking._DRAW_TABLES == {}


class _NoModel:
    """enough of a model for the keyword checks, which come before anything touches it"""


def test_the_sampling_keyword_knows_the_table_mode():
    from open3dsot_amd import tracking
    assert tracking.SAMPLING == ("reference", "device", "table")
    assert tracking._sampling("table") == "table"
    for name in ("reference", "device"):
        assert tracking._sampling(name) == name
    with pytest.raises(ValueError, match="sampling"):
        tracking._sampling("tables")
    with pytest.raises(ValueError, match="follow-up"):
        tracking._sampling("device", "MultiTargetTracker")
    with pytest.raises(ValueError, match="follow-up"):
        tracking._sampling("table", "MultiTargetTracker")


@pytest.mark.parametrize("name", ["MultiTargetTracker", "MultiMotionTracker"])
def test_the_multi_trackers_refuse_table_sampling(name):
    from open3dsot_amd import tracking
    with pytest.raises(ValueError, match="table"):
        getattr(tracking, name)(_NoModel(), 2, sampling="table")
    with pytest.raises(ValueError, match="table"):
        tracking.multi_tracker_for(_NoModel(), 2, sampling="table")
    with pytest.raises(ValueError, match="table"):
        tracking.track_targets(_NoModel(), [None], [None, None], sampling="table")
    with pytest.raises(ValueError, match="table"):
        tracking.evaluate_targets(_NoModel(), [None], np.zeros((1, 2, 15), np.float32), sampling="table")


@pytest.mark.parametrize("name", ["LaneTracker", "MotionLaneTracker"])
def test_the_lane_trackers_take_the_free_running_modes_only(name):
    from open3dsot_amd import tracking
    for sampling in ("reference", "nonsense"):
        with pytest.raises(ValueError, match="sampling"):
            getattr(tracking, name)(_NoModel(), 2, sampling=sampling)
        with pytest.raises(ValueError, match="sampling"):
            tracking.lane_tracker_for(_NoModel(), 2, sampling=sampling)


def test_the_single_loops_get_past_the_keyword_with_table():
    """"table" is refused by nothing before the model is touched: what stops these calls is the model that is none"""
    from open3dsot_amd import tracking
    for make in (lambda: tracking.SequenceTracker(_NoModel(), sampling="table"),
                 lambda: tracking.MotionSequenceTracker(_NoModel(), sampling="table"),
                 lambda: tracking.tracker_for(_NoModel(), sampling="table"),
                 lambda: tracking.evaluate(_NoModel(), [], sampling="table", lanes=2)):
        with pytest.raises((AttributeError, TypeError)):
            make()


def refuses(entry, good, broken):
    """entry(*good with one field replaced, stream NULL) returns O3D_EINVAL for every (field, bad value)"""
    for field, bad in broken:
        args = list(good)
        args[field] = bad
        assert entry(*args, None) == -1, (entry.__name__, field, bad)


def test_the_tabled_entry_points_validate_before_any_launch():
    from open3dsot_amd import capi, points_utils  # noqa: F401
    lib = capi.load()
    for name in ("o3d_track_resample_tabled", "o3d_track_motion_input_tabled", "o3d_track_resample_tabled_lanes",
                 "o3d_track_motion_input_tabled_lanes"):
        assert name in capi.SIGNATURES
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    LMAX = capi.CONSTANTS["O3D_CROP_MULTI_MAX_TARGETS"]
    job = [p, p, 8, p, p, 4, None]                         # src, n_dev, cap, table, dst, S, used
    none = [None, None, 0, None, None, 0, None]
    bad_job = [(0, None), (1, None), (3, None), (4, None), (2, 0), (2, -1), (2, (1 << 29) + 1), (5, 0), (5, -3), (5, (1 << 20) + 1)]
    for field, bad in bad_job:
        broken = list(job)
        broken[field] = bad
        assert lib.o3d_track_resample_tabled(*broken, *none, 1, None) == -1, (field, bad)
        assert lib.o3d_track_resample_tabled(*job, *broken, 2, None) == -1, (field, bad)
    assert lib.o3d_track_resample_tabled(*job, *job, 0, None) == -1 and lib.o3d_track_resample_tabled(*job, *job, 3, None) == -1
    assert lib.o3d_track_resample_tabled(*none, *none, 1, None) == -1
    # prev, cur, counts, capacity, table, N, wlh, first_frame, points, candidate_bc, used
    refuses(lib.o3d_track_motion_input_tabled, [p, p, p, 8, p, 4, p, 1, p, None, None],
            [(0, None), (1, None), (2, None), (4, None), (6, None), (8, None), (3, 0), (3, -2), (5, 0), (5, -1), (5, (1 << 20) + 1)])
    lane_job = [p, p, 2, 8, p, p, 4, None]                 # src, n_dev, stride, cap, table, dst, S, used
    for field, bad in ((0, None), (1, None), (4, None), (5, None), (2, 0), (3, 0), (6, 0)):
        broken = list(lane_job)
        broken[field] = bad
        assert lib.o3d_track_resample_tabled_lanes(*broken, *lane_job, 2, None) == -1, (field, bad)
        assert lib.o3d_track_resample_tabled_lanes(*lane_job, *broken, 2, None) == -1, (field, bad)
    for L in (0, -1, LMAX + 1):
        assert lib.o3d_track_resample_tabled_lanes(*lane_job, *lane_job, L, None) == -1, L
    # prev, cur, counts, capacity, table, N, wlh, lanes, L, points, candidate_bc, used
    refuses(lib.o3d_track_motion_input_tabled_lanes, [p, p, p, 8, p, 4, p, p, 2, p, None, None],
            [(0, None), (1, None), (2, None), (4, None), (6, None), (7, None), (9, None), (3, 0), (5, 0), (8, 0), (8, LMAX + 1)])
