"""K targets of one live scene, free-running (tracking.SceneTracker / MotionSceneTracker) without a GPU: the keyword and type
checks, the refusals of the K-target loops of sampling="reference" that stay, the lane table as a pure function against rows
written out by hand, and the per-target overflow against _matching_overflow run slot by slot."""
import numpy as np
import pytest


class _NoModel:
    """enough of a model for the keyword checks, which come before anything touches it"""


def _motion_model():
    """an M2TRACK by type only: the type check comes before anything touches the model"""
    from open3dsot_amd import m2track
    return object.__new__(m2track.M2TRACK)


GT = np.zeros((1, 2, 15), np.float32)


# ---- 1. keywords and types ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SceneTracker", "MotionSceneTracker"])
def test_sampling_keyword_of_the_scene_trackers(name):
    from open3dsot_amd import tracking
    cls = getattr(tracking, name)
    model = _motion_model() if name == "MotionSceneTracker" else _NoModel()
    with pytest.raises(ValueError, match="sampling"):
        cls(model, 2, sampling="nonsense")
    with pytest.raises(ValueError, match="sampling.*MultiTargetTracker"):
        cls(model, 2, sampling="reference")
    for K in (0, -1, tracking.PU.CROP_MULTI_MAX_TARGETS + 1):
        for sampling in tracking.FREE_RUNNING:
            with pytest.raises(ValueError, match="n_targets"):
                cls(model, K, sampling=sampling)


def test_sampling_keyword_of_the_scene_entry_points():
    from open3dsot_amd import tracking
    for model in (_NoModel(), _motion_model()):
        for sampling, match in (("nonsense", "sampling"), ("reference", "sampling.*MultiTargetTracker")):
            with pytest.raises(ValueError, match=match):
                tracking.scene_tracker_for(model, 2, sampling=sampling)
            with pytest.raises(ValueError, match=match):
                tracking.track_scene(model, [None], [None, None], sampling=sampling)
            with pytest.raises(ValueError, match=match):
                tracking.evaluate_scene(model, [None], GT, sampling=sampling)


def test_each_scene_class_names_the_other_for_the_wrong_model():
    from open3dsot_amd import tracking
    for sampling in tracking.FREE_RUNNING:
        with pytest.raises(TypeError, match="MotionSceneTracker"):
            tracking.SceneTracker(_motion_model(), 2, sampling=sampling)
        with pytest.raises(TypeError, match=r"with SceneTracker"):
            tracking.MotionSceneTracker(_NoModel(), 2, sampling=sampling)
    # scene_tracker_for picks the class by the model's type: each class then fails on ITS first touch of the model, not on the type
    with pytest.raises(ValueError, match="n_targets"):
        tracking.scene_tracker_for(_motion_model(), 0)
    with pytest.raises(ValueError, match="n_targets"):
        tracking.scene_tracker_for(_NoModel(), 0)
    with pytest.raises(AttributeError):
        tracking.scene_tracker_for(_NoModel(), 2)                                       # past every check: model.parameters()


# ---- 2. the five old names still refuse ------------------------------------------------------------------------------------------
def test_the_reference_k_target_loops_still_refuse_the_free_running_modes():
    from open3dsot_amd import tracking
    assert tracking.SAMPLING == ("reference", "device", "table")
    for sampling in ("device", "table"):
        for call in (lambda: tracking.MultiTargetTracker(_NoModel(), 2, sampling=sampling),
                     lambda: tracking.MultiMotionTracker(_NoModel(), 2, sampling=sampling),
                     lambda: tracking.multi_tracker_for(_NoModel(), 2, sampling=sampling),
                     lambda: tracking.track_targets(_NoModel(), [None], [None, None], sampling=sampling),
                     lambda: tracking.evaluate_targets(_NoModel(), [None], GT, sampling=sampling)):
            with pytest.raises(ValueError, match="the K-target loops are a follow-up"):
                call()


# ---- 3. the lane table ----------------------------------------------------------------------------------------------------------
def row(first, has_crop):
    #       active first has_crop t row ref_row rebase
    return [1, first, has_crop, 0, -1, -1, 0]


LANE_ROWS = {   # aggregation -> (t = 1, a steady frame, the frame after enroll(1)); K = 3
    "first": ([row(1, 1)] * 3, [row(0, 0)] * 3, [row(0, 0), row(1, 1), row(0, 0)]),
    "previous": ([row(1, 1)] * 3, [row(0, 1)] * 3, [row(0, 1), row(1, 1), row(0, 1)]),
    "firstandprevious": ([row(1, 1)] * 3, [row(0, 1)] * 3, [row(0, 1), row(1, 1), row(0, 1)]),
    "all": ([row(1, 1)] * 3, [row(0, 1)] * 3, [row(0, 1), row(1, 1), row(0, 1)]),
    None: ([row(1, 1)] * 3, [row(0, 1)] * 3, [row(0, 1), row(1, 1), row(0, 1)]),      # the motion tracker: no bank
}


@pytest.mark.parametrize("aggregation", list(LANE_ROWS))
def test_lane_rows_against_rows_written_out_by_hand(aggregation):
    from open3dsot_amd import points_utils as PU, tracking
    assert PU.LANE_FIELDS == ("active", "first", "has_crop", "t", "row", "ref_row", "rebase") and PU.LANE_COLS == 7
    assert [PU.LANE[f] for f in PU.LANE_FIELDS] == list(range(7))
    want_first, want_steady, want_enrolled = LANE_ROWS[aggregation]
    for first, want in (({0, 1, 2}, want_first), (set(), want_steady), ({1}, want_enrolled)):
        got = tracking.scene_lane_rows(3, first, aggregation)
        assert got.dtype == np.int32 and got.shape == (3, 7) and got.tolist() == want, (aggregation, first)
    assert tracking.scene_lane_rows(1, (), aggregation).tolist() == [want_steady[0]]
    assert tracking.scene_lane_rows(5, [4], aggregation)[4].tolist() == want_enrolled[1]


# ---- 4. overflow per target -----------------------------------------------------------------------------------------------------
def made_up_log():
    """(t = 7, K = 3, 2): slot 0 from frame 0, slot 1 enrolled after frame 2, slot 2 enrolled after frame 4; row 0 is -1"""
    log = np.array([[[-1, -1]] * 3,
                    [[900, 700], [1200, 30], [0, 0]],
                    [[1100, 650], [1300, 900], [0, 0]],
                    [[1001, 1001], [400, 1500], [2, 1]],
                    [[1000, 1000], [1100, 800], [3000, 3000]],
                    [[300, 999], [50, 1200], [1500, 400]],
                    [[1200, 20], [999, 100], [800, 1100]]], np.int32)
    return log, np.array([0, 2, 4])


@pytest.mark.parametrize("aggregation", ["first", "previous", "firstandprevious", "all"])
def test_overflow_per_target_is_matching_overflow_on_each_slots_own_rows(aggregation):
    from open3dsot_amd import tracking
    log, starts = made_up_log()
    if aggregation == "first":                             # a model crop on a slot's first tracked frame only
        for k, s in enumerate(starts):
            log[:, k, 1][np.arange(log.shape[0]) != s + 1] = -1
    caps = dict(search_capacity=1000, model_capacity=1000, bank_capacity=1800)
    got = tracking.scene_matching_overflow(log, starts, aggregation=aggregation, **caps)
    assert got.shape == (3, 3)
    for k, s in enumerate(starts):
        mine = np.ascontiguousarray(log[s:, k])            # row 0 of the cut: the frame the slot was given its box on, unused
        want = tracking._matching_overflow(mine, 1000, 1000, 1800, aggregation)
        assert tuple(got[k]) == want, (aggregation, k)
    # and against figures counted by hand from the table above
    by_hand = {"first": [[3, 0, 0], [1, 1, 0], [1, 0, 0]],
               "previous": [[3, 1, 0], [1, 2, 0], [1, 1, 0]],
               "firstandprevious": [[3, 1, 0], [1, 2, 2], [1, 1, 0]],      # slot 1: 2 x 1000 at its first frame, 1000 + 1000 at its third
               "all": [[3, 1, 4], [1, 2, 2], [1, 1, 0]]}[aggregation]      # slot 0: 700 + 650 + 1000 > 1800 from its third frame on
    assert got.tolist() == by_hand, (aggregation, got.tolist())


def test_motion_overflow_per_target_counts_each_slots_rows_from_its_start():
    from open3dsot_amd import tracking
    log, starts = made_up_log()
    got = tracking.scene_motion_overflow(log, starts, 1000)
    # slot 0: rows 1..6; slot 1: rows 3..6; slot 2: rows 5..6
    assert got.tolist() == [[3, 1, 0], [1, 2, 0], [1, 1, 0]]
    assert tracking.scene_motion_overflow(log, [0, 0, 0], 1000).tolist() == [[3, 1, 0], [3, 2, 0], [2, 2, 0]]
