"""The test epoch on L lanes (tracking.LaneTracker / MotionLaneTracker) without a GPU: the schedule's rule, the lane oracle
against the single-form oracles lane by lane, the validation of the lane entry points and the `lanes` keyword."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import free_running_oracle as FO  # noqa: E402
import lane_oracle as LO  # noqa: E402
import tracking_oracle as TO  # noqa: E402

LENGTH_SETS = [LO.LENGTHS, [1, 1, 1, 1], [4, 2], []]      # the fixture's, all-ones, fewer tracklets than (3 and 7) lanes, none


# ---- the schedule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["given", "longest_first"])
@pytest.mark.parametrize("lanes", [1, 3, 7])
@pytest.mark.parametrize("lengths", LENGTH_SETS)
def test_lane_schedule_follows_its_rule(lengths, lanes, order):
    from open3dsot_amd import tracking
    tracklet, frame = tracking.lane_schedule(lengths, lanes, order)
    want_j, want_t = LO.schedule(lengths, lanes, order)
    steps = len(want_j)
    assert tracklet.dtype == frame.dtype == np.int32 and tracklet.shape == frame.shape == (steps, lanes)      # steps: simulated here
    assert tracklet.tolist() == want_j and frame.tolist() == want_t
    # every (tracklet, t >= 1) exactly once, in increasing t, on one lane, without gaps
    seen = {}
    for s in range(steps):
        for l in range(lanes):
            j, t = int(tracklet[s, l]), int(frame[s, l])
            if j < 0:
                assert t == 0
                continue
            seen.setdefault(j, []).append((s, l, t))
    assert sorted(seen) == [j for j, n in enumerate(lengths) if n >= 2]                # a one-frame tracklet takes no lane
    for j, hits in seen.items():
        assert [t for _, _, t in hits] == list(range(1, lengths[j])), j
        assert len({l for _, l, _ in hits}) == 1, j
        assert [s for s, _, _ in hits] == list(range(hits[0][0], hits[0][0] + lengths[j] - 1)), j
    # a lane is never idle while a tracklet waits; the tracklets start in the order's sequence
    start = {j: hits[0][0] for j, hits in seen.items()}
    for s in range(steps):
        if (tracklet[s] < 0).any():
            assert all(st <= s for st in start.values()), s
    ids = sorted(seen, key=lambda j: -lengths[j]) if order == "longest_first" else sorted(seen)
    assert [start[j] for j in ids] == sorted(start[j] for j in ids)
    if steps:
        assert (tracklet[-1] >= 0).any()                                               # the last step still tracks


def test_lane_schedule_refuses_what_it_cannot_plan():
    from open3dsot_amd import tracking
    for bad in ([3, 0, 2], [0], [2, -1]):
        with pytest.raises(ValueError):
            tracking.lane_schedule(bad, 3)
    with pytest.raises(ValueError):
        tracking.lane_schedule([3], 0)
    with pytest.raises(ValueError, match="order"):
        tracking.lane_schedule([3], 2, order="shortest_first")
    a = tracking.lane_schedule([3, 8, 8, 2], 2, "longest_first")[0]
    assert a[0].tolist() == [1, 2]                                                     # stable: equal lengths keep their order


# ---- the lane oracle against the single-form oracles ----------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("rule", FO.RULES)
def test_lane_oracle_bank_update_equals_the_single_oracle_lane_by_lane(rule):
    rng = np.random.default_rng(2)
    L, crop_cap, bank_cap = 4, 40, 90
    lanes = LO.lane_table(L, active=[1, 1, 0, 1], first=[1, 0, 1, 0], has_crop=[1, 1, 1, 0])
    crop = rng.normal(size=(L, crop_cap, 3)).astype(np.float32)
    counts = np.array([33, 45, 7, 12], np.int32)                                       # 45 > crop_cap: cut to the buffer
    state_in = np.array([[0, 0], [30, 70], [5, 9], [11, 22]], np.int32)
    bank = np.full((L, bank_cap, 3), -7, np.float32)
    state_out = np.full((L, 2), -9, np.int32)
    LO.bank_update_lanes(state_in, crop, counts, rule, lanes, bank, state_out)
    for l in range(L):
        want_bank = np.full((bank_cap, 3), -7, np.float32)
        on = bool(lanes[l, 0] and lanes[l, 2])
        want = FO.bank_update(state_in[l], crop[l, :min(counts[l], crop_cap)], rule, bool(lanes[l, 1]), on, want_bank, bank_cap)
        assert tuple(state_out[l]) == want and np.array_equal(bits(bank[l]), bits(want_bank)), (rule, l)
        if not on:
            assert tuple(state_out[l]) == tuple(state_in[l]) and (bank[l] == -7).all()      # copied through, nothing else written


def test_lane_oracle_draws_equal_the_single_oracles_lane_by_lane():
    rng = np.random.default_rng(4)
    L, cap, S, N = 3, 50, 16, 8
    keys = FO.keys(3)
    src = rng.normal(size=(L, cap, 3)).astype(np.float32)
    counts = np.array([2, 16, 70], np.int32)
    dst, used = LO.resample_drawn_lanes(src, counts, keys[1], S)
    for l in range(L):
        want, want_used = FO.resample_drawn(src[l], counts[l], cap, keys[1], S)
        assert np.array_equal(bits(dst[l]), bits(want)) and np.array_equal(used[l], want_used)
    cur = rng.normal(size=(L, cap, 3)).astype(np.float32)
    wlh = rng.uniform(1, 4, (L, 3)).astype(np.float32)
    counts2 = np.array([[1, 30], [8, 8], [60, 3]], np.int32)
    lanes = LO.lane_table(L, first=[1, 0, 1])
    pts, bc, used = LO.motion_input_drawn_lanes(src, cur, counts2, keys, N, wlh, lanes)
    for l in range(L):
        p, b, u = FO.motion_input_drawn(src[l], cur[l], counts2[l], cap, keys, N, wlh[l], bool(lanes[l, 1]))
        assert np.array_equal(bits(pts[l]), bits(p)) and np.array_equal(bits(bc[l]), bits(b)) and np.array_equal(used[l], u)
    assert LO.motion_input_drawn_lanes(src, cur, counts2, keys, N, wlh, lanes, with_bc=False)[1] is None


def test_lane_oracle_offset_box_and_start_equal_the_single_oracle_lane_by_lane():
    rng = np.random.default_rng(5)
    L, R = 4, 6

    def boxes(n):
        out = np.zeros((n, 15), np.float32)
        out[:, :3], out[:, 3:6] = rng.normal(size=(n, 3)) * 10, rng.uniform(1, 4, (n, 3))
        a = rng.uniform(-3, 3, n)
        out[:, 6], out[:, 7], out[:, 9], out[:, 10], out[:, 14] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1
        return out
    cur, gt = boxes(L), boxes(R)
    yaw = np.concatenate([cur[:, 6:], rng.uniform(-1, 1, (L, 1)).astype(np.float32)], 1)
    offset = rng.normal(size=(L, 4)).astype(np.float32) * np.array([5, 5, 5, 30], np.float32)      # large: limit_box triggers
    lanes = LO.lane_table(L, active=[1, 1, 0, 1], t=[1, 4, 2, 7], row=[1, 4, -1, 5], ref_row=[-1, 3, 0, -1], rebase=[0, 1, 0, 1],
                          has_crop=[1, 0, 1, 1])
    counts = rng.integers(0, 99, (L, 2)).astype(np.int32)
    for limit_box in (False, True):
        out, res, log, st = np.full((L, 15), -7, np.float32), np.full((R, 15), -7, np.float32), np.full((R, 2), -9, np.int32), yaw.copy()
        LO.offset_box_lanes(cur, gt, offset, st, lanes, out, res, counts, log, True, True, limit_box, 11)
        for l in range(L):
            if not lanes[l, 0]:
                assert (out[l] == -7).all() and np.array_equal(st[l], yaw[l])
                continue
            ref = gt[lanes[l, 5]] if lanes[l, 5] >= 0 else cur[l]
            box, state = TO.offset_box(ref, offset[l], True, True, limit_box, seed=11, frame=int(lanes[l, 3]), yaw_state=yaw[l].copy(),
                                       rebase=bool(lanes[l, 6]))
            assert np.array_equal(bits(out[l]), bits(box)) and np.array_equal(bits(st[l]), bits(state))
            assert np.array_equal(bits(res[lanes[l, 4]]), bits(box))
            assert log[lanes[l, 4]].tolist() == [counts[l, 0], counts[l, 1] if lanes[l, 2] else -1]
        untouched = sorted(set(range(R)) - {1, 4, 5})
        assert (res[untouched] == -7).all() and (log[untouched] == -9).all()
    # the start: what init() sets
    lanes = LO.lane_table(L, active=[1, 1, 0, 1], first=[1, 0, 1, 1], t=[1, 2, 1, 1], row=[1, 4, 3, 6])
    c, y, w, s = (np.full(sh, -7, dt) for sh, dt in (((L, 15), np.float32), ((L, 10), np.float32), ((L, 3), np.float32), ((L, 2), np.int32)))
    LO.lane_start(gt, lanes, c, y, w, s)
    for l, row0 in ((0, 0), (3, 5)):
        assert np.array_equal(bits(c[l]), bits(gt[row0])) and np.array_equal(bits(y[l]), bits(np.append(gt[row0, 6:], 0)))
        assert np.array_equal(bits(w[l]), bits(gt[row0, 3:6])) and s[l].tolist() == [0, 0]
    for l in (1, 2):
        assert (c[l] == -7).all() and (y[l] == -7).all() and (w[l] == -7).all() and (s[l] == -7).all()


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def test_lane_entry_points_reject_bad_arguments_before_touching_the_device():
    from open3dsot_amd import capi, points_utils as PU
    lib = capi.load()
    EINVAL, LMAX = capi.CONSTANTS["O3D_EINVAL"], capi.CONSTANTS["O3D_CROP_MULTI_MAX_TARGETS"]
    assert (PU.LANE_COLS, PU.LANE) == (len(LO.FIELDS), LO.COL)                          # the oracle's columns are the header's
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.cast(ctypes.addressof(buf) + 64, ctypes.c_void_p)
    BIG = (1 << 29) + 1

    def refuses(entry, good, breaks):
        for field, bad in breaks:
            broken = list(good)
            broken[field] = bad
            assert entry(*broken, None) == EINVAL, (entry.__name__, field, bad)

    # crop, counts, count_stride, crop_cap, bank, bank_cap, rule, lanes, L, state_in, state_out
    refuses(lib.o3d_track_bank_update_lanes, [p, p, 2, 8, p, 16, 0, p, 2, p, q],
            [(0, None), (1, None), (4, None), (7, None), (9, None), (10, None), (10, p), (2, 0), (3, 0), (3, BIG), (5, 0), (5, BIG),
             (6, -1), (6, 4), (8, 0), (8, -1), (8, LMAX + 1)])
    # per cloud: src, n_dev, stride, cap, key, dst, S, used; then L
    cloud = [p, p, 2, 8, 1, p, 4, None]
    breaks = [(0, None), (1, None), (5, None), (2, 0), (3, 0), (3, BIG), (6, 0), (6, (1 << 20) + 1)]
    refuses(lib.o3d_track_resample_drawn_lanes, cloud + cloud + [2], breaks + [(8 + f, b) for f, b in breaks] + [(16, 0), (16, LMAX + 1)])
    # prev, cur, counts, capacity, key_prev, key_this, N, wlh, lanes, L, points, candidate_bc, used
    refuses(lib.o3d_track_motion_input_drawn_lanes, [p, p, p, 8, 1, 2, 4, p, p, 2, p, None, None],
            [(0, None), (1, None), (2, None), (7, None), (8, None), (10, None), (3, 0), (3, BIG), (6, 0), (6, (1 << 20) + 1), (9, 0),
             (9, LMAX + 1)])
    # cur, gt, R, offset, yaw_state, lanes, L, degrees, use_z, limit_box, seed, out, results, counts, counts_log
    refuses(lib.o3d_track_offset_box_lanes, [p, p, 4, p, p, p, 2, 1, 1, 0, 0, p, p, p, p],
            [(0, None), (1, None), (3, None), (4, None), (5, None), (11, None), (12, None), (13, None), (2, 0), (6, 0), (6, LMAX + 1),
             (10, -1)])
    # gt, R, lanes, L, cur, yaw_state, wlh, state
    refuses(lib.o3d_track_lane_start, [p, 4, p, 2, p, p, p, None],
            [(0, None), (2, None), (4, None), (5, None), (6, None), (1, 0), (3, 0), (3, LMAX + 1)])


class _NoModel:
    """enough of a model for the keyword checks, which come before anything touches it"""


def test_the_lanes_keyword_of_evaluate():
    from open3dsot_amd import tracking
    with pytest.raises(ValueError, match="sampling"):
        tracking.evaluate(_NoModel(), [], lanes=2, sampling="reference")
    with pytest.raises(ValueError, match="sampling"):
        tracking.evaluate(_NoModel(), [], lanes=2)                                      # the default is "reference"
    with pytest.raises(ValueError, match="sampling"):
        tracking.evaluate(_NoModel(), [], lanes=2, sampling="nonsense")


@pytest.mark.parametrize("name", ["MultiTargetTracker", "MultiMotionTracker"])
def test_the_multi_trackers_still_refuse_device_sampling(name):
    from open3dsot_amd import tracking
    with pytest.raises(ValueError, match="follow-up"):
        getattr(tracking, name)(_NoModel(), 2, sampling="device")
    with pytest.raises(ValueError, match="follow-up"):
        tracking.multi_tracker_for(_NoModel(), 2, sampling="device")
