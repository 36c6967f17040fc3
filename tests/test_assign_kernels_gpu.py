"""o3d_scene_assign, o3d_scene_manage_assign and o3d_scene_mot_walk_assign (csrc/scene.hip) through the C ABI, per call, against the
Python restatement tests/assign_oracle.py: every output array equal, integers and bits only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import assign_oracle as AO  # noqa: E402
import mot_oracle as MOT  # noqa: E402
import scene_manage_oracle as SO  # noqa: E402
import test_assign_oracle_cpu as AC  # noqa: E402  (random_case, ok_of, check_result, COST_CASE, GATE)
import test_mot_kernels_gpu as MK  # noqa: E402  (device_walk, random_cases, ROWS, STATE)
import test_mot_oracle_cpu as MC  # noqa: E402  (check_invariants)
import test_scene_manage_kernels_gpu as SK  # noqa: E402  (bits, scene, state_of, device_step, STATE)

pytestmark = pytest.mark.gpu
bits = SK.bits
RANDOM_SHAPES = [(5, 6), (65, 70), (130, 3), (3, 130)]     # a wave crossed in rows, in columns, in both; K > D and D > K


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def up(a, dev, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def device_assign(dev, ov, di, act=None, n_col=None, assignment="optimal", cost="distance", **gates):
    """one o3d_scene_assign launch on uploads, the outputs preset to sentinels -> (match, col_match, (pairs, sum)) read back"""
    from open3dsot_amd import points_utils as PU
    K, D = ov.shape
    out = (torch.full((K,), -7, dtype=torch.int32, device=dev), torch.full((D,), -7, dtype=torch.int32, device=dev),
           torch.full((2,), -7, dtype=torch.int64, device=dev))
    PU.scene_assign(up(ov, dev, np.float32), up(di, dev, np.float32), None if act is None else up(act, dev, np.int32),
                    None if n_col is None else torch.tensor([n_col], dtype=torch.int32, device=dev), assignment=assignment, cost=cost,
                    out=out, **gates)
    m, c, s = (o.cpu().numpy() for o in out)
    return m, c, tuple(int(x) for x in s)


def assert_assign(dev, ov, di, act=None, n_col=None, what=None, stats=None, **kw):
    got = device_assign(dev, ov, di, act, n_col, **kw)
    want = AO.assign(ov, di, act, n_col, stats=stats, **kw)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), (what, "match", got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, "col_match")
    assert got[2] == want[2], (what, "summary", got[2], want[2])
    return got


# ---- o3d_scene_assign ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", AO.COSTS)
def test_assign_1x1_and_the_two_hand_built_cases(dev, cost):
    one = np.full((1, 1), 0.5, np.float32)
    assert assert_assign(dev, one, one, what="1x1", cost=cost)[0].tolist() == [0]
    assert assert_assign(dev, one, one, what="1x1 gated", cost=cost, max_dist=0.25)[0].tolist() == [-1]
    ov = np.zeros((2, 2), np.float32)
    m, c, s = assert_assign(dev, ov, AC.COST_CASE, what="cost", cost="distance")
    assert m.tolist() == [1, 0] and s == (2, 2048 + 1536)
    g = assert_assign(dev, ov, AC.COST_CASE, what="cost, greedy", assignment="greedy")
    assert g[0].tolist() == [0, 1] and g[2] == (2, 1024 + 9216)
    m, c, s = assert_assign(dev, ov, AC.COST_CASE, what="gate", max_dist=AC.GATE)
    assert m.tolist() == [1, 0] and c.tolist() == [1, 0] and s == (2, 2048 + 1536)
    g = assert_assign(dev, ov, AC.COST_CASE, what="gate, greedy", max_dist=AC.GATE, assignment="greedy")
    assert g[0].tolist() == [0, -1] and g[1].tolist() == [0, -1] and g[2] == (1, 1024)


@pytest.mark.parametrize("K,D", RANDOM_SHAPES)
def test_assign_on_random_matrices_equals_the_oracle(dev, K, D):
    """ties and continuous costs, tight and loose gates, random row masks and column counts, both costs; the oracle alone shows
    that the cases are not vacuous: the optimum differs from the greedy walk, and augmenting paths move earlier rows"""
    rng = np.random.default_rng(4000 + 100 * K + D)
    stats, differs = {}, 0
    for trial in range(6):
        ov, di, act, n_col, gates = AC.random_case(rng, K, D, trial)
        for cost in AO.COSTS:
            got = assert_assign(dev, ov, di, act, n_col, (K, D, trial, cost), stats, cost=cost, **gates)
            AC.check_result(got[0], got[1], AC.ok_of(ov, di, act, n_col, gates))
            greedy = assert_assign(dev, ov, di, act, n_col, (K, D, trial, cost, "greedy"), assignment="greedy", cost=cost, **gates)
            ok = AC.ok_of(ov, di, act, n_col, gates)
            want_m, want_c = SO.greedy_match(ov, di, ok)
            assert np.array_equal(greedy[0], want_m) and np.array_equal(greedy[1], want_c)
            assert (greedy[2][0], -greedy[2][1]) <= (got[2][0], -got[2][1])
            differs += greedy[2] != got[2]
            again = device_assign(dev, ov, di, act, n_col, cost=cost, **gates)
            assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and again[2] == got[2]
    print("(K,D) = (%d,%d): optimal != greedy in %d of 12, %s" % (K, D, differs, stats))
    assert differs > 0 and stats["reassigned"] > 0, (differs, stats)


def test_assign_with_every_pair_tied_65x65(dev):
    stats = {}
    m, c, s = assert_assign(dev, np.zeros((65, 65), np.float32), np.ones((65, 65), np.float32), what="tied", stats=stats)
    assert m.tolist() == list(range(65)) and s == (65, 65 * 1024) and stats["steps"] == 65 * 66 // 2
    m, c, s = assert_assign(dev, np.full((65, 65), 0.5, np.float32), np.ones((65, 65), np.float32), what="tied", cost="overlap")
    assert m.tolist() == list(range(65)) and s == (65, 65 * 524288)
    # more rows than columns, every pair tied: evictions all over (the later rows end up with the columns)
    m, c, s = assert_assign(dev, np.zeros((70, 65), np.float32), np.ones((70, 65), np.float32), what="tied, K > D", stats=stats)
    assert s == (65, 65 * 1024) and stats["evicted"] > 0


def test_assign_without_an_admissible_pair_without_columns_and_with_nan(dev):
    rng = np.random.default_rng(8)
    ov, di = rng.random((9, 7)).astype(np.float32), rng.random((9, 7)).astype(np.float32)
    for kw in (dict(n_col=0), dict(max_dist=-1.0), dict(min_iou=2.0), dict(act=np.zeros(9, np.int32)), dict(n_col=-3)):
        for rule in AO.ASSIGNMENTS:
            m, c, s = assert_assign(dev, ov, di, what=kw, assignment=rule, **kw)
            assert (m == -1).all() and (c == -1).all() and s == (0, 0)
    assert assert_assign(dev, ov, di, n_col=99, what="n_col > D")[2][0] == 7
    ov[rng.random((9, 7)) < 0.3] = np.nan
    di[rng.random((9, 7)) < 0.3] = np.nan
    for cost in AO.COSTS:
        for rule in AO.ASSIGNMENTS:
            m, c, _ = assert_assign(dev, ov, di, what="nan", assignment=rule, cost=cost)
            hit = np.flatnonzero(m >= 0)
            assert len(hit) > 0 and not np.isnan(ov[hit, m[hit]]).any() and not np.isnan(di[hit, m[hit]]).any()


def test_the_wrapper_refuses_unknown_names_and_cpu_tensors(dev):
    from open3dsot_amd import points_utils as PU
    z = torch.zeros((2, 2), device=dev)
    with pytest.raises(ValueError, match="assignment"):
        PU.scene_assign(z, z, assignment="hungarian")
    with pytest.raises(ValueError, match="cost"):
        PU.scene_assign(z, z, cost="euclid")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        PU.scene_assign(z.cpu(), z.cpu())


# ---- o3d_scene_manage_assign -----------------------------------------------------------------------------------------------------------
def manage_cases(K, D):
    """the random cases of test_scene_manage_kernels_gpu.test_manage_on_random_matrices_with_ties_equals_the_oracle"""
    rng = np.random.default_rng(1000 * K + D)
    tracks, dets = SK.scene(rng, K, D, 0)
    for trial in range(6):
        pick = (lambda m: rng.integers(0, 4, m) / 4.0) if trial % 2 == 0 else (lambda m: rng.random(m))
        ov = pick(K * D).reshape(K, D).astype(np.float32)
        di = (4.0 * pick(K * D)).reshape(K, D).astype(np.float32)
        active = (rng.random(K) < 0.8).astype(np.int32)
        n_det = D if trial < 2 else int(rng.integers(0, D + 1))
        gates = dict(min_iou=0.25, max_dist=3.0) if trial % 3 else {}
        s = SK.state_of(rng, K, 4, tracks, active)
        counts = rng.integers(0, 40, (K, 2)).astype(np.int32)
        yield trial, s, ov, di, dets, n_det, counts, gates


@pytest.mark.parametrize("K,D", [(5, 6), (65, 70), (130, 3)])
def test_manage_assign_optimal_equals_the_frame_oracle(dev, K, D):
    stats, differs = {}, 0
    for trial, s, ov, di, dets, n_det, counts, gates in manage_cases(K, D):
        cost = AO.COSTS[trial % 2]
        kw = dict(max_misses=1, assignment="optimal", cost=cost, **gates)
        got, _, _ = SK.device_step(dev, s, dets, n_det, counts, 2, scores=(ov, di), **kw)
        want, match, det_match = AO.manage(s, ov, di, dets, n_det, counts, 2, stats=stats, **kw)
        for name in SK.STATE:
            assert got[name].dtype == want[name].dtype and np.array_equal(bits(got[name]), bits(want[name])), (K, D, trial, name)
        assert got["match_log"][2].tolist() == match.tolist()
        differs += not np.array_equal(match, SO.manage(s, ov, di, dets, n_det, counts, 2, max_misses=1, **gates)[1])
    print("(K,D) = (%d,%d): optimal != greedy in %d of 6 frames, %s" % (K, D, differs, stats))
    assert differs > 0 and stats["reassigned"] > 0


def through_the_assign_entries(monkeypatch):
    """points_utils' greedy calls, which go through the two older entries, sent through the new ones with O3D_ASSIGN_GREEDY"""
    from open3dsot_amd import capi
    lib = capi.load()
    manage, walk = lib.o3d_scene_manage_assign, lib.o3d_scene_mot_walk_assign
    g, c = capi.CONSTANTS["O3D_ASSIGN_GREEDY"], capi.CONSTANTS["O3D_COST_OVERLAP"]         # the walk ignores the cost
    monkeypatch.setattr(lib, "o3d_scene_manage", lambda *a: manage(*a[:-1], g, c, a[-1]))
    monkeypatch.setattr(lib, "o3d_scene_mot_walk", lambda *a: walk(*a[:-1], g, c, a[-1]))


def test_manage_assign_greedy_equals_o3d_scene_manage_in_bits(dev, monkeypatch):
    runs = []
    for new_entry in (False, True):
        if new_entry:
            through_the_assign_entries(monkeypatch)
        runs.append([SK.device_step(dev, s, dets, n_det, counts, 2, scores=(ov, di), max_misses=1, **gates)[0]
                     for _, s, ov, di, dets, n_det, counts, gates in manage_cases(65, 70)])
    for old, new in zip(*runs):
        for name in SK.STATE:
            assert np.array_equal(bits(old[name]), bits(new[name])), name
    assert any((r["match_log"][2] >= 0).any() for r in runs[0])


# ---- o3d_scene_mot_walk_assign ---------------------------------------------------------------------------------------------------------
def assert_walk(dev, ov, di, valid, ids, what, state, stats, **kw):
    got = MK.device_walk(dev, ov, di, valid, ids, state, **kw)
    p = dict(MOT.GATES)
    p.update(kw)
    want = AO.mot_walk(ov, di, valid, ids, state, stats=stats, **p)
    for n in MK.ROWS:
        assert got[n].dtype == want[n].dtype and np.array_equal(bits(got[n]), bits(want[n])), (what, n)
    for n in MK.STATE:
        assert got["state"][n].dtype == np.int32 and np.array_equal(got["state"][n], want["state"][n]), (what, n)
    return got, want


@pytest.mark.parametrize("F,G,K", [(3, 5, 6), (4, 65, 70), (2, 130, 3), (2, 3, 130)])
def test_walk_assign_optimal_equals_the_frame_oracle(dev, F, G, K):
    """the random runs of test_mot_kernels_gpu: odd trials start from a mid-sequence state with shared remembered ids"""
    stats, differs, carried = {}, 0, 0
    for trial, ov, di, valid, ids, state, gates in MK.random_cases(F, G, K):
        kw = dict(assignment="optimal", cost=AO.COSTS[trial % 2], **gates)
        got, want = assert_walk(dev, ov, di, valid, ids, (F, G, K, trial), state, stats, **kw)
        MC.check_invariants(got, ov, di, valid, ids, gates)
        carried += int(want["carried"].sum())
        differs += not np.array_equal(want["match_slot"], MOT.walk(ov, di, valid, ids, state, **gates)["match_slot"])
        # split into two calls, and the same call again
        head = MK.device_walk(dev, ov[:1], di[:1], valid[:1], ids[:1], state, **kw)
        tail = MK.device_walk(dev, ov[1:], di[1:], valid[1:], ids[1:], head["state"], **kw)
        again = MK.device_walk(dev, ov, di, valid, ids, state, **kw)
        for n in MK.ROWS:
            assert np.array_equal(bits(np.concatenate([head[n], tail[n]])), bits(got[n])), (trial, n)
            assert np.array_equal(bits(again[n]), bits(got[n])), (trial, n)
        for n in MK.STATE:
            assert np.array_equal(tail["state"][n], got["state"][n]) and np.array_equal(again["state"][n], got["state"][n]), (trial, n)
    print("(F,G,K) = (%d,%d,%d): optimal != greedy in %d of 6 runs, carried %d, %s" % (F, G, K, differs, carried, stats))
    assert differs > 0 and carried > 0 and stats["reassigned"] > 0


def test_walk_assign_greedy_equals_o3d_scene_mot_walk_in_bits(dev, monkeypatch):
    runs = []
    for new_entry in (False, True):
        if new_entry:
            through_the_assign_entries(monkeypatch)
        runs.append([MK.device_walk(dev, ov, di, valid, ids, state, **gates)
                     for _, ov, di, valid, ids, state, gates in MK.random_cases(4, 65, 70)])
    for old, new in zip(*runs):
        for n in MK.ROWS:
            assert np.array_equal(bits(old[n]), bits(new[n])), n
        for n in MK.STATE:
            assert np.array_equal(old["state"][n], new["state"][n]), n
    assert any((r["match_slot"] >= 0).any() for r in runs[0])
