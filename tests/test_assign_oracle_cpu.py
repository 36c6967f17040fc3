"""tests/assign_oracle.py, the Python restatement of the optimal assignment: its result is a one-to-one set
of admissible pairs on the free ends, of the optimum's cardinality and integer cost (brute force, scipy), on hand-built cases
whose answers are written out, with the ties resolved as the written order says.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import assign_oracle as AO  # noqa: E402
import mot_oracle as MOT  # noqa: E402
import scene_manage_oracle as SO  # noqa: E402
import test_mot_oracle_cpu as MC  # noqa: E402  (random_run, check_invariants)

INF = np.inf
GATES = (dict(min_iou=0.25, max_dist=3.0), dict(min_iou=0.0, max_dist=INF), dict(min_iou=0.5, max_dist=1.0))

# the two cases of the issue: track A = row 0, track B = row 1; every overlap 0, so the greedy walk goes by distance
COST_CASE = np.array([[1.0, 2.0], [1.5, 9.0]], np.float32)      # greedy (0,0) + (1,1) = 10 m; optimal (0,1) + (1,0) = 3.5 m
GATE = 3.0                                                      # (1,1) at 9 m is beyond it: B is admissible to d0 only


def random_case(rng, K, D, trial):
    """trial-th random (K,D) case -> (ov, di, row_active | None, n_col | None, gates): costs from a small value set (exact ties)
    on even trials, continuous on odd ones; tight and loose gates; a random row mask and column count from trial 2 on"""
    pick = (lambda m: rng.integers(0, 4, m) / 4.0) if trial % 2 == 0 else (lambda m: rng.random(m))
    ov = pick(K * D).reshape(K, D).astype(np.float32)
    di = (4.0 * pick(K * D)).reshape(K, D).astype(np.float32)
    act = None if trial < 2 else (rng.random(K) < 0.8).astype(np.int32)
    n_col = None if trial < 2 else int(rng.integers(0, D + 1))
    return ov, di, act, n_col, GATES[trial % 3]


def ok_of(ov, di, act, n_col, gates):
    K, D = ov.shape
    return SO.admissible(ov, di, np.ones(K, np.int32) if act is None else act, D if n_col is None else n_col, **gates)


def check_result(m, c, ok):
    """one-to-one, admissible only, the two arrays inverse to each other"""
    hit = np.flatnonzero(m >= 0)
    assert len(set(m[hit].tolist())) == len(hit) and all(ok[r, m[r]] for r in hit)
    assert all(c[m[r]] == r for r in hit) and int((c >= 0).sum()) == len(hit)
    assert not ok[np.ix_(m < 0, c < 0)].any()              # a maximum matching leaves no admissible pair free


def brute_force(q, ok):
    """(the most pairs, the smallest sum of q among the sets with that many) over every matching"""
    R, C = ok.shape
    best = [(0, 0)]

    def rec(r, taken, n, s):
        if r == R:
            if (n, -s) > (best[0][0], -best[0][1]):
                best[0] = (n, s)
            return
        rec(r + 1, taken, n, s)
        for c in range(C):
            if ok[r, c] and not taken >> c & 1:
                rec(r + 1, taken | 1 << c, n + 1, s + int(q[r, c]))
    rec(0, 0, 0, 0)
    return best[0]


def test_quantize_is_the_stated_fp32_arithmetic():
    di = np.array([-1.0, 0.0, 0.5, 1.0 / 3.0, 1023.9996, 1024.0, 5000.0, INF], np.float32)
    assert AO.quantize(None, di, "distance").tolist() == [0, 0, 512, 341, 1048576, 1048576, 1048576, 1048576]
    ov = np.array([-1.0, 0.0, 0.25, 1.0, 2.0, 1.0 - 2.0 ** -24], np.float32)
    assert AO.quantize(ov, None, "overlap").tolist() == [1048576, 1048576, 786432, 0, 0, 0]
    assert AO.quantize(np.float32(0.1), None, "overlap") == int(np.rint((np.float32(1) - np.float32(0.1)) * np.float32(1048576)))
    with pytest.raises(ValueError):
        AO.quantize(ov, di, "euclid")


def test_the_two_rules_differ_in_cost_on_the_2x2_case():
    ov = np.zeros((2, 2), np.float32)
    g = AO.assign(ov, COST_CASE, assignment="greedy")
    o = AO.assign(ov, COST_CASE, assignment="optimal")
    assert g[0].tolist() == [0, 1] and g[1].tolist() == [0, 1] and g[2] == (2, 1024 + 9216)
    assert o[0].tolist() == [1, 0] and o[1].tolist() == [1, 0] and o[2] == (2, 2048 + 1536)


def test_the_two_rules_differ_in_cardinality_on_the_gated_2x2_case():
    ov = np.zeros((2, 2), np.float32)
    g = AO.assign(ov, COST_CASE, max_dist=GATE, assignment="greedy")
    stats = {}
    o = AO.assign(ov, COST_CASE, max_dist=GATE, assignment="optimal", stats=stats)
    assert g[0].tolist() == [0, -1] and g[1].tolist() == [0, -1] and g[2] == (1, 1024)          # B missed, d1 left over
    assert o[0].tolist() == [1, 0] and o[1].tolist() == [1, 0] and o[2] == (2, 2048 + 1536)
    assert stats["reassigned"] == 1 and stats["evicted"] == 0                                  # B's path moved A from d0 to d1


def test_a_cheaper_row_evicts_an_earlier_one_when_only_one_can_be_matched():
    stats = {}
    m, c, s = AO.assign(np.zeros((2, 1), np.float32), np.array([[2.0], [1.0]], np.float32), stats=stats)
    assert m.tolist() == [-1, 0] and c.tolist() == [1] and s == (1, 1024) and stats["evicted"] == 1


@pytest.mark.parametrize("cost", AO.COSTS)
def test_cardinality_and_cost_equal_brute_force_up_to_6x6(cost):
    rng = np.random.default_rng(3)
    differs = 0
    for trial in range(120):
        K, D = (int(x) for x in rng.integers(1, 7, 2))
        ov, di, act, n_col, gates = random_case(rng, K, D, trial % 6)
        ok = ok_of(ov, di, act, n_col, gates)
        m, c, s = AO.assign(ov, di, act, n_col, assignment="optimal", cost=cost, **gates)
        check_result(m, c, ok)
        assert s == brute_force(AO.quantize(ov, di, cost), ok), trial
        g = AO.assign(ov, di, act, n_col, assignment="greedy", cost=cost, **gates)
        assert (g[2][0], -g[2][1]) <= (s[0], -s[1])
        differs += g[2] != s
    assert differs > 0                                      # the greedy walk is not the optimum on some of them


@pytest.mark.parametrize("K,D", [(8, 8), (30, 40), (70, 65)])
def test_cardinality_and_cost_equal_scipy_on_the_padded_matrix(K, D):
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(10 * K + D)
    for trial in range(6):
        ov, di, act, n_col, gates = random_case(rng, K, D, trial)
        for cost in AO.COSTS:
            ok = ok_of(ov, di, act, n_col, gates)
            q = AO.quantize(ov, di, cost)
            m, c, s = AO.assign(ov, di, act, n_col, assignment="optimal", cost=cost, **gates)
            check_result(m, c, ok)
            P = np.full((K, D + K), float(AO.BIG))
            P[:, :D] = np.where(ok, q, 4.0 * AO.BIG)
            rows, cols = opt.linear_sum_assignment(P)
            pairs = [(r, k) for r, k in zip(rows, cols) if k < D]
            assert all(ok[r, k] for r, k in pairs)
            assert s == (len(pairs), sum(int(q[r, k]) for r, k in pairs)), (trial, cost)


def test_exact_ties_resolve_as_the_written_order_says():
    # every pair tied: row r ends on column r (the lowest free column; the tie with a held column goes to the held, lower one
    # first, which leads on to nothing strictly shorter), after r + 1 steps
    stats = {}
    m, c, s = AO.assign(np.zeros((4, 6), np.float32), np.ones((4, 6), np.float32), stats=stats)
    assert m.tolist() == [0, 1, 2, 3] and c.tolist() == [0, 1, 2, 3, -1, -1] and s == (4, 4096) and stats["steps"] == 1 + 2 + 3 + 4
    # two optima of equal cost, (0,0) + (1,1) and (0,1) + (1,0): row 0 is inserted first and takes column 0, row 1 then reaches
    # the free column 1 directly at the same length as through column 0
    m, _, _ = AO.assign(np.zeros((2, 2), np.float32), np.array([[1, 1], [1, 1]], np.float32))
    assert m.tolist() == [0, 1]
    # more rows than columns, all tied: matching the new row directly, evicting row 0 and evicting row 1 all end at the same
    # length in a private column, and the lowest column number is row 0's: of tied rows the LATER ones end up with the columns
    stats = {}
    m, c, _ = AO.assign(np.zeros((4, 2), np.float32), np.ones((4, 2), np.float32), stats=stats)
    assert m.tolist() == [-1, -1, 0, 1] and c.tolist() == [2, 3] and stats["evicted"] == 2
    # a tie between a direct column and a path through a held one: the lowest column number is explored first, the direct column
    # still ends the path
    di = np.array([[1, 3, 9], [1, 1, 9], [9, 1, 1]], np.float32)
    m, _, s = AO.assign(np.zeros((3, 3), np.float32), di)
    assert m.tolist() == [0, 1, 2] and s == (3, 3072)


def test_a_taken_row_or_column_is_never_touched():
    rng = np.random.default_rng(5)
    ov, di = rng.random((9, 7)).astype(np.float32), rng.random((9, 7)).astype(np.float32)
    ok = np.ones((9, 7), bool)
    ok[[2, 5], :] = False                                   # rows 2 and 5, columns 0 and 3 are taken or out of play
    ok[:, [0, 3]] = False
    m, c = AO.optimal_match(ov, di, ok)
    assert (m[[2, 5]] == -1).all() and (c[[0, 3]] == -1).all() and not np.isin(m, [0, 3]).any() and (m >= 0).sum() == 5
    check_result(m, c, ok)
    m2, c2 = AO.optimal_match(ov, di, ok, rows=[r for r in range(9) if r not in (2, 5)])
    assert np.array_equal(m, m2) and np.array_equal(c, c2)  # inserting a row without a pair changes nothing


def test_no_column_no_admissible_pair_and_nan():
    ov, di = np.full((3, 4), 0.5, np.float32), np.ones((3, 4), np.float32)
    for kw in (dict(n_col=0), dict(max_dist=0.5), dict(min_iou=0.6), dict(row_active=np.zeros(3, np.int32))):
        m, c, s = AO.assign(ov, di, **kw)
        assert (m == -1).all() and (c == -1).all() and s == (0, 0), kw
    ov[0, 0], di[1, 1] = np.nan, np.nan                     # a NaN is never admissible, under either cost
    for cost in AO.COSTS:
        m, c, s = AO.assign(ov, di, cost=cost)
        assert m[0] != 0 and m[1] != 1 and s[0] == 3
        check_result(m, c, ok_of(ov, di, None, None, dict(min_iou=0.0, max_dist=INF)))


def test_the_frame_oracles_with_greedy_are_the_existing_oracles_and_with_optimal_differ():
    rng = np.random.default_rng(11)
    differs = 0
    for trial in range(6):
        K, D = 7, 9
        ov, di, act, n_col, gates = random_case(rng, K, D, trial)
        act = np.ones(K, np.int32) if act is None else act
        s = SO.new_state(K, 4, np.zeros((K, 15), np.float32))
        s["active"][:] = act
        dets = rng.normal(size=(D, 15)).astype(np.float32)
        counts = np.zeros((K, 2), np.int32)
        n = D if n_col is None else n_col
        want = SO.manage(s, ov, di, dets, n, counts, 1, **gates)
        got = AO.manage(s, ov, di, dets, n, counts, 1, assignment="greedy", **gates)
        opt = AO.manage(s, ov, di, dets, n, counts, 1, assignment="optimal", **gates)
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(a, b)
        for name in want[0]:
            assert np.array_equal(got[0][name], want[0][name]), name
        m, c = AO.optimal_match(ov, di, SO.admissible(ov, di, act, n, **gates))
        assert np.array_equal(opt[1], m) and np.array_equal(opt[2], c) and np.array_equal(opt[0]["match_log"][1], m)
        differs += not np.array_equal(opt[1], want[1])
        fov, fdi, valid, ids = MC.random_run(rng, 5, 6, 7, ties=trial % 2 == 0)
        w = MOT.walk(fov, fdi, valid, ids, **gates)
        g = AO.mot_walk(fov, fdi, valid, ids, assignment="greedy", **gates)
        o = AO.mot_walk(fov, fdi, valid, ids, assignment="optimal", **gates)
        for name in ("match_slot", "match_id", "match_ov", "match_di", "per_frame", "carried"):
            assert np.array_equal(g[name], w[name]), name
        MC.check_invariants(o, fov, fdi, valid, ids, gates)
        assert (o["per_frame"][:, 2] >= 0).all() and o["per_frame"][0, 2] >= w["per_frame"][0, 2]    # frame 0 has no carry yet
        differs += not np.array_equal(o["match_slot"], w["match_slot"])
    assert differs >= 2 and SO.greedy_match is AO._GREEDY    # the swap is undone
