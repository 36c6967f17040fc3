"""tests/mot_oracle.py, the numpy restatement of the CLEAR-MOT bookkeeping, on hand-built cases whose
answers are written out, and its invariants on random inputs.  No GPU."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mot_oracle as MOT  # noqa: E402

INF = np.inf


def matrices(F, G, K, pairs):
    """ov = -1, di = +inf everywhere but pairs: {(f,g,k): (ov, di)}"""
    ov, di = np.full((F, G, K), -1.0, np.float32), np.full((F, G, K), INF, np.float32)
    for (f, g, k), (o, d) in pairs.items():
        ov[f, g, k], di[f, g, k] = o, d
    return ov, di


def diagonal(F, G, ids):
    """object g sits on column g in every frame (overlap 0.9, distance 0.1), every other pair beyond the gate (5 m)"""
    ov, di = np.zeros((F, G, G), np.float32), np.full((F, G, G), 5.0, np.float32)
    for g in range(G):
        ov[:, g, g], di[:, g, g] = 0.9, 0.1
    return ov, di, np.ones((F, G), np.int32), np.asarray(ids, np.int32).reshape(F, G)


def totals(out):
    return dict(zip(MOT.FRAME_COLS, out["per_frame"][:, :7].sum(0).tolist()))


def test_perfect_tracking():
    ov, di, valid, ids = diagonal(4, 3, [[7, 8, 9]] * 4)
    out = MOT.walk(ov, di, valid, ids)
    assert totals(out) == dict(gt=12, hyp=12, tp=12, fp=0, fn=0, idsw=0, frag=0)
    assert out["match_slot"].tolist() == [[0, 1, 2]] * 4 and out["match_id"].tolist() == [[7, 8, 9]] * 4
    assert not out["carried"][0].any() and out["carried"][1:].all()
    s = MOT.summary(out["per_frame"], out["match_slot"], out["match_ov"], out["match_di"], valid)
    assert s["mota"] == 1.0 and s["idsw"] == 0 and s["recall"] == 1.0 and s["precision"] == 1.0 and s["frames"] == 4
    assert s["motp_dist"] == pytest.approx(float(np.float32(0.1)), rel=1e-12) and s["motp_iou"] == pytest.approx(float(np.float32(0.9)), rel=1e-12)
    assert s["mostly_tracked"] == 1.0 and s["mostly_lost"] == 0.0 and s["objects"] == 3


def test_two_targets_exchange_their_ids_at_one_frame():
    ov, di, valid, ids = diagonal(4, 2, [[5, 6], [5, 6], [6, 5], [6, 5]])
    out = MOT.walk(ov, di, valid, ids)
    # at frame 2 the remembered id sits on the other object's column, 5 m away: the carry is inadmissible, the walk re-pairs
    assert out["per_frame"][:, 5].tolist() == [0, 0, 2, 0] and totals(out)["idsw"] == 2 and totals(out)["fn"] == 0
    assert out["match_id"].tolist() == [[5, 6], [5, 6], [6, 5], [6, 5]] and out["carried"].tolist() == [[False] * 2, [True] * 2, [False] * 2, [True] * 2]
    s = MOT.summary(out["per_frame"], out["match_slot"], out["match_ov"], out["match_di"], valid)
    assert s["mota"] == 1.0 - 2.0 / 8.0


@pytest.mark.parametrize("new_id", [False, True])
def test_a_gap_resumed_under_the_same_or_a_new_id(new_id):
    ov, di, valid, ids = diagonal(5, 1, [[3], [3], [-1], [-1], [4 if new_id else 3]])
    out = MOT.walk(ov, di, valid, ids)
    assert totals(out) == dict(gt=5, hyp=3, tp=3, fp=0, fn=2, idsw=int(new_id), frag=1)
    assert out["per_frame"][:, 4].tolist() == [0, 0, 1, 1, 0] and out["per_frame"][4, 5:7].tolist() == [int(new_id), 1]
    assert out["match_slot"][:, 0].tolist() == [0, 0, -1, -1, 0] and np.isinf(out["match_di"][2:4, 0]).all() and (out["match_ov"][2:4, 0] == -1).all()
    assert out["state"]["last_id"].tolist() == [4 if new_id else 3]


def test_an_extra_hypothesis_is_a_false_positive():
    ov, di = matrices(2, 1, 2, {(0, 0, 0): (0.8, 0.2), (1, 0, 0): (0.8, 0.2)})         # column 1: 5 m away from everything
    ov[:, 0, 1], di[:, 0, 1] = 0.0, 5.0
    out = MOT.walk(ov, di, np.ones((2, 1), np.int32), np.array([[1, 2], [1, -1]], np.int32))
    assert totals(out) == dict(gt=2, hyp=3, tp=2, fp=1, fn=0, idsw=0, frag=0) and out["per_frame"][:, 3].tolist() == [1, 0]


def test_a_kept_identity_beats_a_better_pair_until_it_is_inadmissible():
    # object 0 remembers id 1 (column 0).  Frame 1: column 1 (id 2) scores better, column 0 still passes the gate: kept.
    # Frame 2: column 0 is beyond the gate: dropped, the walk takes column 1, an identity switch.
    pairs = {(0, 0, 0): (0.9, 0.1), (0, 0, 1): (0.0, 1.9), (1, 0, 0): (0.1, 1.5), (1, 0, 1): (0.9, 0.1),
             (2, 0, 0): (0.0, 2.5), (2, 0, 1): (0.9, 0.1)}
    ov, di = matrices(3, 1, 2, pairs)
    out = MOT.walk(ov, di, np.ones((3, 1), np.int32), np.array([[1, 2]] * 3, np.int32))
    assert out["match_id"][:, 0].tolist() == [1, 1, 2] and out["carried"][:, 0].tolist() == [False, True, False]
    assert out["per_frame"][:, 5].tolist() == [0, 0, 1] and out["per_frame"][:, 3].tolist() == [1, 1, 1]
    assert out["match_ov"][1, 0] == np.float32(0.1) and out["match_di"][1, 0] == np.float32(1.5)


def test_two_objects_remembering_one_id_the_lower_g_keeps_it():
    state = dict(last_id=np.array([7, 7], np.int32), tracked_prev=np.ones(2, np.int32), ever=np.ones(2, np.int32))
    # column 0 carries id 7 and is closer to object 1; column 1 (id 8) is admissible for both
    ov, di = matrices(1, 2, 2, {(0, 0, 0): (0.2, 1.0), (0, 1, 0): (0.9, 0.1), (0, 0, 1): (0.5, 0.5), (0, 1, 1): (0.1, 1.5)})
    out = MOT.walk(ov, di, np.ones((1, 2), np.int32), np.array([[7, 8]], np.int32), state)
    assert out["match_slot"].tolist() == [[0, 1]] and out["carried"].tolist() == [[True, False]]
    assert out["per_frame"][0].tolist() == [2, 2, 2, 0, 0, 1, 0, 0] and out["state"]["last_id"].tolist() == [7, 8]
    assert state["last_id"].tolist() == [7, 7]                                          # nothing passed in is changed
    # when object 0's pair with column 0 is inadmissible, object 1 takes it
    ov[0, 0, 0], di[0, 0, 0] = 0.0, 9.0
    out = MOT.walk(ov, di, np.ones((1, 2), np.int32), np.array([[7, 8]], np.int32), state)
    assert out["match_slot"].tolist() == [[1, 0]] and out["carried"].tolist() == [[False, True]] and out["per_frame"][0, 5] == 1


def test_an_invalid_object_keeps_its_memory_across_the_gap():
    ov, di, valid, ids = diagonal(4, 2, [[1, 2], [1, 2], [1, 2], [1, 2]])
    valid[1:3, 0] = 0
    ov[1:3, 0, :], di[1:3, 0, :] = 0.9, 0.0            # whatever the matrices hold there: an invalid g is never matched
    out = MOT.walk(ov, di, valid, ids)
    assert out["match_slot"][:, 0].tolist() == [0, -1, -1, 0] and out["carried"][3, 0]
    assert totals(out) == dict(gt=6, hyp=8, tp=6, fp=2, fn=0, idsw=0, frag=0)             # no fn, no frag: tracked_prev was kept
    mid = MOT.walk(ov[:2], di[:2], valid[:2], ids[:2])["state"]
    assert mid["last_id"].tolist() == [1, 2] and mid["tracked_prev"].tolist() == [1, 1] and mid["ever"].tolist() == [1, 1]
    s = MOT.summary(out["per_frame"], out["match_slot"], out["match_ov"], out["match_di"], valid)
    assert s["objects"] == 2 and s["mostly_tracked"] == 1.0


def test_summary_of_nothing_is_all_zero():
    s = MOT.summary(np.zeros((0, 8), np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32),
                    np.zeros((0, 2), np.int32))
    assert all(v == 0 for v in s.values()) and set(s) >= {"mota", "motp_dist", "motp_iou", "recall", "precision", "mostly_tracked", "mostly_lost"}


def test_mostly_tracked_and_mostly_lost_thresholds():
    valid = np.ones((5, 3), np.int32)
    slot = np.full((5, 3), -1, np.int32)
    slot[:4, 0] = 0                                        # 4 of 5: mostly tracked
    slot[:1, 1] = 1                                        # 1 of 5: mostly lost
    slot[:2, 2] = 2                                        # 2 of 5: neither
    per_frame = np.zeros((5, 8), np.int32)
    s = MOT.summary(per_frame, slot, np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), valid)
    assert s["mostly_tracked"] == pytest.approx(1 / 3) and s["mostly_lost"] == pytest.approx(1 / 3) and s["objects"] == 3


# ---- random inputs -------------------------------------------------------------------------------------------------------------------
def random_run(rng, F, G, K, ties=False, p_valid=0.8, p_present=0.8):
    """random matrices (from a small value set with ties=True), valid masks and ids; an id lives on a column for a few frames,
    then the column goes empty, and retired ids come back on another column after a gap"""
    pick = (lambda m: rng.integers(0, 4, m) / 4.0) if ties else (lambda m: rng.random(m))
    ov = pick(F * G * K).reshape(F, G, K).astype(np.float32)
    di = (4.0 * pick(F * G * K)).reshape(F, G, K).astype(np.float32)
    valid = (rng.random((F, G)) < p_valid).astype(np.int32)
    ids = np.full((F, K), -1, np.int32)
    cur, pool, next_id = np.full((K,), -1), [], 0
    for f in range(F):
        for k in range(K):
            if cur[k] >= 0 and rng.random() < 0.3:
                pool.append(int(cur[k]))
                cur[k] = -1
            elif cur[k] < 0 and rng.random() < p_present:
                if pool and rng.random() < 0.5:
                    cur[k] = pool.pop(int(rng.integers(0, len(pool))))
                else:
                    cur[k], next_id = next_id, next_id + 1
        ids[f] = cur
    return ov, di, valid, ids


def check_invariants(out, ov, di, valid, ids, gates, state=None):
    F, G, K = ov.shape
    state = MOT.new_state(G) if state is None else state
    pf = out["per_frame"]
    assert (pf[:, 2] + pf[:, 4] == pf[:, 0]).all() and (pf[:, 2] + pf[:, 3] == pf[:, 1]).all() and (pf[:, 7] == 0).all()
    assert (pf[:, 0] == (valid != 0).sum(1)).all() and (pf[:, 1] == (ids >= 0).sum(1)).all()
    for f in range(F):
        ok = MOT.admissible(ov[f], di[f], valid[f], ids[f], **gates)
        m = out["match_slot"][f]
        hit = np.flatnonzero(m >= 0)
        assert len(set(m[hit].tolist())) == len(hit) and all(ok[g, m[g]] for g in hit)                 # one-to-one and admissible
        free_g, free_k = m < 0, ~np.isin(np.arange(K), m[hit])
        assert not ok[np.ix_(free_g, free_k)].any()                                                   # no admissible pair is left free
        assert np.array_equal(out["match_id"][f], np.where(m >= 0, ids[f][np.maximum(m, 0)], -1))
        assert np.array_equal(out["match_ov"][f][hit], ov[f][hit, m[hit]]) and np.array_equal(out["match_di"][f][hit], di[f][hit, m[hit]])
        assert (out["match_ov"][f][m < 0] == -1).all() and np.isinf(out["match_di"][f][m < 0]).all()


@pytest.mark.parametrize("F,G,K,ties", [(6, 5, 6, True), (6, 5, 6, False), (4, 12, 9, True), (3, 9, 14, False)])
def test_invariants_and_split_walks_on_random_inputs(F, G, K, ties):
    rng = np.random.default_rng(100 * G + K + ties)
    for gates in (dict(min_iou=0.25, max_dist=3.0), dict(min_iou=0.0, max_dist=INF), dict(min_iou=0.5, max_dist=1.0)):
        ov, di, valid, ids = random_run(rng, F, G, K, ties)
        whole = MOT.walk(ov, di, valid, ids, **gates)
        check_invariants(whole, ov, di, valid, ids, gates)
        for cuts in itertools.chain([(c,) for c in range(F + 1)], [(1, 2), (2, F - 1)]):
            state, parts = None, []
            for lo, hi in zip((0,) + cuts, cuts + (F,)):
                part = MOT.walk(ov[lo:hi], di[lo:hi], valid[lo:hi], ids[lo:hi], state, **gates)
                state = part["state"]
                parts.append(part)
            for name in ("match_slot", "match_id", "match_ov", "match_di", "per_frame", "carried"):
                assert np.array_equal(np.concatenate([p[name] for p in parts]), whole[name]), (cuts, name)
            assert all(np.array_equal(state[k], whole["state"][k]) for k in state), cuts


def test_pair_scores_frames_masks_and_equals_score_pair():
    import metrics_oracle as MO
    rng = np.random.default_rng(3)
    box = lambda x: np.array([x, 0.3 * x, 0, 2, 4, 1.5, 1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)      # noqa: E731
    gt = np.stack([[box(0.0), box(10.0)], [box(0.5), box(10.5)]])
    hyp = gt[:, ::-1] + rng.normal(scale=0.1, size=gt.shape).astype(np.float32) * (np.arange(15) < 3)
    valid, ids = np.array([[1, 1], [0, 1]], np.int32), np.array([[4, -1], [4, 5]], np.int32)
    ov, di = MOT.pair_scores_frames(gt, valid, hyp, ids)
    live = (valid[:, :, None] != 0) & (ids[:, None, :] >= 0)
    assert (ov[~live] == -1).all() and np.isinf(di[~live]).all() and live.sum() == 4
    o, d = MO.score_pair(gt[1, 1], hyp[1, 0])
    assert ov[1, 1, 0] == np.float32(o) > 0.5 and di[1, 1, 0] == np.float32(d)


def test_matched_count_equals_the_optimal_assignment_where_it_is_forced():
    """frames without memory, gates under which every valid object has exactly one admissible column (distinct columns): the
    greedy match and the Hungarian optimum then take the same number of pairs -- all of them"""
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(17)
    for trial in range(10):
        G, K = int(rng.integers(2, 9)), int(rng.integers(9, 14))
        valid = (rng.random((1, G)) < 0.8).astype(np.int32)
        ids = np.arange(K, dtype=np.int32)[None].copy()
        col = rng.permutation(K)[:G]
        ov, di = rng.random((1, G, K)).astype(np.float32) * 0.2, 3.0 + rng.random((1, G, K)).astype(np.float32)
        ov[0, np.arange(G), col], di[0, np.arange(G), col] = 0.5 + 0.5 * rng.random(G), rng.random(G)
        out = MOT.walk(ov, di, valid, ids, min_iou=0.3, max_dist=2.0)
        ok = MOT.admissible(ov[0], di[0], valid[0], ids[0], 0.3, 2.0)
        assert (ok.sum(1) == (valid[0] != 0)).all()
        rows, cols = opt.linear_sum_assignment(np.where(ok, 0.0, 1.0))
        assert int(out["per_frame"][0, 2]) == int(ok[rows, cols].sum()) == int(valid.sum())
