"""o3d_scene_pair_scores_frames (csrc/metrics.hip) and o3d_scene_mot_walk (csrc/scene.hip) through the C ABI, per call, against
the numpy restatement tests/mot_oracle.py: every output array and every state array equal (the floats
are copies, so in bits)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mot_oracle as MOT  # noqa: E402
import scene_manage_oracle as SO  # noqa: E402
import test_mot_oracle_cpu as MC  # noqa: E402  (random_run, check_invariants, matrices)
import test_scene_manage_kernels_gpu as SK  # noqa: E402  (bits, box, scene, to_camera)

pytestmark = pytest.mark.gpu
bits = SK.bits
ROWS = ("match_slot", "match_id", "match_ov", "match_di", "per_frame")
STATE = ("last_id", "tracked_prev", "ever")
SHAPES = [(1, 1, 1), (3, 5, 6), (4, 65, 70), (2, 130, 3), (2, 3, 130)]
GATES = (dict(min_iou=0.25, max_dist=3.0), dict(min_iou=0.0, max_dist=np.inf), dict(min_iou=0.5, max_dist=1.0))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def up(a, dev, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def device_walk(dev, ov, di, valid, ids, state=None, **gates):
    """one o3d_scene_mot_walk launch on uploads -> the five row arrays and the new state, read back"""
    from open3dsot_amd import points_utils as PU
    F, G, K = ov.shape
    state = MOT.new_state(G) if state is None else state
    s = [up(state[n], dev, np.int32) for n in STATE]
    p = dict(MOT.GATES)
    p.update(gates)
    # sentinels: the call must write every row
    out = (torch.full((F, G), -7, dtype=torch.int32, device=dev), torch.full((F, G), -7, dtype=torch.int32, device=dev),
           torch.full((F, G), 9.0, device=dev), torch.full((F, G), 9.0, device=dev), torch.full((F, 8), -7, dtype=torch.int32, device=dev))
    PU.scene_mot_walk(up(ov, dev, np.float32), up(di, dev, np.float32), up(valid, dev, np.int32), up(ids, dev, np.int32), *s, out=out, **p)
    got = {n: o.cpu().numpy() for n, o in zip(ROWS, out)}
    got["state"] = {n: t.cpu().numpy() for n, t in zip(STATE, s)}
    return got


def assert_walk(dev, ov, di, valid, ids, what, state=None, **gates):
    got = device_walk(dev, ov, di, valid, ids, state, **gates)
    p = dict(MOT.GATES)
    p.update(gates)
    want = MOT.walk(ov, di, valid, ids, state, **p)
    for n in ROWS:
        assert got[n].dtype == want[n].dtype and np.array_equal(bits(got[n]), bits(want[n])), (what, n)
    for n in STATE:
        assert got["state"][n].dtype == np.int32 and np.array_equal(got["state"][n], want["state"][n]), (what, n)
    return got, want


def random_state(rng, G, ids):
    """a mid-sequence state: remembered ids drawn from those of the run (some shared by two objects), any flags"""
    pool = np.unique(ids[ids >= 0])
    last = rng.choice(pool, G) if len(pool) else np.full((G,), -1)
    last = np.where(rng.random(G) < 0.3, -1, last).astype(np.int32)
    ever = (last >= 0).astype(np.int32)
    return dict(last_id=last, tracked_prev=(ever & (rng.random(G) < 0.5)).astype(np.int32), ever=ever)


def later_round(ov, di, valid, ids, state, want, gates):
    """the leftover matches of frame 0 that were not the first free admissible pair of their row: they needed a later round"""
    ok = MOT.admissible(ov[0], di[0], valid[0], ids[0], **gates)
    m, carried = want["match_slot"][0], want["carried"][0]
    free_cols = ~np.isin(np.arange(ov.shape[2]), m[carried])
    n = 0
    for g in np.flatnonzero((m >= 0) & ~carried):
        row = [(-ov[0, g, k], di[0, g, k], k) for k in np.flatnonzero(ok[g] & free_cols)]
        n += min(row)[2] != m[g]
    return n


def random_cases(F, G, K):
    """six runs per shape: exact ties or continuous scores x the three gates; odd trials start from a mid-sequence state.  The
    seed is one for which the oracle alone satisfies not_vacuous at every shape"""
    rng = np.random.default_rng(7005 + 100 * G + K)
    for trial in range(6):
        ov, di, valid, ids = MC.random_run(rng, F, G, K, ties=trial % 2 == 0)
        state = random_state(rng, G, ids) if trial % 2 else None
        yield trial, ov, di, valid, ids, state, GATES[trial % 3]


def tally(F, G, K, run):
    seen = dict(carried=0, later=0, idsw=0, frag=0, tp=0, fp=0, fn=0)
    for trial, ov, di, valid, ids, state, gates in random_cases(F, G, K):
        want = run(trial, ov, di, valid, ids, state, gates)
        seen["carried"] += int(want["carried"].sum())
        seen["later"] += later_round(ov, di, valid, ids, state, want, gates)
        for n, c in (("tp", 2), ("fp", 3), ("fn", 4), ("idsw", 5), ("frag", 6)):
            seen[n] += int(want["per_frame"][:, c].sum())
    return seen


def not_vacuous(seen, F, G, K):
    """carried matches, identity switches and fragmentations occur; with 5 or more on both sides, so does a leftover match that
    needed a later round"""
    if G * K == 1:
        return seen["tp"] > 0
    return all(seen[n] > 0 for n in ("carried", "idsw", "frag", "tp")) and (seen["later"] > 0 or min(G, K) < 5)


# ---- o3d_scene_mot_walk on random matrices --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,G,K", SHAPES)
def test_walk_on_random_matrices_equals_the_oracle(dev, F, G, K):
    def run(trial, ov, di, valid, ids, state, gates):
        got, want = assert_walk(dev, ov, di, valid, ids, (F, G, K, trial), state, **gates)
        MC.check_invariants(got, ov, di, valid, ids, gates)
        return want
    seen = tally(F, G, K, run)
    print("(F,G,K) = (%d,%d,%d): %s" % (F, G, K, seen))
    assert not_vacuous(seen, F, G, K), seen


def test_walk_split_over_two_calls_and_repeated(dev):
    F, G, K = 4, 65, 70
    for trial, ov, di, valid, ids, state, gates in random_cases(F, G, K):
        whole = device_walk(dev, ov, di, valid, ids, state, **gates)
        again = device_walk(dev, ov, di, valid, ids, state, **gates)
        head = device_walk(dev, ov[:1], di[:1], valid[:1], ids[:1], state, **gates)
        tail = device_walk(dev, ov[1:], di[1:], valid[1:], ids[1:], head["state"], **gates)
        for n in ROWS:
            assert np.array_equal(bits(again[n]), bits(whole[n])), (trial, n)
            assert np.array_equal(bits(np.concatenate([head[n], tail[n]])), bits(whole[n])), (trial, n)
        for n in STATE:
            assert np.array_equal(again["state"][n], whole["state"][n]) and np.array_equal(tail["state"][n], whole["state"][n]), (trial, n)


# ---- o3d_scene_mot_walk on written-out matrices ---------------------------------------------------------------------------------------
def test_walk_keeps_an_identity_against_a_better_pair_until_it_is_inadmissible(dev):
    pairs = {(0, 0, 0): (0.9, 0.1), (0, 0, 1): (0.0, 1.9), (1, 0, 0): (0.1, 1.5), (1, 0, 1): (0.9, 0.1),
             (2, 0, 0): (0.0, 2.5), (2, 0, 1): (0.9, 0.1)}
    ov, di = MC.matrices(3, 1, 2, pairs)
    got, _ = assert_walk(dev, ov, di, np.ones((3, 1), np.int32), np.array([[1, 2]] * 3, np.int32), "carry")
    assert got["match_id"][:, 0].tolist() == [1, 1, 2] and got["per_frame"][:, 5].tolist() == [0, 0, 1]
    assert got["match_ov"][1, 0] == np.float32(0.1) and got["match_di"][1, 0] == np.float32(1.5)


def test_walk_gives_a_shared_memory_of_one_id_to_the_lower_object(dev):
    state = dict(last_id=np.array([7, 7], np.int32), tracked_prev=np.ones(2, np.int32), ever=np.ones(2, np.int32))
    ov, di = MC.matrices(1, 2, 2, {(0, 0, 0): (0.2, 1.0), (0, 1, 0): (0.9, 0.1), (0, 0, 1): (0.5, 0.5), (0, 1, 1): (0.1, 1.5)})
    valid, ids = np.ones((1, 2), np.int32), np.array([[7, 8]], np.int32)
    got, _ = assert_walk(dev, ov, di, valid, ids, "shared", state)
    assert got["match_slot"].tolist() == [[0, 1]] and got["per_frame"][0].tolist() == [2, 2, 2, 0, 0, 1, 0, 0]
    ov[0, 0, 0], di[0, 0, 0] = 0.0, 9.0
    got, _ = assert_walk(dev, ov, di, valid, ids, "shared, object 0 out of reach", state)
    assert got["match_slot"].tolist() == [[1, 0]] and got["state"]["last_id"].tolist() == [8, 7]
    # the precondition broken: id 7 on both columns -> the lowest column is the one the carry looks at
    got, want = assert_walk(dev, ov, di, valid, np.array([[7, 7]], np.int32), "one id twice", state)
    assert want["carried"].tolist() == [[False, True]] and got["match_slot"].tolist() == [[1, 0]]


def test_walk_through_an_all_invalid_frame_and_a_frame_without_ids(dev):
    rng = np.random.default_rng(5)
    ov, di, valid, ids = MC.random_run(rng, 5, 9, 7, p_valid=0.9, p_present=0.9)
    valid[1], ids[3] = 0, -1
    got, want = assert_walk(dev, ov, di, valid, ids, "gaps", min_iou=0.0, max_dist=np.inf)
    assert got["per_frame"][1].tolist() == [0, int((ids[1] >= 0).sum()), 0, int((ids[1] >= 0).sum()), 0, 0, 0, 0]
    assert got["per_frame"][3].tolist() == [int(valid[3].sum()), 0, 0, 0, int(valid[3].sum()), 0, 0, 0]
    assert (got["match_slot"][[1, 3]] == -1).all() and want["carried"][2].any() and got["per_frame"][4, 6] > 0


# ---- o3d_scene_pair_scores_frames ----------------------------------------------------------------------------------------------------
def frames_scene(F, G, K):
    """F frames of G ground-truth boxes and K hypothesis boxes (jittered copies of ground-truth boxes, or boxes far away), a
    random valid mask and ids with empty columns"""
    rng = np.random.default_rng(50 * G + K)
    gt, hyp = [], []
    for f in range(F):
        a, b = SK.scene(rng, G, K, min(K, 2) - 1)
        gt.append(a)
        hyp.append(b)
    valid = (rng.random((F, G)) < 0.8).astype(np.int32)
    ids = np.where(rng.random((F, K)) < 0.8, np.arange(K)[None, :] + 100, -1).astype(np.int32)
    if G * K == 1:
        valid[:], ids[:] = 1, 100
    return np.stack(gt), valid, np.stack(hyp), ids


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("F,G,K", SHAPES)
def test_pair_scores_frames_equal_the_frame_entry_score_boxes_and_the_oracle(dev, F, G, K, dim):
    from open3dsot_amd import metrics, points_utils as PU
    gt, valid, hyp, ids = frames_scene(F, G, K)
    u = 2 if G != 5 else 1                                 # one case in the camera frame
    if u == 1:
        gt, hyp = SK.to_camera(gt).reshape(F, G, 15), SK.to_camera(hyp).reshape(F, K, 15)
    g_dev, h_dev, v_dev, i_dev = up(gt, dev, np.float32), up(hyp, dev, np.float32), up(valid, dev, np.int32), up(ids, dev, np.int32)
    ov, di = PU.scene_pair_scores_frames(g_dev, v_dev, h_dev, i_dev, dim, u)
    assert ov.shape == (F, G, K) and ov.dtype == torch.float32 and di.shape == (F, G, K)
    live = torch.from_numpy((valid[:, :, None] != 0) & (ids[:, None, :] >= 0)).to(dev)
    assert bool((ov[~live] == -1).all()) and bool(torch.isinf(di[~live]).all()) and bool((di[~live] > 0).all())
    # o3d_track_score on the expanded pairs
    a = g_dev[:, :, None, :].expand(F, G, K, 15).contiguous()
    b = h_dev[:, None, :, :].expand(F, G, K, 15).contiguous()
    so, sd = metrics.score_boxes(a, b, dim, (0, 0, 1) if u == 2 else (0, -1, 0))
    assert torch.equal(ov[live].view(torch.int32), so[live].view(torch.int32))
    assert torch.equal(di[live].view(torch.int32), sd[live].view(torch.int32))
    # o3d_scene_pair_scores frame by frame: rows = the objects, columns = the K boxes
    n_all = torch.tensor([K], dtype=torch.int32, device=dev)
    for f in range(F):
        fo, fd = PU.scene_pair_scores(g_dev[f], v_dev[f], h_dev[f], n_all, dim, u)
        assert torch.equal(ov[f][live[f]].view(torch.int32), fo[live[f]].view(torch.int32)), f
        assert torch.equal(di[f][live[f]].view(torch.int32), fd[live[f]].view(torch.int32)), f
    want_ov, want_di = MOT.pair_scores_frames(gt, valid, hyp, ids, dim, u)
    assert np.array_equal(bits(ov.cpu().numpy()), bits(want_ov)) and np.array_equal(bits(di.cpu().numpy()), bits(want_di))
    if G * K > 1:
        assert 0 < float(ov[live].max()) < 1 and int((ov[live] > 0).sum()) >= 1                # real overlaps, not all 0


def test_both_launches_on_boxes_with_nan(dev):
    """a NaN in a box: overlap 0 and a NaN distance by the arithmetic, which no gate admits -- the object is missed, the
    hypothesis is a false positive, and nothing else moves"""
    from open3dsot_amd import points_utils as PU
    gt, valid, hyp, ids = frames_scene(3, 5, 6)
    valid[:], ids[:] = 1, np.arange(6) + 100
    hyp[:, :5] = gt                                        # every object has an exact copy: matched on column g
    hyp[1, 2, 0] = np.nan
    gt[2, 4, 0] = np.nan
    ov, di = PU.scene_pair_scores_frames(up(gt, dev, np.float32), up(valid, dev, np.int32), up(hyp, dev, np.float32), up(ids, dev, np.int32))
    ov, di = ov.cpu().numpy(), di.cpu().numpy()
    want_ov, want_di = MOT.pair_scores_frames(gt, valid, hyp, ids)
    assert np.array_equal(bits(ov), bits(want_ov)) and np.array_equal(np.isnan(di), np.isnan(want_di))
    assert np.array_equal(bits(di[~np.isnan(di)]), bits(want_di[~np.isnan(di)]))
    assert np.isnan(di[1, :, 2]).all() and np.isnan(di[2, 4, :]).all() and (ov[1, :, 2] == 0).all()
    got, _ = assert_walk(dev, ov, di, valid, ids, "nan", min_iou=0.0, max_dist=3.0)
    assert got["match_slot"].tolist() == [[0, 1, 2, 3, 4], [0, 1, -1, 3, 4], [0, 1, 2, 3, -1]]
    assert got["per_frame"][:, 2:7].tolist() == [[5, 1, 0, 0, 0], [4, 2, 1, 0, 0], [4, 2, 1, 0, 1]]
