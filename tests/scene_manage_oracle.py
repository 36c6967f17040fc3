"""numpy restatement of the scene trackers' device-side lifecycle (o3d_scene_pair_scores in csrc/metrics.hip, o3d_scene_manage in
csrc/scene.hip) as pure functions: nothing passed in is changed.  The greedy match is written as the
contract words it -- sort the admissible pairs, walk them -- where the kernel keeps per-track candidates and never sorts.  Test
infrastructure only -- the product has no CPU path."""
import numpy as np

import metrics_oracle as MO

SLOT_COLS, LANE_COLS = 4, 7            # slot = {id, misses, starved, start}; lane = {active, first, has_crop, t, row, ref_row, rebase}
BANK_FIRST = 0
PARAMS = dict(min_iou=0.0, max_dist=np.inf, max_misses=2, min_points=0, max_starved=0, enroll=1)


def clamp_n(n_det, D):
    return min(max(int(n_det), 0), int(D))


def pair_scores(tracks, active, dets, n_det, dim=3, up=2):
    """step 1 -> (overlaps, distances) (K,D) float32: metrics_oracle.score_pair(a = tracks[k], b = dets[d]) rounded once to
    fp32 for an active k and d < n_det, -1 / +inf elsewhere"""
    tracks, dets = np.asarray(tracks, np.float32).reshape(-1, 15), np.asarray(dets, np.float32).reshape(-1, 15)
    K, D = tracks.shape[0], dets.shape[0]
    n = clamp_n(n_det, D)
    ov, di = np.full((K, D), -1.0, np.float32), np.full((K, D), np.inf, np.float32)
    for k in range(K):
        if not active[k]:
            continue
        for d in range(n):
            o, s = MO.score_pair(tracks[k], dets[d], dim, up)
            ov[k, d], di[k, d] = np.float32(o), np.float32(s)
    return ov, di


def admissible(ov, di, active, n, min_iou, max_dist):
    """step 2 -> (K,D) bool, fp32 compares (a NaN compares false)"""
    ov, di = np.asarray(ov, np.float32), np.asarray(di, np.float32)
    K, D = ov.shape
    with np.errstate(invalid="ignore"):
        ok = (ov >= np.float32(min_iou)) & (di <= np.float32(max_dist))
    ok &= (np.asarray(active).reshape(K, 1) != 0) & (np.arange(D).reshape(1, D) < n)
    return ok


def greedy_match(ov, di, ok):
    """step 3 -> (match (K,), det_match (D,)) int32: the admissible pairs sorted by (overlap descending, distance ascending, k,
    d), walked once"""
    K, D = ok.shape
    pairs = sorted((-float(ov[k, d]), float(di[k, d]), int(k), int(d)) for k, d in zip(*np.nonzero(ok)))
    match, det_match = np.full((K,), -1, np.int32), np.full((D,), -1, np.int32)
    for _, _, k, d in pairs:
        if match[k] < 0 and det_match[d] < 0:
            match[k], det_match[d] = d, k
    return match, det_match


def manage(state, ov, di, dets, n_det, counts, t, has_dets=1, count_col=0, rule=2, **params):
    """steps 2 to 8.  state: dict of cur (K,15), yaw_state (K,10), canon_wlh (K,3), results (T,K,15), active (K,), slot (K,4),
    next_id (1,), bank_state_next (K,2) | None, lanes (K,7), ids_log (T,K), match_log (T,K), dropped_log (T,); counts (K,2).
    rule: the shape_aggregation's number (0 = first), -1 for the motion tracker.  -> (the new state, match, det_match)"""
    p = dict(PARAMS)
    p.update(params)
    s = {k: (None if v is None else np.array(v, copy=True)) for k, v in state.items()}
    K = s["cur"].shape[0]
    dets = np.asarray(dets, np.float32).reshape(-1, 15)
    D, T = dets.shape[0], s["results"].shape[0]
    n = clamp_n(n_det, D) if has_dets else 0
    act_in = s["active"] != 0
    ov, di = np.asarray(ov, np.float32).reshape(K, D), np.asarray(di, np.float32).reshape(K, D)
    match, det_match = greedy_match(ov, di, admissible(ov, di, act_in, n, p["min_iou"], p["max_dist"]))
    ids_in = s["slot"][:, 0].copy()
    for k in range(K):
        if not act_in[k]:
            continue
        _, misses, starved, _ = s["slot"][k]
        if has_dets:
            misses = 0 if match[k] >= 0 else misses + 1
        if p["min_points"] > 0:
            starved = starved + 1 if counts[k][count_col] < p["min_points"] else 0
        s["slot"][k, 1:3] = misses, starved
        if misses > p["max_misses"] or (p["min_points"] > 0 and starved > p["max_starved"]):
            s["active"][k], s["slot"][k, 0] = 0, -1
    first, dropped = np.zeros((K,), bool), 0
    if p["enroll"]:
        free = [k for k in range(K) if not s["active"][k]]
        for d in range(n):
            if det_match[d] >= 0 or not np.isfinite(dets[d]).all():
                continue
            if not free:
                dropped += 1
                continue
            k = free.pop(0)
            s["cur"][k] = dets[d]
            s["yaw_state"][k, :9], s["yaw_state"][k, 9] = dets[d, 6:15], 0.0
            s["canon_wlh"][k] = dets[d, 3:6]
            if 0 <= t < T:
                s["results"][t, k] = dets[d]
            if s["bank_state_next"] is not None:
                s["bank_state_next"][k] = 0
            s["active"][k] = 1
            s["slot"][k] = int(s["next_id"][0]), 0, 0, t
            s["next_id"][0] += 1
            first[k] = True
    s["lanes"][:] = lane_rows(K, first, rule)
    if 0 <= t < T:
        s["ids_log"][t] = np.where(first, s["slot"][:, 0], ids_in)
        s["match_log"][t] = match
        s["dropped_log"][t] = dropped
    return s, match, det_match


def lane_rows(K, first, rule):
    """step 7: tracking.scene_lane_rows with has_crop = first || rule != first"""
    rows = np.zeros((K, LANE_COLS), np.int32)
    rows[:, 0] = 1
    rows[:, 1] = first
    rows[:, 2] = np.asarray(first, bool) | (rule != BANK_FIRST)
    rows[:, 4] = rows[:, 5] = -1
    return rows


def step(state, dets, n_det, counts, t, dim=3, up=2, **kw):
    """steps 1 to 8 on `state` -> manage()'s result"""
    ov, di = pair_scores(state["cur"], state["active"], dets, n_det, dim, up)
    return manage(state, ov, di, dets, n_det, counts, t, **kw)


def new_state(K, T, boxes0, matching=True):
    """the state after init(points0, boxes0) with n0 = len(boxes0) <= K boxes"""
    boxes0 = np.asarray(boxes0, np.float32).reshape(-1, 15)
    n0 = boxes0.shape[0]
    unit = np.zeros((15,), np.float32)
    unit[3:6], unit[[6, 10, 14]] = 1.0, 1.0
    cur = np.tile(unit, (K, 1))
    cur[:n0] = boxes0
    s = dict(cur=cur, yaw_state=np.concatenate([cur[:, 6:15], np.zeros((K, 1), np.float32)], 1), canon_wlh=cur[:, 3:6].copy(),
             results=np.zeros((T, K, 15), np.float32), active=(np.arange(K) < n0).astype(np.int32),
             slot=np.zeros((K, SLOT_COLS), np.int32), next_id=np.array([n0], np.int32),
             bank_state_next=np.zeros((K, 2), np.int32) if matching else None, lanes=np.zeros((K, LANE_COLS), np.int32),
             ids_log=np.full((T, K), -1, np.int32), match_log=np.full((T, K), -1, np.int32), dropped_log=np.zeros((T,), np.int32))
    s["results"][0] = cur
    s["slot"][:, 0] = np.where(np.arange(K) < n0, np.arange(K), -1)
    s["ids_log"][0] = s["slot"][:, 0]
    return s
