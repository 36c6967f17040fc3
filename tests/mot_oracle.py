"""numpy restatement of the CLEAR-MOT bookkeeping of a managed scene (o3d_scene_pair_scores_frames in csrc/metrics.hip,
o3d_scene_mot_walk in csrc/scene.hip, metrics.ClearMOT) as pure functions: nothing passed in is changed.
The leftover match is scene_manage_oracle.greedy_match -- sort the admissible pairs, walk them -- where the kernel keeps
per-row candidates and never sorts.  Test infrastructure only -- the product has no CPU path."""
import numpy as np

import metrics_oracle as MO
import scene_manage_oracle as SO

FRAME_COLS = ("gt", "hyp", "tp", "fp", "fn", "idsw", "frag")
GATES = dict(min_iou=0.0, max_dist=2.0)


def pair_scores_frames(gt, gt_valid, hyp, hyp_ids, dim=3, up=2):
    """-> (overlaps, distances) (F,G,K) float32: metrics_oracle.score_pair(a = gt[f,g], b = hyp[f,k]) rounded once to fp32 where
    gt_valid[f,g] != 0 and hyp_ids[f,k] >= 0, -1 / +inf elsewhere"""
    gt, hyp = np.asarray(gt, np.float32), np.asarray(hyp, np.float32)
    F, G, K = gt.shape[0], gt.shape[1], hyp.shape[1]
    ov, di = np.full((F, G, K), -1.0, np.float32), np.full((F, G, K), np.inf, np.float32)
    for f in range(F):
        for g in range(G):
            if not gt_valid[f][g]:
                continue
            for k in range(K):
                if hyp_ids[f][k] >= 0:
                    o, s = MO.score_pair(gt[f, g], hyp[f, k], dim, up)
                    ov[f, g, k], di[f, g, k] = np.float32(o), np.float32(s)
    return ov, di


def new_state(G):
    """last_id, tracked_prev, ever before the first frame"""
    return dict(last_id=np.full((G,), -1, np.int32), tracked_prev=np.zeros((G,), np.int32), ever=np.zeros((G,), np.int32))


def admissible(ov, di, valid, ids, min_iou, max_dist):
    """one frame -> (G,K) bool, fp32 compares (a NaN compares false)"""
    ov, di = np.asarray(ov, np.float32), np.asarray(di, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (ov >= np.float32(min_iou)) & (di <= np.float32(max_dist))
    return ok & (np.asarray(valid).reshape(-1, 1) != 0) & (np.asarray(ids).reshape(1, -1) >= 0)


def match_frame(ov, di, valid, ids, last_id, min_iou, max_dist):
    """carry, then the greedy walk over what is left -> (match (G,), col_match (K,), carried (G,) bool)"""
    G, K = ov.shape
    ok = admissible(ov, di, valid, ids, min_iou, max_dist)
    match, col = np.full((G,), -1, np.int32), np.full((K,), -1, np.int32)
    for g in range(G):
        if valid[g] and last_id[g] >= 0:
            ks = np.flatnonzero(np.asarray(ids) == last_id[g])
            if len(ks) and ok[g, ks[0]] and col[ks[0]] < 0:
                match[g], col[ks[0]] = ks[0], g
    carried = match >= 0
    free = ok & (match < 0)[:, None] & (col < 0)[None, :]
    m2, c2 = SO.greedy_match(ov, di, free)
    return np.where(carried, match, m2).astype(np.int32), np.where(col >= 0, col, c2).astype(np.int32), carried


def walk(ov, di, gt_valid, hyp_ids, state=None, min_iou=0.0, max_dist=2.0):
    """the F frames of ov, di (F,G,K) in order from `state` (None: new_state) -> dict of match_slot, match_id (F,G) int32,
    match_ov, match_di (F,G) float32, per_frame (F,8) int32, carried (F,G) bool (which matches the carry made: not an output of
    the kernel), state (the new one)"""
    ov, di = np.asarray(ov, np.float32), np.asarray(di, np.float32)
    F, G, K = ov.shape
    gt_valid, hyp_ids = np.asarray(gt_valid).reshape(F, G), np.asarray(hyp_ids).reshape(F, K)
    s = {k: np.array(v, np.int32) for k, v in (state if state is not None else new_state(G)).items()}
    out = dict(match_slot=np.full((F, G), -1, np.int32), match_id=np.full((F, G), -1, np.int32),
               match_ov=np.full((F, G), -1.0, np.float32), match_di=np.full((F, G), np.inf, np.float32),
               per_frame=np.zeros((F, 8), np.int32), carried=np.zeros((F, G), bool))
    for f in range(F):
        valid, ids = gt_valid[f] != 0, hyp_ids[f]
        match, col, out["carried"][f] = match_frame(ov[f], di[f], valid, ids, s["last_id"], min_iou, max_dist)
        tp = fn = idsw = frag = 0
        for g in range(G):
            if not valid[g]:
                continue
            k = match[g]
            if k >= 0:
                tp += 1
                idsw += int(s["last_id"][g] >= 0 and s["last_id"][g] != ids[k])
                frag += int(s["ever"][g] != 0 and s["tracked_prev"][g] == 0)
                s["last_id"][g], s["ever"][g], s["tracked_prev"][g] = ids[k], 1, 1
                out["match_slot"][f, g], out["match_id"][f, g] = k, ids[k]
                out["match_ov"][f, g], out["match_di"][f, g] = ov[f, g, k], di[f, g, k]
            else:
                fn += 1
                s["tracked_prev"][g] = 0
        present = ids >= 0
        out["per_frame"][f] = int(valid.sum()), int(present.sum()), tp, int((present & (col < 0)).sum()), fn, idsw, frag, 0
    out["state"] = s
    return out


def summary(per_frame, match_slot, match_ov, match_di, gt_valid):
    """what metrics.ClearMOT.compute() returns, from the rows of walk() over a whole sequence"""
    per_frame, gt_valid = np.asarray(per_frame, np.int64), np.asarray(gt_valid) != 0
    tot = dict(zip(FRAME_COLS, per_frame[:, :7].sum(0).tolist()))
    hit = np.asarray(match_slot) >= 0
    ratio = lambda a, b: float(a) / float(b) if b else 0.0      # noqa: E731
    n_valid, n_hit = gt_valid.sum(0), hit.sum(0)
    seen = n_valid > 0
    res = dict(frames=int(per_frame.shape[0]), **tot)
    res["mota"] = 1.0 - ratio(tot["fn"] + tot["fp"] + tot["idsw"], tot["gt"]) if tot["gt"] else 0.0
    res["motp_dist"] = ratio(np.asarray(match_di, np.float64)[hit].sum(), tot["tp"])
    res["motp_iou"] = ratio(np.asarray(match_ov, np.float64)[hit].sum(), tot["tp"])
    res["recall"], res["precision"] = ratio(tot["tp"], tot["gt"]), ratio(tot["tp"], tot["hyp"])
    res["objects"] = int(seen.sum())
    res["mostly_tracked"] = ratio((seen & (5 * n_hit >= 4 * n_valid)).sum(), seen.sum())
    res["mostly_lost"] = ratio((seen & (5 * n_hit <= n_valid)).sum(), seen.sum())
    return res
