"""Python restatement of the optimal assignment of the scene trackers and CLEAR-MOT (optimal_match in csrc/scene.hip;
o3d_scene_assign, o3d_scene_manage_assign, o3d_scene_mot_walk_assign) as pure functions: nothing passed in
is changed.  The costs are quantised in numpy float32 as the kernel does it, everything after that is Python ints.  The frame-level
oracles are scene_manage_oracle.manage and mot_oracle.walk themselves, called with the match swapped.  Test infrastructure only --
the product has no CPU path."""
import contextlib

import numpy as np

import mot_oracle as MOT
import scene_manage_oracle as SO

BIG = 1 << 32
INF = 1 << 62
ASSIGNMENTS = ("greedy", "optimal")
COSTS = ("distance", "overlap")
_GREEDY = SO.greedy_match                                # the walk itself, whatever the name holds later (_matching)


def quantize(ov, di, cost="distance"):
    """the integer cost of every pair -> int64 array in [0, 2^20]; each product is one rounded fp32 multiply (a NaN, never
    admissible, gives an arbitrary number here)"""
    f = np.float32
    with np.errstate(invalid="ignore"):
        if cost == "distance":
            q = np.rint(np.minimum(np.maximum(np.asarray(di, f), f(0)), f(1024)) * f(1024))
        elif cost == "overlap":
            q = np.rint((f(1) - np.minimum(np.maximum(np.asarray(ov, f), f(0)), f(1))) * f(1048576))
        else:
            raise ValueError(cost)
    return np.nan_to_num(q, nan=0.0).astype(np.int64)


def optimal_match(ov, di, ok, cost="distance", rows=None, stats=None):
    """-> (match (R,), col_match (C,)) int32 on the pairs of `ok` (R,C) bool (admissible, both ends free): the most pairs, among
    those the smallest sum of q, and of several such sets the one the written order gives.  Column numbers: real c = c, the
    private `stay unmatched` column of row r = C + r, at cost BIG.  rows: the rows to insert (None: all; a row without a pair
    of `ok` changes nothing either way).  stats (a dict | None) += steps: the columns picked; reassigned: the insertions whose
    path moved an earlier row; evicted: those that left an earlier row unmatched."""
    ok = np.asarray(ok, bool)
    R, C = ok.shape
    q = quantize(ov, di, cost).reshape(R, C).tolist()
    adm = ok.tolist()
    u, v = [0] * R, [0] * C
    col_row, row_col = [-1] * C, [-1] * R
    steps = reassigned = evicted = 0
    for i in (range(R) if rows is None else rows):
        length, dlength = [INF] * C, [INF] * R           # tentative lengths of the real and of the private columns
        way, used = [-1] * C, [False] * C
        r0, j0, l0 = i, -1, 0                             # the current row, the column it was reached from, its length
        while True:
            base = l0 - u[r0]
            for c in range(C):
                if adm[r0][c] and not used[c]:
                    cand = base + q[r0][c] - v[c]
                    if cand < length[c]:
                        length[c], way[c] = cand, j0
            dlength[r0] = base + BIG
            best = min([(length[c], c) for c in range(C) if not used[c] and length[c] < INF]
                       + [(dlength[r], C + r) for r in range(R) if dlength[r] < INF])
            steps += 1
            dend, jend = best
            if jend >= C or col_row[jend] < 0:
                break
            used[jend] = True
            r0, j0, l0 = col_row[jend], jend, dend
        for c in range(C):
            if used[c]:
                v[c] += length[c] - dend
                u[col_row[c]] += dend - length[c]
        u[i] += dend
        c = jend
        if c >= C:                                        # the private column of row t: t stays, or becomes, unmatched
            t = c - C
            c = -1 if t == i else row_col[t]
            row_col[t] = -1
            evicted += t != i
        reassigned += any(used)                           # the path went through a column that a row held
        while c >= 0:
            pc = way[c]
            r = i if pc < 0 else col_row[pc]
            col_row[c], row_col[r] = r, c
            c = pc
    if stats is not None:
        for k, n in (("steps", steps), ("reassigned", reassigned), ("evicted", evicted)):
            stats[k] = stats.get(k, 0) + int(n)
    return np.array(row_col, np.int32).reshape(R), np.array(col_row, np.int32).reshape(C)


def match(ov, di, ok, assignment="optimal", cost="distance", stats=None):
    """the rule `assignment` on the pairs of `ok`"""
    if assignment == "greedy":
        return _GREEDY(ov, di, ok)
    if assignment != "optimal":
        raise ValueError(assignment)
    return optimal_match(ov, di, ok, cost, stats=stats)


def pair_sum(ov, di, match_, cost="distance"):
    """summary of o3d_scene_assign -> (pairs, the sum of q over them), Python ints"""
    q = quantize(ov, di, cost)
    hit = [(r, int(c)) for r, c in enumerate(match_) if c >= 0]
    return len(hit), sum(int(q[r, c]) for r, c in hit)


def assign(ov, di, row_active=None, n_col=None, min_iou=0.0, max_dist=np.inf, assignment="optimal", cost="distance", stats=None):
    """o3d_scene_assign -> (match (K,), col_match (D,), (pairs, sum of q))"""
    ov, di = np.asarray(ov, np.float32), np.asarray(di, np.float32)
    K, D = ov.shape
    act = np.ones((K,), np.int32) if row_active is None else np.asarray(row_active)
    n = D if n_col is None else SO.clamp_n(n_col, D)
    m, c = match(ov, di, SO.admissible(ov, di, act, n, min_iou, max_dist), assignment, cost, stats)
    return m, c, pair_sum(ov, di, m, cost)


@contextlib.contextmanager
def _matching(assignment, cost, stats):
    """scene_manage_oracle.manage and mot_oracle.match_frame look their match up as scene_manage_oracle.greedy_match at call
    time: inside this block that name is the rule asked for, so both oracles run unedited, every other line theirs"""
    keep = SO.greedy_match
    SO.greedy_match = lambda ov, di, ok: match(ov, di, ok, assignment, cost, stats)
    try:
        yield
    finally:
        SO.greedy_match = keep


def manage(state, ov, di, dets, n_det, counts, t, assignment="greedy", cost="distance", stats=None, **kw):
    """scene_manage_oracle.manage with the match made by `assignment` under `cost` (o3d_scene_manage_assign)"""
    with _matching(assignment, cost, stats):
        return SO.manage(state, ov, di, dets, n_det, counts, t, **kw)


def mot_walk(ov, di, gt_valid, hyp_ids, state=None, min_iou=0.0, max_dist=2.0, assignment="greedy", cost="distance", stats=None):
    """mot_oracle.walk with the leftover match made by `assignment` under `cost` (o3d_scene_mot_walk_assign); the carry is its own"""
    with _matching(assignment, cost, stats):
        return MOT.walk(ov, di, gt_valid, hyp_ids, state, min_iou, max_dist)
