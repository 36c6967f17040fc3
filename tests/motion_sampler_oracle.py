"""numpy restatement of the M2-Track half of open3dsot_amd/csrc/train_batch.hip + the launches sampler.MotionBatchBuilder
makes around it: the augmented crop bit for bit in fp32 (aug_point and inside_box in the operation order written at the head
of train_batch.hip, then tracking_oracle.crop_mask), the per-candidate kernels (o3d_train_augment, o3d_train_motion_labels) in
fp64 rounded once, exact integers for the selection and the index draw (sampler_oracle).  The GPU tests compare the kernels
against this; the CPU tests compare this against the reference's own motion_processing with apply_augmentation
(tests/golden/ref_motion_batches.npz).  Test infrastructure only -- the product has no CPU path.  tools/batch_bench.py uses
`build` as the host sampler a user had to write before the device builder existed."""
import numpy as np

import motion_oracle as MO
import sampler_oracle as SO
import tracking_oracle as TO

f32 = np.float32
AUG_FACTOR = f32(1.25)


def rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def inside_box(points, box15, factor):
    """inside_box of track_common.hpp -> (mask (n,) bool, d (n,3) float32): fp32, one operation per numpy operation"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    b = np.asarray(box15, dtype=f32).reshape(15)
    factor = f32(factor)
    dx, dy, dz = p[:, 0] - b[0], p[:, 1] - b[1], p[:, 2] - b[2]
    w, l, h = b[3], b[4], b[5]
    R = b[6:15]
    qx = (R[0] * dx + R[3] * dy) + R[6] * dz
    qy = (R[1] * dx + R[4] * dy) + R[7] * dz
    qz = (R[2] * dx + R[5] * dy) + R[8] * dz
    mask = (np.abs(qx) <= (l * factor) * f32(0.5)) & (np.abs(qy) <= (w * factor) * f32(0.5)) & (np.abs(qz) <= (h * factor) * f32(0.5))
    return mask, np.stack([dx, dy, dz], 1)


def aug_points(points, rec):
    """aug_point for every row: rec = None | dict(enabled, box (15), A (9), c (3)) float32 -> (n,3) float32"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    if rec is None or not rec["enabled"]:
        return p
    mask, d = inside_box(p, rec["box"], AUG_FACTOR)
    A, c = np.asarray(rec["A"], f32).reshape(9), np.asarray(rec["c"], f32).reshape(3)
    out = p.copy()
    for i in range(3):
        v = ((A[3 * i] * d[:, 0] + A[3 * i + 1] * d[:, 1]) + A[3 * i + 2] * d[:, 2]) + c[i]
        assert v.dtype == f32
        out[mask, i] = v[mask]
    return out


def crop_aug(points, box15, scale, offset, mode, rec=None, capacity=None):
    """one target of o3d_track_crop_groups_aug -> (count, rows): the crop of the augmented points"""
    return TO.crop(aug_points(points, rec), box15, scale, offset, mode, capacity)


def augment(gt15, draw6):
    """o3d_train_augment for one record: fp64 inside, rounded once -> (box (15) float32, rec)"""
    gt = np.asarray(gt15, f32).reshape(15)
    dr = np.asarray(draw6, f32).reshape(6).astype(np.float64)
    R = gt[6:].astype(np.float64).reshape(3, 3)
    M = R @ rz(dr[3] * (np.pi / 180.0))
    fx, fy = (-1.0 if dr[4] != 0 else 1.0), (-1.0 if dr[5] != 0 else 1.0)
    c = (gt[:3].astype(np.float64) + R @ dr[:3]).astype(f32)
    box = np.concatenate([c, gt[3:6], (M @ np.diag([fx, fx, 1.0])).reshape(-1).astype(f32)]).astype(f32)
    A = (M @ np.diag([fx, fy, 1.0]) @ R.T).reshape(-1).astype(f32)
    return box, {"enabled": 1, "box": gt.copy(), "A": A, "c": c}


def augment64(gt15, draw6):
    """the same in fp64 without the final rounding -> (c (3), R' (9), A (9)): what the GPU test measures the rounding against"""
    gt = np.asarray(gt15, f32).reshape(15).astype(np.float64)
    dr = np.asarray(draw6, f32).reshape(6).astype(np.float64)
    R = gt[6:].reshape(3, 3)
    M = R @ rz(dr[3] * (np.pi / 180.0))
    fx, fy = (-1.0 if dr[4] != 0 else 1.0), (-1.0 if dr[5] != 0 else 1.0)
    return gt[:3] + R @ dr[:3], (M @ np.diag([fx, fx, 1.0])).reshape(-1), (M @ np.diag([fx, fy, 1.0]) @ R.T).reshape(-1)


def transform_box64(c, R, cr, Rr):
    return Rr.T @ (c - cr), Rr.T @ R


def motion_labels64(prev_gt, this_gt, ref_box, degrees, motion_threshold):
    """o3d_train_motion_labels for one candidate in fp64, nothing rounded -> dict"""
    p, t, r = (np.asarray(b, f32).reshape(15).astype(np.float64) for b in (prev_gt, this_gt, ref_box))
    c_this, R_this = transform_box64(t[:3], t[6:].reshape(3, 3), r[:3], r[6:].reshape(3, 3))
    c_prev, R_prev = transform_box64(p[:3], p[6:].reshape(3, 3), r[:3], r[6:].reshape(3, 3))
    c_mot, R_mot = transform_box64(c_this, R_this, c_prev, R_prev)

    def label(c, R):
        th = np.arctan2(R[1, 0], R[0, 0])
        return np.concatenate([c, [th * (180.0 / np.pi) if degrees else th]])
    return {"this_box": np.concatenate([c_this, t[3:6], R_this.reshape(-1)]), "prev_box": np.concatenate([c_prev, p[3:6], R_prev.reshape(-1)]),
            "canon_box": np.concatenate([np.zeros(3), p[3:6], np.eye(3).reshape(-1)]),
            "box_label": label(c_this, R_this), "box_label_prev": label(c_prev, R_prev), "motion_label": label(c_mot, R_mot),
            "motion_state_label": int(np.sqrt(((c_this - c_prev) ** 2).sum()) > float(f32(motion_threshold))),
            "motion_distance": float(np.sqrt(((c_this - c_prev) ** 2).sum())), "bbox_size": t[3:6].copy()}


def motion_labels(prev_gt, this_gt, ref_box, degrees, motion_threshold):
    """the same, rounded once as the kernel stores it"""
    out = motion_labels64(prev_gt, this_gt, ref_box, degrees, motion_threshold)
    return {k: (v.astype(f32) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def select(counts, B, caps):
    """o3d_train_select_motion -> (sel (B,) int32, n_valid, overflow)"""
    c = np.asarray(counts, np.int64).reshape(-1, 3)
    valid = np.flatnonzero((c[:, 0] > 10) & (c[:, 2] > 20))
    if valid.size == 0:
        return np.full(B, -1, np.int32), 0, 0
    sel = valid[np.arange(B) % valid.size]
    return sel.astype(np.int32), int(valid.size), int((c[sel][:, 1:] > np.asarray(caps)[None, :]).sum())


def sample(sel, counts, pools, caps, N, prev_box, this_box, canon_box, candidate_id, idx_prev=None, idx_this=None, seed=0, counter=0,
           with_bc=True):
    """o3d_train_motion_sample on the host for arbitrary crop pools.  sel (B,); counts (J,3); pools = (prev (J,cap0,3), this
    (J,cap1,3)); the three box sets (J,15) -> dict of points (B,2N,5), candidate_bc (B,2N,9), seg_label (B,2N) int64,
    used_prev / used_this (B,N) int32"""
    B = len(sel)
    out = {"points": np.zeros((B, 2 * N, 5), f32), "seg_label": np.zeros((B, 2 * N), np.int64),
           "used_prev": np.full((B, N), -1, np.int32), "used_this": np.full((B, N), -1, np.int32)}
    if with_bc:
        out["candidate_bc"] = np.zeros((B, 2 * N, 9), f32)
    for r, j in enumerate(sel):
        if j < 0:
            continue
        xyz = np.zeros((2, N, 3), f32)
        for half, (given, name) in enumerate(((idx_prev, "used_prev"), (idx_this, "used_this"))):
            n = min(int(counts[j][1 + half]), caps[half])
            if n <= 2:
                continue
            src = pools[half][j][:n]
            idx = np.asarray(given[j], np.int64) if given is not None else SO.sample_indices(SO.draw_key(seed, counter, j, half), n, N)
            ok = (idx >= 0) & (idx < n)
            xyz[half][ok] = src[idx[ok]]
            out[name][r][ok] = idx[ok]
        wlh = np.asarray(canon_box[j], f32)[3:6]
        idx = np.concatenate([np.arange(N), np.arange(N)])
        pts, bc = MO.motion_input(xyz[0], xyz[1], idx, N, wlh, int(candidate_id[j]) == 0, with_bc=with_bc)
        out["points"][r] = pts
        if with_bc:
            out["candidate_bc"][r] = bc
        out["seg_label"][r][:N] = inside_box(xyz[0], prev_box[j], AUG_FACTOR)[0]
        out["seg_label"][r][N:] = inside_box(xyz[1], this_box[j], AUG_FACTOR)[0]
    return out


def candidate(frames, boxes, smp, cfg, offset, aug_prev, aug_this, caps, idx_prev=None, idx_this=None, seed=0, counter=0, j=0):
    """Everything the device computes for ONE candidate.  frames: list of (n,3) float32; boxes (T,15) float32; smp = (prev,
    this, candidate_id); cfg: the data keys (open3dsot_amd.sampler.MOTION_DATA_KEYS); offset (3): the jitter; aug_prev /
    aug_this (6) (ignored without use_augmentation) -> dict"""
    f1, f2, cid = smp
    N = cfg["point_sample_size"]
    prev_gt, this_gt, rec_prev, rec_this = np.asarray(boxes[f1], f32), np.asarray(boxes[f2], f32), None, None
    inbox, _ = TO.crop(frames[f1], prev_gt, 1.0, 0.0, TO.SUBWINDOW)
    if cfg["use_augmentation"]:
        prev_gt, rec_prev = augment(prev_gt, aug_prev)
        this_gt, rec_this = augment(this_gt, aug_this)
    ref_box, _ = TO.offset_box(prev_gt, SO.pack_offsets(offset), cfg["degrees"], False, cfg["data_limit_box"])
    c1, crop1 = crop_aug(frames[f1], ref_box, cfg["bb_scale"], cfg["bb_offset"], TO.SUBWINDOW, rec_prev, caps[0])
    c2, crop2 = crop_aug(frames[f2], ref_box, cfg["bb_scale"], cfg["bb_offset"], TO.SUBWINDOW, rec_this, caps[1])
    lab = motion_labels(prev_gt, this_gt, ref_box, cfg["degrees"], cfg["motion_threshold"])
    counts = np.array([inbox, c1, c2], np.int32)
    s = _sample_at(j, counts, (crop1[None], crop2[None]), N, lab, cid, idx_prev, idx_this, seed, counter, cfg["box_aware"])
    out = {"counts": counts, "ref_box": ref_box, "prev_gt": prev_gt, "this_gt": this_gt, "rec_prev": rec_prev, "rec_this": rec_this}
    out.update(lab)
    out.update({k: v[0] for k, v in s.items()})
    out["motion_state_label"] = np.int64(lab["motion_state_label"])
    if cfg["box_aware"]:
        out["prev_bc"] = SO.boxcloud(out["points"][:N, :3], lab["prev_box"])
        out["this_bc"] = SO.boxcloud(out["points"][N:, :3], lab["this_box"])
    return out


def _sample_at(j, counts, pools, N, lab, cid, idx_prev, idx_this, seed, counter, with_bc):
    """`sample` for one candidate that sits at place j of the batch (the key of the device draw holds j)"""
    c = np.zeros((j + 1, 3), np.int32)
    c[j] = counts
    wide = tuple(np.concatenate([np.zeros((j,) + p.shape[1:], f32), p], 0) for p in pools)
    boxes = [np.concatenate([np.zeros((j, 15), f32), lab[k][None]], 0) for k in ("prev_box", "this_box", "canon_box")]
    given = [None if i is None else np.concatenate([np.zeros((j, N), np.int64), np.asarray(i, np.int64)[None]], 0) for i in (idx_prev, idx_this)]
    return sample([j], c, wide, tuple(max(p.shape[1], 1) for p in pools), N, *boxes, [0] * j + [cid], given[0], given[1], seed, counter,
                  with_bc)


BATCH_KEYS = ("points", "candidate_bc", "seg_label", "box_label", "box_label_prev", "motion_label", "motion_state_label", "bbox_size",
              "prev_bc", "this_bc")


def build(tracklets, samples, cfg, B, offset, aug_prev, aug_this, caps, idx_prev=None, idx_this=None, seed=0, counter=0):
    """MotionBatchBuilder.build on the host.  tracklets: {key: (frames, boxes)}; samples: J tuples (key, prev, this,
    candidate_id) -> (the batch dict with n_valid / overflow / sel, the per-candidate dicts)"""
    cands = [candidate(tracklets[s[0]][0], tracklets[s[0]][1], s[1:], cfg, offset[j], None if aug_prev is None else aug_prev[j],
                       None if aug_this is None else aug_this[j], caps, None if idx_prev is None else idx_prev[j],
                       None if idx_this is None else idx_this[j], seed, counter, j)
             for j, s in enumerate(samples)]
    sel, n_valid, overflow = select(np.stack([c["counts"] for c in cands]), B, caps)
    batch = {}
    for k in BATCH_KEYS:
        if k in cands[0]:
            batch[k] = np.stack([np.asarray(cands[j][k]) if j >= 0 else np.zeros_like(np.asarray(cands[0][k])) for j in sel])
    batch.update(sel=sel, n_valid=n_valid, overflow=overflow)
    return batch, cands


THETA_TOL = {False: 2e-6, True: 1.2e-4}      # radians | degrees: three chained float32 roundings of rotation entries + the label's own


def check_against_reference(got, ref, k, cfg):
    """`got` (one sample's outputs) against sample `k` of tests/golden/ref_motion_batches.npz: xyz within 2e-5 m, channels 3
    and 4 and seg_label exact outside near_face, the BoxClouds within 1e-4, label centres within 2e-5, theta within THETA_TOL,
    motion_state_label and bbox_size exact"""
    N2 = got["points"].shape[0]
    near = np.unpackbits(ref[k + "near_face"])[:N2].astype(bool)
    assert near.sum() <= 16
    assert np.abs(got["points"][:, :3] - ref[k + "points"][:, :3]).max() <= 2e-5
    assert np.array_equal(got["points"][~near, 3:], ref[k + "points"][~near, 3:])
    assert np.array_equal(np.asarray(got["seg_label"])[~near], ref[k + "seg_label"][~near])
    tol = THETA_TOL[bool(cfg["degrees"])]
    for name in ("box_label", "box_label_prev", "motion_label"):
        assert np.abs(got[name][:3] - ref[k + name][:3]).max() <= 2e-5, name
        assert abs(float(got[name][3]) - float(ref[k + name][3])) <= tol, (name, got[name][3], ref[k + name][3])
    assert int(got["motion_state_label"]) == int(ref[k + "motion_state_label"])
    assert np.array_equal(np.asarray(got["bbox_size"], f32), ref[k + "bbox_size"].astype(f32))
    if cfg["box_aware"]:
        for name in ("candidate_bc", "prev_bc", "this_bc"):
            assert np.abs(got[name] - ref[k + name]).max() <= 1e-4, name
    else:
        assert k + "prev_bc" not in ref
