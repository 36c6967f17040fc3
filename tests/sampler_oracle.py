"""numpy restatement of open3dsot_amd/csrc/train_batch.hip + the launches open3dsot_amd/sampler.py makes around it: fp32 in
the kernels' fixed operation order for everything they compute in fp32 (the crops and seg_label through
tracking_oracle.crop_mask), double rounded once where the kernels do that (the boxes), exact integer arithmetic for the index
draw and the selection.  The GPU tests compare the kernels against this; the CPU tests compare this against the reference's
own siamese_processing (tests/golden/ref_train_batches.npz).  Test infrastructure only -- the product has no CPU path.
tools/batch_bench.py uses `build` as the host sampler a user had to write before the device builder existed: it is a port of
the reference's sampler, not the reference."""
import numpy as np

import tracking_oracle as TO

f32 = np.float32
M32 = 0xFFFFFFFF


def mix32(x):
    """the MurmurHash3 finaliser on uint32 values held in uint64 arrays"""
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def draw_key(seed, counter, j, cloud):
    a = (int(seed) * 0x9E3779B1) & M32
    b = (int(counter) * 0x85EBCA77 + int(j) * 0xC2B2AE3D + int(cloud) * 0x27D4EB2F + 0x165667B1) & M32
    return int(mix32(a ^ b))


def sample_indices(key, n, S):
    """the draw of train_batch.hip for a cloud of n rows resampled to S rows -> (S,) int64, or None when n <= 2"""
    if n <= 2:
        return None
    i = np.arange(S, dtype=np.uint64)
    if n == S:
        return i.astype(np.int64)
    key = np.uint64(key)
    if S > n:
        return ((mix32(key ^ ((i * 0x9E3779B1 + 0x85EBCA77) & M32)) * np.uint64(n)) >> 32).astype(np.int64)
    b = int(n - 1).bit_length()
    h = (b + 1) // 2
    mask = np.uint64((1 << h) - 1)

    def E(x):
        L, R = x >> np.uint64(h), x & mask
        for rnd in range(4):
            f = mix32(key ^ ((R * 0x9E3779B1 + rnd * 0x85EBCA77 + 0xC2B2AE3D) & M32)) & mask
            L, R = R, L ^ f
        return (L << np.uint64(h)) | R
    x = E(i)
    steps = 1
    while True:
        walk = x >= n
        if not walk.any():
            break
        x[walk] = E(x[walk])
        steps += 1
        assert steps <= (1 << (2 * h)), "the cycle walk is bounded by the domain"
    return x.astype(np.int64)


def select(counts, B, caps):
    """o3d_train_select -> (sel (B,) int32, n_valid, overflow)"""
    c = np.asarray(counts, np.int64).reshape(-1, 3)
    valid = np.flatnonzero((c[:, 0] + c[:, 1] > 20) & (c[:, 2] > 20))
    if valid.size == 0:
        return np.full(B, -1, np.int32), 0, 0
    sel = valid[np.arange(B) % valid.size]
    return sel.astype(np.int32), int(valid.size), int((c[sel] > np.asarray(caps)[None, :]).sum())


def labels(gt_search, sample_bb, template_bb, offset_s4):
    """o3d_train_labels for one candidate -> (search_box (15), box_label (4), bbox_size (3), model_box (15)) float32"""
    gt, sb = np.asarray(gt_search, f32).astype(np.float64), np.asarray(sample_bb, f32).astype(np.float64)
    Rs, R = sb[6:].reshape(3, 3), gt[6:].reshape(3, 3)
    d = gt[:3] - sb[:3]
    c = np.array([(Rs[0, r] * d[0] + Rs[1, r] * d[1]) + Rs[2, r] * d[2] for r in range(3)])
    rot = np.array([[(Rs[0, r] * R[0, k] + Rs[1, r] * R[1, k]) + Rs[2, r] * R[2, k] for k in range(3)] for r in range(3)])
    search_box = np.concatenate([c, gt[3:6], rot.reshape(-1)]).astype(f32)
    box_label = np.array([search_box[0], search_box[1], search_box[2], -f32(offset_s4[3])], f32)
    model_box = np.concatenate([np.zeros(3), np.asarray(template_bb, f32)[3:6], np.eye(3).reshape(-1)]).astype(f32)
    return search_box, box_label, search_box[3:6].copy(), model_box


def boxcloud(points, box15):
    """get_point_to_box_distance of (n,3) points against a (15) box: fp64, rounded once -> (n,9) float32"""
    from open3dsot_amd import synth
    b = np.asarray(box15, np.float64)
    return synth.boxcloud(np.asarray(points, f32), b[:3], b[6:].reshape(3, 3), b[3:6])


def pack_offsets(off3):
    """a 3-vector jitter (x, y, angle) -> the (x, y, 0, theta) row that o3d_track_offset_box_multi takes, float32"""
    o = np.asarray(off3, np.float64)
    return np.array([o[0], o[1], 0.0, o[2]], f32)


def candidate(frames, boxes, sample, cfg, off_t, off_s, caps, idx_t=None, idx_s=None, seed=0, counter=0, j=0):
    """Everything the device computes for ONE candidate.  frames: list of (n,3) float32; boxes (T,15) float32; sample =
    (first, template, search, candidate_id); cfg: the data keys (open3dsot_amd.sampler.DATA_KEYS); off_t / off_s: the two
    jitters (3).  idx_t / idx_s None: the device draw keyed by (seed, counter, j).  -> dict"""
    f0, f1, f2 = sample[:3]
    M, N = cfg["template_size"], cfg["search_size"]
    o_t, o_s = pack_offsets(off_t), pack_offsets(off_s)
    template_bb, _ = TO.offset_box(boxes[f1], o_t, cfg["degrees"], False, cfg["data_limit_box"])
    sample_bb, _ = TO.offset_box(boxes[f2], o_s, cfg["degrees"], False, cfg["data_limit_box"])
    c0, crop0 = TO.crop(frames[f0], boxes[f0], cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL, caps[0])
    c1, crop1 = TO.crop(frames[f1], template_bb, cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL, caps[1])
    c2, crop2 = TO.crop(frames[f2], sample_bb, cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW, caps[2])
    search_box, box_label, bbox_size, model_box = labels(boxes[f2], sample_bb, template_bb, o_s)
    model = np.concatenate([crop0, crop1], 0)
    out = {"counts": np.array([c0, c1, c2], np.int32), "box_label": box_label, "bbox_size": bbox_size, "search_box": search_box,
           "model_box": model_box, "template_bb": template_bb, "sample_bb": sample_bb}
    for name, cloud, src, S, given in (("template", 0, model, M, idx_t), ("search", 1, crop2, N, idx_s)):
        n = src.shape[0]
        idx = None
        if n > 2:
            idx = np.asarray(given, np.int64) if given is not None else sample_indices(draw_key(seed, counter, j, cloud), n, S)
        pts = np.zeros((S, 3), f32)
        used = np.full(S, -1, np.int64)
        if idx is not None:
            ok = (idx >= 0) & (idx < n)
            pts[ok] = src[idx[ok]]
            used[ok] = idx[ok]
        out[name + "_points"], out["used_" + name[0]] = pts, used.astype(np.int32)
    keep, _ = TO.crop_mask(out["search_points"], search_box, 1.0, 0.0, TO.SUBWINDOW)
    out["seg_label"] = (keep & (out["used_s"] >= 0)).astype(f32)
    if cfg["box_aware"]:
        out["points2cc_dist_t"] = boxcloud(out["template_points"], model_box)
        out["points2cc_dist_s"] = boxcloud(out["search_points"], search_box)
    return out


BATCH_KEYS = ("template_points", "search_points", "box_label", "bbox_size", "seg_label", "points2cc_dist_t", "points2cc_dist_s")


def build(tracklets, samples, cfg, B, off_t, off_s, caps, idx_t=None, idx_s=None, seed=0, counter=0):
    """SiameseBatchBuilder.build on the host.  tracklets: {key: (frames, boxes)}; samples: J tuples (key, first, template,
    search, candidate_id) -> (the batch dict with n_valid / overflow / sel, the per-candidate dicts)"""
    cands = [candidate(tracklets[s[0]][0], tracklets[s[0]][1], s[1:], cfg, off_t[j], off_s[j], caps,
                       None if idx_t is None else idx_t[j], None if idx_s is None else idx_s[j], seed, counter, j)
             for j, s in enumerate(samples)]
    sel, n_valid, overflow = select(np.stack([c["counts"] for c in cands]), B, caps)
    batch = {}
    for k in BATCH_KEYS:
        if k in cands[0]:
            batch[k] = np.stack([cands[j][k] if j >= 0 else np.zeros_like(cands[0][k]) for j in sel])
    batch.update(sel=sel, n_valid=n_valid, overflow=overflow)
    return batch, cands


def sample(sel, counts, pools, caps, M, N, search_box, idx_t=None, idx_s=None, seed=0, counter=0):
    """o3d_train_sample on the host for arbitrary crop pools.  sel (B,); counts (J,3); pools = (first (J,cap0,3), template
    (J,cap1,3), search (J,cap2,3)); search_box (J,15); idx_t (J,M) / idx_s (J,N) | None (the device draw) -> dict of
    template_points (B,M,3), search_points (B,N,3), seg_label (B,N), used_t (B,M), used_s (B,N)"""
    B = len(sel)
    out = {"template_points": np.zeros((B, M, 3), f32), "search_points": np.zeros((B, N, 3), f32), "seg_label": np.zeros((B, N), f32),
           "used_t": np.full((B, M), -1, np.int32), "used_s": np.full((B, N), -1, np.int32)}
    for r, j in enumerate(sel):
        if j < 0:
            continue
        n = [min(int(counts[j][c]), caps[c]) for c in range(3)]
        clouds = (np.concatenate([pools[0][j][:n[0]], pools[1][j][:n[1]]], 0), pools[2][j][:n[2]])
        for cloud, (src, S, given, name) in enumerate(zip(clouds, (M, N), (idx_t, idx_s), ("template", "search"))):
            if src.shape[0] <= 2:
                continue
            idx = np.asarray(given[j], np.int64) if given is not None else sample_indices(draw_key(seed, counter, j, cloud), src.shape[0], S)
            ok = (idx >= 0) & (idx < src.shape[0])
            out[name + "_points"][r][ok] = src[idx[ok]]
            out["used_" + name[0]][r][ok] = idx[ok]
        keep, _ = TO.crop_mask(out["search_points"][r], search_box[j], 1.0, 0.0, TO.SUBWINDOW)
        out["seg_label"][r] = (keep & (out["used_s"][r] >= 0)).astype(f32)
    return out


def check_against_reference(got, ref, k, box_aware):
    """`got` (one sample's outputs) against sample `k` of tests/golden/ref_train_batches.npz under the project's bounds
    (DESIGN.md section 12 / 12b): points within 2e-5 m, BoxCloud within 1e-4, box_label centre within 2e-5 and angle exact,
    bbox_size exact, seg_label exact outside near_face"""
    assert np.abs(got["template_points"] - ref[k + "template_points"]).max() <= 2e-5
    assert np.abs(got["search_points"] - ref[k + "search_points"]).max() <= 2e-5
    assert np.abs(got["box_label"][:3] - ref[k + "box_label"][:3]).max() <= 2e-5
    assert got["box_label"][3] == ref[k + "box_label"][3]
    assert np.array_equal(got["bbox_size"], ref[k + "bbox_size"])
    near = np.unpackbits(ref[k + "near_face"])[:got["seg_label"].shape[0]].astype(bool)
    assert near.sum() <= 16
    assert np.array_equal(got["seg_label"][~near], ref[k + "seg_label"][~near])
    if box_aware:
        assert np.abs(got["points2cc_dist_t"] - ref[k + "points2cc_dist_t"]).max() <= 1e-4
        assert np.abs(got["points2cc_dist_s"] - ref[k + "points2cc_dist_s"]).max() <= 1e-4
