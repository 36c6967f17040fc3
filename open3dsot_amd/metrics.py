"""Scoring tracked boxes on the device: the reference's estimateOverlap / estimateAccuracy (utils/metrics.py:27-72) as one
launch of o3d_track_score (csrc/metrics.hip) over device-resident boxes, and its TorchSuccess / TorchPrecision (:75-125) as
2n + 1 integer counters that the same launch can fill.

  score_boxes        (...,15) annotation boxes, (...,15) result boxes -> overlaps (...), distances (...); no sync
  SuccessPrecision   the Success / Precision curves as device counters: update() or score_boxes(accumulate=...), then
                     compute() = ONE read-back of 2n + 1 integers and the reference's own trapz expression on the host

A box is 15 floats: centre (3), wlh (3), row-major rotation (9), as everywhere in this package.  There is no CPU path.
"""
import torch

from . import capi
from .points_utils import _need_gpu


MAX_THRESHOLDS = 64


def up_index(up_axis):
    """the index of the non-zero component of up_axis; like the reference (fromBoxToPoly), (0,-1,0) and (0,0,1) style axes only"""
    nz = [i for i, c in enumerate(up_axis) if c != 0]
    if len(up_axis) != 3 or nz not in ([1], [2]):
        raise ValueError("up_axis %r: expected one non-zero component, y or z" % (tuple(up_axis),))
    return nz[0]


def _ptr(t):
    return t.data_ptr() if t is not None else None


def score_boxes(a, b, dim=3, up_axis=(0, 0, 1), valid=None, out=None, accumulate=None):
    """estimateOverlap(a, b, dim, up_axis) and estimateAccuracy(a, b, dim, up_axis) for every pair of rows: a (...,15) the
    annotation boxes, b (...,15) the result boxes, float32 on the GPU.  One launch, no sync.
    valid (...) | None: rows with valid == 0 are skipped (their outputs keep what `out` held; zeros when allocated here).
    out = (overlaps, distances) float32 (...) to write into | None: allocated.  accumulate: a SuccessPrecision whose counters
    the launch adds to.  -> (overlaps, distances)."""
    _need_gpu(a, "score_boxes")
    _need_gpu(b, "score_boxes")
    if dim not in (2, 3):
        raise ValueError("dim %r: 2 or 3" % (dim,))
    up = up_index(up_axis)
    if a.shape != b.shape or a.shape[-1] != 15:
        raise ValueError("score_boxes: two (...,15) tensors of the same shape expected, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    dev, lead = a.device, a.shape[:-1]
    a, b = a.contiguous().float(), b.to(dev).contiguous().float()
    n = a.numel() // 15
    if valid is not None:
        _need_gpu(valid, "score_boxes")
        valid = valid.to(torch.int32).contiguous()
        if valid.numel() != n:
            raise ValueError("score_boxes: valid has %d entries for %d pairs" % (valid.numel(), n))
    if out is None:
        out = (torch.zeros(lead, dtype=torch.float32, device=dev), torch.zeros(lead, dtype=torch.float32, device=dev))
    ov, di = out
    for t in (ov, di):
        _need_gpu(t, "score_boxes")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise ValueError("score_boxes: out must be two contiguous float32 tensors of %d entries" % n)
    m = accumulate
    if m is not None and m.counts.device != dev:
        raise ValueError("score_boxes: the metric lives on %s, the boxes on %s" % (m.counts.device, dev))
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_score(
            a.data_ptr(), b.data_ptr(), _ptr(valid), n, int(dim), up, ov.data_ptr(), di.data_ptr(),
            _ptr(m.thresholds[0]) if m else None, m.n if m else 0, _ptr(m.thresholds[1]) if m else None, m.n if m else 0,
            _ptr(m.counts[:m.n]) if m else None, _ptr(m.counts[m.n:2 * m.n]) if m else None, _ptr(m.counts[2 * m.n:]) if m else None,
            torch.cuda.current_stream(dev).cuda_stream), "o3d_track_score")
    return ov, di


def curve_area(counts, total, xaxis, max_value):
    """TorchSuccess.compute / TorchPrecision.compute on threshold counts: counts (n) integers, total = the number of samples,
    xaxis (n) float32 thresholds.  `counts.float() / total` is the reference's `value()` (each entry a float32 count divided by
    len), the rest its own expression, in float32 on the host: equal counts give a bit-identical number.  0 when empty."""
    if int(total) == 0:
        return 0.0
    value = torch.as_tensor(counts, dtype=torch.int64).float() / int(total)
    return float(torch.trapz(value, x=xaxis) * 100 / max_value)


class SuccessPrecision:
    """TorchSuccess(n, max_overlap) and TorchPrecision(n, max_accuracy) of the reference (utils/metrics.py:75-125) as device
    counters.  thresholds (2,n) float32 on the device, computed on the host as the reference computes its Xaxis
    (torch.linspace(0, max, steps=n)) and uploaded once; counts (2n + 1) int64 on the device = the overlaps >= each Success
    threshold, the distances <= each Precision threshold, the number of samples.  The counts of several ranks add up.

        m = SuccessPrecision(device=dev)
        score_boxes(gt, results, accumulate=m)        # or m.update(overlaps, distances) on device tensors
        m.compute()                                   # {"success": ..., "precision": ..., "frames": ...}, one read-back
    """

    def __init__(self, n=21, max_overlap=1, max_accuracy=2, device=None):
        n = int(n)
        if not 1 <= n <= MAX_THRESHOLDS:
            raise ValueError("n must be 1..%d" % MAX_THRESHOLDS)
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("SuccessPrecision: CPU not supported (the counters live on a GPU)")
        capi.load()
        self.n, self.max_overlap, self.max_accuracy = n, max_overlap, max_accuracy
        self.xaxis = (torch.linspace(0, max_overlap, steps=n), torch.linspace(0, max_accuracy, steps=n))
        self.thresholds = torch.stack(self.xaxis).to(dev).contiguous()
        self.counts = torch.zeros((2 * n + 1,), dtype=torch.int64, device=dev)

    def reset(self):
        self.counts.zero_()

    def update(self, overlaps, distances):
        """add device tensors of overlaps and distances (the same number of each) to the counters; no sync"""
        _need_gpu(overlaps, "SuccessPrecision.update")
        _need_gpu(distances, "SuccessPrecision.update")
        o, d = overlaps.reshape(-1, 1).float(), distances.reshape(-1, 1).float()
        if o.shape != d.shape:
            raise ValueError("SuccessPrecision.update: %d overlaps, %d distances" % (o.numel(), d.numel()))
        n = self.n
        self.counts[:n] += (o >= self.thresholds[0]).sum(0)
        self.counts[n:2 * n] += (d <= self.thresholds[1]).sum(0)
        self.counts[2 * n] += o.shape[0]

    def _read(self):
        """the one read-back: the 2n + 1 counters on the host"""
        return self.counts.cpu()

    def compute(self):
        c, n = self._read(), self.n
        total = int(c[2 * n])
        return {"success": curve_area(c[:n], total, self.xaxis[0], self.max_overlap),
                "precision": curve_area(c[n:2 * n], total, self.xaxis[1], self.max_accuracy), "frames": total}


# ---- scoring a managed scene: the CLEAR-MOT bookkeeping (Bernardin & Stiefelhagen 2008) on the device; DESIGN.md section 12k ---
MOT_CHUNK_BYTES = 64 << 20             # the two (chunk,G,K) float32 score matrices of one update() chunk stay under this


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


class ClearMOT:
    """The multi-object counterpart of SuccessPrecision: G ground-truth objects against the K slots of a managed scene tracker
    whose slots change hands (tracking.ManagedSceneTracker: boxes (T,K,15) and ids_log (T,K)), scored where they are.  Per chunk
    of frames two launches, o3d_scene_pair_scores_frames (every pair's overlap and distance, metrics.score_boxes' bits) and
    o3d_scene_mot_walk (one workgroup walks the frames in order: an object keeps the track id it was last matched to while that
    pair passes the gates, the rest is matched greedily by overlap descending, distance ascending -- or, with
    assignment="optimal", by the maximum-cardinality, minimum-cost assignment under cost = "distance" | "overlap", CLEAR-MOT as
    published, through o3d_scene_mot_walk_assign), as include/o3dsot.h states them.  A pair can match when overlap >= min_iou and distance <= max_dist (2 m: the centre distance commonly used for a true
    positive in 3D tracking).  State on the device: the walk's last_id / tracked_prev / ever (G,), totals (8,) int64 = the sums
    of per_frame, sums (2,) float64 = the matched pairs' distances and overlaps, seen / hit (G,) int64 = every object's valid and
    matched frames.  The integer totals of several ranks add up.

        m = ClearMOT(G, device=dev)
        m.update(gt, valid, trk.boxes[:t], trk.ids_log[:t])       # or trk.score_mot(gt, valid, metrics=m); no sync
        m.compute()                                                # {"mota": ..., "idsw": ..., ...}, one read-back

    keep_logs=True keeps every chunk's match rows for logs().  sot: a SuccessPrecision that takes the matched pairs' overlaps
    and distances through its update()."""

    def __init__(self, G, device=None, min_iou=0.0, max_dist=2.0, dim=3, up_axis=(0, 0, 1), keep_logs=False, sot=None,
                 assignment="greedy", cost="distance"):
        from . import points_utils as PU
        PU._assign_args(assignment, cost, "ClearMOT")
        self.assignment, self.cost = assignment, cost
        G = int(G)
        if not 1 <= G <= PU.CROP_MULTI_MAX_TARGETS:
            raise ValueError("G must be 1..%d" % PU.CROP_MULTI_MAX_TARGETS)
        if dim not in (2, 3):
            raise ValueError("dim %r: 2 or 3" % (dim,))
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("ClearMOT: CPU not supported (the state lives on a GPU)")
        capi.load()
        self.G, self.dev, self.dim, self.up = G, dev, int(dim), up_index(up_axis)
        self.min_iou, self.max_dist, self.keep_logs, self.sot = float(min_iou), float(max_dist), bool(keep_logs), sot
        self.state = torch.zeros((3, G), dtype=torch.int32, device=dev)          # last_id, tracked_prev, ever
        self.counts = torch.zeros((8 + 2 * G,), dtype=torch.int64, device=dev)   # totals (8), seen (G), hit (G)
        self.sums = torch.zeros((2,), dtype=torch.float64, device=dev)           # matched distances, matched overlaps
        self.reset()

    def reset(self):
        self.state.zero_()
        self.state[0].fill_(-1)
        self.counts.zero_()
        self.sums.zero_()
        self.frames, self._logs = 0, []

    def chunk_frames(self, K):
        """the frames of one chunk of update() for K columns: the two score matrices within MOT_CHUNK_BYTES, the walk's cap"""
        from . import points_utils as PU
        return max(1, min(PU.SCENE_MOT_MAX_FRAMES, MOT_CHUNK_BYTES // (8 * self.G * int(K))))

    def update(self, gt, valid, boxes, ids):
        """F further frames, in order: gt (F,G,15) float32, valid (F,G) | None (every object annotated in every frame), boxes
        (F,K,15) float32, ids (F,K) int32 (< 0: the slot holds no track), device tensors.  Two launches per chunk and a few
        reductions in torch; no sync."""
        from . import points_utils as PU
        what = "ClearMOT.update"
        for t in (gt, boxes, ids) + (() if valid is None else (valid,)):
            _need_gpu(t, what)
        F, G = gt.shape[0], self.G
        if tuple(gt.shape) != (F, G, 15) or boxes.dim() != 3 or boxes.shape[0] != F or boxes.shape[2] != 15:
            raise ValueError("%s: gt %s and boxes %s for G = %d" % (what, tuple(gt.shape), tuple(boxes.shape), G))
        K = boxes.shape[1]
        if tuple(ids.shape) != (F, K) or (valid is not None and tuple(valid.shape) != (F, G)):
            raise ValueError("%s: ids %s, valid %s for (F,G,K) = %s" % (what, tuple(ids.shape), None if valid is None else
                                                                      tuple(valid.shape), (F, G, K)))
        gt, boxes, ids = gt.float().contiguous(), boxes.float().contiguous(), ids.to(torch.int32).contiguous()
        valid = torch.ones((F, G), dtype=torch.int32, device=self.dev) if valid is None else (valid != 0).to(torch.int32).contiguous()
        step = self.chunk_frames(K)
        with torch.cuda.device(self.dev):
            for lo in range(0, F, step):
                hi = min(lo + step, F)
                v, h = valid[lo:hi], ids[lo:hi]
                ov, di = PU.scene_pair_scores_frames(gt[lo:hi], v, boxes[lo:hi], h, self.dim, self.up)
                rows = PU.scene_mot_walk(ov, di, v, h, self.state[0], self.state[1], self.state[2], self.min_iou, self.max_dist,
                                         assignment=self.assignment, cost=self.cost)
                slot, _, mov, mdi, per_frame = rows
                hit = slot >= 0
                self.counts[:8] += per_frame.sum(0)
                self.counts[8:8 + G] += v.sum(0)
                self.counts[8 + G:] += hit.sum(0)
                zero = torch.zeros((), dtype=torch.float64, device=self.dev)
                self.sums[0] += torch.where(hit, mdi.double(), zero).sum()
                self.sums[1] += torch.where(hit, mov.double(), zero).sum()
                if self.sot is not None:                   # an unmatched row (-1, +inf) passes no threshold: only `total` is set right
                    self.sot.update(mov, mdi)
                    self.sot.counts[2 * self.sot.n] -= (~hit).sum()
                if self.keep_logs:
                    self._logs.append(rows[:4])
        self.frames += F

    def logs(self):
        """keep_logs=True: {match_slot, match_id (T,G) int32, match_ov, match_di (T,G) float32} device tensors over every frame
        since reset(); no sync"""
        if not self.keep_logs:
            raise RuntimeError("ClearMOT.logs: created with keep_logs=False")
        names = ("match_slot", "match_id", "match_ov", "match_di")
        kinds = (torch.int32, torch.int32, torch.float32, torch.float32)
        return {n: torch.cat([c[i] for c in self._logs]) if self._logs else torch.zeros((0, self.G), dtype=k, device=self.dev)
                for i, (n, k) in enumerate(zip(names, kinds))}

    def _read(self):
        """the one read-back: the integer counters and the bits of the two float64 sums"""
        return torch.cat([self.counts, self.sums.view(torch.int64)]).cpu()

    def compute(self):
        """{frames, gt, hyp, tp, fp, fn, idsw, frag, mota, motp_dist, motp_iou, recall, precision, objects, mostly_tracked,
        mostly_lost}: mota = 1 - (fn + fp + idsw) / gt; motp_* the means over the true positives; mostly_tracked / mostly_lost
        the share of the `objects` (those with a valid frame) matched in >= 80 % / <= 20 % of their valid frames.  Every rate is
        0.0 when its denominator is 0."""
        from .points_utils import MOT_FRAME_COLS
        c, G = self._read(), self.G
        tot = dict(zip(MOT_FRAME_COLS, c[:7].tolist()))
        seen, hit = c[8:8 + G], c[8 + G:8 + 2 * G]
        s_di, s_ov = c[8 + 2 * G:].view(torch.float64).tolist()
        live = seen > 0
        objects = int(live.sum())
        res = dict(frames=self.frames, **tot)
        res["mota"] = 1.0 - _ratio(tot["fn"] + tot["fp"] + tot["idsw"], tot["gt"]) if tot["gt"] else 0.0
        res["motp_dist"], res["motp_iou"] = _ratio(s_di, tot["tp"]), _ratio(s_ov, tot["tp"])
        res["recall"], res["precision"] = _ratio(tot["tp"], tot["gt"]), _ratio(tot["tp"], tot["hyp"])
        res["objects"] = objects
        res["mostly_tracked"] = _ratio(int((live & (5 * hit >= 4 * seen)).sum()), objects)
        res["mostly_lost"] = _ratio(int((live & (5 * hit <= seen)).sum()), objects)
        return res
