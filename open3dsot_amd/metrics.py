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
