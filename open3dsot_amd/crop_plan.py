"""The host tables of the grouped crop (o3d_track_crop_groups[_aug]), planned for many steps at once: numpy and the record
dtypes only; device addresses are plain integers.  A step's table is CROP_PLAN rows, one per distinct cloud, whose wg_start /
row_start / sbase are prefix sums over the cloud's workgroups of 256 points; the rows point into a table of CROP_TARGET
records.  The training epoch (sampler.plan_chunk, the per-batch builders) and the test epoch on L lanes
(tracking.plan_lane_steps) lay the tables of P steps end to end in one Tables buffer, fill them with plan_groups and send them
to the device with upload: one copy per chunk.  o3d_track_crop_groups_scratch computes the same prefix sums for one step
(points_utils.crop_groups_plan: the tests hold plan_groups against it), and o3d_track_crop_groups checks them again before it
launches."""
import numpy as np
import torch

from . import points_utils as PU


def _section(layout, name, nbytes):
    off = layout["_end"]
    layout[name] = (off, nbytes)
    layout["_end"] = off + -(-nbytes // 64) * 64


class Tables:
    """The tables of P steps in ONE host buffer (`host`, uint8), which travels to the device in one copy; `base` is the address
    of that copy.  sections = {name: (dtype, per-step shape)}: section `name` holds the P steps' parts end to end and starts on
    a multiple of 64 bytes; view(name) is its (P,) + shape view, dev(name, k) the device address of step k's part."""

    def __init__(self, P, sections, base=0):
        self.P, self.base = int(P), int(base)
        self._per = {name: (int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize, dtype, tuple(shape))
                     for name, (dtype, shape) in sections.items()}
        self._layout = {"_end": 0}
        for name, (nbytes, _, _) in self._per.items():
            _section(self._layout, name, self.P * nbytes)
        self.host = np.zeros(self._layout["_end"], np.uint8)

    def view(self, name):
        nbytes, dtype, shape = self._per[name]
        off = self._layout[name][0]
        return self.host[off:off + self.P * nbytes].view(dtype).reshape((self.P,) + shape)

    def dev(self, name, k=0):
        """the device address of step k's part of section `name`"""
        return self.base + self._layout[name][0] + self._per[name][0] * k


def plan_groups(key, frame, records, fptr, fn, targets_out, plan_out, targets_dev, valid=None):
    """The crop tables of S steps of n records each, in whole-chunk numpy: a pure function of integer arrays.  key (S,n): the
    records of a step with equal keys form one group, the groups stand in the order of their keys and a group's records in the
    order they came in (a stable sort); frame (S,n): the index into fptr / fn (per cloud its address and size) of the cloud a
    record reads, one cloud per group; records (n,) or (S,n) CROP_TARGET; valid (S,n) bool: the other records are dropped and
    belong to no group.  Fills targets_out[:S] (the records, a group's side by side; targets_dev = the device address of
    targets_out) and the first groups[k] rows of plan_out[k] -> (groups, need = the scratch length, grid = the workgroups of
    the count / scatter launches: three (S,) int64 arrays, and order (S,n): targets_out[k, i] is record order[k, i])."""
    key, frame = np.asarray(key, np.int64), np.asarray(frame, np.int64)
    S, n = key.shape
    live = np.ones((S, n), bool) if valid is None else np.asarray(valid, bool)
    order = np.argsort(np.where(live, key, np.iinfo(np.int64).max), axis=1, kind="stable")      # the dropped ones behind the others
    key, live = np.take_along_axis(key, order, 1), np.take_along_axis(live, order, 1)
    targets_out[:S] = records[order] if records.ndim == 1 else np.take_along_axis(records, order, 1)
    new = live.copy()
    new[:, 1:] &= key[:, 1:] != key[:, :-1]
    p, pos = np.nonzero(new)                                                       # one entry per group, step-major
    head = np.ones(p.size, bool)
    head[1:] = p[1:] != p[:-1]
    first = np.flatnonzero(head)[np.cumsum(head) - 1]                              # the entry of the first group of the same step
    g = np.arange(p.size) - first
    last = np.ones(p.size, bool)
    last[:-1] = head[1:]
    k = np.where(last, live.sum(1)[p], np.append(pos[1:], 0)) - pos                # the group's records
    cloud = np.take_along_axis(frame, order, 1)[p, pos]
    pts = fn[cloud]
    wgs = np.maximum(1, -(-pts // 256))

    def before(v):                                                                 # the sum over the earlier groups of the step
        c = np.cumsum(v) - v
        return c - c[first]
    plan = plan_out[:S]
    plan["points"][p, g], plan["n"][p, g], plan["n_targets"][p, g] = fptr[cloud], pts, k
    plan["targets"][p, g] = int(targets_dev) + PU.CROP_TARGET.itemsize * (p * n + pos)
    plan["wg_start"][p, g], plan["row_start"][p, g], plan["sbase"][p, g] = before(wgs), pos, before(wgs * k)
    return (np.bincount(p, minlength=S), np.bincount(p, wgs * k, S).astype(np.int64), np.bincount(p, wgs, S).astype(np.int64),
            order)


class FramePool:
    """The clouds of all tracklets end to end: `tracklets` = per tracklet the list of its frames ((n,3) device tensors).
    Tracklet t owns the pool rows [row0[t], row0[t + 1]); fptr / fn = per pool row the frame's address and size, wgs = its
    workgroups of 256 points (an empty frame still takes one)."""

    def __init__(self, tracklets):
        frames = [x for f in tracklets for x in f]
        self.row0 = np.concatenate([[0], np.cumsum([len(f) for f in tracklets])]).astype(np.int64)
        self.fptr = np.array([x.data_ptr() for x in frames], np.int64)
        self.fn = np.array([x.shape[0] for x in frames], np.int64)
        self.wgs = np.maximum(1, -(-self.fn // 256))

    def worst_scratch(self, rows_per_step):
        """rows_per_step (steps, m): the pool row that each record of a step reads (negative: none) -> the crop scratch of the
        largest step in int32: one word per (record, workgroup of its frame)"""
        rows = np.asarray(rows_per_step, np.int64)
        if not rows.size:
            return 0
        return int(np.where(rows >= 0, self.wgs[np.maximum(rows, 0)], 0).sum(1).max())


def upload(tables, dev_tensor):
    """THE copy of a chunk: tables.host through a pinned copy (the allocator's to recycle) into dev_tensor, on the current
    stream"""
    with torch.cuda.device(dev_tensor.device):
        dev_tensor.copy_(torch.from_numpy(tables.host).pin_memory(), non_blocking=True)
