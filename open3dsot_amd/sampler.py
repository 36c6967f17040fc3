"""Training batches built on the device: the device form of the reference's PointTrackingSampler + siamese_processing
(datasets/sampler.py:16-79,183-243) for BAT and P2B.  Frames and ground-truth boxes go in, the training dict of
trackers.BAT / P2B.training_step comes out, resident in HBM; per batch there is no host synchronisation, ONE pinned upload and
a fixed number of launches on the current stream (csrc/train_batch.hip):

    o3d_track_offset_box_multi   the two jittered boxes of every candidate (getOffsetBB, K = 2J)
    o3d_train_labels             transform_box, box_label, bbox_size, the canonical model box
    o3d_track_crop_groups (3)    the three crops of every candidate, every frame read once
    o3d_train_select             which candidates fill the batch
    o3d_train_sample             regularize_pc of both clouds, seg_label, the batch's label rows
    o3d_boxcloud (2, box_aware)  points2cc_dist_t / points2cc_dist_s

Not covered: M2-Track's motion_processing, use_augmentation, dataset readers.
"""
import math

import numpy as np
import torch

from . import points_utils as PU

# the data keys of cfgs/BAT_Car.yaml:5-15,23 (P2B_Car.yaml: the same but box_aware False)
DATA_KEYS = dict(search_bb_scale=1.25, search_bb_offset=2, model_bb_scale=1.25, model_bb_offset=0, template_size=512,
                 search_size=1024, degrees=True, box_aware=True, num_candidates=4, data_limit_box=False, use_augmentation=False)
DEFAULT_CAPACITY = (4096, 4096, 16384)       # rows of the first-frame, template-frame and search crop buffers


def _cfg(config, key):
    if isinstance(config, dict):
        return config.get(key, DATA_KEYS[key])
    return getattr(config, key, DATA_KEYS[key])


class DeviceTracklet:
    """one tracklet: frames = a list of T (n,3) float32 GPU tensors, boxes = (T,15) float32 on the host ([centre | wlh |
    rotation matrix row-major]; they travel in the builder's one upload)"""

    def __init__(self, frames, boxes, device=None):
        dev = torch.device(device) if device is not None else None
        self.frames = []
        for f in frames:
            t = torch.as_tensor(f, dtype=torch.float32)
            t = t.to(dev if dev is not None else (t.device if t.is_cuda else torch.device("cuda")))
            assert t.dim() == 2 and t.shape[1] == 3
            self.frames.append(t.contiguous())
        self.boxes = np.ascontiguousarray(boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else boxes, dtype=np.float32)
        assert self.boxes.shape == (len(self.frames), 15)

    def __len__(self):
        return len(self.frames)


class DeviceTracklets(list):
    """Tracklets resident in HBM: a list of DeviceTracklet.  DeviceTracklets(frames, boxes) takes the output of
    synth.make_sequence directly (one tracklet), or a list of frame lists with a list of (T,15) boxes (one per tracklet)."""

    def __init__(self, frames=(), boxes=(), device=None):
        super().__init__()
        if len(frames) and isinstance(frames[0], (list, tuple)):
            for f, b in zip(frames, boxes):
                self.append(DeviceTracklet(f, b, device))
        elif len(frames):
            self.append(DeviceTracklet(frames, boxes, device))


def _section(layout, name, nbytes):
    off = layout["_end"]
    layout[name] = (off, nbytes)
    layout["_end"] = off + -(-nbytes // 64) * 64


class SiameseBatchBuilder:
    """build(samples) -> the training dict: template_points (B,M,3), search_points (B,N,3), box_label (B,4), bbox_size (B,3),
    seg_label (B,N) and, with box_aware, points2cc_dist_t (B,M,9) / points2cc_dist_s (B,N,9) -- the keys and shapes of
    synth.make_batch -- plus n_valid (1,) and overflow (1,) int32, all device tensors.

    samples: J = `candidates` (default ceil(1.25 B)) tuples (tracklet: DeviceTracklet, first, template, search: frame indices,
    candidate_id).  The batch takes the first B valid candidates (a candidate is valid iff the reference's two assertions
    hold: template cloud > 20 points, search cloud > 20 points); fewer than B valid ones repeat cyclically.  This
    over-provisioning replaces the reference's retry with another random index (sampler.py:242-243), which needs the host.

    draws: {offset_t (J,3), offset_s (J,3), idx_t (J,M), idx_s (J,N)} teacher-forces the box jitter and the resampling
    indices of every candidate.  Without it the offsets come from a numpy Generator seeded with `seed` (uniform +-0.3 with the
    angle x5 degrees or x deg2rad(5), sampler.py:36-40; normal with covariance diag(1, 1, 5 or deg2rad(5)), :50-54; zero for
    candidate_id 0) and the indices are drawn on the device, keyed by (seed, the build counter, candidate, cloud, row).
    out: {key: tensor} destinations written in place (the fields of a dist.FlatBatch).

    DEVIATION from the reference: the crops live in buffers of fixed `capacity` = (first, template, search) rows.  A crop
    longer than its buffer is truncated to its first `capacity` survivors, and the draw uses the truncated length; `overflow`
    counts the truncated crops among the chosen rows.  With limit_box (data_limit_box) the random replacement is the
    counter-based draw of o3d_track_offset_box, not numpy's.

    All launches go to the current stream; one builder serves one stream at a time.  The pinned staging buffer has two slots,
    each guarded by an event, so the build of batch t+1 may be enqueued while the upload of batch t is in flight.  The
    attributes sel (B,), counts (J,3), crops and, with record_indices, used_t (B,M) / used_s (B,N) show the last build's
    intermediate results (they are overwritten by the next build)."""

    def __init__(self, config, batch_size, candidates=None, capacity=DEFAULT_CAPACITY, seed=0, record_indices=False):
        if _cfg(config, "use_augmentation"):
            raise NotImplementedError("SiameseBatchBuilder: use_augmentation (points_utils.apply_augmentation) is not built")
        self.B = int(batch_size)
        self.J = int(candidates) if candidates is not None else int(math.ceil(1.25 * self.B))
        if not 1 <= self.B <= self.J <= PU.TRAIN_MAX_CANDIDATES:
            raise ValueError("1 <= batch_size <= candidates <= %d" % PU.TRAIN_MAX_CANDIDATES)
        self.caps = tuple(int(c) for c in ((capacity,) * 3 if isinstance(capacity, int) else capacity))
        assert len(self.caps) == 3 and min(self.caps) >= 1
        self.M, self.N = int(_cfg(config, "template_size")), int(_cfg(config, "search_size"))
        self.degrees, self.box_aware = bool(_cfg(config, "degrees")), bool(_cfg(config, "box_aware"))
        self.limit_box = bool(_cfg(config, "data_limit_box"))
        self.num_candidates = int(_cfg(config, "num_candidates"))
        self.scales = (float(_cfg(config, "model_bb_scale")), float(_cfg(config, "model_bb_offset")),
                       float(_cfg(config, "search_bb_scale")), float(_cfg(config, "search_bb_offset")))
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        self.counter = 0
        self.record_indices = bool(record_indices)
        self.device = None

    # ---- buffers (allocated once, on the first build) ---------------------------------------------------------------------------------
    def _allocate(self, dev):
        J, B, M, N = self.J, self.B, self.M, self.N
        self.device = dev
        lay = {"_end": 0}
        _section(lay, "refs", 2 * J * 60)             # rows [0, J): the template frame's box, [J, 2J): the search frame's
        _section(lay, "offs", 2 * J * 16)             # (x, y, 0, theta) of the two jitters
        _section(lay, "first", J * 60)                # the first frame's box
        _section(lay, "targets", 3 * J * PU.CROP_TARGET.itemsize)
        _section(lay, "plan", 3 * J * PU.CROP_PLAN.itemsize)
        self._base_bytes = lay["_end"]
        _section(lay, "idx_t", J * M * 4)             # teacher-forced builds only
        _section(lay, "idx_s", J * N * 4)
        self._layout = lay
        self._up = torch.empty(lay["_end"], dtype=torch.uint8, device=dev)
        self._pinned = [torch.empty(lay["_end"], dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._events = [torch.cuda.Event() for _ in range(2)]
        self._used = [False, False]

        def f32(*shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev)

        def i32(*shape):
            return torch.zeros(shape, dtype=torch.int32, device=dev)
        self._jit = f32(2 * J, 15)
        self._search_box, self._cand_label, self._cand_size, self._model_box = f32(J, 15), f32(J, 4), f32(J, 3), f32(J, 15)
        self.counts = i32(J, 3)
        self.crops = tuple(f32(J, c, 3) for c in self.caps)
        self.sel = i32(B)
        self._bc_boxes = f32(2, 15 * B)
        self.used_t = i32(B, M) if self.record_indices else None
        self.used_s = i32(B, N) if self.record_indices else None
        self._scratch = i32(1 << 16)
        # the target record of crop c of candidate j: everything but its place in the table is fixed
        up = self._up.data_ptr()
        rec = np.zeros((3, J), PU.CROP_TARGET)
        j = np.arange(J, dtype=np.uint64)
        rec["box"][0] = up + lay["first"][0] + 60 * j
        rec["box"][1] = self._jit.data_ptr() + 60 * j
        rec["box"][2] = self._jit.data_ptr() + 60 * (J + j)
        for c in range(3):
            rec["scale"][c], rec["offset"][c] = self.scales[0 if c < 2 else 2], self.scales[1 if c < 2 else 3]
            rec["mode"][c] = PU.CROP_MODEL if c < 2 else PU.CROP_SUBWINDOW
            rec["out"][c] = self.crops[c].data_ptr() + 12 * self.caps[c] * j
            rec["capacity"][c] = self.caps[c]
            rec["count"][c] = self.counts.data_ptr() + 12 * j + 4 * c
        self._rec = rec

    def _view(self, slot, name, dtype, shape):
        off, nbytes = self._layout[name]
        return self._pinned[slot].numpy()[off:off + nbytes].view(dtype).reshape(shape)

    def _dev(self, name):
        return self._up.data_ptr() + self._layout[name][0]

    def draw_offsets(self, candidate_ids):
        """the host draw of the two box jitters of J candidates -> (offset_t (J,3), offset_s (J,3)) float64"""
        J = len(candidate_ids)
        ang = 5.0 if self.degrees else float(np.deg2rad(5))
        off_t = self.rng.uniform(-0.3, 0.3, (J, 3))
        off_t[:, 2] *= ang
        off_s = self.rng.normal(0.0, 1.0, (J, 3)) * np.sqrt(np.array([1.0, 1.0, ang]))
        zero = np.asarray(candidate_ids) == 0
        off_t[zero] = 0.0
        if self.num_candidates > 1:
            off_s[zero] = 0.0
        return off_t, off_s

    def build(self, samples, draws=None, out=None):
        J, B, M, N = self.J, self.B, self.M, self.N
        if len(samples) != J:
            raise ValueError("build() takes %d candidates, got %d" % (J, len(samples)))
        dev = samples[0][0].frames[0].device
        if self.device is None:
            with torch.cuda.device(dev):
                self._allocate(dev)
        assert dev == self.device
        stream = torch.cuda.current_stream(dev)
        slot = self.counter & 1
        if self._used[slot]:
            self._events[slot].synchronize()          # the upload of two builds ago: long done in a running loop
        refs = self._view(slot, "refs", np.float32, (2 * J, 15))
        offs = self._view(slot, "offs", np.float32, (2 * J, 4))
        first = self._view(slot, "first", np.float32, (J, 15))
        targets = self._view(slot, "targets", PU.CROP_TARGET, (3 * J,))
        if draws is None:
            off_t, off_s = self.draw_offsets([s[4] for s in samples])
        else:
            off_t, off_s = np.asarray(draws["offset_t"], np.float64), np.asarray(draws["offset_s"], np.float64)
            assert off_t.shape == (J, 3) and off_s.shape == (J, 3)
        offs[:] = 0
        offs[:J, :2], offs[:J, 3] = off_t[:, :2], off_t[:, 2]
        offs[J:, :2], offs[J:, 3] = off_s[:, :2], off_s[:, 2]
        # the groups: every distinct frame once, with the crops that read it
        groups, order = {}, []
        for j, (trk, f0, f1, f2, _) in enumerate(samples):
            first[j], refs[j], refs[J + j] = trk.boxes[f0], trk.boxes[f1], trk.boxes[f2]
            for c, f in enumerate((f0, f1, f2)):
                key = (id(trk), f)
                if key not in groups:
                    groups[key] = (trk.frames[f], [], [])
                    order.append(key)
                groups[key][1].append(c)
                groups[key][2].append(j)
        G = len(order)
        plan = self._view(slot, "plan", PU.CROP_PLAN, (3 * J,))[:G]
        pos = 0
        tab = self._dev("targets")
        for g, key in enumerate(order):
            pts, cs, js = groups[key]
            k = len(cs)
            targets[pos:pos + k] = self._rec[cs, js]
            plan[g] = (pts.data_ptr(), pts.shape[0], tab + PU.CROP_TARGET.itemsize * pos, k, 0, 0, 0)
            pos += k
        need = PU.crop_groups_plan(plan)[0]
        nbytes = self._base_bytes
        idx_t = idx_s = None
        if draws is not None and draws.get("idx_t") is not None:
            self._view(slot, "idx_t", np.int32, (J, M))[:] = draws["idx_t"]
            self._view(slot, "idx_s", np.int32, (J, N))[:] = draws["idx_s"]
            nbytes = self._layout["_end"]
            idx_t, idx_s = self._dev("idx_t"), self._dev("idx_s")
        with torch.cuda.device(dev):
            if self._scratch.numel() < need:
                self._scratch = torch.empty(need, dtype=torch.int32, device=dev)
            self._up[:nbytes].copy_(self._pinned[slot][:nbytes], non_blocking=True)       # THE upload of this batch
            self._events[slot].record(stream)
            self._used[slot] = True
            up32 = self._up.view(torch.float32)
            r0, o0 = self._layout["refs"][0] // 4, self._layout["offs"][0] // 4
            refs_d, offs_d = up32[r0:r0 + 2 * J * 15], up32[o0:o0 + 2 * J * 4]
            PU.offset_box_multi(refs_d, offs_d, out=self._jit, degrees=self.degrees, use_z=False, limit_box=self.limit_box,
                                seed=(self.seed + 7919 * self.counter) & 0x3fffffff)
            PU.train_labels(refs_d[J * 15:], self._jit[J:], self._jit[:J], offs_d[J * 4:], self._search_box, self._cand_label,
                            self._cand_size, self._model_box)
            PU.crop_groups(plan, self._dev("plan"), self._scratch)
            res = self._outputs(out, dev)
            PU.train_select(self.counts, B, self.caps, self.sel, res["n_valid"], res["overflow"])
            a = PU._TrainSampleArgs(
                self.sel.data_ptr(), self.counts.data_ptr(), self.crops[0].data_ptr(), self.crops[1].data_ptr(), self.crops[2].data_ptr(),
                self.caps[0], self.caps[1], self.caps[2], J, B, M, N, idx_t, idx_s, self.seed & 0xffffffff, self.counter & 0xffffffff,
                self._search_box.data_ptr(), self._model_box.data_ptr(), self._cand_label.data_ptr(), self._cand_size.data_ptr(),
                res["template_points"].data_ptr(), res["search_points"].data_ptr(), res["seg_label"].data_ptr(),
                res["box_label"].data_ptr(), res["bbox_size"].data_ptr(), self._bc_boxes.data_ptr() if self.box_aware else None,
                self.used_t.data_ptr() if self.record_indices else None, self.used_s.data_ptr() if self.record_indices else None)
            PU.train_sample(a, dev)
            if self.box_aware:
                for w, (pts, key) in enumerate(((res["template_points"], "points2cc_dist_t"), (res["search_points"], "points2cc_dist_s"))):
                    b = self._bc_boxes[w]
                    PU.boxcloud_into(res[key], pts, b[:3 * B], b[3 * B:6 * B], b[6 * B:])
        self.counter += 1
        return res

    def _outputs(self, out, dev):
        B, M, N = self.B, self.M, self.N
        shapes = {"template_points": ((B, M, 3), torch.float32), "search_points": ((B, N, 3), torch.float32),
                  "box_label": ((B, 4), torch.float32), "bbox_size": ((B, 3), torch.float32), "seg_label": ((B, N), torch.float32)}
        if self.box_aware:
            shapes.update(points2cc_dist_t=((B, M, 9), torch.float32), points2cc_dist_s=((B, N, 9), torch.float32))
        shapes.update(n_valid=((1,), torch.int32), overflow=((1,), torch.int32))
        res = {}
        for k, (shape, dtype) in shapes.items():
            t = out.get(k) if out is not None else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape, k
            res[k] = t
        return res


class DeviceBatchSampler:
    """An iterator of training dicts with the frame choice of PointTrackingSampler.__getitem__ (sampler.py:218-237): with
    random_sample, a random tracklet and frames (0, two distinct random frames); otherwise the annotations in order, frames
    (0, max(this - 1, 0), this).  The candidate id is index % num_candidates.  Every batch is over-provisioned to the
    builder's J candidates, so that invalid ones (too few points) are skipped on the device."""

    def __init__(self, tracklets, builder, random_sample=False, seed=0, sample_per_epoch=10000):
        self.tracklets, self.builder, self.random_sample = tracklets, builder, bool(random_sample)
        self.rng = np.random.default_rng(int(seed))
        self.num_candidates = builder.num_candidates
        self.starts = np.concatenate([[0], np.cumsum([len(t) for t in tracklets])])
        self.length = (int(sample_per_epoch) if self.random_sample else int(self.starts[-1])) * self.num_candidates
        self.index = 0

    def __len__(self):
        return self.length // self.builder.J

    def sample(self, index):
        """-> (tracklet, first, template, search, candidate_id) of sample `index`"""
        anno, cand = index // self.num_candidates, index % self.num_candidates
        if self.random_sample:
            trk = self.tracklets[int(self.rng.integers(0, len(self.tracklets)))]
            a, b = (self.rng.choice(len(trk), size=2, replace=False) if len(trk) > 1 else (0, 0))
            return trk, 0, int(a), int(b), cand
        t = int(np.searchsorted(self.starts, anno, side="right")) - 1
        this = anno - int(self.starts[t])
        return self.tracklets[t], 0, max(this - 1, 0), this, cand

    def __iter__(self):
        self.index = 0
        return self

    def __next__(self):
        J = self.builder.J
        if self.index + J > self.length:
            raise StopIteration
        samples = [self.sample(self.index + i) for i in range(J)]
        self.index += J
        return self.builder.build(samples)
