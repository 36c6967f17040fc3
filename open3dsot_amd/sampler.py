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

M2-Track's batches (MotionTrackingSampler + motion_processing, sampler.py:82-180,262-288, with apply_augmentation,
points_utils.py:299-361) come from MotionBatchBuilder: one pinned upload and ten launches with augmentation and BoxCloud

    o3d_train_augment            apply_transform for both frames' boxes, and the records that move the points (K = 2J)
    o3d_track_offset_box_multi   the jittered reference box of every candidate
    o3d_train_motion_labels      the three transform_box, the three labels, motion_state_label, bbox_size
    o3d_track_crop_groups_aug (3)  both crops and the in-box count of every candidate, every frame read once
    o3d_train_select_motion      which candidates fill the batch
    o3d_train_motion_sample      regularize_pc of both halves, the five point channels, candidate_bc, seg_label, the label rows
    o3d_boxcloud (2, box_aware)  prev_bc / this_bc

The planned epoch (DeviceBatchSampler(plan_batches=P)): the epoch's order (epoch_order: shuffled like
the reference's DataLoader) and frame choice are made for all samples at once, the tables of P batches travel in one pinned
copy (plan_chunk), and a batch is build_planned: no per-batch upload, no numpy Generator, and one launch in front of the ones
above

    o3d_train_draw               the candidates' boxes gathered from the resident pool; the box jitter, the search offset and
                                 the augmentation drawn with the keyed generator of the resampling indices

Not covered (DESIGN.md sections 13, 13b): use_augmentation for the siamese builder (a small follow-up now: one more fixture and
the search frame's record only).  Real data arrives through datasets.KittiTracklets, which is a
DeviceTracklets.
"""
import math

import numpy as np
import torch

from . import points_utils as PU
from .crop_plan import FramePool, Tables, _section, plan_groups, upload

# the data keys of cfgs/BAT_Car.yaml:5-15,23 (P2B_Car.yaml: the same but box_aware False)
DATA_KEYS = dict(search_bb_scale=1.25, search_bb_offset=2, model_bb_scale=1.25, model_bb_offset=0, template_size=512,
                 search_size=1024, degrees=True, box_aware=True, num_candidates=4, data_limit_box=False, use_augmentation=False)
DEFAULT_CAPACITY = (4096, 4096, 16384)       # rows of the first-frame, template-frame and search crop buffers
# the data keys of cfgs/M2_track_kitti.yaml:5-8,10,17-20,24
MOTION_DATA_KEYS = dict(bb_scale=1.25, bb_offset=2, point_sample_size=1024, degrees=False, data_limit_box=True, num_candidates=4,
                        motion_threshold=0.15, use_augmentation=True, box_aware=True)
DEFAULT_MOTION_CAPACITY = (16384, 16384)     # rows of the previous-frame and current-frame crop buffers


def _cfg(config, key, defaults=DATA_KEYS):
    if isinstance(config, dict):
        return config.get(key, defaults[key])
    return getattr(config, key, defaults[key])


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


# ---- the planned epoch: order, frame choice and the tables of P batches, all whole-array numpy (no device) -------------------
def epoch_order(length, J, shuffle, seed, epoch, rank=0, world=1):
    """-> (n_batches, J) int64 sample indices of `rank`'s batches of epoch `epoch`.  shuffle=False: arange; True:
    default_rng([seed, epoch]).permutation(length) -- DataLoader(shuffle=True, drop_last=True), main.py:75.  Either is cut to
    whole batches of J and to a whole number of rounds over the ranks; every rank computes the same order and takes batches
    rank, rank + world, ... (no collective)."""
    length, J, world = int(length), int(J), int(world)
    if not (J >= 1 and 0 <= rank < world):
        raise ValueError("epoch_order: J >= 1 and 0 <= rank < world")
    order = np.random.default_rng([int(seed), int(epoch)]).permutation(length) if shuffle else np.arange(length)
    n = length // J // world * world
    return order[:n * J].astype(np.int64).reshape(n, J)[rank::world]


def epoch_frames(index, starts, num_candidates, motion, draw=None):
    """The frame choice of PointTrackingSampler / MotionTrackingSampler.__getitem__ for an array of sample indices ->
    (tracklet, frames, candidate id): frames (..., 3) = (0, max(this - 1, 0), this), or (..., 2) = (max(this - 1, 0), this)
    with `motion`; the annotations in order.  draw = random_draw(...)'s arrays: (0, two distinct random frames) of a random
    tracklet instead, sample i taking entry i of the draw."""
    index = np.asarray(index, np.int64)
    anno, cand = index // num_candidates, index % num_candidates
    if draw is not None:
        t, a, b = (d[index] for d in draw)
        return t, np.stack([np.zeros_like(a), a, b], -1), cand
    t = np.searchsorted(starts, anno, side="right") - 1
    this = anno - np.asarray(starts, np.int64)[t]
    prev = np.maximum(this - 1, 0)
    return t, np.stack([prev, this] if motion else [np.zeros_like(this), prev, this], -1), cand


def random_draw(lengths, count, seed, epoch):
    """random_sample for a whole epoch at once, from default_rng([seed, epoch, 1]): per sample a tracklet and two distinct
    frames of it ((0, 0) for a one-frame tracklet) -> (tracklet, a, b), three (count,) int64 arrays"""
    rng = np.random.default_rng([int(seed), int(epoch), 1])
    lengths = np.asarray(lengths, np.int64)
    t = rng.integers(0, len(lengths), count)
    n = lengths[t]
    a = rng.integers(0, n)
    b = (a + 1 + rng.integers(0, np.maximum(n - 1, 1))) % n          # a + 1 .. a + n - 1 (mod n): never a again, unless n == 1
    return t, a, b


class ChunkTables(Tables):
    """The tables of P planned batches of J candidates (crop_plan.Tables: one host buffer, one copy; `base` is the address of
    that copy).  Views, batch-major: rows (P,J,cols) and cand (P,J) int32, targets (P,3J) CROP_TARGET, plan (P,3J) CROP_PLAN of
    which batch k uses the first groups[k], and with `aug` slots (P,3J) int32 / augptr (P,3J) uint64.  need[k] = batch k's
    scratch length, grid[k] = its workgroups of the count / scatter launches."""

    def __init__(self, P, J, cols, aug=False, base=0):
        self.J, self.cols, self.aug = int(J), int(cols), bool(aug)
        n_rec = 3 * self.J
        sections = {"rows": (np.int32, (self.J, self.cols)), "cand": (np.int32, (self.J,))}
        if self.aug:
            sections.update(slots=(np.int32, (n_rec,)), augptr=(np.uint64, (n_rec,)))
        sections.update(targets=(PU.CROP_TARGET, (n_rec,)), plan=(PU.CROP_PLAN, (n_rec,)))
        super().__init__(P, sections, base)
        for name in sections:
            setattr(self, name, self.view(name))
        self.groups, self.need, self.grid = (np.zeros(self.P, np.int64) for _ in range(3))


def plan_chunk(chunk, fptr, fn, rows, cand, rec, crop_cols, aug_base=None):
    """Fill `chunk` for S <= P batches (crop_plan.plan_groups: whole-chunk numpy, a pure function of integer arrays).  fptr, fn:
    per pool row the frame's address and size; rows (S,J,cols) the pool rows of the candidates' frames, cand (S,J) their ids;
    rec (3,J) the builder's fixed CROP_TARGET records; crop c of candidate j reads frame rows[:, j, crop_cols[c]].  Every
    distinct frame of a batch is one group that holds the targets reading it, the groups in the order of their pool rows.
    aug_base: the address of the builder's CROP_AUG records -> slots (the record of target slot i: -1 for crop 0, else
    (c - 1) J + j) and augptr (per group: its first record)."""
    rows, cand = np.asarray(rows, np.int64), np.asarray(cand, np.int64)
    S, J = rows.shape[0], chunk.J
    assert S <= chunk.P and rows.shape == (S, J, chunk.cols) and cand.shape == (S, J) and rec.shape == (3, J)
    chunk.rows[:S], chunk.cand[:S] = rows, cand
    frame = rows[:, :, list(crop_cols)].transpose(0, 2, 1).reshape(S, 3 * J)        # of crop (c, j), at c J + j
    chunk.groups[:S], chunk.need[:S], chunk.grid[:S], order = plan_groups(frame, frame, rec.reshape(-1), fptr, fn, chunk.targets,
                                                                          chunk.plan, chunk.dev("targets"))
    if aug_base is not None:
        c, j = order // J, order % J
        chunk.slots[:S] = np.where(c == 0, -1, (c - 1) * J + j)
        chunk.augptr[:S] = int(aug_base) + PU.CROP_AUG.itemsize * chunk.plan["row_start"][:S].astype(np.int64)


class _DeviceBatchBuilder:
    """What SiameseBatchBuilder and MotionBatchBuilder share: the over-provisioned sizes, the two-slot pinned staging buffer
    and its sections, the crop tables of a batch (every distinct frame one group) and the output dict"""

    def _init_sizes(self, batch_size, candidates, seed, record_indices):
        self.B = int(batch_size)
        self.J = int(candidates) if candidates is not None else int(math.ceil(1.25 * self.B))
        if not 1 <= self.B <= self.J <= PU.TRAIN_MAX_CANDIDATES:
            raise ValueError("1 <= batch_size <= candidates <= %d" % PU.TRAIN_MAX_CANDIDATES)
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        self.counter = 0
        self.record_indices = bool(record_indices)
        self.device = None

    def _allocate_staging(self, lay, dev):
        self.device = dev
        self._layout = lay
        self._up = torch.empty(lay["_end"], dtype=torch.uint8, device=dev)
        self._pinned = [torch.empty(lay["_end"], dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._events = [torch.cuda.Event() for _ in range(2)]
        self._used = [False, False]

    def _view(self, slot, name, dtype, shape):
        off, nbytes = self._layout[name]
        return self._pinned[slot].numpy()[off:off + nbytes].view(dtype).reshape(shape)

    def _dev(self, name):
        return self._up.data_ptr() + self._layout[name][0]

    def _dev32(self, name, count):
        """the first `count` float32 of section `name` of the uploaded buffer, as a tensor"""
        o = self._layout[name][0] // 4
        return self._up.view(torch.float32)[o:o + count]

    def _begin(self, samples):
        """-> (device, stream, slot) of this build; allocates on the first one, waits for the slot's upload of two builds ago"""
        if len(samples) != self.J:
            raise ValueError("build() takes %d candidates, got %d" % (self.J, len(samples)))
        dev = samples[0][0].frames[0].device
        if self.device is None:
            with torch.cuda.device(dev):
                self._allocate(dev)
        assert dev == self.device
        slot = self.counter & 1
        if self._used[slot]:
            self._events[slot].synchronize()          # the upload of two builds ago: long done in a running loop
        return dev, torch.cuda.current_stream(dev), slot

    def _crop_tables(self, slot, samples):
        """-> (the planned CROP_PLAN rows of this batch in the pinned slot, order): crop c of candidate j reads frame
        crop_cols[c] of its sample; every distinct (tracklet, frame) is one group, the groups in the order in which the
        candidates first read them, and a group's targets are self._rec[c, j] of the crops that read it, in the order of the
        candidates (target slot i holds crop order[i] = j C + c)"""
        wanted = [(s[0], s[1 + col]) for s in samples for col in self.crop_cols]
        clouds = {}
        for trk, f in wanted:
            clouds.setdefault((id(trk), f), trk.frames[f])
        ids = {at: i for i, at in enumerate(clouds)}
        key = np.array([[ids[id(trk), f] for trk, f in wanted]], np.int64)
        pool = FramePool([clouds.values()])
        n_rec = key.shape[1]
        plan = self._view(slot, "plan", PU.CROP_PLAN, (1, n_rec))
        groups, need, _, order = plan_groups(key, key, self._rec.T.reshape(-1), pool.fptr, pool.fn,
                                             self._view(slot, "targets", PU.CROP_TARGET, (1, n_rec)), plan, self._dev("targets"))
        self.reserve_scratch(int(need[0]))
        return plan[0, :groups[0]], order[0]

    def _upload(self, slot, nbytes, stream):
        self._up[:nbytes].copy_(self._pinned[slot][:nbytes], non_blocking=True)       # THE upload of this batch
        self._events[slot].record(stream)
        self._used[slot] = True

    # ---- the planned route (DeviceBatchSampler(plan_batches=P) drives it) -------------------------------------------------------------
    def bind(self, tracklets):
        """The resident state of the planned route, made once: every tracklet's boxes end to end in one device pool `_gt` (R,15)
        (tracklet t owns rows [row0[t], row0[t + 1])), per pool row the frame's address and size, the fixed buffers that
        o3d_train_draw writes and the target records that point at them"""
        frames = [x for t in tracklets for x in t.frames]
        dev = frames[0].device
        if self.device is None:
            with torch.cuda.device(dev):
                self._allocate(dev)
        assert dev == self.device
        self._bound = tracklets                            # the frames stay alive as long as their addresses are planned
        self._pool = FramePool([t.frames for t in tracklets])
        self.row0 = self._pool.row0
        with torch.cuda.device(dev):
            self._gt = torch.from_numpy(np.concatenate([t.boxes for t in tracklets])).to(dev)
            self._bind_buffers(dev)

    def reserve_scratch(self, need):
        if self._scratch.numel() < need:
            with torch.cuda.device(self.device):
                self._scratch = torch.empty(int(need), dtype=torch.int32, device=self.device)

    def plan(self, chunk, rows, cand):
        """plan_chunk for this builder's records: rows (S,J,cols) pool rows, cand (S,J) -> the chunk's host tables"""
        plan_chunk(chunk, self._pool.fptr, self._pool.fn, rows, cand, self._rec_planned, self.crop_cols,
                   self._aug.data_ptr() if getattr(self, "augment", False) else None)

    def draws(self):
        """what o3d_train_draw wrote for the last planned build: {refs, first, offs, aug} device tensors (None where the
        builder has none); the next planned build overwrites them"""
        return {"refs": self._p_refs, "first": self._p_first, "offs": self._p_offs, "aug": self._p_aug}

    def _outputs(self, out, dev):
        res = {}
        for k, (shape, dtype) in self._shapes().items():
            t = out.get(k) if out is not None else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape, k
            res[k] = t
        return res


class SiameseBatchBuilder(_DeviceBatchBuilder):
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
        self._init_sizes(batch_size, candidates, seed, record_indices)
        self.caps = tuple(int(c) for c in ((capacity,) * 3 if isinstance(capacity, int) else capacity))
        assert len(self.caps) == 3 and min(self.caps) >= 1
        self.M, self.N = int(_cfg(config, "template_size")), int(_cfg(config, "search_size"))
        self.degrees, self.box_aware = bool(_cfg(config, "degrees")), bool(_cfg(config, "box_aware"))
        self.limit_box = bool(_cfg(config, "data_limit_box"))
        self.num_candidates = int(_cfg(config, "num_candidates"))
        self.scales = (float(_cfg(config, "model_bb_scale")), float(_cfg(config, "model_bb_offset")),
                       float(_cfg(config, "search_bb_scale")), float(_cfg(config, "search_bb_offset")))

    # ---- buffers (allocated once, on the first build) ---------------------------------------------------------------------------------
    def _allocate(self, dev):
        J, B, M, N = self.J, self.B, self.M, self.N
        lay = {"_end": 0}
        _section(lay, "refs", 2 * J * 60)             # rows [0, J): the template frame's box, [J, 2J): the search frame's
        _section(lay, "offs", 2 * J * 16)             # (x, y, 0, theta) of the two jitters
        _section(lay, "first", J * 60)                # the first frame's box
        _section(lay, "targets", 3 * J * PU.CROP_TARGET.itemsize)
        _section(lay, "plan", 3 * J * PU.CROP_PLAN.itemsize)
        self._base_bytes = lay["_end"]
        _section(lay, "idx_t", J * M * 4)             # teacher-forced builds only
        _section(lay, "idx_s", J * N * 4)
        self._allocate_staging(lay, dev)

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
        dev, stream, slot = self._begin(samples)
        refs = self._view(slot, "refs", np.float32, (2 * J, 15))
        offs = self._view(slot, "offs", np.float32, (2 * J, 4))
        first = self._view(slot, "first", np.float32, (J, 15))
        if draws is None:
            off_t, off_s = self.draw_offsets([s[4] for s in samples])
        else:
            off_t, off_s = np.asarray(draws["offset_t"], np.float64), np.asarray(draws["offset_s"], np.float64)
            assert off_t.shape == (J, 3) and off_s.shape == (J, 3)
        offs[:] = 0
        offs[:J, :2], offs[:J, 3] = off_t[:, :2], off_t[:, 2]
        offs[J:, :2], offs[J:, 3] = off_s[:, :2], off_s[:, 2]
        for j, (trk, f0, f1, f2, _) in enumerate(samples):
            first[j], refs[j], refs[J + j] = trk.boxes[f0], trk.boxes[f1], trk.boxes[f2]
        plan = self._crop_tables(slot, samples)[0]              # the groups: every distinct frame once, with the crops that read it
        nbytes = self._base_bytes
        idx_t = idx_s = None
        if draws is not None and draws.get("idx_t") is not None:
            self._view(slot, "idx_t", np.int32, (J, M))[:] = draws["idx_t"]
            self._view(slot, "idx_s", np.int32, (J, N))[:] = draws["idx_s"]
            nbytes = self._layout["_end"]
            idx_t, idx_s = self._dev("idx_t"), self._dev("idx_s")
        with torch.cuda.device(dev):
            self._upload(slot, nbytes, stream)
            return self._launch(self._dev32("refs", 2 * J * 15), self._dev32("offs", 2 * J * 4), plan, self._dev("plan"), idx_t, idx_s, out, dev)

    def _launch(self, refs_d, offs_d, plan, dev_plan, idx_t, idx_s, out, dev):
        """the launches of a build behind its tables, shared by build() and build_planned(): refs_d (2J*15), offs_d (2J*4) on
        the device, plan = the batch's planned CROP_PLAN rows on the host and dev_plan their device copy"""
        J, B, M, N = self.J, self.B, self.M, self.N
        PU.offset_box_multi(refs_d, offs_d, out=self._jit, degrees=self.degrees, use_z=False, limit_box=self.limit_box,
                            seed=(self.seed + 7919 * self.counter) & 0x3fffffff)
        PU.train_labels(refs_d[J * 15:], self._jit[J:], self._jit[:J], offs_d[J * 4:], self._search_box, self._cand_label,
                        self._cand_size, self._model_box)
        PU.crop_groups(plan, dev_plan, self._scratch)
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

    # ---- the planned route ------------------------------------------------------------------------------------------------------------
    crop_cols = (0, 1, 2)                                  # crop c of a candidate reads the frame of column crop_cols[c] of `rows`

    def _bind_buffers(self, dev):
        J = self.J
        self._p_refs, self._p_first = (torch.zeros((n, 15), dtype=torch.float32, device=dev) for n in (2 * J, J))
        self._p_offs, self._p_aug = torch.zeros((2 * J, 4), dtype=torch.float32, device=dev), None
        self._rec_planned = self._rec.copy()
        self._rec_planned["box"][0] = self._p_first.data_ptr() + 60 * np.arange(J, dtype=np.uint64)

    def build_planned(self, chunk, k, out=None):
        """batch k of the uploaded `chunk` (a ChunkTables that plan_chunk filled, its device copy at chunk.base): o3d_train_draw,
        then build()'s launches.  No numpy Generator, no pinned write, no upload, no synchronisation."""
        J, dev = self.J, self.device
        with torch.cuda.device(dev):
            PU.train_draw(self._gt, chunk.dev("rows", k), chunk.dev("cand", k), J, self.seed & 0xffffffff, self.counter & 0xffffffff,
                          self.degrees, self.num_candidates, PU.TRAIN_DRAW_SIAMESE, self._p_refs, self._p_first, self._p_offs, None)
            return self._launch(self._p_refs.view(-1), self._p_offs.view(-1), chunk.plan[k, :chunk.groups[k]], chunk.dev("plan", k),
                                None, None, out, dev)

    def _shapes(self):
        B, M, N = self.B, self.M, self.N
        shapes = {"template_points": ((B, M, 3), torch.float32), "search_points": ((B, N, 3), torch.float32),
                  "box_label": ((B, 4), torch.float32), "bbox_size": ((B, 3), torch.float32), "seg_label": ((B, N), torch.float32)}
        if self.box_aware:
            shapes.update(points2cc_dist_t=((B, M, 9), torch.float32), points2cc_dist_s=((B, N, 9), torch.float32))
        shapes.update(n_valid=((1,), torch.int32), overflow=((1,), torch.int32))
        return shapes


class MotionBatchBuilder(_DeviceBatchBuilder):
    """build(samples) -> the M2-Track training dict: points (B,2N,5), seg_label (B,2N) int64, box_label / box_label_prev /
    motion_label (B,4), motion_state_label (B,) int64 and, with box_aware, candidate_bc (B,2N,9), prev_bc / this_bc (B,N,9) --
    the keys, shapes and dtypes of synth.make_motion_batch -- plus bbox_size (B,3), n_valid (1,) and overflow (1,) int32, all
    device tensors.  The contract is SiameseBatchBuilder's: J = `candidates` (default ceil(1.25 B)) samples (tracklet, prev,
    this: frame indices, candidate_id) per batch, of which the first B valid ones fill it (valid iff the reference's two
    assertions hold: more than 10 points of the un-augmented previous frame inside its box, more than 20 points in the current
    crop, sampler.py:99,120); fixed crop buffers capacity = (prev, this) with `overflow`; two-slot pinned staging; out=.

    draws: {offset (J,3), aug_prev (J,6), aug_this (J,6), idx_prev (J,N), idx_this (J,N)} teacher-forces the box jitter, the
    augmentation (tx, ty, tz, rotation in degrees, flip_x, flip_y per frame) and the resampling indices.  Without it the
    offsets and the augmentation come from a numpy Generator seeded with `seed` (offset: uniform +-0.3 with the angle x5
    degrees or x deg2rad(5), zero for candidate_id 0, sampler.py:106-110; per (candidate, frame): translation uniform +-0.3,
    rotation uniform +-10 degrees, two fair booleans, points_utils.py:353-355 -- the two frames are drawn independently even
    when they are the same frame, as the reference draws them) and the indices are drawn on the device.

    The attributes sel (B,), counts (J,3) = (in-box, previous crop, current crop), crops and, with record_indices, used_prev /
    used_this (B,N) show the last build's intermediate results."""
    motion = True

    def __init__(self, config, batch_size, candidates=None, capacity=DEFAULT_MOTION_CAPACITY, seed=0, record_indices=False):
        self._init_sizes(batch_size, candidates, seed, record_indices)
        self.caps = tuple(int(c) for c in ((capacity,) * 2 if isinstance(capacity, int) else capacity))
        assert len(self.caps) == 2 and min(self.caps) >= 1

        def cfg(key):
            return _cfg(config, key, MOTION_DATA_KEYS)
        self.N = int(cfg("point_sample_size"))
        self.degrees, self.box_aware = bool(cfg("degrees")), bool(cfg("box_aware"))
        self.limit_box, self.augment = bool(cfg("data_limit_box")), bool(cfg("use_augmentation"))
        self.num_candidates = int(cfg("num_candidates"))
        self.scale, self.offset = float(cfg("bb_scale")), float(cfg("bb_offset"))
        self.motion_threshold = float(cfg("motion_threshold"))

    def _allocate(self, dev):
        J, B, N = self.J, self.B, self.N
        lay = {"_end": 0}
        _section(lay, "refs", 2 * J * 60)             # rows [0, J): the previous frame's box, [J, 2J): the current frame's
        _section(lay, "offs", J * 16)                 # (x, y, 0, theta) of the jitter
        _section(lay, "aug", 2 * J * 24)              # the augmentation draws, rows as refs
        _section(lay, "cand", J * 4)                  # candidate_id
        _section(lay, "slots", 3 * J * 4)             # record slot -> row of refs / aug, -1: disabled (the in-box count)
        _section(lay, "augptr", 3 * J * 8)            # per group: its first record
        _section(lay, "targets", 3 * J * PU.CROP_TARGET.itemsize)
        _section(lay, "plan", 3 * J * PU.CROP_PLAN.itemsize)
        self._base_bytes = lay["_end"]
        _section(lay, "idx_prev", J * N * 4)          # teacher-forced builds only
        _section(lay, "idx_this", J * N * 4)
        self._allocate_staging(lay, dev)

        def f32(*shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev)

        def i32(*shape):
            return torch.zeros(shape, dtype=torch.int32, device=dev)
        self._gt_aug, self._ref_box = f32(2 * J, 15), f32(J, 15)
        self._aug = torch.zeros(3 * J * PU.CROP_AUG.itemsize, dtype=torch.uint8, device=dev)
        self._this_box, self._prev_box, self._canon_box = f32(J, 15), f32(J, 15), f32(J, 15)
        self._cand_label, self._cand_label_prev, self._cand_motion = f32(J, 4), f32(J, 4), f32(J, 4)
        self._cand_state, self._cand_size = i32(J), f32(J, 3)
        self.counts = i32(J, 3)
        self.crops = tuple(f32(J, c, 3) for c in self.caps)
        self.sel = i32(B)
        self._bc_boxes, self._xyz = f32(2, 15 * B), f32(2, B, N, 3)
        self.used_prev = i32(B, N) if self.record_indices else None
        self.used_this = i32(B, N) if self.record_indices else None
        self._scratch = i32(1 << 16)
        # the target record c of candidate j: 0 = the in-box count of the previous frame (count only), 1 / 2 = the crops
        rec = np.zeros((3, J), PU.CROP_TARGET)
        j = np.arange(J, dtype=np.uint64)
        rec["box"][0] = self._dev("refs") + 60 * j
        rec["scale"][0], rec["offset"][0], rec["capacity"][0] = 1.0, 0.0, 0
        for c in (1, 2):
            rec["box"][c] = self._ref_box.data_ptr() + 60 * j
            rec["scale"][c], rec["offset"][c] = self.scale, self.offset
            rec["out"][c] = self.crops[c - 1].data_ptr() + 12 * self.caps[c - 1] * j
            rec["capacity"][c] = self.caps[c - 1]
        for c in range(3):
            rec["mode"][c] = PU.CROP_SUBWINDOW
            rec["count"][c] = self.counts.data_ptr() + 12 * j + 4 * c
        self._rec = rec

    def draw_offsets(self, candidate_ids):
        """the host draw of the box jitter of J candidates -> offset (J,3) float64"""
        J = len(candidate_ids)
        off = self.rng.uniform(-0.3, 0.3, (J, 3))
        off[:, 2] *= 5.0 if self.degrees else float(np.deg2rad(5))
        off[np.asarray(candidate_ids) == 0] = 0.0
        return off

    def draw_augmentation(self, J):
        """the host draw of apply_augmentation for both frames of J candidates -> (aug_prev, aug_this) (J,6) float64 = (tx,
        ty, tz, rotation in degrees, flip_x, flip_y)"""
        a = np.concatenate([self.rng.uniform(-0.3, 0.3, (2, J, 3)), self.rng.uniform(-10.0, 10.0, (2, J, 1)),
                            self.rng.integers(0, 2, (2, J, 2)).astype(np.float64)], 2)
        return a[0], a[1]

    def build(self, samples, draws=None, out=None):
        J, B, N = self.J, self.B, self.N
        dev, stream, slot = self._begin(samples)
        refs = self._view(slot, "refs", np.float32, (2 * J, 15))
        offs = self._view(slot, "offs", np.float32, (J, 4))
        cand = self._view(slot, "cand", np.int32, (J,))
        ids = [s[3] for s in samples]
        off = self.draw_offsets(ids) if draws is None else np.asarray(draws["offset"], np.float64)
        assert off.shape == (J, 3)
        offs[:] = 0
        offs[:, :2], offs[:, 3] = off[:, :2], off[:, 2]
        cand[:] = ids
        if self.augment:
            aug = self._view(slot, "aug", np.float32, (2 * J, 6))
            aug[:J], aug[J:] = self.draw_augmentation(J) if draws is None else (draws["aug_prev"], draws["aug_this"])
        for j, (trk, f1, f2, _) in enumerate(samples):
            refs[j], refs[J + j] = trk.boxes[f1], trk.boxes[f2]
        plan, order = self._crop_tables(slot, samples)
        if self.augment:
            self._aug_tables(slot, plan, order)
        nbytes = self._base_bytes
        idx_prev = idx_this = None
        if draws is not None and draws.get("idx_prev") is not None:
            self._view(slot, "idx_prev", np.int32, (J, N))[:] = draws["idx_prev"]
            self._view(slot, "idx_this", np.int32, (J, N))[:] = draws["idx_this"]
            nbytes = self._layout["_end"]
            idx_prev, idx_this = self._dev("idx_prev"), self._dev("idx_this")
        with torch.cuda.device(dev):
            self._upload(slot, nbytes, stream)
            aug_d = slots_d = None
            if self.augment:
                s0 = self._layout["slots"][0] // 4
                aug_d, slots_d = self._dev32("aug", 2 * J * 6), self._up.view(torch.int32)[s0:s0 + 3 * J]
            return self._launch(self._dev32("refs", 2 * J * 15), self._dev32("offs", J * 4), aug_d, slots_d, self._dev("augptr"),
                                self._dev("cand"), plan, self._dev("plan"), idx_prev, idx_this, out, dev)

    def _aug_tables(self, slot, plan, order):
        """slots (the record of target slot i: -1 for the in-box count, else (c - 1) J + j) and augptr (per group: its first
        record) of a batch, as plan_chunk writes them"""
        c, j = order % 3, order // 3
        self._view(slot, "slots", np.int32, (3 * self.J,))[:] = np.where(c == 0, -1, (c - 1) * self.J + j)
        self._view(slot, "augptr", np.uint64, (3 * self.J,))[:len(plan)] = self._aug.data_ptr() + PU.CROP_AUG.itemsize * plan["row_start"].astype(np.int64)

    def _launch(self, gt, offs_d, aug_d, slots_d, augptr_d, cand_d, plan, dev_plan, idx_prev, idx_this, out, dev):
        """the launches of a build behind its tables, shared by build() and build_planned(): gt (2J*15), offs_d (J*4), aug_d
        (2J*6) on the device; slots_d = the record slots (a tensor or an address), augptr_d, cand_d, dev_plan = addresses"""
        J, B, N = self.J, self.B, self.N
        if self.augment:
            PU.train_augment(gt, aug_d, self._gt_aug, self._aug, slots_d, n_slots=3 * J)
            gt = self._gt_aug.view(-1)
        PU.offset_box_multi(gt[:J * 15], offs_d, out=self._ref_box, degrees=self.degrees, use_z=False,
                            limit_box=self.limit_box, seed=(self.seed + 7919 * self.counter) & 0x3fffffff)
        PU.train_motion_labels(gt[:J * 15], gt[J * 15:], self._ref_box, self.degrees, self.motion_threshold, self._this_box,
                               self._prev_box, self._canon_box, self._cand_label, self._cand_label_prev, self._cand_motion,
                               self._cand_state, self._cand_size)
        if self.augment:
            PU.crop_groups_aug(plan, dev_plan, augptr_d, self._scratch)
        else:
            PU.crop_groups(plan, dev_plan, self._scratch)
        res = self._outputs(out, dev)
        PU.train_select_motion(self.counts, B, self.caps, self.sel, res["n_valid"], res["overflow"])
        bc = self.box_aware
        a = PU._TrainMotionSampleArgs(
            self.sel.data_ptr(), self.counts.data_ptr(), self.crops[0].data_ptr(), self.crops[1].data_ptr(), self.caps[0],
            self.caps[1], J, B, N, idx_prev, idx_this, cand_d, self.seed & 0xffffffff, self.counter & 0xffffffff,
            self._prev_box.data_ptr(), self._this_box.data_ptr(), self._canon_box.data_ptr(), self._cand_label.data_ptr(),
            self._cand_label_prev.data_ptr(), self._cand_motion.data_ptr(), self._cand_state.data_ptr(), self._cand_size.data_ptr(),
            res["points"].data_ptr(), res["candidate_bc"].data_ptr() if bc else None, res["seg_label"].data_ptr(),
            res["box_label"].data_ptr(), res["box_label_prev"].data_ptr(), res["motion_label"].data_ptr(),
            res["motion_state_label"].data_ptr(), res["bbox_size"].data_ptr(), self._bc_boxes.data_ptr() if bc else None,
            self._xyz.data_ptr() if bc else None, self.used_prev.data_ptr() if self.record_indices else None,
            self.used_this.data_ptr() if self.record_indices else None)
        PU.train_motion_sample(a, dev)
        if bc:
            for w, key in enumerate(("prev_bc", "this_bc")):
                b = self._bc_boxes[w]
                PU.boxcloud_into(res[key], self._xyz[w], b[:3 * B], b[3 * B:6 * B], b[6 * B:])
        self.counter += 1
        return res

    # ---- the planned route ------------------------------------------------------------------------------------------------------------
    crop_cols = (0, 0, 1)                                  # the in-box count and the previous crop read `prev`, the current crop `this`

    def _bind_buffers(self, dev):
        J = self.J
        self._p_refs, self._p_first = torch.zeros((2 * J, 15), dtype=torch.float32, device=dev), None
        self._p_offs = torch.zeros((J, 4), dtype=torch.float32, device=dev)
        self._p_aug = torch.zeros((2 * J, 6), dtype=torch.float32, device=dev) if self.augment else None
        self._rec_planned = self._rec.copy()
        self._rec_planned["box"][0] = self._p_refs.data_ptr() + 60 * np.arange(J, dtype=np.uint64)

    def build_planned(self, chunk, k, out=None):
        """batch k of the uploaded `chunk` (SiameseBatchBuilder.build_planned): o3d_train_draw, then build()'s launches"""
        J, dev = self.J, self.device
        with torch.cuda.device(dev):
            PU.train_draw(self._gt, chunk.dev("rows", k), chunk.dev("cand", k), J, self.seed & 0xffffffff, self.counter & 0xffffffff,
                          self.degrees, self.num_candidates, PU.TRAIN_DRAW_MOTION_AUG if self.augment else PU.TRAIN_DRAW_MOTION,
                          self._p_refs, None, self._p_offs, self._p_aug)
            return self._launch(self._p_refs.view(-1), self._p_offs.view(-1), self._p_aug.view(-1) if self.augment else None,
                                chunk.dev("slots", k) if self.augment else None, chunk.dev("augptr", k) if self.augment else None,
                                chunk.dev("cand", k), chunk.plan[k, :chunk.groups[k]], chunk.dev("plan", k), None, None, out, dev)

    def _shapes(self):
        B, N = self.B, self.N
        shapes = {"points": ((B, 2 * N, 5), torch.float32), "seg_label": ((B, 2 * N), torch.int64),
                  "box_label": ((B, 4), torch.float32), "box_label_prev": ((B, 4), torch.float32),
                  "motion_label": ((B, 4), torch.float32), "motion_state_label": ((B,), torch.int64),
                  "bbox_size": ((B, 3), torch.float32)}
        if self.box_aware:
            shapes.update(candidate_bc=((B, 2 * N, 9), torch.float32), prev_bc=((B, N, 9), torch.float32),
                          this_bc=((B, N, 9), torch.float32))
        shapes.update(n_valid=((1,), torch.int32), overflow=((1,), torch.int32))
        return shapes


class DeviceBatchSampler:
    """An iterator of training dicts with the frame choice of PointTrackingSampler.__getitem__ (sampler.py:218-237): with
    random_sample, a random tracklet and frames (0, two distinct random frames); otherwise the annotations in order, frames
    (0, max(this - 1, 0), this).  The candidate id is index % num_candidates.  Every batch is over-provisioned to the
    builder's J candidates, so that invalid ones (too few points) are skipped on the device.  With a MotionBatchBuilder the
    frame choice is MotionTrackingSampler's (sampler.py:262-288): the annotations in order, frames (max(this - 1, 0), this);
    random_sample is refused, because the reference forces it off (sampler.py:264).

    plan_batches=P >= 1: the PLANNED epoch.  begin(epoch) makes the epoch's order (epoch_order: with `shuffle` the
    reference's DataLoader(shuffle=True, drop_last=True), rank `rank` of `world` taking every world-th batch) and its frame
    choice for all samples at once, and enqueues the tables of the first P batches as one pinned copy; __next__ only
    launches (builder.build_planned: the boxes and the random draws of a batch are made on the device) and, at a chunk
    boundary, plans and uploads the next P batches.  `uploads` counts the copies of the epoch.  __iter__ begins the next
    epoch (0 first).  Without plan_batches the sampler works batch by batch as it always did."""

    def __init__(self, tracklets, builder, random_sample=False, seed=0, sample_per_epoch=10000, shuffle=False, plan_batches=None,
                 rank=0, world=1):
        self.motion = bool(getattr(builder, "motion", False))
        if self.motion and random_sample:
            raise ValueError("DeviceBatchSampler: MotionTrackingSampler has no random_sample (datasets/sampler.py:264)")
        if plan_batches is None and (shuffle or world != 1):
            raise ValueError("DeviceBatchSampler: shuffle and rank / world belong to the planned epoch (plan_batches=P)")
        if plan_batches is not None and int(plan_batches) < 1:
            raise ValueError("plan_batches must be positive")
        self.tracklets, self.builder, self.random_sample = tracklets, builder, bool(random_sample)
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        self.num_candidates = builder.num_candidates
        self.starts = np.concatenate([[0], np.cumsum([len(t) for t in tracklets])])
        self.length = (int(sample_per_epoch) if self.random_sample else int(self.starts[-1])) * self.num_candidates
        self.index = 0
        self.shuffle, self.rank, self.world = bool(shuffle), int(rank), int(world)
        self.plan_batches = None if plan_batches is None else int(plan_batches)
        self.epoch, self.batches, self.s, self.uploads, self._chunk = -1, 0, 0, 0, None

    def __len__(self):
        if self.plan_batches is not None:
            return self.length // self.builder.J // self.world
        return self.length // self.builder.J

    def sample(self, index):
        """-> (tracklet, first, template, search, candidate_id) of sample `index`; (tracklet, prev, this, candidate_id) with
        a MotionBatchBuilder"""
        anno, cand = index // self.num_candidates, index % self.num_candidates
        if self.random_sample:
            trk = self.tracklets[int(self.rng.integers(0, len(self.tracklets)))]
            a, b = (self.rng.choice(len(trk), size=2, replace=False) if len(trk) > 1 else (0, 0))
            return trk, 0, int(a), int(b), cand
        t = int(np.searchsorted(self.starts, anno, side="right")) - 1
        this = anno - int(self.starts[t])
        if self.motion:
            return self.tracklets[t], max(this - 1, 0), this, cand
        return self.tracklets[t], 0, max(this - 1, 0), this, cand

    # ---- the planned epoch --------------------------------------------------------------------------------------------------------------
    def begin(self, epoch):
        """Plan epoch `epoch` and enqueue the upload of its first chunk -> the number of batches"""
        if self.plan_batches is None:
            raise RuntimeError("DeviceBatchSampler.begin belongs to the planned epoch (plan_batches=P)")
        b, P = self.builder, self.plan_batches
        if getattr(b, "_bound", None) is not self.tracklets:
            b.bind(self.tracklets)
        self.epoch = int(epoch)
        order = epoch_order(self.length, b.J, self.shuffle, self.seed, self.epoch, self.rank, self.world)
        draw = random_draw(np.diff(self.starts), self.length, self.seed, self.epoch) if self.random_sample else None
        self._trk, self._frames, self._cand = epoch_frames(order, self.starts, self.num_candidates, self.motion, draw)
        self._rows = b.row0[self._trk][..., None] + self._frames                   # (n, J, cols): the pool rows
        self.batches, self.s, self.uploads = order.shape[0], 0, 0
        if self._chunk is None:
            with torch.cuda.device(b.device):
                self._chunk = ChunkTables(P, b.J, self._rows.shape[-1], bool(getattr(b, "augment", False)))
                self._tab = torch.zeros(self._chunk.host.size, dtype=torch.uint8, device=b.device)
                self._chunk.base = self._tab.data_ptr()
        if self.batches:
            # the crop scratch of the worst batch, known from the frame sizes
            b.reserve_scratch(b._pool.worst_scratch(self._rows[:, :, list(b.crop_cols)].reshape(self.batches, -1)))
        self._enter(0)
        return self.batches

    def _enter(self, s):
        """what precedes batch s: at a chunk boundary the chunk's plan and its one upload"""
        if s >= self.batches or s % self.plan_batches:
            return
        sl = slice(s, min(s + self.plan_batches, self.batches))
        self.builder.plan(self._chunk, self._rows[sl], self._cand[sl])
        upload(self._chunk, self._tab)
        self.uploads += 1

    def samples(self, s):
        """batch s of the planned epoch as the tuples build() takes (the per-batch route: tests and tools)"""
        return [(self.tracklets[int(t)],) + tuple(int(v) for v in f) + (int(c),)
                for t, f, c in zip(self._trk[s], self._frames[s], self._cand[s])]

    def __iter__(self):
        if self.plan_batches is not None:
            self.begin(self.epoch + 1)
            return self
        self.index = 0
        return self

    def __next__(self, out=None):
        if self.plan_batches is not None:
            if self.s >= self.batches:
                raise StopIteration
            res = self.builder.build_planned(self._chunk, self.s % self.plan_batches, out)
            self.s += 1
            self._enter(self.s)
            return res
        J = self.builder.J
        if self.index + J > self.length:
            raise StopIteration
        samples = [self.sample(self.index + i) for i in range(J)]
        self.index += J
        return self.builder.build(samples)
