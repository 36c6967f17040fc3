"""Track a sequence on the device: the frame loop of MatchingBaseModel.evaluate_one_sequence (models/base_model.py:59-86)
with everything between "a frame arrives" and "the next search region is known" on the GPU.

Per frame t >= 1 (the reference's build_input_dict :240-247 + evaluate_one_sample :44-57):

  o3d_track_crop, one call, two jobs    the search window of frame t by the reference box (generate_subwindow) and the model
                                        crop of frame t-1 by ITS OWN result box (cropAndCenterPC), appended to the bank
  8-byte pinned read-back               the two point counts -- THE ONE HOST SYNC of a frame, see below
  np.random.default_rng(1).choice       the reference's own index draw (regularize_pc, seed=1), twice
  one index upload                      (template_size + search_size) int32 = 6 KB
  o3d_track_resample                    both gathers, straight into the network's static input buffers
  o3d_boxcloud                          the template's BoxCloud against the canonical box (BAT only)
  forward + o3d_best_proposal           replayed as one HIP graph captured once per tracker (eager when the capture fails,
                                        unless O3D_REQUIRE_GRAPH=1)
  o3d_track_offset_box                  getOffsetBB: the new box into the (T,15) results buffer; the host never reads it

Why one sync remains: the reference resamples a crop of n points with `default_rng(1).choice(n, size, replace=size > n)`.
Which indices that call returns depends on n, so index parity with the reference needs n on the host before the draw.  A
device-side sampler removes the sync and changes every index: that is the second mode, below.

sampling="device" (SequenceTracker, MotionSequenceTracker): the free-running loop.  The counts stay
where the crop kernel wrote them, the indices are the keyed draw of the training batches (sample_index in
csrc/track_common.hpp, key = draw_key(seed, 0, 0, cloud), the same key at every frame), and the template bank's {fixed, total}
is device state.  Per frame t >= 1:

  o3d_track_crop, one call, two jobs    the search window into search_buf, the model crop into a staging buffer
  a device copy of the counts           row t of counts_log (T,2) int32; read on request only (counts(), overflow())
  o3d_track_bank_update                 the staged crop into the bank by the shape_aggregation rule; {fixed, total} advances
  o3d_track_resample_drawn              both draws and both gathers, straight into the static inputs
  o3d_boxcloud, forward, o3d_track_offset_box   as above

No copy in either direction and no synchronisation after the first update() (whose graph capture may synchronise).  The price:
every buffer has a fixed capacity (a longer crop keeps its first `capacity` survivors), and the indices are not numpy's -- the
same rule (n <= 2 zero-fills, n == S is the identity, S > n draws with replacement, S < n without), other numbers.

sampling="table" (the same four trackers): that free-running loop with the REFERENCE's indices.  The draw
is a function of (point count, sample size) alone and the count is bounded by a fixed capacity, so the whole function is a table
(capacity + 1, sample size) int32, built once per process with draw_indices and kept in HBM (draw_table); the kernels read row
min(count, capacity) where the "device" mode draws.  As long as no capacity cuts a crop (overflow() == (0, 0, 0)), inputs and
boxes are those of sampling="reference".  Above the C ABI, key and table are two values of ONE argument, the index source of
PU.resample_drawn / motion_input_drawn and their lane forms, which a tracker chooses once, when it is built (draw_src); in the
ABI each o3d_track_*_drawn* entry point named here has a _tabled twin that takes the table.

The test epoch on L lanes (LaneTracker, MotionLaneTracker, evaluate(..., lanes=L)): that free-running
loop L tracklets wide, each lane on its own tracklet's frames.  Which tracklet runs on which lane at which step (lane_schedule),
every crop group and every lane table are host knowledge before the first frame: begin() plans them, uploads them in chunks,
and step() only launches.

K targets of one live scene (SceneTracker, MotionSceneTracker, track_scene, evaluate_scene): that
free-running loop K targets wide on ONE stream of frames that arrive one at a time.  One o3d_track_crop_multi call per frame on
a target table uploaded once, the lane kernels of the test epoch on a lane table that changes on events only, and enroll(): a
slot takes a new object in mid-stream without a host stop.  MultiTargetTracker / MultiMotionTracker stay the K-target loops of
sampling="reference".

The slots' lifecycle on the device (ManagedSceneTracker, ManagedMotionSceneTracker, managed_scene_tracker_for; DESIGN.md section
12j): a scene tracker whose update() also takes the frame's detections as a device tensor.  Two launches after the box update
(o3d_scene_pair_scores, o3d_scene_manage) match detections and tracks, retire the lost slots, enroll the unmatched detections
into free slots and write the next frame's lane table: objects enter and leave without a host stop.  score_mot() /
evaluate_managed_scene() score such a run as multi-object tracking (metrics.ClearMOT).

The template bank: each frame's crop by its own result box is computed once and kept on the device; `shape_aggregation`
(`first`, `previous`, `firstandprevious`, `all`; models/base_model.py:166-195) decides which crops form the template cloud.
"""
import collections
import os

import numpy as np
import torch

from . import capi, points_utils as PU
from .crop_plan import FramePool, Tables, plan_groups, upload

_DEFAULTS = dict(search_bb_scale=1.25, search_bb_offset=2, model_bb_scale=1.25, model_bb_offset=0, template_size=512,
                 search_size=1024, degrees=True, use_z=True, limit_box=False, shape_aggregation="firstandprevious",
                 reference_BB="previous_result")      # cfgs/BAT_Car.yaml :5-10,14,53-57


def _aggregation(name):
    """the branch models/base_model.py:177-194 takes, in its order of tests (substring matches on the upper-cased name)"""
    u = str(name).upper()
    for key in ("FIRSTANDPREVIOUS", "FIRST", "PREVIOUS", "ALL"):
        if key in u:
            return key.lower()
    raise ValueError("shape_aggregation %r: expected first, previous, firstandprevious or all" % (name,))


def draw_indices(num_points, sample_size):
    """regularize_pc's draw (datasets/points_utils.py:24-40 with seed=1) -> int indices, or None for its zero-fill case"""
    if num_points <= 2:
        return None
    if num_points == sample_size:
        return np.arange(num_points)
    return np.random.default_rng(1).choice(num_points, size=sample_size, replace=sample_size > num_points)


SAMPLING = ("reference", "device", "table")
FREE_RUNNING = ("device", "table")


def _sampling(name, multi=None):
    """the `sampling` keyword checked before anything else; multi: the name of a K-target loop, which has no free-running mode yet"""
    if name not in SAMPLING:
        raise ValueError("sampling %r: expected \"reference\", \"device\" or \"table\"" % (name,))
    if multi and name in FREE_RUNNING:
        raise ValueError("%s: sampling=\"%s\" serves the single-target trackers (SequenceTracker, MotionSequenceTracker) and the "
                         "lane trackers; the K-target loops are a follow-up" % (multi, name))
    return name


def draw_table_host(capacity, sample_size):
    """The reference's index draw for EVERY point count up to `capacity`, as one array: (capacity + 1, sample_size) int32, row n
    = draw_indices(n, sample_size) for n > 2 (so row n == sample_size is the identity), rows 0..2 all -1 (the zero-fill case).
    Pure host work, one draw_indices call per row: about a second for the default sizes."""
    capacity, sample_size = int(capacity), int(sample_size)
    if capacity < 1 or sample_size < 1:
        raise ValueError("draw_table: capacity and sample_size must be positive")
    table = np.full((capacity + 1, sample_size), -1, np.int32)
    for n in range(3, capacity + 1):
        table[n] = draw_indices(n, sample_size)
    return table


_DRAW_TABLES = {}


def draw_table(capacity, sample_size, device):
    """draw_table_host on `device`, built and uploaded once per process: the tables are cached by (device, capacity,
    sample_size), so every tracker with the same sizes shares one.  A kernel of sampling="table" indexes it with the
    device-resident point count.  Memory: 4 * (capacity + 1) * sample_size bytes (134 MB for 32768 x 1024 and for 65536 x
    512, the default sizes), until clear_draw_tables()."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, int(capacity), int(sample_size))
    if key not in _DRAW_TABLES:
        _DRAW_TABLES[key] = torch.from_numpy(draw_table_host(capacity, sample_size)).to(device)
    return _DRAW_TABLES[key]


def clear_draw_tables():
    """Forget the cached tables of draw_table (a tracker keeps the ones it holds)."""
    _DRAW_TABLES.clear()


def draw_keys(seed):
    """the two keys of a free-running tracker's index draws: cloud 0 = the template / the previous frame, cloud 1 = the search
    area / the current frame.  They do not change from frame to frame, as the reference's seed=1 makes its indices a function
    of the point count alone."""
    return PU.draw_key(seed, 0, 0, 0), PU.draw_key(seed, 0, 0, 1)


class DrawCache:
    """draw_indices memoised: its result depends on (num_points, sample_size) alone, and a frame of K targets asks for 2K
    draws.  get() -> the int32 indices (read-only, shared between callers) or None for the zero-fill case.  Bounded: the
    least recently used pair goes when `maxsize` pairs are held."""

    def __init__(self, maxsize=2048):
        self.maxsize, self.hits, self.misses = int(maxsize), 0, 0
        self._held = collections.OrderedDict()

    def get(self, num_points, sample_size):
        key = (int(num_points), int(sample_size))
        if key in self._held:
            self.hits += 1
            self._held.move_to_end(key)
            return self._held[key]
        self.misses += 1
        idx = draw_indices(*key)
        if idx is not None:
            idx = idx.astype(np.int32)
            idx.setflags(write=False)
        self._held[key] = idx
        if len(self._held) > self.maxsize:
            self._held.popitem(last=False)
        return idx

    def __len__(self):
        return len(self._held)


def _is_motion(model):
    from .m2track import M2TRACK
    return isinstance(model, M2TRACK)


_OTHER_FAMILY = {      # class -> where the models of the other family go
    "MultiTargetTracker": "the motion tracker follows one target per MotionSequenceTracker, K targets per MultiMotionTracker",
    "MultiMotionTracker": "the matching trackers (BAT, P2B) follow K targets with MultiTargetTracker",
    "LaneTracker": "the motion tracker runs on MotionLaneTracker", "MotionLaneTracker": "the matching trackers run on LaneTracker",
    "SceneTracker": "the motion tracker follows the K targets of a live scene with MotionSceneTracker",
    "MotionSceneTracker": "the matching trackers (BAT, P2B) follow the K targets of a live scene with SceneTracker"}


def _require_family(model, motion, name):
    """class `name` serves one model family: the motion tracker (m2track.M2TRACK) or the matching trackers"""
    if _is_motion(model) != motion:
        family = "motion tracker (M2TRACK)" if motion else "matching trackers (BAT, P2B)"
        raise TypeError("%s serves the %s; %s" % (name, family, _OTHER_FAMILY[name]))


def _reference_rule(reference_BB):
    """the config's reference_BB -> (by_gt, back): under previous_result a frame starts from the tracker's last box; under
    previous_gt / current_gt (by_gt) from the ground-truth box of frame t - back, back = 1 / 0"""
    u = str(reference_BB).upper()
    if not any(k in u for k in ("PREVIOUS_RESULT", "CURRENT_GT", "PREVIOUS_GT")):
        raise ValueError("reference_BB %r" % (reference_BB,))
    by_gt = "PREVIOUS_RESULT" not in u
    return by_gt, 1 if by_gt and "PREVIOUS_GT" in u else 0


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def _score_space(cfg):
    """(dim, up_axis) of estimateOverlap / estimateAccuracy: the config's IoU_space and up_axis, 3 and (0,0,1) when absent"""
    return int(getattr(cfg, "IoU_space", 3)), tuple(getattr(cfg, "up_axis", (0, 0, 1)))


def _boxes15(boxes, device, keep=False):
    """a tensor, an ndarray or a list of boxes as pack_box takes them (an empty one included) -> (n,15) float32, contiguous,
    on `device`; keep: a tensor stays on the device it is on"""
    if torch.is_tensor(boxes) and keep:
        b = boxes.to(torch.float32)
    elif torch.is_tensor(boxes) or isinstance(boxes, np.ndarray):
        b = PU._dev32(boxes, device)
    else:
        b = torch.stack([PU.pack_box(x, device) for x in boxes]) if len(boxes) else torch.zeros((0, 15), device=device)
    return b.reshape(-1, 15).contiguous()


class _DeviceTracker:
    """What the tracking loops share: the box state on the device (the last result box, R0 + accumulated yaw, the canonical
    box's wlh), the (T,15) results buffer with its device-side frame counter, the crop call with the frame's one count
    read-back (and buffer growth when a crop exceeds its capacity), the index staging, the network as a HIP graph captured
    once per tracker (eager when the capture fails, unless O3D_REQUIRE_GRAPH=1) and the one box update (_offset_box).  With
    n_targets = K the per-target state has a leading K axis (`lead`): cur (K,15), yaw_state (K,10), boxes (T,K,15), counts_dev
    (2K,).  Subclasses provide `_update()` and `_forward()` on their static inputs."""
    _NAME = "tracker"

    def __init__(self, model, seed, use_graph, max_frames, defaults, n_targets=None, sampling="reference", record_indices=False):
        self.sampling = _sampling(sampling)
        self.free_running, self.tabled, self.record_indices = sampling in FREE_RUNNING, sampling == "table", bool(record_indices)
        p = next(model.parameters())
        if not p.is_cuda:
            raise RuntimeError("%s: CPU not supported (the model must live on a GPU)" % self._NAME)
        capi.load()
        self.model, self.dev, self.seed = model, p.device, int(seed)
        for k, v in defaults.items():
            setattr(self, k, getattr(model.config, k, v))
        self.use_graph = use_graph
        self.require_graph = os.environ.get("O3D_REQUIRE_GRAPH", "0") == "1"
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.lead = lead = () if n_targets is None else (int(n_targets),)
        self.counts_dev = torch.zeros((2 * (n_targets or 1),), dtype=torch.int32, device=self.dev)
        self.counts_host, self.counts_log = None, None
        if self.free_running:         # the counts stay on the device: row t of counts_log, written by a stream-ordered copy
            self.counts_log = torch.full((int(max_frames),) + lead + (2,), -1, dtype=torch.int32, device=self.dev)
            self.keys = None if self.tabled else draw_keys(self.seed)      # "table": the indices come from draw_table
        else:
            self.counts_host = torch.zeros(self.counts_dev.shape, dtype=torch.int32).pin_memory()
        self.cur = torch.zeros(lead + (15,), **f32)        # the last result box: the next frame's crops read it
        self.yaw_state = torch.zeros(lead + (10,), **f32)
        self.canon_wlh = torch.zeros(lead + (3,), **f32)   # the canonical box: zero centre, this wlh, identity
        self.boxes = torch.zeros((int(max_frames),) + lead + (15,), **f32)
        self.frame = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.scratch = None
        self.graph, self.out, self.graph_failed = None, None, None
        self.t = 0
        self.log = []

    # ---- state -------------------------------------------------------------------------------------------------------------
    def _pack(self, box0):
        return PU.pack_box(box0, self.dev)

    def _restart(self, b, k=Ellipsis, row=True):
        """the last result box (of target k) := b, its yaw state restarted from b's rotation; row: b is also the result of the
        most recent frame"""
        self.cur[k].copy_(b)
        self.yaw_state[k][..., :9].copy_(b[..., 6:15])
        self.yaw_state[k][..., 9] = 0.0
        if row:
            self.boxes[self.t - 1][k].copy_(b)

    def init(self, points0, box0):
        PU._need_gpu(points0, self._NAME + ".init")
        b = self._pack(box0)
        self.t, self.log = 1, []
        self._restart(b)
        self.canon_wlh.copy_(b[..., 3:6])
        self.frame.fill_(1)
        if self.free_running:
            self.counts_log.fill_(-1)
        self.prev_points = points0.contiguous().float()
        return self.boxes[0]

    def set_box(self, box):
        """Overwrite the last result box (re-initialisation from a detector, teacher forcing in the tests): the next update
        crops around it and offsets from it."""
        self._restart(PU.pack_box(box, self.dev))

    def _grow_boxes(self):
        T = self.boxes.shape[0]
        if self.t >= T:
            bigger = torch.zeros((2 * T,) + self.boxes.shape[1:], dtype=torch.float32, device=self.dev)
            bigger[:T].copy_(self.boxes)
            self.boxes = bigger
            if self.free_running:                          # counts_log grows with boxes
                log = torch.full((2 * T,) + self.counts_log.shape[1:], -1, dtype=torch.int32, device=self.dev)
                log[:T].copy_(self.counts_log)
                self.counts_log = log

    def _crop_counts(self, make_jobs):
        """The frame's one crop call + the count read-back.  make_jobs() -> [(crop job, grow)]: the job's count lands in
        counts[j]; grow(n) is called when its n survivors exceed the job's buffer, and the call is made again.  -> counts"""
        def launch():
            jobs = make_jobs()
            self.scratch = PU.crop_jobs([j for j, _ in jobs], self.scratch)
            return [(job[5].shape[0], grow) for job, grow in jobs]
        return self._counts_loop(launch)

    def _counts_loop(self, launch):
        """launch() makes the crop call and -> [(capacity, grow)], one per count in `counts`; the counts are read back (the
        one sync of the frame); where one exceeds its capacity, grow(n) is called once with the largest such n and the call
        is made again.  -> counts"""
        while True:
            caps = launch()
            self.counts_host.copy_(self.counts_dev, non_blocking=True)
            torch.cuda.current_stream(self.dev).synchronize()                    # the one sync of the frame
            ns = self.counts_host[:len(caps)].tolist()
            over = {}                                                            # grow -> its largest overflowing count
            for n, (cap, grow) in zip(ns, caps):
                if n > cap:
                    over[grow] = max(n, over.get(grow, 0))
            if not over:
                return ns
            for grow, n in over.items():                                         # a crop larger than its buffer: grow, crop again
                grow(n)

    def _index_buffers(self, n):
        """idx (n,) int32 on the device and its pinned host copy, which _stage_indices fills and uploads"""
        self.idx = torch.zeros((n,), dtype=torch.int32, device=self.dev)
        self.idx_host = torch.zeros((n,), dtype=torch.int32).pin_memory()

    def _stage_indices(self, *draws):
        """draws: (point count, sample size) pairs.  The reference's own index draw for each (draw_indices), laid end to end
        in idx_host, then ONE upload into idx.  -> per draw, whether it is the zero-fill case (its part of idx is not read)"""
        drawn = [draw_indices(n, size) for n, size in draws]
        at = 0
        for i, (_, size) in zip(drawn, draws):
            if i is not None:
                self.idx_host[at:at + size] = torch.from_numpy(i.astype(np.int32))
            at += size
        self.idx.copy_(self.idx_host, non_blocking=True)
        return [i is None for i in drawn]

    def _network(self):
        """the forward on the static inputs -> its device tensors (the same objects at every replay)"""
        if self.use_graph is False or self.graph_failed:
            self.out = self._forward()
            return self.out
        if self.graph is None:
            try:
                side = torch.cuda.Stream(self.dev)
                side.wait_stream(torch.cuda.current_stream(self.dev))
                with torch.cuda.stream(side):
                    self._forward()
                torch.cuda.current_stream(self.dev).wait_stream(side)
                torch.cuda.synchronize(self.dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = self._forward()
                self.graph, self.out = g, out
            except Exception as e:      # noqa: BLE001  (whatever the capture raised: eager unless a graph is required)
                if self.require_graph or self.use_graph is True:
                    raise
                self.graph_failed = repr(e)
                torch.cuda.synchronize(self.dev)
                self.out = self._forward()
                return self.out
        self.graph.replay()
        return self.out

    def _forward(self):
        with torch.no_grad():
            return self.model.evaluate_one_sample(self.inputs)

    def _offset_box(self, ref, offset, rebase=None):
        """The frame's one box update, getOffsetBB with the config's keywords: `ref` moved by `offset` into cur and into row
        `frame` of the results.  rebase (the caller gave ref): a flag, or (K,) int32 | None where `lead` and `active` exist."""
        c = self
        if c.lead:
            PU.offset_box_multi(ref, offset, yaw_state=c.yaw_state, out=c.cur, results=c.boxes, frame=c.frame, rebase=rebase,
                                active=c.active, degrees=c.degrees, use_z=c.use_z, limit_box=c.limit_box, seed=c.seed)
        else:
            PU.offset_box(ref, offset.reshape(-1), out=c.cur, yaw_state=c.yaw_state, rebase=rebase, degrees=c.degrees,
                          use_z=c.use_z, limit_box=c.limit_box, seed=c.seed, results=c.boxes, frame=c.frame)

    # ---- one frame ---------------------------------------------------------------------------------------------------------
    def _run(self, points, *args):
        """update(): the checks, then the subclass's _update on the tracker's device"""
        PU._need_gpu(points, self._NAME + ".update")
        if self.t < 1:
            raise RuntimeError(self._NAME + ".update before init")
        self._check(*args)
        with torch.cuda.device(self.dev):
            return self._update(points.contiguous().float(), *args)

    def _check(self, *args):
        pass

    def _done(self, pts, entry):
        """the end of _update: the frame becomes the previous one, `entry` its line of the log -> a device VIEW of its row"""
        self.prev_points = pts
        if entry is not None:                              # the free-running loop keeps no host log: counts()
            self.log.append(entry)
        self.t += 1
        return self.boxes[self.t - 1]

    def _log_counts(self, k=2):
        """the free-running loop's record of the frame: counts_dev[:k] -> row t of counts_log, a device copy in stream order"""
        self.counts_log[self.t, :k].copy_(self.counts_dev[:k])

    def counts(self):
        """sampling="device" / "table" only: (t,2) int32 on the host, row f the two crop counts of frame f as the crop kernel counted
        them (before the cut to the buffers' capacities), -1 where no crop was made (row 0; the model crop under `first`
        after frame 1).  One sync."""
        if not self.free_running:
            raise RuntimeError("%s.counts: sampling=\"reference\" keeps the counts in `log`" % self._NAME)
        return self.counts_log[:self.t].cpu().numpy()

    def results(self):
        """(T,15) float32 on the host, (T,K,15) with n_targets = K: row 0 the initial box, row t the result of frame t (one sync)"""
        return self.boxes[:self.t].cpu().numpy()

    def score(self, gt_boxes, valid=None, metrics=None):
        """Score rows [0:t] of the results buffer against gt_boxes (t,15) ((t,K,15) with n_targets = K; host or device), where
        they are, in ONE launch of o3d_track_score: estimateOverlap / estimateAccuracy with the model config's IoU_space and
        up_axis (3 and (0,0,1) when absent, as in cfgs/BAT_Car.yaml).  valid (t[,K]) | None: rows with 0 are not scored.
        metrics: a metrics.SuccessPrecision that the same launch adds to.  -> (overlaps, distances) (t[,K]) device tensors;
        no sync."""
        from . import metrics as MT
        gt = PU._dev32(gt_boxes, self.dev)
        if tuple(gt.shape) != (self.t,) + self.lead + (15,):
            raise ValueError("%s.score: gt_boxes %s for results %s" % (self._NAME, tuple(gt.shape), (self.t,) + self.lead + (15,)))
        if valid is not None:
            valid = torch.as_tensor(valid).to(self.dev)
        return MT.score_boxes(gt, self.boxes[:self.t], *_score_space(self.model.config), valid=valid, accumulate=metrics)


class _KTargets:
    """What the two K-target loops (MultiTargetTracker, MultiMotionTracker) share on top of _DeviceTracker's leading K axis:
    the pack of K boxes, set_box / retire per target, and the target table of o3d_track_crop_multi: 2K o3d_crop_target
    records in a pinned buffer, group 0 in [0:K], group 1 in [K:2K], target k of group g counting into counts[g K + k]."""

    @staticmethod
    def _n_targets(n_targets):
        K = int(n_targets)
        if not 1 <= K <= PU.CROP_MULTI_MAX_TARGETS:
            raise ValueError("n_targets must be 1..%d" % PU.CROP_MULTI_MAX_TARGETS)
        return K

    def _k_state(self, K):
        self.K = K
        self.active = torch.ones((K,), dtype=torch.int32, device=self.dev)
        self.retired = set()                                       # the host's copy of `active == 0`
        self.crop_tab_host = torch.zeros((2 * K * PU.CROP_TARGET.itemsize,), dtype=torch.uint8).pin_memory()
        self.crop_tab = torch.zeros((2 * K * PU.CROP_TARGET.itemsize,), dtype=torch.uint8, device=self.dev)
        self.crop_rec = self.crop_tab_host.numpy().view(PU.CROP_TARGET)
        self.draws = DrawCache()
        self.crop_calls = 0

    def _k_stage(self, record_dtype, n_records, idx_cols):
        """the one upload per frame of a sampling="reference" K-loop, a pinned buffer and its device copy: n_records job
        records (job_rec), then the K targets' indices (idx_rec (K, idx_cols) int32, on the device at idx_ptr)"""
        jb = n_records * record_dtype.itemsize
        self.stage_host = torch.zeros((jb + 4 * self.K * idx_cols,), dtype=torch.uint8).pin_memory()
        self.stage = torch.zeros((jb + 4 * self.K * idx_cols,), dtype=torch.uint8, device=self.dev)
        self.job_rec = self.stage_host.numpy()[:jb].view(record_dtype)
        self.idx_rec = self.stage_host.numpy()[jb:].view(np.int32).reshape(self.K, idx_cols)
        self.idx_ptr = self.stage.data_ptr() + jb

    def _pack(self, boxes):
        b = _boxes15(boxes, self.dev)
        if b.shape[0] != self.K:
            raise ValueError("%d boxes for %d targets" % (b.shape[0], self.K))
        return b

    def init(self, points0, boxes0):
        boxes = super().init(points0, boxes0)
        self.active.fill_(1)
        self.retired.clear()
        self.crop_calls = 0
        return boxes

    def set_box(self, k, box):
        """Overwrite target k's last result box (the single tracker's set_box for one target)."""
        self._restart(PU.pack_box(box, self.dev), k)

    def retire(self, k):
        """Stop following target k: from the next update on its rows repeat its last box and its yaw state stays as it is.
        Its slot is NOT compacted away -- it still runs through the crops, the resampling and the network (the batch keeps
        its shape, so the captured graph stays valid); only its box update is switched off.  Where update() takes the caller's
        reference boxes (MultiTargetTracker under such a reference_BB rule), its row of `ref_boxes` is ignored: its reference
        stays its own last box."""
        self.active[k] = 0
        self.retired.add(int(k) % self.K)

    def _crop_group(self, g, boxes, scale, offset, mode, out, capacity):
        """Group g (0 or 1) of the target table: target k crops by boxes[k] ((K,15) on the device) into the `capacity` rows at
        the device address out[k] ((K,) uint64).  -> the group's part of the device table, for PU.crop_multi"""
        K, size = self.K, PU.CROP_TARGET.itemsize
        kk = np.arange(K, dtype=np.uint64)
        r = self.crop_rec[g * K:(g + 1) * K]
        r["box"], r["scale"], r["offset"], r["mode"] = boxes.data_ptr() + 60 * kk, scale, offset, mode
        r["out"], r["capacity"], r["count"] = out, capacity, self.counts_dev.data_ptr() + 4 * (kk + np.uint64(g * K))
        return self.crop_tab[g * K * size:(g + 1) * K * size]

    def _crop_multi(self, groups):
        """the table's upload and the one o3d_track_crop_multi call of groups = [(points, its part of the table)]"""
        self.crop_tab.copy_(self.crop_tab_host, non_blocking=True)
        self.scratch = PU.crop_multi(groups, self.scratch)
        self.crop_calls += 1                   # one per frame, one more whenever a crop outgrew its buffer


class _MatchingTracker(_DeviceTracker):
    """What SequenceTracker (one target, K = 1, no leading axis) and MultiTargetTracker (K targets) share: the config rules
    (reference_BB, shape_aggregation), the batch-K static inputs of the network, the canonical boxes of the BoxCloud, the
    search buffer and the template bank (one per target) with its slot rules.  bank_fixed / bank_total / slots / counts are
    ints for the single tracker and (K,) int64 arrays for K targets; the same expressions serve both.  For the free-running
    loops with a leading axis it also holds the family's one _feed and its two crop groups."""
    _REF_KW = "ref_box"

    def __init__(self, model, seed, use_graph, max_frames, search_capacity, model_capacity, n_targets=None, sampling="reference",
                 record_indices=False, bank_capacity=None):
        super().__init__(model, seed, use_graph, max_frames, _DEFAULTS, n_targets, sampling, record_indices)
        self.K = K = n_targets or 1
        self.aggregation = _aggregation(self.shape_aggregation)
        self.needs_ref_box = _reference_rule(self.reference_BB)[0]
        self.with_boxcloud = hasattr(model, "mlp_bc")
        M, N = int(self.template_size), int(self.search_size)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.inputs = {"template_points": torch.zeros((K, M, 3), **f32), "search_points": torch.zeros((K, N, 3), **f32)}
        if self.with_boxcloud:
            self.inputs["points2cc_dist_t"] = torch.zeros((K, M, 9), **f32)
        self.canon_centre = torch.zeros((K, 3), **f32)
        self.canon_rot = torch.eye(3, **f32).reshape(1, 9).repeat(K, 1).contiguous()
        self.search_buf = torch.empty(self.lead + (int(search_capacity), 3), **f32)
        self.model_capacity = int(model_capacity)
        self.bank_capacity = int(bank_capacity) if bank_capacity is not None else 8 * self.model_capacity
        if self.free_running:         # fixed sizes: nothing can grow a buffer without reading a count
            if min(int(search_capacity), self.model_capacity, self.bank_capacity) < 1:
                raise ValueError("search_capacity, model_capacity and bank_capacity must be positive")
            lead = self.lead                   # () for the single tracker, (L,) for the lanes of LaneTracker
            self.staging = torch.empty(lead + (self.model_capacity, 3), **f32)      # the frame's model crop, before it enters the bank
            self.bank = torch.empty(lead + (self.bank_capacity, 3), **f32)
            self.bank_state = torch.zeros((2,) + lead + (2,), dtype=torch.int32, device=self.dev)      # {fixed, total}, two slots by frame parity
            i32 = dict(dtype=torch.int32, device=self.dev)
            self.used_t = torch.full(lead + (M,), -1, **i32) if self.record_indices else None
            self.used_s = torch.full(lead + (N,), -1, **i32) if self.record_indices else None
            if self.tabled:           # the reference's draw for every count a buffer can hold: shared between trackers
                self.table_t = draw_table(self.bank_capacity, M, self.dev)
                self.table_s = draw_table(int(search_capacity), N, self.dev)
            self.draw_src = (self.table_t, self.table_s) if self.tabled else self.keys      # PU.resample_drawn's sources: (template, search)
            if lead:                  # _feed's views, by frame parity p: (state_in, state_out, the template counts = its column 1)
                self._states = [(self.bank_state[1 - p], self.bank_state[p], self.bank_state[p].view(-1)[1:]) for p in (0, 1)]
                self._model_counts = self.counts_dev[1:]
        else:
            self.bank = torch.empty(self.lead + (2 * self.model_capacity, 3), **f32)
        # log, per frame: (search count, model count of the crop made this frame | None, template points)

    def init(self, points0, box0):
        box = super().init(points0, box0)
        if self.free_running:              # the book-keeping is device state
            self.bank_state.zero_()
        else:
            self.bank_fixed, self.bank_total = (np.zeros(self.lead, np.int64), np.zeros(self.lead, np.int64)) if self.lead else (0, 0)
        return box

    def _check(self, ref):
        if self.needs_ref_box and ref is None:
            raise ValueError("reference_BB %r needs update(points, %s=...)" % (self.reference_BB, self._REF_KW))

    def _model_slot(self):
        """where this frame's model crop goes in the bank (of every target), or None when the template does not change"""
        first = self.t == 1
        if self.aggregation == "first":
            return 0 * self.bank_fixed if first else None
        if self.aggregation == "previous":
            return 0 * self.bank_fixed
        if self.aggregation == "firstandprevious":
            return 0 * self.bank_fixed if first else self.bank_fixed + 0
        return self.bank_total + 0                              # all: appended

    def _ensure_bank(self, need):
        old = self.bank
        if need > old.shape[-2]:
            self.bank = torch.empty(self.lead + (max(need, 2 * old.shape[-2]), 3), dtype=torch.float32, device=self.dev)
            self.bank[..., :old.shape[-2], :].copy_(old)

    def _grow_search(self, n):
        self.search_buf = torch.empty(self.lead + (2 * n, 3), dtype=torch.float32, device=self.dev)

    def _grow_model(self, n):
        self.model_capacity = 2 * n

    def _banked(self, slot, nm):
        """the bank's book-keeping after a model crop of nm points at `slot`"""
        c = self
        c.bank_total = slot + nm
        if c.t == 1:
            c.bank_fixed = nm + 0                  # the first frame's crop stays at the head of the bank
            if c.aggregation == "firstandprevious":            # getModel([first, previous]) at t = 1: the same crop twice
                c._ensure_bank(2 * int(np.max(nm)) + c.model_capacity)
                for bank, n in zip(c.bank.reshape(-1, c.bank.shape[-2], 3), np.atleast_1d(nm)):
                    bank[n:2 * n].copy_(bank[:n])
                c.bank_total = 2 * nm

    def _boxcloud(self):
        """the templates' BoxClouds against the canonical boxes (BAT only)"""
        if self.with_boxcloud:
            PU.boxcloud_into(self.inputs["points2cc_dist_t"], self.inputs["template_points"], self.canon_centre, self.canon_wlh,
                             self.canon_rot)

    # ---- the free-running loops with a leading axis (LaneTracker, SceneTracker, ManagedSceneTracker) ---------------------------
    def _feed(self, lanes, parity):
        """Everything between the crops and the box update, on the lane table `lanes`: the staged model crops into the banks, both
        draws and gathers, the BoxClouds, the network -> (the offsets (L,4), state_out: what the next frame reads as state_in)"""
        c = self
        state_in, state_out, totals = c._states[parity]
        PU.bank_update_lanes(c.staging, c._model_counts, 2, c.bank, c.aggregation, lanes, state_in, state_out)
        PU.resample_drawn_lanes([(c.bank, totals, 2, c.draw_src[0], c.inputs["template_points"], c.used_t),
                                 (c.search_buf, c.counts_dev, 2, c.draw_src[1], c.inputs["search_points"], c.used_s)])
        c._boxcloud()
        return c._network()[0], state_out

    # the two crop groups of a scene frame; group g counts into column g of the counts (K,2)
    _FRAME_GROUP = 0          # group 0 (the search windows) crops the frame, group 1 (the model crops) the one before; a managed
    #                           slot starves on column 0, and its bank restarts in _feed's state_out under `aggregation`
    _GATED = 1                # the model crop is made only for the slots whose bank takes one (scene_lane_rows' has_crop)

    def _crop_groups(self, ref):
        """per group (boxes (K,15), scale, offset, mode, out (K,capacity,3)): the search windows by `ref`, the model crops by cur"""
        c = self
        return [(ref, c.search_bb_scale, c.search_bb_offset, PU.CROP_SUBWINDOW, c.search_buf),
                (c.cur, c.model_bb_scale, c.model_bb_offset, PU.CROP_MODEL, c.staging)]


def _matching_overflow(counts, search_capacity, model_capacity, bank_capacity, aggregation):
    """counts (t,2) of one tracked sequence (row 0 unused) -> (truncated search crops, truncated model crops, frames on which
    the bank was full) under the fixed capacities of a free-running matching tracker"""
    over_s = int((counts[1:, 0] > search_capacity).sum())
    over_m = int((counts[1:, 1] > model_capacity).sum())
    fixed = total = full = 0
    for t in range(1, counts.shape[0]):                    # the transitions of o3d_track_bank_update, before its clip
        if counts[t, 1] < 0:
            continue
        nm, first = min(int(counts[t, 1]), model_capacity), t == 1
        slot = total if aggregation == "all" else fixed if aggregation == "firstandprevious" and not first else 0
        need = 2 * nm if aggregation == "firstandprevious" and first else slot + nm
        full += need > bank_capacity
        fixed, total = (nm if first else fixed), min(need, bank_capacity)
    return over_s, over_m, int(full)


class SequenceTracker(_MatchingTracker):
    """Device-resident tracking loop for the matching trackers (trackers.BAT, trackers.P2B).

        trk = SequenceTracker(model)            # model on the GPU, eval mode
        trk.init(points0, box0)                 # (N,3) float32 GPU tensor; box0 = (center, wlh, rot) or a 15-vector
        box = trk.update(points)                # a (15,) device VIEW of the new box (no sync for it)
        boxes = trk.results()                   # (T,15) on the host, one sync

    `update(points, ref_box=...)` searches around (and offsets from) the given box instead of the previous result: the
    reference's `reference_BB: previous_gt / current_gt`.  `seed` feeds limit_box's replacement draw only.
    use_graph: None = capture, fall back to eager when the capture fails (O3D_REQUIRE_GRAPH=1: raise instead); False = eager.

    sampling="device": the free-running loop of the module docstring.  When update() returns, the frame is only ENQUEUED:
    nothing has been read back, and the caller's frame tensor must not be rewritten from another stream before the NEXT frame
    has been enqueued (its model crop reads it; `prev_points` keeps the reference alive).  `seed` also keys the index draws.
    search_capacity / model_capacity / bank_capacity (default 8 * model_capacity) are then the fixed sizes of the search
    buffer, the staging buffer of a frame's model crop and the template bank: a longer crop keeps its first survivors, the
    draw uses min(count, capacity), and a full bank (aggregation `all`) drops further rows.  `log` stays empty; counts() ->
    (t,2) (search count, model-crop count | -1) on the host, overflow() -> how often a capacity cut something (one sync each).
    record_indices=True keeps the last frame's indices in used_t (template_size,) / used_s (search_size,), device int32, -1
    for a zero-filled cloud.  update(points, ref_box=<device tensor>) stays free of host stops as well.

    sampling="table": that free-running loop with tables as the index sources of the resample launch -- every index is read
    from draw_table(bank_capacity, template_size) / draw_table(search_capacity, search_size), the reference's own draw for every
    count, so the network's inputs and the boxes are those of sampling="reference" bit for bit as long as overflow() is
    (0, 0, 0).  `seed` feeds limit_box only, as in "reference".  The tables cost 4 * (capacity + 1) * size bytes each, once per
    process and device.
    """
    _NAME = "SequenceTracker"

    def __init__(self, model, seed=0, use_graph=None, max_frames=1024, search_capacity=32768, model_capacity=8192,
                 sampling="reference", record_indices=False, bank_capacity=None):
        super().__init__(model, seed, use_graph, max_frames, search_capacity, model_capacity, None, sampling, record_indices,
                         bank_capacity)
        if not self.free_running:
            self._index_buffers(int(self.template_size) + int(self.search_size))

    def _crops(self, pts, ref, slot):
        """the frame's one crop call + the count read-back -> (search count, model count | None)"""
        c = self

        def make_jobs():
            jobs = [((pts, ref, c.search_bb_scale, c.search_bb_offset, PU.CROP_SUBWINDOW, c.search_buf, c.counts_dev[0:1]), c._grow_search)]
            if slot is not None:
                c._ensure_bank(slot + c.model_capacity)
                jobs.append(((c.prev_points, c.cur, c.model_bb_scale, c.model_bb_offset, PU.CROP_MODEL,
                              c.bank[slot:slot + c.model_capacity], c.counts_dev[1:2]), c._grow_model))
            return jobs
        ns = c._crop_counts(make_jobs)
        return ns[0], (ns[1] if slot is not None else None)

    def update(self, points, ref_box=None):
        return self._run(points, ref_box)

    def _update_free(self, pts, ref_box):
        """the frame of sampling="device": enqueued, nothing read back"""
        c = self
        c._grow_boxes()
        ref = c.cur if ref_box is None else PU.pack_box(ref_box, c.dev)
        first = c.t == 1
        has_crop = first or c.aggregation != "first"
        jobs = [(pts, ref, c.search_bb_scale, c.search_bb_offset, PU.CROP_SUBWINDOW, c.search_buf, c.counts_dev[0:1])]
        if has_crop:
            jobs.append((c.prev_points, c.cur, c.model_bb_scale, c.model_bb_offset, PU.CROP_MODEL, c.staging, c.counts_dev[1:2]))
        c.scratch = PU.crop_jobs(jobs, c.scratch)
        c._log_counts(len(jobs))
        state_in, state_out = c.bank_state[(c.t + 1) & 1], c.bank_state[c.t & 1]
        PU.bank_update(c.staging, c.counts_dev[1:2], c.bank, c.aggregation, first, has_crop, state_in, state_out)
        PU.resample_drawn([(c.bank, state_out[1:2], c.draw_src[0], c.inputs["template_points"], c.used_t),
                           (c.search_buf, c.counts_dev[0:1], c.draw_src[1], c.inputs["search_points"], c.used_s)])
        c._boxcloud()
        best, _ = c._network()
        c._offset_box(ref, best, ref_box is not None)
        return c._done(pts, None)

    def overflow(self):
        """sampling="device" / "table" only -> (truncated search crops, truncated model crops, frames on which the bank was full): how
        often a fixed capacity cut something, worked out on the host from counts() and the capacities (one sync)."""
        return _matching_overflow(self.counts(), self.search_buf.shape[0], self.model_capacity, self.bank_capacity, self.aggregation)

    def _update(self, pts, ref_box):
        if self.free_running:
            return self._update_free(pts, ref_box)
        c, M = self, int(self.template_size)
        c._grow_boxes()
        ref = c.cur if ref_box is None else PU.pack_box(ref_box, c.dev)
        slot = c._model_slot()
        ns, nm = c._crops(pts, ref, slot)
        if slot is not None:
            c._banked(slot, nm)
        nt = c.bank_total
        zero_t, zero_s = c._stage_indices((nt, M), (ns, int(c.search_size)))
        PU.resample_jobs([(None if zero_t else c.bank, c.idx[:M], c.inputs["template_points"]),
                          (None if zero_s else c.search_buf, c.idx[M:], c.inputs["search_points"])])
        c._boxcloud()
        best, _ = c._network()
        c._offset_box(ref, best, ref_box is not None)
        return c._done(pts, (ns, nm, nt))


class MultiTargetTracker(_KTargets, _MatchingTracker):
    """Device-resident tracking loop for K targets in the same frames (the matching trackers: trackers.BAT, trackers.P2B).
    What SequenceTracker does per target happens here once per frame for all of them:

        trk = MultiTargetTracker(model, K)      # model on the GPU, eval mode
        trk.init(points0, boxes0)               # (N,3) float32 GPU tensor; boxes0 (K,15) or K boxes as pack_box takes them
        boxes = trk.update(points)              # a (K,15) device VIEW of the new boxes (no sync for it)
        all_boxes = trk.results()               # (T,K,15) on the host, one sync

    Per frame t >= 1, whatever K:

      o3d_track_crop_multi, one call    group 0: frame t against the K reference boxes (search windows); group 1: frame t-1
                                        against the K result boxes (model crops, appended to each target's bank).  Every
                                        point is read once per group.  (Its 96 K-byte target table is uploaded in front.)
      pinned read-back of 2K counts     the one host sync of the frame, shared by the K targets
      2K index draws                    default_rng(1).choice, memoised by (count, size): DrawCache
      one upload                        the 2K resample jobs and the K (template_size + search_size) indices, one pinned buffer
      o3d_track_resample_multi          all 2K gathers straight into rows of the batched static inputs (K,M,3), (K,N,3)
      o3d_boxcloud, B = K               the templates' BoxClouds against the canonical boxes (BAT only)
      forward + o3d_best_proposal       batch K, replayed as one HIP graph captured once per tracker (eager when the capture
                                        fails, unless O3D_REQUIRE_GRAPH=1)
      o3d_track_offset_box_multi        the K new boxes into row t of the (T,K,15) results buffer

    The template bank is per target: bank[k] holds target k's crops with SequenceTracker's slot rules for the four
    shape_aggregation modes.  `update(points, ref_boxes=...)` (K,15): the reference's `reference_BB: previous_gt / current_gt`.
    `seed`: target k's limit_box draws use seed + k.  log, per frame: (search counts (K), model counts (K) | None, template
    counts (K)); crop_calls: the crop calls since init (one per frame, one more whenever a crop outgrew its buffer).
    sampling: "reference" only ("device" and "table" raise ValueError here: the K-target free-running loop is SceneTracker)."""
    _NAME, _REF_KW = "MultiTargetTracker", "ref_boxes"

    def __init__(self, model, n_targets, seed=0, use_graph=None, max_frames=1024, search_capacity=32768, model_capacity=8192,
                 sampling="reference"):
        _sampling(sampling, self._NAME)
        _require_family(model, False, "MultiTargetTracker")
        K = self._n_targets(n_targets)
        super().__init__(model, seed, use_graph, max_frames, search_capacity, model_capacity, K)
        self._k_state(K)
        self.rebase_all = torch.ones((K,), dtype=torch.int32, device=self.dev)
        # the frame's one upload: 2K resample jobs [template 0..K-1, search 0..K-1], then the K * (M + N) indices
        self._k_stage(PU.RESAMPLE_JOB, 2 * K, int(self.template_size) + int(self.search_size))

    def _crops(self, pts, ref, slots):
        """the frame's one crop call + the count read-back -> (search counts (K), model counts (K) | None)"""
        c, K = self, self.K
        kk = np.arange(K, dtype=np.uint64)

        def launch():
            cap = c.search_buf.shape[1]
            groups = [(pts, c._crop_group(0, ref, c.search_bb_scale, c.search_bb_offset, PU.CROP_SUBWINDOW,
                                          c.search_buf.data_ptr() + 12 * cap * kk, cap))]
            caps = [(cap, c._grow_search)] * K
            if slots is not None:
                c._ensure_bank(int(slots.max()) + c.model_capacity)
                out = c.bank.data_ptr() + 12 * (c.bank.shape[1] * kk + slots.astype(np.uint64))
                groups.append((c.prev_points, c._crop_group(1, c.cur, c.model_bb_scale, c.model_bb_offset, PU.CROP_MODEL, out,
                                                            c.model_capacity)))
                caps += [(c.model_capacity, c._grow_model)] * K
            c._crop_multi(groups)
            return caps
        ns = c._counts_loop(launch)
        return np.array(ns[:K], np.int64), (np.array(ns[K:], np.int64) if slots is not None else None)

    # ---- one frame ---------------------------------------------------------------------------------------------------------
    def update(self, points, ref_boxes=None):
        return self._run(points, ref_boxes)

    def _update(self, pts, ref_boxes):
        c, K, M, N = self, self.K, int(self.template_size), int(self.search_size)
        c._grow_boxes()
        ref = c.cur if ref_boxes is None else c._pack(ref_boxes)
        if ref_boxes is not None and c.retired:        # a retired target's reference is its own last box, not the caller's
            rows = sorted(c.retired)
            ref = ref.clone()
            ref[rows] = c.cur[rows]
        slots = c._model_slot()
        ns, nm = c._crops(pts, ref, slots)
        if slots is not None:
            c._banked(slots, nm)
        nt = c.bank_total.copy()
        # the frame's one upload: the indices and the 2K resample jobs
        zero = np.zeros((2 * K,), np.int32)
        for k in range(K):
            it, isr = c.draws.get(nt[k], M), c.draws.get(ns[k], N)
            if it is None:
                zero[k] = 1
            else:
                c.idx_rec[k, :M] = it
            if isr is None:
                zero[K + k] = 1
            else:
                c.idx_rec[k, M:] = isr
        kk = np.arange(K, dtype=np.uint64)
        j = c.job_rec
        j["src"][:K], j["src"][K:] = c.bank.data_ptr() + 12 * c.bank.shape[1] * kk, c.search_buf.data_ptr() + 12 * c.search_buf.shape[1] * kk
        j["n_src"][:K], j["n_src"][K:] = nt, ns
        j["idx"][:K], j["idx"][K:] = c.idx_ptr + 4 * (M + N) * kk, c.idx_ptr + 4 * ((M + N) * kk + np.uint64(M))
        j["dst"][:K], j["dst"][K:] = c.inputs["template_points"].data_ptr() + 12 * M * kk, c.inputs["search_points"].data_ptr() + 12 * N * kk
        j["n"][:K], j["n"][K:] = M, N
        j["zero"] = zero
        c.stage.copy_(c.stage_host, non_blocking=True)
        PU.resample_multi(c.stage, 2 * K)
        c._boxcloud()
        best, _ = c._network()
        c._offset_box(ref, best, c.rebase_all if ref_boxes is not None else None)
        return c._done(pts, (ns, nm, nt))


# cfgs/M2_track_kitti.yaml :5-8,32-33
_MOTION_DEFAULTS = dict(bb_scale=1.25, bb_offset=2, point_sample_size=1024, degrees=False, use_z=True, limit_box=False)


class _MotionTracker(_DeviceTracker):
    """What the loops of the motion tracker (m2track.M2TRACK) share: the batch-K static inputs of the network and the two crop
    buffers, with `lead` = () for one target, (K,) / (L,) for K targets or L lanes, and, free-running, the record of the
    indices, the index source and the feed of the loops with a leading axis."""

    def __init__(self, model, seed, use_graph, max_frames, capacity, n_targets=None, sampling="reference", record_indices=False):
        if sampling in FREE_RUNNING and int(capacity) < 1:         # a fixed size: nothing can grow a buffer without reading a count
            raise ValueError("capacity must be positive")
        super().__init__(model, seed, use_graph, max_frames, _MOTION_DEFAULTS, n_targets, sampling, record_indices)
        dev, lead, N = self.dev, self.lead, int(self.point_sample_size)
        f32 = dict(dtype=torch.float32, device=dev)
        self.box_aware = bool(getattr(model, "box_aware", False))
        self.inputs = {"points": torch.zeros((n_targets or 1, 2 * N, 5), **f32)}
        if self.box_aware:
            self.inputs["candidate_bc"] = torch.zeros((n_targets or 1, 2 * N, 9), **f32)
        self.crop_buf = torch.empty((2,) + lead + (int(capacity), 3), **f32)      # [0] the previous frame's crops, [1] the current one's
        if self.free_running:
            self._halves = (self.crop_buf[0], self.crop_buf[1])            # views made once: nothing grows crop_buf here
            self.used = torch.full(lead + (2 * N,), -1, dtype=torch.int32, device=dev) if self.record_indices else None
            self.used_prev, self.used_this = (self.used[..., :N], self.used[..., N:]) if self.record_indices else (None, None)
            if self.tabled:           # one table for both halves: the reference draws both with seed=1
                self.table = draw_table(int(capacity), N, dev)
            self.draw_src = self.table if self.tabled else self.keys      # the source of PU.motion_input_drawn and its lane form

    # ---- the free-running loops with a leading axis (MotionLaneTracker, MotionSceneTracker, ManagedMotionSceneTracker) ----------
    def _feed(self, lanes, parity):
        """Everything between the crops and the box update, on the lane table `lanes`: gather, time stamp, prior-targetness
        mask and candidate BoxCloud into the static inputs, the network.  -> (the offsets (L,4), None: there is no bank)"""
        c = self
        PU.motion_input_drawn_lanes(c._halves[0], c._halves[1], c.counts2, c.draw_src, c.canon_wlh, lanes, c.inputs["points"],
                                    c.inputs["candidate_bc"] if c.box_aware else False, c.used)
        return c._network(), None

    # the two crop groups of a scene frame; group g counts into column g of the counts (K,2)
    _FRAME_GROUP = 1          # group 0 crops the frame before, group 1 the frame; a managed slot starves on column 1
    _GATED = None             # both are made on every frame, whatever the lane rows say
    aggregation = None        # no template bank: scene_lane_rows and o3d_scene_manage take no rule

    def _crop_groups(self, ref):
        """per group (boxes (K,15), scale, offset, mode, out (K,capacity,3)): both by the last boxes"""
        return [(self.cur, self.bb_scale, self.bb_offset, PU.CROP_SUBWINDOW, self.crop_buf[h]) for h in (0, 1)]


class MotionSequenceTracker(_MotionTracker):
    """Device-resident tracking loop for the motion tracker (m2track.M2TRACK): the frame loop of evaluate_one_sequence over
    MotionBaseModel.build_input_dict (models/base_model.py:255-304).  Same surface as SequenceTracker (init, update, set_box,
    results, log, out).  Per frame t >= 1:

      o3d_track_crop, one call, two jobs    frame t-1 and frame t, both by the last result box (generate_subwindow twice)
      8-byte pinned read-back               the two point counts -- the one host sync of the frame (see the module docstring)
      draw_indices twice, one index upload  2 x point_sample_size int32 = 8 KB
      o3d_track_motion_input                gather + time stamp + prior-targetness mask + candidate BoxCloud, one launch, into
                                            the network's static inputs; first_frame = (t == 1)
      forward                               replayed as one HIP graph captured once per tracker
      o3d_track_offset_box                  reads estimation_boxes where the forward left it; the new box goes to results

    log, per frame: (previous-frame count, current-frame count).

    sampling="device": the free-running loop (module docstring) -- o3d_track_crop, a device copy of the
    two counts into row t of counts_log, o3d_track_motion_input_drawn (counts read on the device, indices drawn there), the
    forward, o3d_track_offset_box.  When update() returns, the frame is only ENQUEUED, and the caller's frame tensor must not
    be rewritten from another stream before the NEXT frame has been enqueued (`prev_points` keeps the reference alive).
    `capacity` is then the fixed size of both crop buffers (a longer crop keeps its first survivors); `log` stays empty,
    counts() -> (t,2) (previous-frame count, current-frame count), overflow() -> (truncated previous, truncated current, 0);
    record_indices=True keeps the last frame's indices in used_prev / used_this (point_sample_size,), -1 for a zero-filled half.

    sampling="table": that loop with a table as the index source -- both halves read draw_table(capacity, point_sample_size), the
    reference's own draw, so inputs and boxes are those of sampling="reference" bit for bit while overflow() is (0, 0, 0)."""
    _NAME = "MotionSequenceTracker"

    def __init__(self, model, seed=0, use_graph=None, max_frames=1024, capacity=32768, sampling="reference", record_indices=False):
        super().__init__(model, seed, use_graph, max_frames, capacity, None, sampling, record_indices)
        if not self.free_running:
            self._index_buffers(2 * int(self.point_sample_size))

    def _crops(self, pts):
        c = self

        def grow(n):                                   # both jobs share it: called once, with the larger of the two counts
            c.crop_buf = torch.empty((2, 2 * n, 3), dtype=torch.float32, device=c.dev)

        def make_jobs():
            return [((src, c.cur, c.bb_scale, c.bb_offset, PU.CROP_SUBWINDOW, c.crop_buf[h], c.counts_dev[h:h + 1]), grow)
                    for h, src in enumerate((c.prev_points, pts))]
        return c._crop_counts(make_jobs)

    def update(self, points):
        return self._run(points)

    def _update_free(self, pts):
        """the frame of sampling="device": enqueued, nothing read back"""
        c = self
        c._grow_boxes()
        c.scratch = PU.crop_jobs([(src, c.cur, c.bb_scale, c.bb_offset, PU.CROP_SUBWINDOW, c.crop_buf[h], c.counts_dev[h:h + 1])
                                  for h, src in enumerate((c.prev_points, pts))], c.scratch)
        c._log_counts()
        PU.motion_input_drawn(c.crop_buf[0], c.crop_buf[1], c.counts_dev, c.draw_src, c.canon_wlh, c.t == 1, c.inputs["points"],
                              c.inputs["candidate_bc"] if c.box_aware else False, c.used)
        est = c._network()
        c._offset_box(c.cur, est)
        return c._done(pts, None)

    def overflow(self):
        """sampling="device" / "table" only -> (truncated previous-frame crops, truncated current-frame crops, 0: there is no bank), on the
        host from counts() and the capacity (one sync)."""
        counts = self.counts()
        cap = self.crop_buf.shape[1]
        return int((counts[1:, 0] > cap).sum()), int((counts[1:, 1] > cap).sum()), 0

    def _update(self, pts):
        if self.free_running:
            return self._update_free(pts)
        c, N = self, int(self.point_sample_size)
        c._grow_boxes()
        n_prev, n_this = c._crops(pts)
        zero = c._stage_indices((n_prev, N), (n_this, N))
        PU.motion_input(c.crop_buf[0, :n_prev], c.crop_buf[1, :n_this], c.idx, c.canon_wlh, c.t == 1, zero=zero,
                        out_points=c.inputs["points"], out_bc=c.inputs["candidate_bc"] if c.box_aware else False)
        est = c._network()
        c._offset_box(c.cur, est)
        return c._done(pts, (n_prev, n_this))


class MultiMotionTracker(_KTargets, _MotionTracker):
    """Device-resident tracking loop of the motion tracker (m2track.M2TRACK) for K targets in the same frames: what
    MotionSequenceTracker does per target happens here once per frame for all of them.  The surface is MultiTargetTracker's:

        trk = MultiMotionTracker(model, K)      # model on the GPU, eval mode
        trk.init(points0, boxes0)               # (N,3) float32 GPU tensor; boxes0 (K,15) or K boxes as pack_box takes them
        boxes = trk.update(points)              # a (K,15) device VIEW of the new boxes (no sync for it)
        all_boxes = trk.results()               # (T,K,15) on the host, one sync

    Per frame t >= 1, whatever K:

      o3d_track_crop_multi, one call    group 0: frame t-1, group 1: frame t, both against the K last result boxes
                                        (generate_subwindow) into crop_buf (2,K,capacity,3).  (Its 96 K-byte target table is
                                        uploaded in front.)
      pinned read-back of 2K counts     the one host sync of the frame, shared by the K targets
      2K index draws                    default_rng(1).choice, memoised by (count, point_sample_size): DrawCache
      one upload                        the K o3d_motion_job records and the K x 2N indices, one pinned buffer
      o3d_track_motion_input_multi      gather + time stamp + prior-targetness mask + candidate BoxCloud of all K targets,
                                        one launch, into the batch-K static inputs; first_frame = (t == 1)
      forward, batch K                  replayed as one HIP graph captured once per tracker (eager when the capture fails,
                                        unless O3D_REQUIRE_GRAPH=1)
      o3d_track_offset_box_multi        the K new boxes into row t of the (T,K,15) results buffer

    log, per frame: (previous-frame counts (K), current-frame counts (K)); crop_calls: the crop calls since init (one per
    frame, one more whenever a crop outgrew the buffer: all 2K rows then grow to twice the largest count).
    sampling: "reference" only ("device" and "table" raise ValueError here: the K-target free-running loop is
    MotionSceneTracker)."""
    _NAME = "MultiMotionTracker"

    def __init__(self, model, n_targets, seed=0, use_graph=None, max_frames=1024, capacity=32768, sampling="reference"):
        _sampling(sampling, self._NAME)
        _require_family(model, True, "MultiMotionTracker")
        K = self._n_targets(n_targets)
        super().__init__(model, seed, use_graph, max_frames, capacity, K)
        self._k_state(K)
        # the frame's one upload: K motion jobs, then the K * 2N indices
        self._k_stage(PU.MOTION_JOB, K, 2 * int(self.point_sample_size))

    def _crops(self, pts):
        """the frame's one crop call + the count read-back -> (previous-frame counts (K), current-frame counts (K))"""
        c, K = self, self.K
        kk = np.arange(K, dtype=np.uint64)

        def grow(n):                                   # all 2K crops share it: called once, with the largest count
            c.crop_buf = torch.empty((2, K, 2 * n, 3), dtype=torch.float32, device=c.dev)

        def launch():
            cap = c.crop_buf.shape[2]
            c._crop_multi([(src, c._crop_group(g, c.cur, c.bb_scale, c.bb_offset, PU.CROP_SUBWINDOW,
                                               c.crop_buf[g].data_ptr() + 12 * cap * kk, cap))
                           for g, src in enumerate((c.prev_points, pts))])
            return [(cap, grow)] * (2 * K)
        ns = c._counts_loop(launch)
        return np.array(ns[:K], np.int64), np.array(ns[K:], np.int64)

    def update(self, points):
        return self._run(points)

    def _update(self, pts):
        c, K, N = self, self.K, int(self.point_sample_size)
        c._grow_boxes()
        n_prev, n_this = c._crops(pts)
        # the frame's one upload: the indices and the K motion jobs
        zero = np.zeros((2, K), np.int32)
        for k in range(K):
            for h, n in enumerate((n_prev[k], n_this[k])):
                i = c.draws.get(n, N)
                if i is None:
                    zero[h, k] = 1
                else:
                    c.idx_rec[k, h * N:(h + 1) * N] = i
        kk = np.arange(K, dtype=np.uint64)
        j, cap = c.job_rec, c.crop_buf.shape[2]
        j["prev"], j["cur"] = c.crop_buf[0].data_ptr() + 12 * cap * kk, c.crop_buf[1].data_ptr() + 12 * cap * kk
        j["n_prev"], j["n_this"] = n_prev, n_this
        j["idx"] = c.idx_ptr + 8 * N * kk
        j["zero_prev"], j["zero_this"] = zero[0], zero[1]
        c.stage.copy_(c.stage_host, non_blocking=True)
        PU.motion_input_multi(c.stage, K, N, c.canon_wlh, c.t == 1, c.inputs["points"],
                              c.inputs["candidate_bc"] if c.box_aware else False)
        est = c._network()
        c._offset_box(c.cur, est)
        return c._done(pts, (n_prev, n_this))


def _lane_sampling(name, who):
    """the `sampling` keyword of a lane tracker: a lane never reads a count back, so only the free-running modes run on lanes"""
    if _sampling(name) not in FREE_RUNNING:
        raise ValueError("%s: sampling=%r draws its indices on the host, from counts that a lane tracker never reads back; "
                         "expected \"device\" or \"table\"" % (who, name))
    return name


# ---- the test epoch on L lanes --------------------------------------------------------------------------
ORDERS = ("given", "longest_first")


def lane_schedule(lengths, lanes, order="given"):
    """Which tracklet runs on which lane at which step.  lengths: the tracklets' frame counts; -> (tracklet, frame), two
    (steps, lanes) int32 arrays: tracklet[s, l] = the tracklet lane l tracks at step s (-1: idle), frame[s, l] = its frame
    index t >= 1 (0 when idle).  Tracklets are taken in the given order (order="longest_first": by decreasing length, a stable
    sort); at each step every idle lane, in lane order, takes the next unassigned tracklet of at least 2 frames and starts it
    at t = 1, a busy lane advances by one frame.  A tracklet of length 1 takes no lane (its only result is its first box); a
    length below 1 raises ValueError.  steps = the step after which all tracklets are done."""
    L = int(lanes)
    if L < 1:
        raise ValueError("lanes must be positive")
    if order not in ORDERS:
        raise ValueError("order %r: expected \"given\" or \"longest_first\"" % (order,))
    lengths = [int(n) for n in lengths]
    if any(n < 1 for n in lengths):
        raise ValueError("a tracklet needs at least one frame")
    todo = sorted(range(len(lengths)), key=lambda j: -lengths[j]) if order == "longest_first" else list(range(len(lengths)))
    todo = [j for j in todo if lengths[j] >= 2]
    on, at, taken = [-1] * L, [0] * L, 0
    tracklet, frame = [], []
    while True:
        for l in range(L):
            if on[l] >= 0:
                if at[l] + 1 < lengths[on[l]]:
                    at[l] += 1
                else:
                    on[l], at[l] = -1, 0
        for l in range(L):
            if on[l] < 0 and taken < len(todo):
                on[l], at[l], taken = todo[taken], 1, taken + 1
        if all(j < 0 for j in on):
            break
        tracklet.append(list(on))
        frame.append(list(at))
    return np.array(tracklet, np.int32).reshape(-1, L), np.array(frame, np.int32).reshape(-1, L)


def plan_lane_steps(tables, tracklet, frame, row0, pool, clouds, addr, by_gt, back, crop_all=True):
    """The tables of S steps of L lanes into `tables` (a crop_plan.Tables with the sections lanes (L, LANE_COLS) int32, plan
    (2L,) CROP_PLAN and targets (2L,) CROP_TARGET, its device copy at tables.base): a pure function of integer arrays.
    tracklet, frame (S,L): the steps' slice of lane_schedule; row0, pool: the crop_plan.FramePool of the tracklets' frames
    (boxes and results share its rows); clouds: per cloud (frames back from t, cropped by the reference box?, scale, offset,
    mode, the address of out (L,cap,3), cap, gated?); addr = {"cur", "gt", "counts"}: the addresses of the lanes' current boxes
    (L,15), the ground-truth pool (R,15) and the counts (L,2).  by_gt: the reference box of frame t is the ground truth of
    pool row t - back (reference_BB previous_gt: back = 1, current_gt: 0), else the lane's current box.  A gated cloud is
    cropped only where the step has_crop: everywhere with crop_all, else on a tracklet's first step (shape_aggregation
    `first`).  Every active (lane, cloud) is one group of one target, cloud c of lane l in the order of its slot c L + l; an
    idle lane has none.  -> (groups, need = the scratch length, starts = a lane starts a tracklet: three (S,) arrays)"""
    js, ts = np.asarray(tracklet, np.int64), np.asarray(frame, np.int64)
    (S, L), F = js.shape, PU.LANE
    on = js >= 0
    row = np.where(on, row0[np.maximum(js, 0)] + ts, 0)                    # the pool row of frame t
    first = on & (ts == 1)
    has_crop = on & (first | bool(crop_all))
    ref_row = np.where(on & bool(by_gt), row - back, -1)
    lanes = tables.view("lanes")[:S]
    for name, v in (("active", on), ("first", first), ("has_crop", has_crop), ("t", ts), ("row", np.where(on, row, -1)),
                    ("ref_row", ref_row), ("rebase", on & bool(by_gt))):
        lanes[:, :, F[name]] = v
    ll = np.arange(L, dtype=np.int64)
    cur = np.broadcast_to(addr["cur"] + 60 * ll, (S, L))
    ref = addr["gt"] + 60 * ref_row if by_gt else cur
    n = len(clouds) * L
    rec, cloud, valid = np.zeros((S, n), PU.CROP_TARGET), np.zeros((S, n), np.int64), np.zeros((S, n), bool)
    for c, (shift, by_ref, scale, offset, mode, out, cap, gated) in enumerate(clouds):
        sl = slice(c * L, (c + 1) * L)
        cloud[:, sl], valid[:, sl] = np.where(on, row - shift, 0), has_crop if gated else on
        r = rec[:, sl]
        r["box"], r["scale"], r["offset"], r["mode"] = ref if by_ref else cur, scale, offset, mode
        r["out"], r["capacity"], r["count"] = out + 12 * cap * ll, cap, addr["counts"] + 8 * ll + 4 * c
    groups, need, _, _ = plan_groups(np.broadcast_to(np.arange(n), (S, n)), cloud, rec, pool.fptr, pool.fn, tables.view("targets"),
                                     tables.view("plan"), tables.dev("targets"), valid)
    return groups, need, first.any(1)


class _Lanes:
    """What LaneTracker and MotionLaneTracker put on top of their single-target bases' state with a leading L axis: the epoch
    plan.  begin() lays all tracklets' ground-truth boxes end to end in one pool (R,15) and gives the results the same rows
    (tracklet j owns rows [row0_j, row0_j + T_j)), runs lane_schedule, and from then on everything a step needs is host
    knowledge: per step the lane table (L, LANE_COLS) and one o3d_crop_plan group with one o3d_crop_target per (lane, cloud).
    They are built for plan_steps steps at a time in one host buffer (plan_lane_steps) and uploaded with ONE copy before the
    chunk's first step; step() only launches: the step's crop groups, the family's _feed on the step's lane table, the box
    update (_offset).  A subclass provides _clouds() (its two crops per lane) and tells _lane_state its reference rule: by_gt,
    back and crop_all of plan_lane_steps."""

    def _lane_state(self, L, plan_steps, by_gt=False, back=0, crop_all=True):
        self.L, self.plan_steps, self._rule = L, int(plan_steps), (bool(by_gt), int(back), bool(crop_all))
        if self.plan_steps < 1:
            raise ValueError("plan_steps must be positive")
        P = self.plan_steps
        self.counts2 = self.counts_dev.view(L, 2)
        self._tables = Tables(P, {"lanes": (np.int32, (L, PU.LANE_COLS)), "plan": (PU.CROP_PLAN, (2 * L,)),
                                  "targets": (PU.CROP_TARGET, (2 * L,))})
        self._tab = torch.zeros((self._tables.host.size,), dtype=torch.uint8, device=self.dev)
        self._tables.base = self._tab.data_ptr()
        self._plan_h = self._tables.view("plan")
        lanes_d = self._tab[:P * L * PU.LANE_COLS * 4].view(torch.int32).view(P, L, PU.LANE_COLS)        # the first section
        self._lane_rows = [lanes_d[k] for k in range(P)]                   # step k of the chunk: its (L, LANE_COLS) table on the device
        self._groups, self._starts = [0] * P, [False] * P
        self.steps, self.s, self.uploads = 0, 0, 0
        self.schedule = None

    def init(self, *a, **k):
        raise RuntimeError("%s: begin(tracklets) and step() run the epoch; init / update belong to the single trackers" % self._NAME)

    update = init

    # ---- the plan ----------------------------------------------------------------------------------------------------------
    def begin(self, tracklets, order="given"):
        """Plan the epoch over `tracklets` -- a sampler.DeviceTracklets, or any iterable of (frames, boxes) -- and enqueue what
        precedes its first step: the two pools, the first chunk's tables, the first lanes' start.  -> the number of steps."""
        frames, boxes = [], []
        for item in tracklets:
            f, b = (item.frames, item.boxes) if hasattr(item, "frames") else item
            f = list(f)
            for x in f:
                PU._need_gpu(x, self._NAME + ".begin")
            b = PU._dev32(b, self.dev).reshape(-1, 15)
            if len(f) != b.shape[0]:
                raise ValueError("%d frames, %d ground-truth boxes" % (len(f), b.shape[0]))
            frames.append([x.contiguous().float() for x in f])
            boxes.append(b)
        self.lengths = [len(f) for f in frames]
        self.schedule = lane_schedule(self.lengths, self.L, order)
        self.frames, self.steps, self.s, self.uploads = frames, self.schedule[0].shape[0], 0, 0
        self._pool = FramePool(frames)                                                     # per pool row: the frame's address and size
        self.row0 = self._pool.row0
        R = int(self.row0[-1])
        with torch.cuda.device(self.dev):
            self.gt = torch.cat(boxes).contiguous() if R else torch.zeros((0, 15), dtype=torch.float32, device=self.dev)
            self.boxes = torch.zeros((R, 15), dtype=torch.float32, device=self.dev)          # the result pool
            self.counts_log = torch.full((R, 2), -1, dtype=torch.int32, device=self.dev)
            if R:
                first = torch.from_numpy(self.row0[:-1]).to(self.dev)
                self.boxes.index_copy_(0, first, self.gt.index_select(0, first))             # row 0 of every tracklet: its first box
            # the crop scratch of the worst step: every busy lane reads frame t and frame t - 1
            js, ts = self.schedule[0].astype(np.int64), self.schedule[1].astype(np.int64)
            rows = np.where(js >= 0, self.row0[np.maximum(js, 0)] + ts, -1)
            worst = self._pool.worst_scratch(np.concatenate([rows, rows - 1], 1))
            if self.scratch is None or self.scratch.numel() < worst:
                self.scratch = torch.empty((max(worst, 1),), dtype=torch.int32, device=self.dev)
            if self.free_running and hasattr(self, "bank_state"):
                self.bank_state.zero_()
            self._enter(0)
        return self.steps

    def _plan_chunk(self, c):
        """the tables of steps [c P, (c + 1) P) into the host buffer"""
        sl = slice(c * self.plan_steps, min((c + 1) * self.plan_steps, self.steps))
        addr = {"cur": self.cur.data_ptr(), "gt": self.gt.data_ptr(), "counts": self.counts_dev.data_ptr()}
        groups, need, starts = plan_lane_steps(self._tables, self.schedule[0][sl], self.schedule[1][sl], self.row0, self._pool,
                                               self._clouds(), addr, *self._rule)
        assert need.max() <= self.scratch.numel()                          # begin() sized it for the worst step
        S = sl.stop - sl.start
        self._groups[:S], self._starts[:S] = groups.tolist(), starts.tolist()

    def _enter(self, s):
        """what precedes step s: at a chunk boundary the chunk's one upload; where a lane starts a tracklet, its start"""
        if s >= self.steps:
            return
        k = s % self.plan_steps
        if k == 0:
            self._plan_chunk(s // self.plan_steps)
            upload(self._tables, self._tab)
            self.uploads += 1
        if self._starts[k]:
            PU.lane_start(self.gt, self._lane_rows[k], self.cur, self.yaw_state, self.canon_wlh,
                          self.bank_state[(s + 1) & 1] if hasattr(self, "bank_state") else None)

    # ---- the loop ----------------------------------------------------------------------------------------------------------
    def step(self):
        """Enqueue one step of the schedule: no host synchronisation, no copy to the host, and no upload outside a chunk
        boundary.  -> False when the epoch is done (the call that enqueued its last step included)."""
        if self.schedule is None:
            raise RuntimeError(self._NAME + ".step before begin")
        s = self.s
        if s >= self.steps:
            return False
        k = s % self.plan_steps
        with torch.cuda.device(self.dev):
            PU.crop_groups(self._plan_h[k, :self._groups[k]], self._tables.dev("plan", k), self.scratch)
            lanes = self._lane_rows[k]
            self._offset(lanes, self._feed(lanes, s & 1)[0])
            self.s = s + 1
            self._enter(self.s)
        return self.s < self.steps

    def run(self, tracklets, order="given"):
        """begin(), then every step -> the result pool (R,15), a device tensor; nothing is read back"""
        self.begin(tracklets, order)
        while self.step():
            pass
        return self.boxes

    def _offset(self, lanes, offset):
        c = self
        PU.offset_box_lanes(c.cur, c.gt, offset, c.yaw_state, lanes, c.cur, c.boxes, c.counts2, c.counts_log, degrees=c.degrees,
                            use_z=c.use_z, limit_box=c.limit_box, seed=c.seed)

    # ---- state and results -------------------------------------------------------------------------------------------------
    def set_box(self, lane, box):
        """Overwrite lane `lane`'s current box (teacher forcing in the tests): a device copy; its yaw state restarts from the
        box's rotation.  No result row changes."""
        self._restart(PU.pack_box(box, self.dev), lane, row=False)

    def _rows(self, j):
        return slice(int(self.row0[j]), int(self.row0[j + 1]))

    def results(self, j):
        """(T_j,15): tracklet j's rows of the result pool, a device VIEW; row 0 its first box, row t the result of frame t"""
        return self.boxes[self._rows(j)]

    def counts(self, j):
        """(T_j,2) int32 on the host: tracklet j's rows of the counts log, as the single trackers' counts() (one sync)"""
        return self.counts_log[self._rows(j)].cpu().numpy()

    def score(self, metrics=None):
        """Score the result pool against the ground-truth pool in ONE o3d_track_score launch (every tracklet's frame 0 scores
        its first box against itself, as the reference does); metrics: a SuccessPrecision that the same launch adds to.
        -> (overlaps (R), distances (R)) device tensors; no sync."""
        from . import metrics as MT
        return MT.score_boxes(self.gt, self.boxes, *_score_space(self.model.config), accumulate=metrics)


class LaneTracker(_Lanes, _MatchingTracker):
    """The test epoch of the matching trackers (trackers.BAT, trackers.P2B) on L lanes: SequenceTracker's free-running loop
    (sampling="device"), L tracklets wide, each lane on its own tracklet's frames.

        trk = LaneTracker(model, 4)             # model on the GPU, eval mode
        trk.run(tracklets)                      # every step enqueued; nothing read back
        boxes = trk.results(j)                  # (T_j,15) device view

    Per step, whatever L: o3d_track_crop_groups (3 launches: one group per (lane, cloud), the search window by the lane's
    reference box and the model crop of the previous frame by its own result box), o3d_track_bank_update_lanes,
    o3d_track_resample_drawn_lanes, o3d_boxcloud (BAT), the batch-L network as one replayed HIP graph,
    o3d_track_offset_box_lanes (which also writes the step's rows of the counts log); o3d_track_lane_start in front of a step
    on which a lane starts a tracklet.  An idle lane keeps its slot: no crop, no state change, no result.  The capacities are
    fixed, as for SequenceTracker(sampling="device"); overflow() reports what they cut.  reference_BB previous_gt / current_gt
    read the ground-truth pool on the device.  record_indices=True keeps the last step's indices in used_t (L,template_size)
    and used_s (L,search_size).  sampling="table": tables as the index sources of the resample launch -- every lane
    reads the two tables of SequenceTracker(sampling="table"), and its indices are the reference's."""
    _NAME = "LaneTracker"

    def __init__(self, model, lanes, seed=0, use_graph=None, search_capacity=32768, model_capacity=8192, bank_capacity=None,
                 record_indices=False, plan_steps=256, sampling="device"):
        _lane_sampling(sampling, self._NAME)
        _require_family(model, False, "LaneTracker")
        L = _KTargets._n_targets(lanes)
        super().__init__(model, seed, use_graph, 1, search_capacity, model_capacity, L, sampling, record_indices, bank_capacity)
        self._lane_state(L, plan_steps, *_reference_rule(self.reference_BB), self.aggregation != "first")

    def _clouds(self):
        """the clouds of plan_lane_steps: the search window of frame t, the model crop of frame t - 1 where the bank takes one"""
        c = self
        return ((0, True, c.search_bb_scale, c.search_bb_offset, PU.CROP_SUBWINDOW, c.search_buf.data_ptr(), c.search_buf.shape[1], False),
                (1, False, c.model_bb_scale, c.model_bb_offset, PU.CROP_MODEL, c.staging.data_ptr(), c.model_capacity, True))

    def overflow(self):
        """-> (truncated search crops, truncated model crops, frames on which a bank was full) over all tracklets, on the host
        from the counts log and the capacities (one sync)"""
        log = self.counts_log.cpu().numpy()
        per = [_matching_overflow(log[self._rows(j)], self.search_buf.shape[1], self.model_capacity, self.bank_capacity, self.aggregation)
               for j in range(len(self.lengths))]
        return tuple(int(sum(p[i] for p in per)) for i in range(3))


class MotionLaneTracker(_Lanes, _MotionTracker):
    """The test epoch of the motion tracker (m2track.M2TRACK) on L lanes: MotionSequenceTracker's free-running loop, L
    tracklets wide.  The surface is LaneTracker's.  Per step: o3d_track_crop_groups (3 launches: the previous and the current
    frame of every busy lane by its last result box), o3d_track_motion_input_drawn_lanes, the batch-L network as one replayed
    HIP graph, o3d_track_offset_box_lanes.  `capacity` is the fixed size of every crop buffer; record_indices=True keeps the
    last step's indices in used (L,2N).  sampling="table": a table as the index source, every lane and both halves on
    the one table of MotionSequenceTracker(sampling="table")."""
    _NAME = "MotionLaneTracker"

    def __init__(self, model, lanes, seed=0, use_graph=None, capacity=32768, record_indices=False, plan_steps=256, sampling="device"):
        _lane_sampling(sampling, self._NAME)
        _require_family(model, True, "MotionLaneTracker")
        L = _KTargets._n_targets(lanes)
        super().__init__(model, seed, use_graph, 1, capacity, L, sampling, record_indices)
        self._lane_state(L, plan_steps)

    def _clouds(self):
        c, cap = self, self.crop_buf.shape[2]
        return tuple((1 - h, True, c.bb_scale, c.bb_offset, PU.CROP_SUBWINDOW, c.crop_buf[h].data_ptr(), cap, False) for h in (0, 1))

    def overflow(self):
        """-> (truncated previous-frame crops, truncated current-frame crops, 0) over all tracklets (one sync)"""
        log, cap = self.counts_log.cpu().numpy(), self.crop_buf.shape[2]
        return int((log[:, 0] > cap).sum()), int((log[:, 1] > cap).sum()), 0


# ---- K targets of one live scene, free-running -----------------------------------------------------------
def _scene_sampling(name, who):
    """the `sampling` keyword of a scene tracker, checked before anything else: the free-running modes only"""
    if _sampling(name) not in FREE_RUNNING:
        raise ValueError("%s: sampling=\"reference\" reads 2K counts back per frame, which is the loop of MultiTargetTracker / "
                         "MultiMotionTracker; expected \"device\" or \"table\"" % who)
    return name


def scene_lane_rows(K, first=(), aggregation=None):
    """The (K, LANE_COLS) int32 lane table of one frame of a scene tracker, a pure function: `active` is 1 for every slot (a
    retired slot keeps running, only its box update is off, which o3d_track_offset_box_multi's own `active` decides), `first`
    is 1 for the slots in `first` (every slot at t = 1, later the freshly enrolled ones), `has_crop` = first or aggregation !=
    "first" (aggregation None, the motion tracker: both crops are made on every frame).  The columns of the epoch plan (t, row,
    ref_row, rebase) are not read by the launches of a scene frame: 0, -1, -1, 0."""
    rows = np.zeros((int(K), PU.LANE_COLS), np.int32)
    is_first = np.zeros((int(K),), bool)
    is_first[sorted(first)] = True
    rows[:, PU.LANE["active"]] = 1
    rows[:, PU.LANE["first"]] = is_first
    rows[:, PU.LANE["has_crop"]] = is_first | (aggregation != "first")
    rows[:, PU.LANE["row"]] = rows[:, PU.LANE["ref_row"]] = -1
    return rows


def scene_matching_overflow(log, starts, search_capacity, model_capacity, bank_capacity, aggregation):
    """log (t,K,2): the counts of a SceneTracker; starts (K,): the frame after which slot k began to follow its object (0, or the
    frame an enroll() followed) -> (K,3): _matching_overflow of every slot on its own rows, from its start frame on"""
    return np.array([_matching_overflow(log[int(s):, k], search_capacity, model_capacity, bank_capacity, aggregation)
                     for k, s in enumerate(starts)], np.int64).reshape(-1, 3)


def scene_motion_overflow(log, starts, capacity):
    """scene_matching_overflow for a MotionSceneTracker, by MotionLaneTracker.overflow's rule -> (K,3): (previous-frame cuts,
    current-frame cuts, 0) of every slot from its start frame on"""
    return np.array([[int((log[int(s) + 1:, k, 0] > capacity).sum()), int((log[int(s) + 1:, k, 1] > capacity).sum()), 0]
                     for k, s in enumerate(starts)], np.int64).reshape(-1, 3)


class _Scene(_KTargets):
    """What SceneTracker and MotionSceneTracker put on top of _KTargets (the pack of K boxes, set_box, retire, the pinned target
    table) and of their free-running bases' state with a leading K axis:

      the fixed crop table    2K o3d_crop_target records whose pointers never change (boxes in fixed (K,15) buffers, outs in
                              fixed buffers, counts in counts_dev laid out lane-major (K,2)): filled and uploaded ONCE, by the
                              constructor
      the lane table          (K, LANE_COLS) on the device, scene_lane_rows of the slots with a pending `first`; rewritten on
                              events only (the first frame, the frame after a `first`, the frame after an enroll())
      enroll                  a slot takes a NEW object from the most recent frame, with device writes only
      the counts log          counts_log (T,K,2), row t written by stream-ordered device copies
      the frame               _update, written once for both families: what differs is the family's (_MatchingTracker /
                              _MotionTracker: _crop_groups, _FRAME_GROUP, _GATED, _feed) and SceneTracker's _reference
      overflow                per slot, from the slot's own start frame"""

    def _scene_state(self, K, groups):
        """groups: the family's _crop_groups; group g counts into column g"""
        self._k_state(K)
        self.counts2 = self.counts_dev.view(K, 2)
        kk = np.arange(K, dtype=np.uint64)
        self._groups = []
        for g, (boxes, scale, offset, mode, out) in enumerate(groups):
            cap = out.shape[1]
            self._groups.append(self._crop_group(g, boxes, scale, offset, mode, out.data_ptr() + 12 * cap * kk, cap))
            self.crop_rec["count"][g * K:(g + 1) * K] = self.counts_dev.data_ptr() + 4 * (2 * kk + np.uint64(g))      # lane-major
        self.crop_tab.copy_(self.crop_tab_host)                            # the one upload of the table
        self.lanes = torch.zeros((K, PU.LANE_COLS), dtype=torch.int32, device=self.dev)
        self.lane_uploads = 0
        self._pending, self._on_device, self._cropped = set(), None, True
        self._start = np.zeros((K,), np.int64)

    def init(self, points0, boxes0):
        boxes = super().init(points0, boxes0)
        self._pending, self._on_device = set(range(self.K)), None          # t = 1 is every slot's first tracked frame
        self._start[:] = 0
        self.lane_uploads = 0                              # since init, as crop_calls
        return boxes

    def enroll(self, k, box):
        """Slot k starts following a NEW object from the most recent frame (`prev_points`): slot k's init.  Its last box, yaw
        state, canonical wlh and row t - 1 of the results are set from `box`, its template bank restarts empty, it is active
        again, and its NEXT update() is its first tracked frame (the bank's `first` branch; the motion tracker's prior
        targetness 1 / 0).  Device writes and, for a host box, one asynchronous copy from pinned memory: nothing is read back."""
        if self.t < 1:
            raise RuntimeError(self._NAME + ".enroll before init")
        k = int(k) % self.K
        with torch.cuda.device(self.dev):
            if torch.is_tensor(box) and box.is_cuda:
                b = PU.pack_box(box, self.dev)
            else:
                b = PU.pack_box(box, "cpu").pin_memory().to(self.dev, non_blocking=True)
            self._restart(b, k)
            self.canon_wlh[k].copy_(b[3:6])
            if hasattr(self, "bank_state"):
                self.bank_state[(self.t + 1) & 1, k].zero_()               # the slot the next frame reads as state_in
            self.active[k] = 1
        self.retired.discard(k)
        self._pending.add(k)
        self._start[k] = self.t - 1

    def _lane_event(self):
        """the lane table of this frame, uploaded only where it differs from the one on the device -> (lanes, the slots with
        has_crop, on the host: True = every slot, else their list)"""
        first = frozenset(self._pending)
        if first != self._on_device:
            rows = scene_lane_rows(self.K, first, self.aggregation)
            self.lanes.copy_(torch.from_numpy(rows).pin_memory(), non_blocking=True)
            cropped = np.flatnonzero(rows[:, PU.LANE["has_crop"]]).tolist()
            self._on_device, self._cropped = first, True if len(cropped) == self.K else cropped
            self.lane_uploads += 1
        return self.lanes, self._cropped

    def _crop_scene(self, clouds):
        """the frame's one o3d_track_crop_multi call: clouds[g] | None = the points of group g of the fixed table"""
        self.scratch = PU.crop_multi([(pts, self._groups[g]) for g, pts in enumerate(clouds) if pts is not None], self.scratch)
        self.crop_calls += 1

    # ---- one frame ---------------------------------------------------------------------------------------------------------
    ref = None                # SceneTracker: its own (K,15) buffer, which the fixed table points at and _reference fills
    _ALL_MADE = (True, True)  # _log_scene_counts' `made` of a frame that makes both groups for every slot

    def _update(self, pts, ref_boxes=None):
        """The frame of a live scene, whichever family: the reference boxes (the last ones where the class keeps no `ref`), the
        lane table (uploaded on an event only), the one crop call, the counts log, the family's _feed, the one box update."""
        c = self
        c._grow_boxes()
        ref = c.cur if c.ref is None else c._reference(ref_boxes)
        lanes, cropped = c._lane_event()
        clouds, made, g = [c.prev_points, c.prev_points], c._ALL_MADE, c._GATED
        clouds[c._FRAME_GROUP] = pts
        if cropped is not True and g is not None:          # the family's gated group: made for the slots in `cropped` only
            made = [True, True]
            made[g] = cropped
            if not cropped:
                clouds[g] = None
        c._crop_scene(clouds)
        c._log_scene_counts(made)
        offsets, state_out = c._feed(lanes, c.t & 1)
        c._offset_box(ref, offsets, c.rebase_all if ref_boxes is not None else None)
        return c._frame_done(pts, state_out)

    def _log_scene_counts(self, made):
        """row t of the counts log: column g of every slot where made[g] is True, of the slots made[g] lists otherwise"""
        row = self.counts_log[self.t]
        if made is self._ALL_MADE or all(m is True for m in made):
            row.copy_(self.counts2)
            return
        for g, m in enumerate(made):
            if m is True:
                row[:, g].copy_(self.counts2[:, g])
            else:
                for k in m:
                    row[k, g:g + 1].copy_(self.counts2[k, g:g + 1])

    def _frame_done(self, pts, state_out):
        self._pending.clear()
        return self._done(pts, None)

    def counts(self):
        """(t,K,2) int32 on the host: row f the two crop counts of every slot at frame f, as the crop kernel counted them (before
        the cut to the capacities), -1 where no crop was made.  One sync."""
        return self.counts_log[:self.t].cpu().numpy()

    def overflow(self, per_target=False):
        """How often a fixed capacity cut something, on the host from counts() and the capacities (one sync): three sums over
        the targets, as LaneTracker.overflow; per_target=True -> (K,3), row k worked out on slot k's rows from its own start
        frame (0, or the frame its last enroll() followed)."""
        per = self._overflow_rows(self.counts())
        return per if per_target else tuple(int(v) for v in per.sum(0))


class SceneTracker(_Scene, _MatchingTracker):
    """K targets of one live scene, free-running (the matching trackers: trackers.BAT, trackers.P2B): MultiTargetTracker's
    loop without its host stop.  Frames arrive one at a time, nothing is read back, nothing is uploaded per frame.

        trk = SceneTracker(model, K)            # sampling="device" | "table"; model on the GPU, eval mode
        trk.init(points0, boxes0)               # as MultiTargetTracker
        boxes = trk.update(points)              # a (K,15) device VIEW of the new boxes: the frame is only ENQUEUED
        trk.retire(1); trk.enroll(1, box)       # slot 1 stops, then follows a new object from the most recent frame
        all_boxes = trk.results()               # (T,K,15) on the host, one sync

    Per frame t >= 1, whatever K:

      a device copy into ref (K,15)     the last boxes, or the caller's ref_boxes (a device tensor keeps the loop free of host
                                        stops) with the retired rows replaced by their last boxes
      o3d_track_crop_multi, one call    group 0: frame t against ref into search_buf (K,search_capacity,3); group 1 (only when
                                        some slot takes a model crop): frame t-1 against the last boxes into staging
                                        (K,model_capacity,3).  Its target table was uploaded once, by the constructor.
      device copies of the counts       row t of counts_log (T,K,2)
      o3d_track_bank_update_lanes       on the lane table of _Scene; bank_state (2,K,2) alternates by frame parity
      o3d_track_resample_drawn_lanes    or its table twin: the index source is chosen once (draw_src)
      o3d_boxcloud, forward + o3d_best_proposal at batch K    one replayed HIP graph (eager when the capture fails, unless
                                        O3D_REQUIRE_GRAPH=1)
      o3d_track_offset_box_multi        MultiTargetTracker's call: device frame counter, per-target active and rebase

    Every lane kernel hands slot k's operands to the device function of the single-target form, so row k is a single
    free-running SequenceTracker's row; with sampling="table" and nothing cut (overflow() == (0, 0, 0)) the inputs and boxes are
    MultiTargetTracker's bit for bit.  The capacities are fixed, as for SequenceTracker(sampling="device").  `seed`: target k's
    limit_box draws use seed + k; under "device" it also keys the index draws, the same two keys for every slot.
    record_indices=True keeps the last frame's indices in used_t (K,template_size) / used_s (K,search_size)."""
    _NAME, _REF_KW = "SceneTracker", "ref_boxes"

    def __init__(self, model, n_targets, seed=0, use_graph=None, max_frames=1024, search_capacity=32768, model_capacity=8192,
                 bank_capacity=None, sampling="device", record_indices=False):
        _scene_sampling(sampling, self._NAME)
        _require_family(model, False, "SceneTracker")
        K = self._n_targets(n_targets)
        super().__init__(model, seed, use_graph, max_frames, search_capacity, model_capacity, K, sampling, record_indices,
                         bank_capacity)
        self.ref = torch.zeros((K, 15), dtype=torch.float32, device=self.dev)
        self.rebase_all = torch.ones((K,), dtype=torch.int32, device=self.dev)
        self._scene_state(K, self._crop_groups(self.ref))

    def update(self, points, ref_boxes=None):
        return self._run(points, ref_boxes)

    def _reference(self, ref_boxes):
        """a device copy into ref (K,15), which the fixed table points at: the last boxes, or the caller's"""
        c = self
        c.ref.copy_(c.cur if ref_boxes is None else c._pack(ref_boxes))
        if ref_boxes is not None:
            for k in sorted(c.retired):                    # a retired target's reference is its own last box, not the caller's
                c.ref[k].copy_(c.cur[k])
        return c.ref

    def _overflow_rows(self, log):
        return scene_matching_overflow(log, self._start, self.search_buf.shape[1], self.model_capacity, self.bank_capacity,
                                       self.aggregation)


class MotionSceneTracker(_Scene, _MotionTracker):
    """K targets of one live scene, free-running, for the motion tracker (m2track.M2TRACK): MultiMotionTracker's loop without
    its host stop.  The surface is SceneTracker's (no ref_boxes: the motion tracker always starts from its last result).  Per
    frame: o3d_track_crop_multi, one call on the fixed table (group 0: frame t-1, group 1: frame t, both against the last
    boxes, into crop_buf (2,K,capacity,3), the counts lane-major (K,2)), a device copy of the counts into row t of counts_log,
    o3d_track_motion_input_drawn_lanes or its table twin on the lane table (`first` per slot: the prior targetness of a slot's
    first tracked frame is 1 / 0), the batch-K forward as one replayed HIP graph, o3d_track_offset_box_multi.
    record_indices=True keeps the last frame's indices in used (K,2N)."""
    _NAME = "MotionSceneTracker"

    def __init__(self, model, n_targets, seed=0, use_graph=None, max_frames=1024, capacity=32768, sampling="device",
                 record_indices=False):
        _scene_sampling(sampling, self._NAME)
        _require_family(model, True, "MotionSceneTracker")
        K = self._n_targets(n_targets)
        super().__init__(model, seed, use_graph, max_frames, capacity, K, sampling, record_indices)
        self._scene_state(K, self._crop_groups(self.cur))

    def update(self, points):
        return self._run(points)

    def _overflow_rows(self, log):
        return scene_motion_overflow(log, self._start, self.crop_buf.shape[2])


# ---- the slots' lifecycle on the device: associate detections, retire, enroll ------------------------------
_MANAGE_DEFAULTS = dict(min_iou=0.0, max_dist=float("inf"), max_misses=2, min_points=0, max_starved=0, enroll=True, max_detections=256,
                        assignment="greedy", cost="distance")


def _unit_box():
    """the box a free slot holds until a detection takes it: centre 0, wlh (1,1,1), identity"""
    b = np.zeros((15,), np.float32)
    b[3:6], b[[6, 10, 14]] = 1.0, 1.0
    return b


class _Managed:
    """What ManagedSceneTracker and ManagedMotionSceneTracker put on top of a scene tracker: per frame, after the box update, two
    launches (o3d_scene_pair_scores, o3d_scene_manage) that match the frame's detections with the K tracks, count missed frames
    and starved crops, retire the lost slots, enroll the unmatched detections into the free slots with SceneTracker.enroll's
    writes, and write the NEXT frame's lane table.  The frame is _Scene._update with three differences, each one override here:
    the lane table belongs to the device (_lane_event uploads nothing, no _pending), both crop groups are made on every frame,
    because the host no longer knows which slot is `first`, and _frame_done runs _manage by the family's _FRAME_GROUP / aggregation.

      slot (K,4) int32        {id, misses, starved, start} per slot, id -1 = free; `active` stays id >= 0
      next_id (1,) int32      the next track id
      ids_log, match_log (T,K), dropped_log (T,)    row t: who held slot k after frame t, the detection it matched, the
                                                     detections that found no free slot; they grow with `boxes`

    manage = dict(min_iou, max_dist, max_misses, min_points, max_starved, enroll, max_detections, assignment, cost); the overlap
    and the distance are metrics.score_boxes' with the model config's IoU_space / up_axis, as in score().  assignment="optimal"
    matches by the maximum-cardinality, minimum-cost assignment under cost = "distance" | "overlap" 
    instead of the greedy walk: still two launches per frame, no host stop, no upload."""

    def _managed_state(self, manage):
        from . import metrics as MT
        p = dict(_MANAGE_DEFAULTS)
        unknown = set(manage or {}) - set(p)
        if unknown:
            raise ValueError("%s: manage has no %s; expected %s" % (self._NAME, sorted(unknown), sorted(p)))
        p.update(manage or {})
        self.max_detections = int(p.pop("max_detections"))
        if not 1 <= self.max_detections <= PU.SCENE_MAX_DETECTIONS:
            raise ValueError("%s: max_detections must be 1..%d" % (self._NAME, PU.SCENE_MAX_DETECTIONS))
        PU._assign_args(p["assignment"], p["cost"], self._NAME)
        self.manage = dict(min_iou=float(p["min_iou"]), max_dist=float(p["max_dist"]), max_misses=int(p["max_misses"]),
                           min_points=int(p["min_points"]), max_starved=int(p["max_starved"]), enroll=bool(p["enroll"]),
                           assignment=p["assignment"], cost=p["cost"])
        self.score_dim, self._up_axis = _score_space(self.model.config)
        self.score_up = MT.up_index(self._up_axis)
        K, T, i32 = self.K, self.boxes.shape[0], dict(dtype=torch.int32, device=self.dev)
        self.slot = torch.zeros((K, PU.SCENE_SLOT_COLS), **i32)
        self.next_id = torch.zeros((1,), **i32)
        self.n_det = torch.zeros((1,), **i32)
        self.ids_log, self.match_log = torch.full((T, K), -1, **i32), torch.full((T, K), -1, **i32)
        self.dropped_log = torch.zeros((T,), **i32)
        self._pairs = torch.empty((2, K * self.max_detections), dtype=torch.float32, device=self.dev)
        self._no_dets = torch.empty((0, 15), dtype=torch.float32, device=self.dev)

    def init(self, points0, boxes0):
        """n0 <= K boxes: slot k < n0 follows boxes0[k] with id k; the other slots are free and hold the unit box."""
        b = _boxes15(boxes0, self.dev)
        n0, K = b.shape[0], self.K
        if n0 > K:
            raise ValueError("%d boxes for %d slots" % (n0, K))
        padded = torch.from_numpy(np.tile(_unit_box(), (K, 1))).to(self.dev)
        padded[:n0].copy_(b)
        boxes = super().init(points0, padded)
        self._pending = set()                              # the parent's host copy of `first`: not kept here, the device owns it
        occupied = np.arange(K) < n0
        slot = np.zeros((K, PU.SCENE_SLOT_COLS), np.int32)
        slot[:, 0] = np.where(occupied, np.arange(K), -1)
        self.slot.copy_(torch.from_numpy(slot))
        self.active.copy_(torch.from_numpy(occupied.astype(np.int32)))
        self.next_id.fill_(n0)
        self.ids_log.fill_(-1)
        self.match_log.fill_(-1)
        self.dropped_log.zero_()
        self.ids_log[0].copy_(self.slot[:, 0])
        self.lanes.copy_(torch.from_numpy(scene_lane_rows(K, np.flatnonzero(occupied).tolist(), self.aggregation)))
        return boxes

    def _grow_boxes(self):
        T = self.boxes.shape[0]
        super()._grow_boxes()
        if self.boxes.shape[0] != T:                       # the three logs grow with boxes
            for name, fill in (("ids_log", -1), ("match_log", -1), ("dropped_log", 0)):
                old = getattr(self, name)
                log = torch.full((self.boxes.shape[0],) + old.shape[1:], fill, dtype=torch.int32, device=self.dev)
                log[:T].copy_(old)
                setattr(self, name, log)

    def update(self, points, detections=None, n_detections=None, ref_boxes=None):
        """One frame, only enqueued.  detections: (D,15) boxes, D <= max_detections, or None (no detection set for this frame:
        nothing is matched, missed or enrolled; the starvation rule and the lane table still run).  A device float32 tensor
        keeps the frame free of host stops; a host array or a list of boxes travels as one asynchronous copy from pinned
        memory.  n_detections: None (= D), an int, or a device int32 (1,) tensor: the first n_detections rows count.
        -> a (K,15) device VIEW of the boxes after the frame, the enrolled ones included."""
        if ref_boxes is not None:                          # in front of the detections' checks, and those in front of _run's
            raise ValueError("%s.update takes no ref_boxes: a managed tracker starts every slot from its own last box" % self._NAME)
        return self._run(points, self._detections(detections), n_detections)

    def _check(self, dets, n_detections):
        """nothing is left for _run to check: update() has refused ref_boxes, which the parent's _check would ask for"""

    def _detections(self, detections):
        """the checks of update()'s detection set, before anything touches the device -> a (D,15) float32 tensor | None"""
        if detections is None:
            return None
        d = _boxes15(detections, "cpu", keep=True)
        if d.shape[0] > self.max_detections:
            raise ValueError("%s.update: %d detections for max_detections = %d" % (self._NAME, d.shape[0], self.max_detections))
        return d

    def _update(self, pts, dets, n_detections):
        """the detections onto the device (_dets: what _frame_done hands to _manage), then the scene tracker's frame"""
        if dets is not None and not dets.is_cuda:
            dets = dets.pin_memory().to(self.dev, non_blocking=True)
        n_det = self.n_det
        if dets is not None and torch.is_tensor(n_detections):
            PU._i32(n_detections, 1, self._NAME + ".update")
            n_det = n_detections
        elif dets is not None:
            n_det.fill_(dets.shape[0] if n_detections is None else int(n_detections))
        self._dets = (dets, n_det)
        return super()._update(pts)

    def _lane_event(self):
        """the lane table is the device's (o3d_scene_manage writes the next frame's): no upload, every group for every slot"""
        return self.lanes, True

    def _frame_done(self, pts, state_out):
        """the family's rule: a slot starves on the count of its crop of the frame; its bank restarts in state_out (None: no bank)"""
        self._manage(*self._dets, self._FRAME_GROUP, state_out, self.aggregation)
        return self._done(pts, None)

    def _manage(self, dets, n_det, count_col, bank_state_next, rule):
        """the two management launches of a frame, after its box update"""
        has = dets is not None
        if not has:
            dets = self._no_dets
        K, D = self.K, dets.shape[0]
        ov, di = (self._pairs[i, :K * D].view(K, D) for i in (0, 1))
        if D:
            PU.scene_pair_scores(self.cur, self.active, dets, n_det, self.score_dim, self.score_up, out=(ov, di))
        PU.scene_manage(ov, di, dets, n_det, self.cur, self.yaw_state, self.canon_wlh, self.boxes, self.frame, self.active, self.slot,
                        self.next_id, self.counts2, count_col, bank_state_next, self.lanes, rule, self.ids_log, self.match_log,
                        self.dropped_log, has_dets=has, **self.manage)

    # ---- manual events: the parent's device writes plus the slot row, the lane row and the id ---------------------------------------
    def enroll(self, k, box):
        """SceneTracker.enroll as device writes into the managed state: slot k takes the next id."""
        super().enroll(k, box)
        k = int(k) % self.K
        self._pending.clear()                              # `first` is written into the device's lane row below
        with torch.cuda.device(self.dev):
            self.slot[k].zero_()
            self.slot[k, 0:1].copy_(self.next_id)
            self.slot[k, 3] = self.t - 1
            self.next_id += 1
            self.lanes[k, PU.LANE["first"]] = 1
            self.lanes[k, PU.LANE["has_crop"]] = 1
            self.ids_log[self.t - 1, k:k + 1].copy_(self.slot[k, 0:1])

    def retire(self, k):
        """SceneTracker.retire, and slot k is free: a later detection may take it."""
        super().retire(k)
        self.slot[int(k) % self.K, 0] = -1

    # ---- read-backs, one sync each -----------------------------------------------------------------------------------------------------
    def status(self):
        """{active, ids, misses, starved, start}, each (K,) int32 on the host"""
        s = torch.cat([self.active.view(-1, 1), self.slot], 1).cpu().numpy()
        return dict(active=s[:, 0], ids=s[:, 1], misses=s[:, 2], starved=s[:, 3], start=s[:, 4])

    def events(self):
        """(ids_log (t,K), match_log (t,K), dropped_log (t,)) int32 on the host, rows [0:t]"""
        t, K = self.t, self.K
        e = torch.cat([self.ids_log[:t], self.match_log[:t], self.dropped_log[:t, None]], 1).cpu().numpy()
        return e[:, :K], e[:, K:2 * K], e[:, 2 * K]

    def tracks(self):
        """{id: (first_frame, boxes (n,15))}: every object ever followed, its boxes from the frame it was enrolled on (or 0) to
        the last frame its slot carried its id, from results() and ids_log"""
        res, ids = self.results(), self.events()[0]
        out = {}
        for f, k in zip(*np.nonzero(ids >= 0)):
            out.setdefault(int(ids[f, k]), (int(f), []))[1].append(res[f, k])
        return {i: (f, np.stack(rows)) for i, (f, rows) in out.items()}

    def score_mot(self, gt_boxes, valid=None, metrics=None, **gates):
        """Score rows [0:t] of the run against gt_boxes (t,G,15), where they are: boxes[:t] and ids_log[:t] go to a
        metrics.ClearMOT, whose overlap and distance are the model config's, as in score().  A slot
        follows no fixed object here, so G need not be K.  valid (t,G) | None: 0 where an object has no annotation.  metrics:
        a ClearMOT to add to | None: a new one with **gates (min_iou, max_dist, keep_logs, sot, assignment, cost).  Device tensors travel as they
        are: no host stop and no upload.  -> the ClearMOT; compute() is its one read-back."""
        from . import metrics as MT
        gt = PU._dev32(gt_boxes, self.dev)
        if gt.dim() != 3 or gt.shape[0] != self.t or gt.shape[2] != 15:
            raise ValueError("%s.score_mot: gt_boxes %s for %d frames" % (self._NAME, tuple(gt.shape), self.t))
        if valid is not None:
            valid = torch.as_tensor(valid).to(self.dev)
        if metrics is None:
            metrics = MT.ClearMOT(gt.shape[1], self.dev, dim=self.score_dim, up_axis=self._up_axis, **gates)
        elif gates:
            raise ValueError("%s.score_mot: the gates %s belong to the ClearMOT that is passed" % (self._NAME, sorted(gates)))
        elif (metrics.dim, metrics.up) != (self.score_dim, self.score_up):
            raise ValueError("%s.score_mot: the ClearMOT scores dim %d, up %d; the model config says %d, %d"
                             % (self._NAME, metrics.dim, metrics.up, self.score_dim, self.score_up))
        metrics.update(gt, valid, self.boxes[:self.t], self.ids_log[:self.t])
        return metrics

    def overflow(self, per_target=False):
        """the scene tracker's overflow(), with every slot's start frame taken from `slot`"""
        self._start[:] = self.status()["start"]
        return super().overflow(per_target)


class ManagedSceneTracker(_Managed, SceneTracker):
    """SceneTracker with the slots' lifecycle on the device:

        trk = ManagedSceneTracker(model, K, manage=dict(max_misses=1, max_dist=3.0))
        trk.init(points0, boxes0)                          # n0 <= K boxes; the other slots are free
        boxes = trk.update(points, detections, n)          # detections (D,15) and n (1,) int32 on the device: no host stop
        trk.status(); trk.events(); trk.tracks()           # one sync each

    A frame is SceneTracker's with the model crop made for every slot, followed by the two management launches of _Managed.  A
    free slot still runs through the crops and the batch-K forward (the batch keeps its shape)."""
    _NAME = "ManagedSceneTracker"

    def __init__(self, model, n_targets, manage=None, **kw):
        super().__init__(model, n_targets, **kw)
        if self.needs_ref_box:
            raise ValueError("%s: reference_BB %r needs the caller's ref_boxes, which a managed tracker does not take"
                             % (self._NAME, self.reference_BB))
        self._managed_state(manage)

    def _overflow_rows(self, log):
        if self.aggregation == "first":        # the model crop is made on every frame, but banked on a slot's first frame only
            log = log.copy()
            for k, s in enumerate(self._start):
                log[int(s) + 2:, k, 1] = -1
        return super()._overflow_rows(log)


class ManagedMotionSceneTracker(_Managed, MotionSceneTracker):
    """MotionSceneTracker with the slots' lifecycle on the device: ManagedSceneTracker's surface for the motion tracker.  The
    starvation rule reads the current-frame crop's count (column 1); there is no template bank to restart."""
    _NAME = "ManagedMotionSceneTracker"

    def __init__(self, model, n_targets, manage=None, **kw):
        super().__init__(model, n_targets, **kw)
        self._managed_state(manage)


def tracker_for(model, **kw):
    """the tracker class of a model: MotionSequenceTracker for m2track.M2TRACK, SequenceTracker for the matching trackers"""
    return (MotionSequenceTracker if _is_motion(model) else SequenceTracker)(model, **kw)


def multi_tracker_for(model, n_targets, **kw):
    """tracker_for for K targets: MultiMotionTracker for m2track.M2TRACK, MultiTargetTracker for the matching trackers"""
    return (MultiMotionTracker if _is_motion(model) else MultiTargetTracker)(model, n_targets, **kw)


def scene_tracker_for(model, n_targets, **kw):
    """the scene tracker class of a model: MotionSceneTracker for m2track.M2TRACK, SceneTracker for the matching trackers"""
    return (MotionSceneTracker if _is_motion(model) else SceneTracker)(model, n_targets, **kw)


def managed_scene_tracker_for(model, n_targets, **kw):
    """scene_tracker_for with the slots' lifecycle on the device: ManagedMotionSceneTracker for m2track.M2TRACK,
    ManagedSceneTracker for the matching trackers; kw: the scene tracker's keywords and manage=dict(...)"""
    return (ManagedMotionSceneTracker if _is_motion(model) else ManagedSceneTracker)(model, n_targets, **kw)


def lane_tracker_for(model, lanes, **kw):
    """the lane tracker class of a model: MotionLaneTracker for m2track.M2TRACK, LaneTracker for the matching trackers"""
    return (MotionLaneTracker if _is_motion(model) else LaneTracker)(model, lanes, **kw)


def track_sequence(model, frames, box0, ref_boxes=None, seed=0, use_graph=None, sampling="reference"):
    """The convenience loop: frames = a sequence of (N_t,3) GPU tensors, box0 the target's box in frames[0]; ref_boxes[t]
    (optional, matching trackers only) is handed to update() of frame t.  The tracker class follows the model's type.
    sampling: "reference" (numpy's index draw, one host sync per frame) | "device" (the free-running loop, its own draw) |
    "table" (the free-running loop on the reference's draw, read from a device table).
    -> (T,15) result boxes on the host."""
    trk = tracker_for(model, seed=seed, use_graph=use_graph, sampling=sampling)
    _drive(trk, frames, box0, ref_boxes)
    return trk.results()


def _drive(trk, frames, box0, refs=None, retire=None, by_rule=False):
    """The frame loop of every convenience function: trk.init(frames[0], box0), then one update() per frame, with refs[t] where
    refs is given.  by_rule: refs is the ground truth and the tracker's reference_BB decides (generate_search_area,
    models/base_model.py:208-214): nothing under previous_result (and for a motion tracker), refs[t - 1] under previous_gt,
    refs[t] under current_gt.  retire (T,K) bool on the host | None: a target is retired in front of its first False frame."""
    back = 0
    if by_rule:
        by_gt, back = _reference_rule(trk.reference_BB) if hasattr(trk, "reference_BB") else (False, 0)
        refs = refs if by_gt else None
    elif refs is not None and isinstance(trk, _MotionTracker):
        raise ValueError("the motion tracker always starts from its previous result: ref_boxes is not supported")
    trk.init(frames[0], box0)
    for t in range(1, len(frames)):
        if retire is not None:
            for k in np.flatnonzero(retire[t - 1] & ~retire[t]):
                trk.retire(int(k))
        if refs is None:
            trk.update(frames[t])
        else:
            trk.update(frames[t], refs[t - back])


def track_targets(model, frames, boxes0, ref_boxes=None, seed=0, use_graph=None, sampling="reference"):
    """track_sequence for K targets in the same frames: boxes0 (K,15) the targets' boxes in frames[0]; ref_boxes[t] (K,15)
    (optional, matching trackers only) is handed to update() of frame t.  The tracker class follows the model's type.
    -> (T,K,15) result boxes on the host."""
    return _track_k(multi_tracker_for, model, frames, boxes0, ref_boxes, seed=seed, use_graph=use_graph, sampling=sampling)


def _track_k(make, model, frames, boxes0, ref_boxes, **kw):
    """the loop of track_targets / track_scene on make(model, K, **kw)"""
    b0 = boxes0 if torch.is_tensor(boxes0) or isinstance(boxes0, np.ndarray) else list(boxes0)
    trk = make(model, len(b0), **kw)
    _drive(trk, frames, b0, ref_boxes)
    return trk.results()


def track_scene(model, frames, boxes0, ref_boxes=None, seed=0, use_graph=None, sampling="device", **capacities):
    """track_targets on a scene tracker (SceneTracker / MotionSceneTracker by the model's type): the K targets of one scene
    free-running, sampling "device" | "table"; capacities: the tracker's fixed sizes (under "table" also the sizes of its draw
    tables).  ref_boxes[t] as a device tensor keeps the loop free of host stops.  -> (T,K,15) result boxes on the host."""
    _scene_sampling(sampling, "track_scene")
    return _track_k(scene_tracker_for, model, frames, boxes0, ref_boxes, seed=seed, use_graph=use_graph, sampling=sampling,
                    **capacities)


def _track_with_gt(trk, frames, gt):
    """the frame loop of evaluate_one_sequence on `trk`: it starts from gt[0]; under reference_BB previous_gt / current_gt the
    matching ground-truth box goes to update() (generate_search_area, models/base_model.py:208-214).  gt: (T[,K],15) on the
    tracker's device."""
    if len(frames) != gt.shape[0]:
        raise ValueError("%d frames, %d ground-truth boxes" % (len(frames), gt.shape[0]))
    _drive(trk, frames, gt[0], gt, by_rule=True)


def evaluate_sequence(model, frames, gt_boxes, seed=0, use_graph=None, tracker=None, metrics=None, sampling="reference"):
    """The device form of evaluate_one_sequence (models/base_model.py:59-86): frames = a sequence of (N_t,3) GPU tensors,
    gt_boxes (T,15) host or device.  The tracker starts from gt_boxes[0], follows the config's reference_BB rule, and the
    whole sequence is scored ONCE at its end, on the device (frame 0 scores the first box against itself, as the reference
    does).  tracker: one to reuse (its captured graph with it) | None: tracker_for(model).  metrics: a SuccessPrecision to add to.
    -> (ious (T), distances (T), results (T,15)) device tensors; no sync beyond the tracker's own."""
    _sampling(sampling)
    trk = tracker if tracker is not None else tracker_for(model, seed=seed, use_graph=use_graph, sampling=sampling)
    gt = PU._dev32(gt_boxes, trk.dev).reshape(-1, 15)
    _track_with_gt(trk, frames, gt)
    ious, distances = trk.score(gt, metrics=metrics)
    return ious, distances, trk.boxes[:trk.t]


def evaluate_targets(model, frames, gt_boxes, valid=None, seed=0, use_graph=None, tracker=None, metrics=None, sampling="reference"):
    """evaluate_sequence over track_targets: gt_boxes (T,K,15), the K targets' boxes in the same frames.  valid (T,K) | None on
    the host: 0 where a target has no annotation; a target is retired at its first such frame (its later rows repeat its last
    box and are not scored, whatever `valid` says there).  -> (ious (T,K), distances (T,K), results (T,K,15)) device tensors."""
    _sampling(sampling, "evaluate_targets")
    trk = tracker if tracker is not None else multi_tracker_for(model, gt_boxes.shape[1], seed=seed, use_graph=use_graph)
    return _evaluate_k(trk, frames, gt_boxes, valid, metrics)


def evaluate_scene(model, frames, gt_boxes, valid=None, seed=0, use_graph=None, tracker=None, metrics=None, sampling="device",
                   **capacities):
    """evaluate_targets on a scene tracker (sampling "device" | "table"; capacities: its fixed sizes): the same contract and
    the same return value, and no host stop per frame (the ground truth is uploaded once, retire() is a device write).
    tracker: a SceneTracker / MotionSceneTracker to reuse."""
    _scene_sampling(sampling, "evaluate_scene")
    trk = tracker if tracker is not None else scene_tracker_for(model, gt_boxes.shape[1], seed=seed, use_graph=use_graph,
                                                                sampling=sampling, **capacities)
    return _evaluate_k(trk, frames, gt_boxes, valid, metrics)


def evaluate_managed_scene(model, frames, gt_boxes, valid=None, detections=None, n_detections=None, n_targets=None, manage=None,
                           mot=None, sampling="table", **capacities):
    """A managed scene tracker over `frames` with a detection set per frame, scored as multi-object tracking (DESIGN.md section
    12k).  gt_boxes (T,G,15), valid (T,G) | None on the host: 0 where an object has no annotation.  The tracker
    (managed_scene_tracker_for(model, n_targets or G, manage=manage, sampling=sampling, **capacities; seed, use_graph among
    them) starts from frame 0's valid boxes and runs one update(frames[t], detections[t], n_detections[t:t+1]) per frame.
    detections (T,D,15) with n_detections (T,) | None (= D each); detections=None: every frame's valid ground-truth boxes,
    moved to the front on the host once and uploaded once.  mot: a metrics.ClearMOT to add to | a dict of its gates | None.
    assignment / cost ("optimal", "distance" | "overlap": DESIGN.md section 12l) go into `manage` for the tracker and into the
    gates of `mot` for the metric; the two are chosen independently.
    No host stop per frame.  -> (the ClearMOT's compute() dict, the tracker)."""
    _scene_sampling(sampling, "evaluate_managed_scene")
    gt_host = np.ascontiguousarray(_host(gt_boxes), dtype=np.float32)
    if gt_host.ndim != 3 or gt_host.shape[2] != 15 or gt_host.shape[0] != len(frames):
        raise ValueError("gt_boxes %s for %d frames" % (gt_host.shape, len(frames)))
    T, G = gt_host.shape[:2]
    live = np.ones((T, G), bool) if valid is None else np.asarray(_host(valid)) != 0
    if live.shape != (T, G):
        raise ValueError("valid must be (T,G) = %s" % ((T, G),))
    if detections is None:
        order = np.argsort(~live, axis=1, kind="stable")                     # the valid objects first, in ascending g
        detections = np.take_along_axis(gt_host, order[:, :, None], axis=1)
        n_detections = live.sum(1)
    manage = dict(manage or {})
    manage.setdefault("max_detections", max(int(detections.shape[1]), 1))
    trk = managed_scene_tracker_for(model, int(n_targets) if n_targets is not None else G, manage=manage, sampling=sampling,
                                    **capacities)
    dev = trk.dev
    dets = PU._dev32(detections, dev).reshape(T, -1, 15)
    if n_detections is None:
        n_det = torch.full((T,), dets.shape[1], dtype=torch.int32, device=dev)
    else:
        n_det = torch.as_tensor(np.asarray(_host(n_detections), dtype=np.int32)).to(dev)
    gt, live_dev = torch.from_numpy(gt_host).to(dev), torch.from_numpy(live.astype(np.int32)).to(dev)
    trk.init(frames[0], gt_host[0][live[0]])
    for t in range(1, T):
        trk.update(frames[t], dets[t], n_det[t:t + 1])
    if isinstance(mot, dict) or mot is None:
        m = trk.score_mot(gt, live_dev, **(mot or {}))
    else:
        m = trk.score_mot(gt, live_dev, metrics=mot)
    return m.compute(), trk


def _evaluate_k(trk, frames, gt_boxes, valid, metrics):
    """the loop of evaluate_targets / evaluate_scene on a K-target tracker"""
    gt = PU._dev32(gt_boxes, trk.dev).reshape(gt_boxes.shape[0], trk.K, 15)
    if len(frames) != gt.shape[0]:
        raise ValueError("%d frames, %d ground-truth boxes" % (len(frames), gt.shape[0]))
    live = None
    if valid is not None:
        live = np.asarray(_host(valid)) != 0
        if live.shape != (gt.shape[0], trk.K) or not live[0].all():
            raise ValueError("valid must be (T,K) with every target annotated in frame 0")
        live = np.logical_and.accumulate(live, axis=0)
    _drive(trk, frames, gt[0], gt, retire=live, by_rule=True)
    ious, distances = trk.score(gt, valid=live, metrics=metrics)
    return ious, distances, trk.boxes[:trk.t]


def evaluate(model, tracklets, metrics=None, seed=0, use_graph=None, sampling="reference", lanes=None, order="given", **capacities):
    """The test epoch (test_step / validation_step of the reference over its tracklets): every tracklet of `tracklets` -- a
    sampler.DeviceTracklets, or any iterable of (frames, boxes) -- goes through evaluate_sequence on ONE tracker (one captured
    graph for the epoch) and adds to ONE metrics.SuccessPrecision (`metrics` | None: a new one); the metric is read back once,
    at the end.  -> {"success", "precision", "frames", "tracklets"}.
    lanes=L (with sampling="device" or "table"; `order` as lane_schedule takes it): the epoch runs L tracklets at a time on a
    lane tracker (LaneTracker / MotionLaneTracker) and the two pools are scored in one launch.  sampling="reference" cannot run
    on lanes: numpy's index draw needs every count on the host; sampling="table" is the lane epoch on the reference's indices.
    capacities: the tracker's fixed sizes (search_capacity, model_capacity, bank_capacity | capacity), which under "table" are
    also the sizes of its draw tables."""
    from . import metrics as MT
    _sampling(sampling)
    if lanes is not None:
        if sampling not in FREE_RUNNING:
            raise ValueError("evaluate: lanes=%r needs sampling=\"device\" or \"table\" (sampling=\"reference\" draws its indices on "
                             "the host, from counts that a lane tracker never reads back)" % (lanes,))
        trk = lane_tracker_for(model, lanes, seed=seed, use_graph=use_graph, sampling=sampling, **capacities)
        m = metrics if metrics is not None else MT.SuccessPrecision(device=trk.dev)
        trk.run(tracklets, order=order)
        if trk.lengths:                        # an empty epoch scores nothing, as the loop below
            trk.score(metrics=m)
        out = m.compute()
        out["tracklets"] = len(trk.lengths)
        return out
    trk = tracker_for(model, seed=seed, use_graph=use_graph, sampling=sampling, **capacities)
    m = metrics if metrics is not None else MT.SuccessPrecision(device=trk.dev)
    count = 0
    for item in tracklets:
        frames, boxes = (item.frames, item.boxes) if hasattr(item, "frames") else item
        evaluate_sequence(model, frames, boxes, tracker=trk, metrics=m)
        count += 1
    out = m.compute()
    out["tracklets"] = count
    return out
