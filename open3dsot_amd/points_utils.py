"""Device-side mirror of the two input-preparation helpers that sit on the critical path of every
tracked frame (models/bat.py:41-55 `prepare_input`) -- SURVEY.md section 8f-2.

  get_point_to_box_distance   datasets/points_utils.py:127-143  -> csrc/boxcloud.hip (one launch, clouds
                              already resident; the reference runs scipy cdist in fp64 on the host and
                              copies the result to the GPU)
  regularize_pc               datasets/points_utils.py:24-40    -> the index draw stays numpy's (same
                              generator, same call => the same indices as the reference); the row gather
                              runs on the device when the cloud lives there.
A box is passed as (center (3), wlh (3) = width/length/height, rot (3,3) rotation matrix) -- the three
attributes of datasets/data_classes.py::Box the reference reads (`center`, `wlh`,
`orientation.rotation_matrix`).
"""
import ctypes

import numpy as np
import torch

from . import capi


def _dev32(x, dev):
    return torch.as_tensor(np.asarray(x, dtype=np.float32) if not torch.is_tensor(x) else x, dtype=torch.float32,
                           device=dev).contiguous()


def boxcloud_into(out, points, center, wlh, rot, wlh_factor=1.0):
    """One o3d_boxcloud launch (no sync, nothing allocated): contiguous float32 GPU tensors points (B,N,3), center / wlh (B,3),
    rot (B,9) -> written into out (B,N,9)"""
    dev = points.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_boxcloud(points.data_ptr(), center.data_ptr(), wlh.data_ptr(), rot.data_ptr(), float(wlh_factor),
                                            points.shape[0], points.shape[1], out.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "o3d_boxcloud")
    return out


def get_point_to_box_distance(points, center, wlh, rot, wlh_factor=1.0):
    """points (N,3) or (B,N,3) on the GPU; center/wlh (3) or (B,3); rot (3,3) or (B,3,3) -> (N,9) / (B,N,9)"""
    if not points.is_cuda:
        raise RuntimeError("get_point_to_box_distance: CPU not supported (tensor must be a GPU tensor)")
    single = points.dim() == 2
    pts = (points.unsqueeze(0) if single else points).contiguous().float()
    B, N, three = pts.shape
    if three != 3:
        raise ValueError("points must be (..., 3)")
    dev = pts.device
    c = _dev32(center, dev).reshape(-1, 3)
    s = _dev32(wlh, dev).reshape(-1, 3)
    r = _dev32(rot, dev).reshape(-1, 9)
    if not (c.shape[0] == s.shape[0] == r.shape[0] == B):
        raise ValueError("one box per cloud expected")
    out = boxcloud_into(torch.empty((B, N, 9), device=dev, dtype=torch.float32), pts, c, s, r, wlh_factor)
    return out[0] if single else out


def regularize_pc(points, sample_size, seed=None):
    """points (n,3) tensor (any device) -> (resampled (sample_size,3) on the same device, indices | None).
    The indices are drawn exactly as the reference draws them (numpy, points_utils.py:24-40)."""
    num_points = points.shape[0]
    idx = None
    rng = np.random if seed is None else np.random.default_rng(seed)
    if num_points > 2:
        if num_points != sample_size:
            idx = rng.choice(num_points, size=sample_size, replace=sample_size > num_points)
        else:
            idx = np.arange(num_points)
    if idx is None:
        return torch.zeros((sample_size, 3), dtype=torch.float32, device=points.device), None
    return points.index_select(0, torch.as_tensor(idx, dtype=torch.long, device=points.device)), idx


# ---- the tracking front end (csrc/track.hip): crops, resampling and the box update on the device ---------------------------
# A box travels as the triple (center, wlh, rot) above or, between kernels, as ONE (15,) float32 GPU tensor
# [center (3) | wlh (3) | rot (9) row-major] -- `pack_box` / `unpack_box`.
CROP_SUBWINDOW, CROP_MODEL = capi.CONSTANTS["O3D_CROP_SUBWINDOW"], capi.CONSTANTS["O3D_CROP_MODEL"]
CROP_MAX_JOBS = capi.CONSTANTS["O3D_CROP_MAX_JOBS"]
_CropJob = capi.struct("o3d_crop_job")
_ResampleJob = capi.struct("o3d_resample_job")


def _need_gpu(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError("%s: CPU not supported (tensor must be a GPU tensor)" % what)


def pack_box(box, device):
    """(center, wlh, rot) or a (15,) vector -> (15,) float32 tensor on `device`"""
    if torch.is_tensor(box) and box.numel() == 15:
        return box.to(device=device, dtype=torch.float32).reshape(15).contiguous()
    if not torch.is_tensor(box) and len(box) == 15:
        return _dev32(box, device).reshape(15)
    c, s, r = box
    return torch.cat([_dev32(c, device).reshape(3), _dev32(s, device).reshape(3), _dev32(r, device).reshape(9)])


def unpack_box(box15):
    """(15,) -> (center (3), wlh (3), rot (3,3)) views"""
    return box15[0:3], box15[3:6], box15[6:15].reshape(3, 3)


def _crop_operands(box, out, count):
    """what every crop target needs: box15, out (capacity,3) and count (1,) on the GPU"""
    assert box.is_cuda and box.dtype == torch.float32 and box.is_contiguous() and box.numel() == 15
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and count.is_cuda and count.dtype == torch.int32


def _resample_fields(job):
    """(src (n_src,3) | None, idx (n,) int32 | None, dst (n,3)) -> the six fields of its o3d_resample_job; src None: dst is
    zero-filled (regularize_pc with <= 2 points)"""
    src, idx, dst = job
    assert dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous()
    n = dst.numel() // 3
    if src is None:
        return 0, 0, 0, dst.data_ptr(), n, 1
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and idx.dtype == torch.int32 and idx.numel() >= n
    return src.data_ptr(), src.shape[0], idx.data_ptr(), dst.data_ptr(), n, 0


def crop_jobs(jobs, scratch=None, stream=None):
    """One o3d_track_crop call.  jobs: up to 4 tuples (points (n,3) f32 GPU contiguous, box15 GPU, scale, offset, mode,
    out (capacity,3) f32 GPU, count (1,) int32 GPU).  Nothing is read back here."""
    assert 1 <= len(jobs) <= CROP_MAX_JOBS
    dev = jobs[0][0].device
    table = (_CropJob * len(jobs))()
    for j, (pts, box, scale, offset, mode, out, count) in enumerate(jobs):
        assert pts.is_cuda and pts.dtype == torch.float32 and pts.is_contiguous() and pts.dim() == 2 and pts.shape[1] == 3
        _crop_operands(box, out, count)
        table[j] = _CropJob(pts.data_ptr(), pts.shape[0], box.data_ptr(), float(scale), float(offset), int(mode),
                            out.data_ptr(), out.shape[0], count.data_ptr())
    lib = capi.load()
    need = lib.o3d_track_crop_scratch(ctypes.addressof(table), len(jobs))
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty((max(need, 1),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        capi.check(lib.o3d_track_crop(ctypes.addressof(table), len(jobs), scratch.data_ptr(), scratch.numel(), s), "o3d_track_crop")
    return scratch


def resample_jobs(jobs):
    """One o3d_track_resample call.  jobs: 1 or 2 tuples (src (n_src,3) | None, idx (n,) int32 | None, dst (n,3)); src None:
    dst is zero-filled (regularize_pc with <= 2 points)."""
    table = (_ResampleJob * len(jobs))(*[_ResampleJob(*_resample_fields(job)) for job in jobs])
    dev = jobs[0][2].device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_resample(ctypes.addressof(table), len(jobs), torch.cuda.current_stream(dev).cuda_stream),
                   "o3d_track_resample")


# ---- K targets per launch (o3d_track_*_multi): the job tables live on the DEVICE ------------------------------------------------
# The tables are arrays of C structs holding device pointers.  They are described here as numpy record types with the C
# layout, so that a caller (tracking.MultiTargetTracker, tracking.MultiMotionTracker) fills a whole table in a pinned buffer with a few array assignments
# and uploads it with one asynchronous copy.
CROP_MULTI_MAX_TARGETS = capi.CONSTANTS["O3D_CROP_MULTI_MAX_TARGETS"]
CROP_MULTI_CHUNK = capi.CONSTANTS["O3D_CROP_MULTI_CHUNK"]      # targets the crop stages in LDS at a time
CROP_TARGET = capi.dtype("o3d_crop_target")
RESAMPLE_JOB = capi.dtype("o3d_resample_job")
MOTION_JOB = capi.dtype("o3d_motion_job")
_CropGroup = capi.struct("o3d_crop_group")


def crop_target_table(targets, device):
    """targets: tuples (box15 GPU, scale, offset, mode, out (capacity,3) f32 GPU, count (1,) int32 GPU) -> the o3d_crop_target
    table as a uint8 tensor on `device` (a blocking upload: for tests and tools; the tracker fills a pinned buffer).  The
    caller keeps the tensors alive."""
    tab = np.zeros((len(targets),), CROP_TARGET)
    for k, (box, scale, offset, mode, out, count) in enumerate(targets):
        _crop_operands(box, out, count)
        tab[k] = (box.data_ptr(), scale, offset, mode, out.data_ptr(), out.shape[0], count.data_ptr())
    return torch.from_numpy(tab.view(np.uint8)).to(device)


def resample_job_table(jobs, device):
    """jobs: tuples (src (n_src,3) | None, idx (n,) int32 | None, dst (n,3)) as resample_jobs takes -> the o3d_resample_job
    table as a uint8 tensor on `device` (a blocking upload)"""
    tab = np.zeros((len(jobs),), RESAMPLE_JOB)
    tab[:] = [_resample_fields(job) for job in jobs]
    return torch.from_numpy(tab.view(np.uint8)).to(device)


def crop_multi(groups, scratch=None):
    """One o3d_track_crop_multi call.  groups: 1 or 2 tuples (points (n,3) f32 GPU contiguous, table) with table a uint8 GPU
    tensor of o3d_crop_target records (crop_target_table, or a CROP_TARGET array uploaded by the caller): every point of a
    group is tested against all of its targets.  Nothing is read back here.  -> the scratch buffer (reuse it)."""
    assert 1 <= len(groups) <= 2
    dev = groups[0][0].device
    table = (_CropGroup * len(groups))()
    for g, (pts, tab) in enumerate(groups):
        assert pts.is_cuda and pts.dtype == torch.float32 and pts.is_contiguous() and pts.dim() == 2 and pts.shape[1] == 3
        assert tab.is_cuda and tab.dtype == torch.uint8 and tab.is_contiguous() and tab.numel() % CROP_TARGET.itemsize == 0
        table[g] = _CropGroup(pts.data_ptr(), pts.shape[0], tab.data_ptr(), tab.numel() // CROP_TARGET.itemsize)
    lib = capi.load()
    need = lib.o3d_track_crop_multi_scratch(ctypes.addressof(table), len(groups))
    if need < 0:
        raise capi.O3DError("o3d_track_crop_multi: bad table (1..%d targets per group)" % CROP_MULTI_MAX_TARGETS)
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty((max(need, 1),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        capi.check(lib.o3d_track_crop_multi(ctypes.addressof(table), len(groups), scratch.data_ptr(), scratch.numel(),
                                            torch.cuda.current_stream(dev).cuda_stream), "o3d_track_crop_multi")
    return scratch


def resample_multi(table, n_jobs=None):
    """One o3d_track_resample_multi launch over a uint8 GPU tensor of o3d_resample_job records (resample_job_table, or a
    RESAMPLE_JOB array uploaded by the caller); n_jobs: the first n_jobs records (default: all)."""
    assert table.is_cuda and table.dtype == torch.uint8 and table.is_contiguous()
    n = table.numel() // RESAMPLE_JOB.itemsize if n_jobs is None else int(n_jobs)
    assert n * RESAMPLE_JOB.itemsize <= table.numel()
    dev = table.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_resample_multi(table.data_ptr(), n, torch.cuda.current_stream(dev).cuda_stream),
                   "o3d_track_resample_multi")


def offset_box_multi(ref, offset, yaw_state=None, out=None, results=None, frame=None, rebase=None, active=None, degrees=True,
                     use_z=False, limit_box=True, seed=0):
    """One o3d_track_offset_box_multi launch on device operands (no sync): ref (K,15), offset (K,4), yaw_state (K,10) | None,
    out (K,15) | None, results (T,K,15) with frame (1,) int32 | None, rebase / active (K,) int32 | None.  Target k is updated
    as offset_box updates it with seed + k.  -> out (allocated when None and no results)."""
    _need_gpu(ref, "offset_box_multi")
    _need_gpu(offset, "offset_box_multi")
    dev, K = ref.device, ref.numel() // 15
    assert ref.dtype == torch.float32 and ref.is_contiguous() and ref.numel() == 15 * K and K >= 1
    assert offset.dtype == torch.float32 and offset.is_contiguous() and offset.numel() == 4 * K
    if out is None and results is None:
        out = torch.empty((K, 15), dtype=torch.float32, device=dev)
    for t, width, dt in ((yaw_state, 10, torch.float32), (out, 15, torch.float32), (rebase, 1, torch.int32), (active, 1, torch.int32)):
        assert t is None or (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == width * K)
    if results is not None:
        assert results.is_cuda and results.dtype == torch.float32 and results.is_contiguous() and results.numel() % (15 * K) == 0
        assert frame is not None and frame.dtype == torch.int32

    def ptr(t):
        return t.data_ptr() if t is not None else None
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_offset_box_multi(
            ref.data_ptr(), offset.data_ptr(), ptr(yaw_state), ptr(rebase), ptr(active), K, int(bool(degrees)), int(bool(use_z)),
            int(bool(limit_box)), int(seed) & 0x3fffffff, ptr(out), ptr(results),
            results.numel() // (15 * K) if results is not None else 0, ptr(frame), torch.cuda.current_stream(dev).cuda_stream),
            "o3d_track_offset_box_multi")
    return out


def _crop(points, box, scale, offset, mode, what):
    _need_gpu(points, what)
    pts = points.contiguous().float()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    dev = pts.device
    b = pack_box(box, dev)
    out = torch.empty((max(pts.shape[0], 1), 3), dtype=torch.float32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    crop_jobs([(pts, b, scale, offset, mode, out, count)])
    return out[:int(count.item())], b


def generate_subwindow(points, sample_bb, scale, offset=2):
    """datasets/points_utils.py:218-250 (oriented=True): the points of `points` (N,3, GPU) inside `sample_bb` scaled by
    `scale` and padded by `offset`, in the frame of the box, in their original order -> (n,3).  One sync (the count)."""
    return _crop(points, sample_bb, scale, offset, CROP_SUBWINDOW, "generate_subwindow")[0]


def cropAndCenterPC(points, box, offset=0, scale=1.0):
    """datasets/points_utils.py:103-124 (normalize=False) -> (cropped (n,3) in the box frame, canonical box = (zero centre,
    wlh, identity) on the device)"""
    out, b = _crop(points, box, scale, offset, CROP_MODEL, "cropAndCenterPC")
    return out, (torch.zeros(3, device=out.device), b[3:6].clone(), torch.eye(3, device=out.device))


def getModel(PCs, boxes, offset=0, scale=1.0):
    """datasets/points_utils.py:88-100: the crops of the clouds `PCs` by their `boxes`, concatenated -> (points, canonical
    box of the last one)"""
    if len(PCs) == 0:
        raise ValueError("getModel needs at least one cloud")
    parts, canon = [], None
    for pc, box in zip(PCs, boxes):
        p, canon = cropAndCenterPC(pc, box, offset=offset, scale=scale)
        parts.append(p)
    return torch.cat(parts, 0), canon


def offset_box(ref15, offset4, out=None, yaw_state=None, rebase=False, degrees=True, use_z=False, limit_box=True, seed=0,
               results=None, frame=None):
    """One o3d_track_offset_box launch on device operands (no sync); returns `out` (allocated when None and no results)."""
    _need_gpu(ref15, "getOffsetBB")
    _need_gpu(offset4, "getOffsetBB")
    dev = ref15.device
    assert ref15.dtype == torch.float32 and ref15.is_contiguous() and ref15.numel() == 15
    assert offset4.dtype == torch.float32 and offset4.is_contiguous() and offset4.numel() >= 4
    if out is None and results is None:
        out = torch.empty((15,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_offset_box(
            ref15.data_ptr(), offset4.data_ptr(), yaw_state.data_ptr() if yaw_state is not None else None, int(bool(rebase)),
            int(bool(degrees)), int(bool(use_z)), int(bool(limit_box)), int(seed) & 0x7fffffff,
            out.data_ptr() if out is not None else None, results.data_ptr() if results is not None else None,
            results.shape[0] if results is not None else 0, frame.data_ptr() if frame is not None else None,
            torch.cuda.current_stream(dev).cuda_stream), "o3d_track_offset_box")
    return out


def getOffsetBB(box, offset, degrees=True, use_z=False, limit_box=True, seed=0, frame=0, yaw_state=None):
    """datasets/points_utils.py:43-85 on the device: `box` (center, wlh, rot) moved by `offset` (4,) GPU tensor = (x, y, z,
    theta) in the box frame -> (center, wlh, rot) GPU tensors.  `limit_box`'s random replacement (the reference draws from the
    unseeded global numpy generator, so nothing can be pinned) is a counter-based hash of (seed, frame, component).
    yaw_state: a (10,) GPU tensor {R0, yaw} that carries the orientation of a chain of updates (see o3d_track_offset_box)."""
    _need_gpu(offset, "getOffsetBB")
    dev = offset.device
    fr = torch.full((1,), int(frame), dtype=torch.int32, device=dev)
    res = torch.empty((int(frame) + 1, 15), dtype=torch.float32, device=dev)
    out = offset_box(pack_box(box, dev), offset.contiguous().float().reshape(-1), torch.empty(15, device=dev), yaw_state, False,
                     degrees, use_z, limit_box, seed, res, fr)
    return unpack_box(out)


# ---- the motion tracker's input (MotionBaseModel.build_input_dict, models/base_model.py:255-304) ---------------------------
def motion_input(prev_crop, this_crop, idx, wlh, first_frame, zero=(False, False), out_points=None, out_bc=None):
    """One o3d_track_motion_input launch (no sync): the two crops (n,3) of the previous and the current frame in the frame of
    the reference box, gathered by idx (2N,) int32 [rows < N from prev_crop, rows >= N from this_crop] -> (points (2N,5),
    candidate_bc (2N,9)).  wlh (3,) GPU: the canonical box; zero[h]: half h is zero-filled (its crop and its indices are not
    read; the crop may be None).  out_bc=False skips the BoxCloud (box_aware=False) and returns None for it; the outputs are
    allocated when None."""
    _need_gpu(wlh, "motion_input")
    dev = wlh.device
    zp, zt = bool(zero[0]), bool(zero[1])
    for src, z in ((prev_crop, zp), (this_crop, zt)):
        if not (z and src is None):
            _need_gpu(src, "motion_input")
            assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 2 and src.shape[1] == 3
    if idx is not None:
        _need_gpu(idx, "motion_input")
        assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() % 2 == 0
        n2 = idx.numel()
    elif out_points is not None:
        n2 = out_points.numel() // 5
    else:
        raise ValueError("motion_input needs idx or out_points to know the sample size")
    assert wlh.dtype == torch.float32 and wlh.is_contiguous() and wlh.numel() == 3
    if out_points is None:
        out_points = torch.empty((n2, 5), dtype=torch.float32, device=dev)
    if out_bc is None:
        out_bc = torch.empty((n2, 9), dtype=torch.float32, device=dev)
    elif out_bc is False:
        out_bc = None
    assert out_points.is_cuda and out_points.dtype == torch.float32 and out_points.is_contiguous() and out_points.numel() == 5 * n2
    assert out_bc is None or (out_bc.is_cuda and out_bc.dtype == torch.float32 and out_bc.is_contiguous() and out_bc.numel() == 9 * n2)
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_motion_input(
            prev_crop.data_ptr() if prev_crop is not None else None, prev_crop.shape[0] if prev_crop is not None else 0,
            this_crop.data_ptr() if this_crop is not None else None, this_crop.shape[0] if this_crop is not None else 0,
            idx.data_ptr() if idx is not None else None, n2 // 2, int(zp), int(zt), wlh.data_ptr(), int(bool(first_frame)),
            out_points.data_ptr(), out_bc.data_ptr() if out_bc is not None else None,
            torch.cuda.current_stream(dev).cuda_stream), "o3d_track_motion_input")
    return out_points, out_bc


def _motion_fields(job):
    """(prev_crop (n,3) | None, this_crop (n,3) | None, idx (2N,) int32 | None, (zero_prev, zero_this)) as motion_input takes
    them -> the seven fields of its o3d_motion_job"""
    prev, this, idx, zero = job
    for src in (prev, this):
        assert src is None or (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 2 and src.shape[1] == 3)
    assert idx is None or (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous())
    return (prev.data_ptr() if prev is not None else 0, prev.shape[0] if prev is not None else 0,
            this.data_ptr() if this is not None else 0, this.shape[0] if this is not None else 0,
            idx.data_ptr() if idx is not None else 0, int(bool(zero[0])), int(bool(zero[1])))


def motion_job_table(jobs, device):
    """jobs: K tuples (prev_crop | None, this_crop | None, idx (2N,) int32 | None, (zero_prev, zero_this)) -> the
    o3d_motion_job table as a uint8 tensor on `device` (a blocking upload: for tests and tools; the tracker fills a pinned
    buffer).  The caller keeps the tensors alive."""
    tab = np.zeros((len(jobs),), MOTION_JOB)
    tab[:] = [_motion_fields(job) for job in jobs]
    return torch.from_numpy(tab.view(np.uint8)).to(device)


def motion_input_multi(table, K, N, wlh, first_frame, out_points, out_bc):
    """One o3d_track_motion_input_multi launch (no sync) over a uint8 GPU tensor that starts with K o3d_motion_job records
    (motion_job_table, or a MOTION_JOB array uploaded by the caller): wlh (K,3) GPU, the canonical boxes -> out_points
    (K,2N,5) and out_bc (K,2N,9), or None / False to skip the BoxCloud (box_aware=False).  Row k is motion_input's for job k."""
    _need_gpu(wlh, "motion_input_multi")
    _need_gpu(table, "motion_input_multi")
    _need_gpu(out_points, "motion_input_multi")
    K, N = int(K), int(N)
    if out_bc is None or out_bc is False:
        out_bc = None
    else:
        _need_gpu(out_bc, "motion_input_multi")
    assert 1 <= K <= CROP_MULTI_MAX_TARGETS and N >= 1
    assert table.dtype == torch.uint8 and table.is_contiguous() and K * MOTION_JOB.itemsize <= table.numel()
    assert wlh.dtype == torch.float32 and wlh.is_contiguous() and wlh.numel() == 3 * K
    assert out_points.dtype == torch.float32 and out_points.is_contiguous() and out_points.numel() == 10 * K * N
    assert out_bc is None or (out_bc.dtype == torch.float32 and out_bc.is_contiguous() and out_bc.numel() == 18 * K * N)
    dev = wlh.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_motion_input_multi(
            table.data_ptr(), K, N, wlh.data_ptr(), int(bool(first_frame)), out_points.data_ptr(),
            out_bc.data_ptr() if out_bc is not None else None, torch.cuda.current_stream(dev).cuda_stream),
            "o3d_track_motion_input_multi")
    return out_points, out_bc


# ---- the free-running loop (tracking.py, sampling="device"): counts and indices never leave the device -------------------------
BANK_RULES = {"first": capi.CONSTANTS["O3D_BANK_FIRST"], "previous": capi.CONSTANTS["O3D_BANK_PREVIOUS"],
              "firstandprevious": capi.CONSTANTS["O3D_BANK_FIRSTANDPREVIOUS"], "all": capi.CONSTANTS["O3D_BANK_ALL"]}


def _mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def draw_key(seed, counter, j, cloud):
    """the key of the keyed index draw (the formula at the head of csrc/train_batch.hip) -> a uint32 as a Python int"""
    a = (int(seed) * 0x9E3779B1) & 0xFFFFFFFF
    b = (int(counter) * 0x85EBCA77 + int(j) * 0xC2B2AE3D + int(cloud) * 0x27D4EB2F + 0x165667B1) & 0xFFFFFFFF
    return _mix32(a ^ b)


def _key_bits(key):
    """a uint32 key -> the C int that carries its bits"""
    key = int(key) & 0xFFFFFFFF
    return key - (1 << 32) if key >= (1 << 31) else key


def _count_operand(t):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= 1


def _draw_table(table, cap, S, what):
    """a table of tracking.draw_table for clouds of up to `cap` rows resampled to S: (cap + 1, S) int32 on the GPU.  The kernels
    index it with a device-resident count up to cap, so its shape is checked here, on every call."""
    _need_gpu(table, what)
    assert table.dtype == torch.int32 and table.is_contiguous() and tuple(table.shape) == (cap + 1, S), (what, tuple(table.shape), (cap + 1, S))


_DRAW_ENTRIES = {      # the wrapper -> its C entry point for keys, for tables
    "resample_drawn": ("o3d_track_resample_drawn", "o3d_track_resample_tabled"),
    "motion_input_drawn": ("o3d_track_motion_input_drawn", "o3d_track_motion_input_tabled"),
    "resample_drawn_lanes": ("o3d_track_resample_drawn_lanes", "o3d_track_resample_tabled_lanes"),
    "motion_input_drawn_lanes": ("o3d_track_motion_input_drawn_lanes", "o3d_track_motion_input_tabled_lanes")}


def _draw_sources(what, sources, caps_sizes):
    """The index sources of one launch of the wrapper `what` -> (the name of the C entry point, their C arguments, the C argument
    of an absent source).  Key and table are two values of one argument here and two entry points in the C ABI: a Python or numpy
    integer is a KEY (the keyed draw), a tensor is a TABLE (tracking.draw_table: the reference's draw), checked against the
    (cap, S) of its cloud.  All sources of a launch are of one kind."""
    tables = [torch.is_tensor(s) for s in sources]
    if any(tables) != all(tables):
        raise ValueError("%s: the index sources of one launch must be all keys or all tables" % what)
    if not tables[0]:
        return _DRAW_ENTRIES[what][0], [_key_bits(s) for s in sources], 0
    for table, (cap, S) in zip(sources, caps_sizes):
        _draw_table(table, cap, S, what)
    return _DRAW_ENTRIES[what][1], [t.data_ptr() for t in sources], None


def resample_drawn(jobs):
    """One o3d_track_resample_drawn launch, or its table twin's (no sync).  jobs: 1 or 2 tuples (src (cap,3) f32 GPU, n_dev (1,)
    int32 GPU, source, dst (S,3), used (S,) int32 GPU | None): with n = min(n_dev[0], cap), dst is resampled from the first n rows
    of src (zeros when n <= 2).  source (_draw_sources): a key draws the indices on the device; with a table (cap + 1, S) int32
    GPU, row i of dst is src[table[n, i]], zeros where that entry lies outside [0, n).  used receives the indices (-1 for a
    zero-filled cloud)."""
    assert 1 <= len(jobs) <= 2
    for src, n_dev, _, dst, used in jobs:
        _need_gpu(src, "resample_drawn")
        _need_gpu(dst, "resample_drawn")
        assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 2 and src.shape[1] == 3
        assert dst.dtype == torch.float32 and dst.is_contiguous() and dst.numel() % 3 == 0
        _count_operand(n_dev)
        assert used is None or (used.is_cuda and used.dtype == torch.int32 and used.is_contiguous() and used.numel() >= dst.numel() // 3)
    entry, draws, absent = _draw_sources("resample_drawn", [j[2] for j in jobs], [(j[0].shape[0], j[3].numel() // 3) for j in jobs])
    args = []
    for (src, n_dev, _, dst, used), draw in zip(jobs, draws):
        args += [src.data_ptr(), n_dev.data_ptr(), src.shape[0], draw, dst.data_ptr(), dst.numel() // 3,
                 used.data_ptr() if used is not None else None]
    if len(jobs) == 1:
        args += [None, None, 0, absent, None, 0, None]
    dev = jobs[0][3].device
    with torch.cuda.device(dev):
        capi.check(getattr(capi.load(), entry)(*args, len(jobs), torch.cuda.current_stream(dev).cuda_stream), entry)


def bank_update(crop, count, bank, rule, first, has_crop, state_in, state_out):
    """One o3d_track_bank_update launch (no sync): the staged model crop `crop` (crop_cap,3) with its device count (1,) int32
    goes into `bank` (bank_cap,3) by the shape_aggregation `rule` (a key of BANK_RULES); state_in / state_out (2,) int32 GPU =
    {fixed, total} before and after (two different tensors).  has_crop False: the state is copied through."""
    for t in (crop, bank):
        _need_gpu(t, "bank_update")
        assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 3
    _count_operand(count)
    for s in (state_in, state_out):
        assert s.is_cuda and s.dtype == torch.int32 and s.is_contiguous() and s.numel() == 2
    dev = bank.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_bank_update(
            crop.data_ptr(), count.data_ptr(), crop.shape[0], bank.data_ptr(), bank.shape[0], BANK_RULES[rule], int(bool(first)),
            int(bool(has_crop)), state_in.data_ptr(), state_out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "o3d_track_bank_update")


def _motion_sources(what, source, cap, N):
    """the index source of a motion form: (key of the previous crop, key of the current one), or ONE table (cap + 1, N) for both
    halves (the reference draws both with seed=1) -> _draw_sources' entry point and C arguments"""
    if torch.is_tensor(source):
        return _draw_sources(what, [source], [(cap, N)])[:2]
    key_prev, key_this = source
    return _draw_sources(what, [key_prev, key_this], [(cap, N), (cap, N)])[:2]


def motion_input_drawn(prev_crop, this_crop, counts, keys, wlh, first_frame, out_points, out_bc=None, used=None):
    """One o3d_track_motion_input_drawn launch, or its table twin's (no sync): motion_input with the two counts read from `counts`
    (2,) int32 GPU (capped at the crops' common capacity) and the 2N indices taken on the device from `keys` (_motion_sources).
    out_points (2N,5); out_bc (2N,9) | None / False (box_aware=False); used (2N,) int32 GPU | None: the indices, -1 for a
    zero-filled row."""
    for t in (prev_crop, this_crop):
        _need_gpu(t, "motion_input_drawn")
        assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 3
    assert prev_crop.shape[0] == this_crop.shape[0]
    _need_gpu(out_points, "motion_input_drawn")
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= 2
    assert wlh.is_cuda and wlh.dtype == torch.float32 and wlh.is_contiguous() and wlh.numel() == 3
    assert out_points.dtype == torch.float32 and out_points.is_contiguous() and out_points.numel() % 10 == 0
    n2 = out_points.numel() // 5
    entry, draws = _motion_sources("motion_input_drawn", keys, prev_crop.shape[0], n2 // 2)
    if out_bc is None or out_bc is False:
        out_bc = None
    else:
        assert out_bc.is_cuda and out_bc.dtype == torch.float32 and out_bc.is_contiguous() and out_bc.numel() == 9 * n2
    assert used is None or (used.is_cuda and used.dtype == torch.int32 and used.is_contiguous() and used.numel() >= n2)
    dev = wlh.device
    with torch.cuda.device(dev):
        capi.check(getattr(capi.load(), entry)(
            prev_crop.data_ptr(), this_crop.data_ptr(), counts.data_ptr(), prev_crop.shape[0], *draws, n2 // 2, wlh.data_ptr(),
            int(bool(first_frame)), out_points.data_ptr(), out_bc.data_ptr() if out_bc is not None else None,
            used.data_ptr() if used is not None else None, torch.cuda.current_stream(dev).cuda_stream), entry)
    return out_points, out_bc


# ---- the free-running loop L lanes wide (tracking.LaneTracker / MotionLaneTracker; o3d_track_*_lanes) -----------------------------
# A lane is the leading axis of every buffer; `lanes` is the (L, LANE_COLS) int32 GPU table of the step.
LANE_FIELDS = ("active", "first", "has_crop", "t", "row", "ref_row", "rebase")
LANE_COLS = capi.CONSTANTS["O3D_LANE_COLS"]
LANE = {name: capi.CONSTANTS["O3D_%s" % ("lane_" + name).upper()] for name in LANE_FIELDS}      # O3D_LANE_ACTIVE, ...


def _f32(t, shape, what):
    _need_gpu(t, what)
    assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), (what, tuple(t.shape), tuple(shape))


def _i32(t, numel, what):
    _need_gpu(t, what)
    assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == numel, (what, tuple(t.shape), numel)


def _lane_table(lanes, what):
    _need_gpu(lanes, what)
    assert lanes.dtype == torch.int32 and lanes.is_contiguous() and lanes.dim() == 2 and lanes.shape[1] == LANE_COLS
    return lanes.shape[0]


def _strided_count(t, stride, L):
    """a count per lane: element l * stride of the int32 GPU tensor (or view) t"""
    assert t.is_cuda and t.dtype == torch.int32 and t.stride(-1) == 1 and stride >= 1
    assert t.storage_offset() + (L - 1) * stride < t.untyped_storage().nbytes() // 4


def bank_update_lanes(crop, counts, count_stride, bank, rule, lanes, state_in, state_out):
    """One o3d_track_bank_update_lanes launch (no sync): bank_update per lane.  crop (L,crop_cap,3), lane l's count =
    counts.flatten()[l * count_stride], bank (L,bank_cap,3), lanes (L,LANE_COLS), state_in / state_out (L,2) int32."""
    L = _lane_table(lanes, "bank_update_lanes")
    _f32(crop, (L, crop.shape[1], 3), "bank_update_lanes")
    _f32(bank, (L, bank.shape[1], 3), "bank_update_lanes")
    _strided_count(counts, count_stride, L)
    _i32(state_in, 2 * L, "bank_update_lanes")
    _i32(state_out, 2 * L, "bank_update_lanes")
    dev = bank.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_bank_update_lanes(
            crop.data_ptr(), counts.data_ptr(), int(count_stride), crop.shape[1], bank.data_ptr(), bank.shape[1], BANK_RULES[rule],
            lanes.data_ptr(), L, state_in.data_ptr(), state_out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "o3d_track_bank_update_lanes")


def resample_drawn_lanes(jobs):
    """One o3d_track_resample_drawn_lanes launch, or its table twin's (no sync).  jobs: 2 tuples (src (L,cap,3), n_dev, stride,
    source, dst (L,S,3), used (L,S) int32 | None); lane l's count is element l * stride of n_dev (an int32 GPU tensor or view);
    source: resample_drawn's, a key or a table (cap + 1, S) int32, the same for every lane of its cloud."""
    assert len(jobs) == 2
    L = jobs[0][0].shape[0]
    for src, n_dev, stride, _, dst, used in jobs:
        _f32(src, (L, src.shape[1], 3), "resample_drawn_lanes")
        _f32(dst, (L, dst.shape[1], 3), "resample_drawn_lanes")
        _strided_count(n_dev, stride, L)
        if used is not None:
            _i32(used, L * dst.shape[1], "resample_drawn_lanes")
    entry, draws, _ = _draw_sources("resample_drawn_lanes", [j[3] for j in jobs], [(j[0].shape[1], j[4].shape[1]) for j in jobs])
    args = []
    for (src, n_dev, stride, _, dst, used), draw in zip(jobs, draws):
        args += [src.data_ptr(), n_dev.data_ptr(), int(stride), src.shape[1], draw, dst.data_ptr(), dst.shape[1],
                 used.data_ptr() if used is not None else None]
    dev = jobs[0][4].device
    with torch.cuda.device(dev):
        capi.check(getattr(capi.load(), entry)(*args, L, torch.cuda.current_stream(dev).cuda_stream), entry)


def motion_input_drawn_lanes(prev_crop, this_crop, counts, keys, wlh, lanes, out_points, out_bc=None, used=None):
    """One o3d_track_motion_input_drawn_lanes launch, or its table twin's (no sync): motion_input_drawn per lane, every lane on
    the same `keys` (_motion_sources).  prev_crop / this_crop (L,cap,3), counts (L,2) int32, wlh (L,3), lanes (L,LANE_COLS):
    `first` is the lane's first_frame; out_points (L,2N,5), out_bc (L,2N,9) | None / False, used (L,2N) int32 | None."""
    L = _lane_table(lanes, "motion_input_drawn_lanes")
    cap, n2 = prev_crop.shape[1], out_points.shape[1]
    _f32(prev_crop, (L, cap, 3), "motion_input_drawn_lanes")
    _f32(this_crop, (L, cap, 3), "motion_input_drawn_lanes")
    _f32(wlh, (L, 3), "motion_input_drawn_lanes")
    _f32(out_points, (L, n2, 5), "motion_input_drawn_lanes")
    _i32(counts, 2 * L, "motion_input_drawn_lanes")
    assert n2 % 2 == 0
    entry, draws = _motion_sources("motion_input_drawn_lanes", keys, cap, n2 // 2)
    if out_bc is None or out_bc is False:
        out_bc = None
    else:
        _f32(out_bc, (L, n2, 9), "motion_input_drawn_lanes")
    if used is not None:
        _i32(used, L * n2, "motion_input_drawn_lanes")
    dev = wlh.device
    with torch.cuda.device(dev):
        capi.check(getattr(capi.load(), entry)(
            prev_crop.data_ptr(), this_crop.data_ptr(), counts.data_ptr(), cap, *draws, n2 // 2, wlh.data_ptr(), lanes.data_ptr(), L,
            out_points.data_ptr(), out_bc.data_ptr() if out_bc is not None else None,
            used.data_ptr() if used is not None else None, torch.cuda.current_stream(dev).cuda_stream), entry)
    return out_points, out_bc


def offset_box_lanes(cur, gt, offset, yaw_state, lanes, out, results, counts=None, counts_log=None, degrees=True, use_z=False,
                     limit_box=True, seed=0):
    """One o3d_track_offset_box_lanes launch (no sync): offset_box per lane.  cur (L,15), gt (R,15) the ground-truth pool,
    offset (L,4), yaw_state (L,10), lanes (L,LANE_COLS), out (L,15) (may be cur), results (R,15) the result pool; counts (L,2)
    with counts_log (R,2) int32 | None: the frame's crop counts go to the lane's row of the log."""
    L = _lane_table(lanes, "offset_box_lanes")
    R = gt.shape[0]
    _f32(cur, (L, 15), "offset_box_lanes")
    _f32(gt, (R, 15), "offset_box_lanes")
    _f32(yaw_state, (L, 10), "offset_box_lanes")
    _f32(out, (L, 15), "offset_box_lanes")
    _f32(results, (R, 15), "offset_box_lanes")
    _need_gpu(offset, "offset_box_lanes")
    assert offset.dtype == torch.float32 and offset.is_contiguous() and offset.numel() == 4 * L
    if counts_log is not None:
        _i32(counts, 2 * L, "offset_box_lanes")
        _i32(counts_log, 2 * R, "offset_box_lanes")
    dev = cur.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_offset_box_lanes(
            cur.data_ptr(), gt.data_ptr(), R, offset.data_ptr(), yaw_state.data_ptr(), lanes.data_ptr(), L, int(bool(degrees)),
            int(bool(use_z)), int(bool(limit_box)), int(seed) & 0x7fffffff, out.data_ptr(), results.data_ptr(),
            counts.data_ptr() if counts_log is not None else None, counts_log.data_ptr() if counts_log is not None else None,
            torch.cuda.current_stream(dev).cuda_stream), "o3d_track_offset_box_lanes")
    return out


def lane_start(gt, lanes, cur, yaw_state, wlh, state=None):
    """One o3d_track_lane_start launch (no sync): every lane of lanes (L,LANE_COLS) that is active and first takes its
    tracklet's first box, row (row - t) of gt (R,15), into cur (L,15), yaw_state (L,10) and wlh (L,3), and zeroes its row of
    state (L,2) int32 | None (the template bank's {fixed, total})."""
    L = _lane_table(lanes, "lane_start")
    _f32(gt, (gt.shape[0], 15), "lane_start")
    _f32(cur, (L, 15), "lane_start")
    _f32(yaw_state, (L, 10), "lane_start")
    _f32(wlh, (L, 3), "lane_start")
    if state is not None:
        _i32(state, 2 * L, "lane_start")
    dev = cur.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_lane_start(gt.data_ptr(), gt.shape[0], lanes.data_ptr(), L, cur.data_ptr(), yaw_state.data_ptr(),
                                                    wlh.data_ptr(), state.data_ptr() if state is not None else None,
                                                    torch.cuda.current_stream(dev).cuda_stream), "o3d_track_lane_start")


# ---- the lifecycle of a scene tracker's slots on the device (tracking.ManagedSceneTracker; csrc/metrics.hip, csrc/scene.hip) ------
SCENE_MAX_DETECTIONS = capi.CONSTANTS["O3D_SCENE_MAX_DETECTIONS"]
SCENE_SLOT_COLS = capi.CONSTANTS["O3D_SCENE_SLOT_COLS"]      # slot = {id, misses, starved, start}


def scene_pair_scores(tracks, active, dets, n_det, dim=3, up=2, out=None):
    """One o3d_scene_pair_scores launch (no sync): tracks (K,15), active (K,) int32, dets (D,15), n_det (1,) int32 on the device
    -> (overlaps, distances) (K,D) float32, written into out = (overlaps, distances) when given.  Pair (k, d) holds what
    metrics.score_boxes(tracks[k], dets[d]) gives, bit for bit; inactive rows and columns >= n_det hold -1 / +inf."""
    what = "scene_pair_scores"
    K, D = tracks.shape[0], dets.shape[0]
    _f32(tracks, (K, 15), what)
    _f32(dets, (D, 15), what)
    _i32(active, K, what)
    _i32(n_det, 1, what)
    dev = tracks.device
    if out is None:
        out = (torch.empty((K, D), dtype=torch.float32, device=dev), torch.empty((K, D), dtype=torch.float32, device=dev))
    for o in out:
        _f32(o, (K, D), what)
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_scene_pair_scores(tracks.data_ptr(), active.data_ptr(), K, dets.data_ptr(), n_det.data_ptr(), D,
                                                     int(dim), int(up), out[0].data_ptr(), out[1].data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream), what)
    return out


ASSIGNMENTS = {"greedy": capi.CONSTANTS["O3D_ASSIGN_GREEDY"], "optimal": capi.CONSTANTS["O3D_ASSIGN_OPTIMAL"]}
ASSIGN_COSTS = {"distance": capi.CONSTANTS["O3D_COST_DISTANCE"], "overlap": capi.CONSTANTS["O3D_COST_OVERLAP"]}


def _assign_args(assignment, cost, what):
    """(assignment, cost) as the header numbers them; an unknown name is refused here, by name"""
    if assignment not in ASSIGNMENTS:
        raise ValueError("%s: assignment must be one of %s, got %r" % (what, sorted(ASSIGNMENTS), assignment))
    if cost not in ASSIGN_COSTS:
        raise ValueError("%s: cost must be one of %s, got %r" % (what, sorted(ASSIGN_COSTS), cost))
    return ASSIGNMENTS[assignment], ASSIGN_COSTS[cost]


def scene_assign(overlaps, distances, row_active=None, n_col=None, min_iou=0.0, max_dist=float("inf"), assignment="optimal",
                 cost="distance", out=None):
    """One o3d_scene_assign launch (no sync): who belongs to whom on overlaps / distances (K,D) float32 on the device.  A pair is
    admissible when its row is in play (row_active (K,) int32 | None: all), its column is below n_col ((1,) int32 on the device |
    None: D), overlap >= min_iou and distance <= max_dist.  assignment="optimal": the most admissible pairs and among those the
    smallest sum of the integer cost (cost="distance": 1/1024 m units, "overlap": (1 - overlap) * 2^20), as include/o3dsot.h
    states it; "greedy": the walk of o3d_scene_manage.  -> (match (K,) int32 = column | -1, col_match (D,) int32 = row | -1,
    summary (2,) int64 = {pairs, sum of the cost}), written into `out` when given."""
    what = "scene_assign"
    K, D = overlaps.shape
    _f32(overlaps, (K, D), what)
    _f32(distances, (K, D), what)
    if row_active is not None:
        _i32(row_active, K, what)
    if n_col is not None:
        _i32(n_col, 1, what)
    rule_args = _assign_args(assignment, cost, what)
    dev = overlaps.device
    if out is None:
        out = (torch.empty((K,), dtype=torch.int32, device=dev), torch.empty((D,), dtype=torch.int32, device=dev),
               torch.empty((2,), dtype=torch.int64, device=dev))
    match, col_match, summary = out
    _i32(match, K, what)
    _i32(col_match, D, what)
    _need_gpu(summary, what)
    assert summary.dtype == torch.int64 and summary.numel() == 2 and summary.is_contiguous(), what
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_scene_assign(
            overlaps.data_ptr(), distances.data_ptr(), row_active.data_ptr() if row_active is not None else None,
            n_col.data_ptr() if n_col is not None else None, K, D, float(min_iou), float(max_dist), *rule_args, match.data_ptr(),
            col_match.data_ptr(), summary.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), what)
    return out


def scene_manage(overlaps, distances, dets, n_det, cur, yaw_state, canon_wlh, results, frame, active, slot, next_id, counts,
                 count_col, bank_state_next, lanes, rule, ids_log, match_log, dropped_log, min_iou=0.0, max_dist=float("inf"),
                 max_misses=2, min_points=0, max_starved=0, enroll=True, has_dets=True, *, assignment="greedy", cost="distance"):
    """One o3d_scene_manage launch (no sync) after the frame's offset_box_multi: the match on overlaps / distances (K,D) -- the
    greedy walk, or with assignment="optimal" the maximum-cardinality, minimum-cost assignment under `cost` ("distance" |
    "overlap") through o3d_scene_manage_assign --,
    the miss and starvation counters, retire, enroll and the next frame's lane table, as include/o3dsot.h states them.  dets
    (D,15), n_det (1,) int32, cur (K,15), yaw_state (K,10), canon_wlh (K,3), results (T,K,15), frame (1,) int32, active (K,) int32,
    slot (K,SCENE_SLOT_COLS) int32, next_id (1,) int32, counts (K,2) int32 with count_col 0 | 1, bank_state_next (K,2) int32 |
    None, lanes (K,LANE_COLS) int32, rule: a shape_aggregation name | None (the motion tracker), ids_log / match_log (T,K) and
    dropped_log (T,) int32."""
    what = "scene_manage"
    K, D, T = cur.shape[0], dets.shape[0], results.shape[0]
    for t, shape in ((overlaps, (K, D)), (distances, (K, D)), (dets, (D, 15)), (cur, (K, 15)), (yaw_state, (K, 10)),
                     (canon_wlh, (K, 3)), (results, (T, K, 15))):
        _f32(t, shape, what)
    for t, numel in ((n_det, 1), (frame, 1), (active, K), (slot, K * SCENE_SLOT_COLS), (next_id, 1), (counts, 2 * K),
                     (ids_log, T * K), (match_log, T * K), (dropped_log, T)):
        _i32(t, numel, what)
    assert _lane_table(lanes, what) == K
    if bank_state_next is not None:
        _i32(bank_state_next, 2 * K, what)
    rule_args = _assign_args(assignment, cost, what)
    dev = cur.device
    with torch.cuda.device(dev):
        lib = capi.load()
        args = (overlaps.data_ptr(), distances.data_ptr(), dets.data_ptr(), n_det.data_ptr(), K, D, cur.data_ptr(), yaw_state.data_ptr(),
                canon_wlh.data_ptr(), results.data_ptr(), T, frame.data_ptr(), active.data_ptr(), slot.data_ptr(), next_id.data_ptr(),
                counts.data_ptr(), int(count_col), bank_state_next.data_ptr() if bank_state_next is not None else None, lanes.data_ptr(),
                BANK_RULES[rule] if rule is not None else -1, ids_log.data_ptr(), match_log.data_ptr(), dropped_log.data_ptr(),
                float(min_iou), float(max_dist), int(max_misses), int(min_points), int(max_starved), int(bool(enroll)),
                int(bool(has_dets)))
        stream = torch.cuda.current_stream(dev).cuda_stream
        if assignment == "greedy":                         # the entry it always went through
            capi.check(lib.o3d_scene_manage(*args, stream), what)
        else:
            capi.check(lib.o3d_scene_manage_assign(*args, *rule_args, stream), what + "_assign")


# ---- scoring a managed scene on the device (metrics.ClearMOT; csrc/metrics.hip, csrc/scene.hip) -----------
SCENE_MOT_MAX_FRAMES = capi.CONSTANTS["O3D_SCENE_MOT_MAX_FRAMES"]
MOT_FRAME_COLS = ("gt", "hyp", "tp", "fp", "fn", "idsw", "frag")       # per_frame's columns 0..6; column 7 is 0


def scene_pair_scores_frames(gt, gt_valid, hyp, hyp_ids, dim=3, up=2, out=None):
    """One o3d_scene_pair_scores_frames launch (no sync): gt (F,G,15), gt_valid (F,G) int32, hyp (F,K,15), hyp_ids (F,K) int32 on
    the device -> (overlaps, distances) (F,G,K) float32, written into out = (overlaps, distances) when given.  Pair (f,g,k) holds
    what metrics.score_boxes(gt[f,g], hyp[f,k]) gives, bit for bit; the pairs of an invalid g or of a column without an id hold
    -1 / +inf."""
    what = "scene_pair_scores_frames"
    F, G, K = gt.shape[0], gt.shape[1], hyp.shape[1]
    _f32(gt, (F, G, 15), what)
    _f32(hyp, (F, K, 15), what)
    _i32(gt_valid, F * G, what)
    _i32(hyp_ids, F * K, what)
    dev = gt.device
    if out is None:
        out = (torch.empty((F, G, K), dtype=torch.float32, device=dev), torch.empty((F, G, K), dtype=torch.float32, device=dev))
    for o in out:
        _f32(o, (F, G, K), what)
    if F == 0:                                             # empty tensors have no address to pass
        return out
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_scene_pair_scores_frames(gt.data_ptr(), gt_valid.data_ptr(), hyp.data_ptr(), hyp_ids.data_ptr(), F, G,
                                                            K, int(dim), int(up), out[0].data_ptr(), out[1].data_ptr(),
                                                            torch.cuda.current_stream(dev).cuda_stream), what)
    return out


def scene_mot_walk(overlaps, distances, gt_valid, hyp_ids, last_id, tracked_prev, ever, min_iou=0.0, max_dist=float("inf"), out=None,
                   *, assignment="greedy", cost="distance"):
    """One o3d_scene_mot_walk launch (no sync): the CLEAR-MOT walk over the F frames of overlaps / distances (F,G,K) in order, as
    include/o3dsot.h states it; with assignment="optimal" the leftover match of every frame is the maximum-cardinality,
    minimum-cost assignment under `cost` ("distance" | "overlap"), through o3d_scene_mot_walk_assign.  gt_valid (F,G), hyp_ids (F,K) int32; last_id, tracked_prev, ever (G,) int32: the carried state,
    updated in place.  -> (match_slot (F,G) int32, match_id (F,G) int32, match_ov (F,G), match_di (F,G) float32, per_frame (F,8)
    int32 = MOT_FRAME_COLS and a 0), written into `out` when given."""
    what = "scene_mot_walk"
    F, G, K = overlaps.shape
    _f32(overlaps, (F, G, K), what)
    _f32(distances, (F, G, K), what)
    _i32(gt_valid, F * G, what)
    _i32(hyp_ids, F * K, what)
    for t in (last_id, tracked_prev, ever):
        _i32(t, G, what)
    dev = overlaps.device
    if out is None:
        i32 = dict(dtype=torch.int32, device=dev)
        out = (torch.empty((F, G), **i32), torch.empty((F, G), **i32), torch.empty((F, G), dtype=torch.float32, device=dev),
               torch.empty((F, G), dtype=torch.float32, device=dev), torch.empty((F, 8), **i32))
    slot, ids, mov, mdi, per_frame = out
    _i32(slot, F * G, what)
    _i32(ids, F * G, what)
    _f32(mov, (F, G), what)
    _f32(mdi, (F, G), what)
    _i32(per_frame, F * 8, what)
    rule_args = _assign_args(assignment, cost, what)
    if F == 0:
        return out
    with torch.cuda.device(dev):
        lib = capi.load()
        args = (overlaps.data_ptr(), distances.data_ptr(), gt_valid.data_ptr(), hyp_ids.data_ptr(), F, G, K, float(min_iou),
                float(max_dist), last_id.data_ptr(), tracked_prev.data_ptr(), ever.data_ptr(), slot.data_ptr(), ids.data_ptr(),
                mov.data_ptr(), mdi.data_ptr(), per_frame.data_ptr())
        stream = torch.cuda.current_stream(dev).cuda_stream
        if assignment == "greedy":                         # the entry it always went through
            capi.check(lib.o3d_scene_mot_walk(*args, stream), what)
        else:
            capi.check(lib.o3d_scene_mot_walk_assign(*args, *rule_args, stream), what + "_assign")
    return out


def _box_device(box, what):
    """the GPU a box lives on (a (15,) tensor or a (center, wlh, rot) triple of tensors); anything else is refused"""
    parts = (box,) if torch.is_tensor(box) else tuple(box)
    for x in parts:
        _need_gpu(x, what)
    return parts[0].device


def transform_box(box, ref_box):
    """datasets/points_utils.py:253-258 on the device: `box` expressed in the frame of `ref_box` -> (center, wlh, rot) GPU
    tensors (transform_box(b, b) is the canonical box of b).  Not on the per-frame path: a 3x3 product in torch."""
    dev = _box_device(box, "transform_box")
    _box_device(ref_box, "transform_box")
    c, s, r = unpack_box(pack_box(box, dev))
    rc, _, rr = unpack_box(pack_box(ref_box, dev))
    return rr.t() @ (c - rc), s.clone(), rr.t() @ r


def points_in_box(box, points, wlh_factor=1.0):
    """nuscenes.utils.geometry_utils.points_in_box on the device: points (3,N) GPU tensor -> (N,) bool, the points inside `box`
    scaled by wlh_factor, faces included (the projections onto the three edges from corner 0 of Box.corners).  A mirror for
    callers of the reference's name; the tracker's own mask comes from o3d_track_motion_input, the batch builder's from
    `inside_box` below (one kernel, a fixed fp32 operation order)."""
    _need_gpu(points, "points_in_box")
    if points.dim() != 2 or points.shape[0] != 3:
        raise ValueError("points must be (3, N)")
    c, s, r = unpack_box(pack_box(box, points.device))
    q = r.t() @ (points.float() - c[:, None])                      # the box frame: x pairs with l, y with w
    half = (torch.stack([s[1], s[0], s[2]]) * float(wlh_factor) * 0.5)[:, None]
    return (q.abs() <= half).all(0)


# ---- training batches built on the device (csrc/train_batch.hip; open3dsot_amd/sampler.py is the caller) --------------------
CROP_MAX_GROUPS = capi.CONSTANTS["O3D_CROP_MAX_GROUPS"]
TRAIN_MAX_CANDIDATES = capi.CONSTANTS["O3D_TRAIN_MAX_CANDIDATES"]
CROP_PLAN = capi.dtype("o3d_crop_plan")
_TrainSampleArgs = capi.struct("o3d_train_sample_args")


def crop_groups_plan(plan):
    """The host planner of o3d_track_crop_groups (no device call): fills wg_start / row_start / sbase of the CROP_PLAN array
    `plan` (points, n, targets, n_targets set by the caller) in place -> (scratch length in int32, workgroups of the count /
    scatter launches, workgroups of the scan launch).  Raises O3DError on a bad table."""
    assert plan.dtype == CROP_PLAN and plan.ndim == 1 and plan.flags.c_contiguous
    grid = (ctypes.c_int * 2)()
    need = capi.load().o3d_track_crop_groups_scratch(plan.ctypes.data, plan.shape[0], ctypes.addressof(grid))
    if need < 0:
        raise capi.O3DError("o3d_track_crop_groups: bad table (1..%d groups of 1..%d targets)" % (CROP_MAX_GROUPS, CROP_MULTI_MAX_TARGETS))
    return need, grid[0], grid[1]


def crop_groups(plan, dev_plan, scratch):
    """One o3d_track_crop_groups call (three launches, no sync): plan = the planned CROP_PLAN array on the host, dev_plan =
    its copy on the GPU (a uint8 tensor, or an address), scratch = an int32 GPU tensor of at least crop_groups_plan's length."""
    dev = scratch.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_crop_groups(
            plan.ctypes.data, dev_plan.data_ptr() if torch.is_tensor(dev_plan) else int(dev_plan), plan.shape[0], scratch.data_ptr(),
            scratch.numel(), torch.cuda.current_stream(dev).cuda_stream), "o3d_track_crop_groups")


def crop_groups_table(groups, device):
    """groups: tuples (points (n,3) f32 GPU contiguous, table = a uint8 GPU tensor of o3d_crop_target records) -> (plan, its
    device copy, scratch length): a blocking upload, for tests and tools; the batch builder fills a pinned buffer."""
    plan = np.zeros((len(groups),), CROP_PLAN)
    for g, (pts, tab) in enumerate(groups):
        assert pts.is_cuda and pts.dtype == torch.float32 and pts.is_contiguous() and pts.dim() == 2 and pts.shape[1] == 3
        assert tab.is_cuda and tab.dtype == torch.uint8 and tab.is_contiguous() and tab.numel() % CROP_TARGET.itemsize == 0
        plan[g] = (pts.data_ptr(), pts.shape[0], tab.data_ptr(), tab.numel() // CROP_TARGET.itemsize, 0, 0, 0)
    need = crop_groups_plan(plan)[0]
    return plan, torch.from_numpy(plan.view(np.uint8).copy()).to(device), need


# ---- the preload crop of a dataset reader (csrc/preload.hip; open3dsot_amd/datasets.py is the caller) -----------------------
PRELOAD_MAX_FRAMES = capi.CONSTANTS["O3D_PRELOAD_MAX_FRAMES"]
PRELOAD_MAX_BOXES = capi.CONSTANTS["O3D_PRELOAD_MAX_BOXES"]
PRELOAD_MAX_ROWS = capi.CONSTANTS["O3D_PRELOAD_MAX_ROWS"]
PRELOAD_MAX_STEPS = capi.CONSTANTS["O3D_PRELOAD_MAX_STEPS"]
PRELOAD_COLS = 6      # a frame record: first raw row, n, first box, number of boxes, workgroup start, scratch base


def preload_plan(frames, raw_rows):
    """The host planner of preload_count / preload_scatter (no device call): frames (F,6) int32 with columns 0 (first
    raw row), 1 (n) and 3 (number of boxes) set; fills columns 2, 4 and 5 in place -> (scratch length in int32, workgroups of
    the count / scatter launches, B).  Raises O3DError on a bad table."""
    assert frames.dtype == np.int32 and frames.ndim == 2 and frames.shape[1] == PRELOAD_COLS and frames.flags.c_contiguous
    grid = (ctypes.c_int * 2)()
    need = capi.load().o3d_preload_scratch(frames.ctypes.data, frames.shape[0], int(raw_rows), ctypes.addressof(grid))
    if need < 0:
        raise capi.O3DError("o3d_preload_scratch: bad table (0..%d frames of 0..%d boxes, %d raw rows at most)"
                            % (PRELOAD_MAX_FRAMES, PRELOAD_MAX_BOXES, PRELOAD_MAX_ROWS))
    return need, grid[0], grid[1]


def _preload_operands(raw, frames, dev_frames, bounds, transform, scratch, poses=None, steps=None, translate32=0):
    _need_gpu(raw, "preload")
    widths = (3, 4, 5) if steps is not None else (3, 4) if poses is not None else (4,)
    assert raw.dtype == torch.float32 and raw.is_contiguous() and raw.dim() == 2 and raw.shape[1] in widths
    assert frames.dtype == np.int32 and frames.ndim == 2 and frames.shape[1] == PRELOAD_COLS and frames.flags.c_contiguous
    for t, dt in ((dev_frames, torch.int32), (bounds, torch.float32), (scratch, torch.int32)):
        _need_gpu(t, "preload")
        assert t.dtype == dt and t.is_contiguous() and t.device == raw.device
    assert dev_frames.numel() == frames.size and bounds.numel() % 6 == 0
    if poses is not None:
        _need_gpu(poses, "preload")
        assert transform is None and poses.dtype == torch.float64 and poses.is_contiguous() and poses.device == raw.device
        assert poses.numel() == 12 * frames.shape[0]
    if steps is not None:
        _need_gpu(steps, "preload")
        assert transform is None and poses is None and translate32 in (0, 1)
        assert steps.dtype == torch.float64 and steps.is_contiguous() and steps.device == raw.device
        assert steps.dim() == 3 and steps.shape[0] == frames.shape[0] and 1 <= steps.shape[1] <= PRELOAD_MAX_STEPS and steps.shape[2] == 12
    if transform is not None:
        transform = np.ascontiguousarray(transform, np.float64)
        assert transform.shape == (3, 4)
    return transform


_PRELOAD_ENTRIES = {"count": ("o3d_preload_count", "o3d_preload_posed_count", "o3d_preload_steps_count"),
                    "scatter": ("o3d_preload_scatter", "o3d_preload_posed_scatter", "o3d_preload_steps_scatter")}


def _preload_entry(which, raw, transform, poses, steps, translate32):
    """what tells the three pairs of entry points apart -> (name, the arguments between raw's rows and the frame table, the
    arguments between B and the scratch): the plain pair takes a host transform | NULL, the posed and the steps pair the
    floats of a raw row and their per-record table"""
    plain, posed, stepped = _PRELOAD_ENTRIES[which]
    if steps is not None:
        return stepped, (raw.shape[1],), (steps.data_ptr(), steps.shape[1], int(translate32))
    if poses is not None:
        return posed, (raw.shape[1],), (poses.data_ptr(),)
    return plain, (), (None if transform is None else transform.ctypes.data,)


def preload_count(raw, frames, dev_frames, bounds, transform, scratch, counts, poses=None, steps=None, translate32=0):
    """One count call (two launches, no sync): raw (rows,4) float32 GPU, frames = the planned (F,6) int32 table on the host and
    dev_frames its GPU copy, bounds (B,6) float32 GPU, transform = (3,4) float64 on the host | None, scratch = an int32 GPU
    tensor of at least preload_plan's length -> counts (B,) int32 GPU, written in place.
    poses = (F,12) float64 GPU, one transform per frame record: the posed entry point instead, raw (rows, 3 | 4), transform
    None.  steps = (F,n_steps,12) float64 GPU, a chain of rounded rigid steps per frame record, translate32 = 0 (the translation
    is added in fp64 and rounded) | 1 (added in fp32): the steps entry point instead, raw (rows, 3 | 4 | 5), transform and
    poses None"""
    transform = _preload_operands(raw, frames, dev_frames, bounds, transform, scratch, poses, steps, translate32)
    _need_gpu(counts, "preload_count")
    B = bounds.numel() // 6
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= B
    name, width, how = _preload_entry("count", raw, transform, poses, steps, translate32)
    dev = raw.device
    with torch.cuda.device(dev):
        capi.check(getattr(capi.load(), name)(
            raw.data_ptr(), raw.shape[0], *width, frames.ctypes.data, dev_frames.data_ptr(), frames.shape[0], bounds.data_ptr(), B,
            *how, scratch.data_ptr(), scratch.numel(), counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), name)


def preload_scatter(raw, frames, dev_frames, bounds, transform, scratch, out_row, pool, pool_rows=None, poses=None, steps=None,
                    translate32=0):
    """One scatter launch after preload_count on the same operands: out_row (B,) int64 GPU = the first pool row of every box,
    pool (rows,3) float32 GPU, written in place; no row at or beyond pool_rows (default: all of pool) is written.
    poses, steps, translate32: as for preload_count (the posed / the steps entry point)"""
    transform = _preload_operands(raw, frames, dev_frames, bounds, transform, scratch, poses, steps, translate32)
    _need_gpu(out_row, "preload_scatter")
    _need_gpu(pool, "preload_scatter")
    B = bounds.numel() // 6
    assert out_row.dtype == torch.int64 and out_row.is_contiguous() and out_row.numel() >= B
    assert pool.dtype == torch.float32 and pool.is_contiguous() and pool.dim() == 2 and pool.shape[1] == 3
    pool_rows = pool.shape[0] if pool_rows is None else int(pool_rows)
    assert 0 <= pool_rows <= pool.shape[0]
    name, width, how = _preload_entry("scatter", raw, transform, poses, steps, translate32)
    dev = raw.device
    with torch.cuda.device(dev):
        capi.check(getattr(capi.load(), name)(
            raw.data_ptr(), raw.shape[0], *width, frames.ctypes.data, dev_frames.data_ptr(), frames.shape[0], bounds.data_ptr(), B,
            *how, scratch.data_ptr(), scratch.numel(), out_row.data_ptr(), pool.data_ptr(), pool_rows,
            torch.cuda.current_stream(dev).cuda_stream), name)


def train_select(counts, B, caps, sel, n_valid, overflow):
    """One o3d_train_select launch: counts (J,3) int32 GPU, caps = (cap_first, cap_template, cap_search) -> sel (B,), n_valid
    (1,), overflow (1,) int32 GPU tensors, written in place"""
    for t in (counts, sel, n_valid, overflow):
        _need_gpu(t, "train_select")
        assert t.dtype == torch.int32 and t.is_contiguous()
    J = counts.numel() // 3
    assert counts.numel() == 3 * J and sel.numel() >= B
    dev = counts.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_train_select(counts.data_ptr(), J, int(B), int(caps[0]), int(caps[1]), int(caps[2]), sel.data_ptr(),
                                                n_valid.data_ptr(), overflow.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "o3d_train_select")


def train_labels(gt_search, sample_bb, template_bb, offset, search_box, box_label, bbox_size, model_box):
    """One o3d_train_labels launch on (J,15) / (J,4) float32 GPU tensors; the last four are written in place"""
    J = gt_search.numel() // 15
    for t, width in ((gt_search, 15), (sample_bb, 15), (template_bb, 15), (offset, 4), (search_box, 15), (box_label, 4),
                     (bbox_size, 3), (model_box, 15)):
        _need_gpu(t, "train_labels")
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == width * J
    dev = gt_search.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_train_labels(gt_search.data_ptr(), sample_bb.data_ptr(), template_bb.data_ptr(), offset.data_ptr(), J,
                                                search_box.data_ptr(), box_label.data_ptr(), bbox_size.data_ptr(), model_box.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "o3d_train_labels")


def train_sample(args, device):
    """One o3d_train_sample launch: args = a filled _TrainSampleArgs (the caller keeps its tensors alive)"""
    with torch.cuda.device(device):
        capi.check(capi.load().o3d_train_sample(ctypes.addressof(args), torch.cuda.current_stream(device).cuda_stream),
                   "o3d_train_sample")


# ---- M2-Track training batches (csrc/train_batch.hip; sampler.MotionBatchBuilder is the caller) -----------------------------
CROP_AUG = capi.dtype("o3d_crop_aug")
_TrainMotionSampleArgs = capi.struct("o3d_train_motion_sample_args")


def _addr(t):
    return None if t is None else (t.data_ptr() if torch.is_tensor(t) else int(t))


def train_augment(gt, draw, out_box, aug, slot_src=None, n_slots=None):
    """One o3d_train_augment launch: gt (K,15), draw (K,6) float32 GPU -> out_box (K,15) and the records `aug` (a uint8 GPU
    tensor of n_slots CROP_AUG records, or an address with slot_src given); slot_src (n_slots,) int32 GPU | None, or an
    address with n_slots given"""
    for t, width in ((gt, 15), (draw, 6), (out_box, 15)):
        _need_gpu(t, "train_augment")
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() % width == 0
    K = gt.numel() // 15
    assert draw.numel() == 6 * K and out_box.numel() == 15 * K
    if torch.is_tensor(slot_src):
        assert slot_src.is_cuda and slot_src.dtype == torch.int32 and slot_src.is_contiguous()
        n_slots = slot_src.numel()
    n_slots = K if slot_src is None else int(n_slots)
    assert not torch.is_tensor(aug) or (aug.is_cuda and aug.is_contiguous() and aug.numel() * aug.element_size() >= n_slots * CROP_AUG.itemsize)
    dev = gt.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_train_augment(gt.data_ptr(), draw.data_ptr(), _addr(slot_src), K, n_slots, out_box.data_ptr(), _addr(aug),
                                                 torch.cuda.current_stream(dev).cuda_stream), "o3d_train_augment")


def crop_groups_aug(plan, dev_plan, dev_aug, scratch):
    """One o3d_track_crop_groups_aug call (three launches, no sync): crop_groups with dev_aug = the DEVICE array of
    plan.shape[0] pointers to CROP_AUG records (an int64 GPU tensor, an address, or None = no record anywhere)"""
    dev = scratch.device
    assert not torch.is_tensor(dev_aug) or (dev_aug.is_cuda and dev_aug.dtype == torch.int64 and dev_aug.is_contiguous()
                                            and dev_aug.numel() >= plan.shape[0])
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_track_crop_groups_aug(
            plan.ctypes.data, _addr(dev_plan), _addr(dev_aug), plan.shape[0], scratch.data_ptr(), scratch.numel(),
            torch.cuda.current_stream(dev).cuda_stream), "o3d_track_crop_groups_aug")


def inside_box(points, box15, factor=1.0):
    """One o3d_train_inside_box launch: points (n,3) float32 GPU contiguous, box15 (15,) GPU -> (n,) int32 mask, the inclusive
    test of points_in_box in the kernels' fp32 operation order"""
    _need_gpu(points, "inside_box")
    _need_gpu(box15, "inside_box")
    assert points.dtype == torch.float32 and points.is_contiguous() and points.dim() == 2 and points.shape[1] == 3
    assert box15.dtype == torch.float32 and box15.is_contiguous() and box15.numel() == 15
    dev = points.device
    mask = torch.empty((points.shape[0],), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_train_inside_box(points.data_ptr(), points.shape[0], box15.data_ptr(), float(factor), mask.data_ptr(),
                                                    torch.cuda.current_stream(dev).cuda_stream), "o3d_train_inside_box")
    return mask


def train_motion_labels(prev_gt, this_gt, ref_box, degrees, motion_threshold, this_box, prev_box, canon_box, box_label,
                        box_label_prev, motion_label, motion_state, bbox_size):
    """One o3d_train_motion_labels launch on (J,15) float32 GPU tensors; the last eight are written in place ((J,15) x 3,
    (J,4) x 3, motion_state (J,) int32, bbox_size (J,3))"""
    J = prev_gt.numel() // 15
    for t, width, dt in ((prev_gt, 15, torch.float32), (this_gt, 15, torch.float32), (ref_box, 15, torch.float32),
                         (this_box, 15, torch.float32), (prev_box, 15, torch.float32), (canon_box, 15, torch.float32),
                         (box_label, 4, torch.float32), (box_label_prev, 4, torch.float32), (motion_label, 4, torch.float32),
                         (motion_state, 1, torch.int32), (bbox_size, 3, torch.float32)):
        _need_gpu(t, "train_motion_labels")
        assert t.dtype == dt and t.is_contiguous() and t.numel() == width * J
    dev = prev_gt.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_train_motion_labels(
            prev_gt.data_ptr(), this_gt.data_ptr(), ref_box.data_ptr(), J, int(bool(degrees)), float(motion_threshold), this_box.data_ptr(),
            prev_box.data_ptr(), canon_box.data_ptr(), box_label.data_ptr(), box_label_prev.data_ptr(), motion_label.data_ptr(),
            motion_state.data_ptr(), bbox_size.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "o3d_train_motion_labels")


def train_select_motion(counts, B, caps, sel, n_valid, overflow):
    """One o3d_train_select_motion launch: counts (J,3) int32 GPU = (in-box, previous crop, current crop), caps = (cap_prev,
    cap_this) -> sel (B,), n_valid (1,), overflow (1,) int32 GPU tensors, written in place"""
    for t in (counts, sel, n_valid, overflow):
        _need_gpu(t, "train_select_motion")
        assert t.dtype == torch.int32 and t.is_contiguous()
    J = counts.numel() // 3
    assert counts.numel() == 3 * J and sel.numel() >= B
    dev = counts.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_train_select_motion(counts.data_ptr(), J, int(B), int(caps[0]), int(caps[1]), sel.data_ptr(),
                                                       n_valid.data_ptr(), overflow.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "o3d_train_select_motion")


def train_motion_sample(args, device):
    """One o3d_train_motion_sample launch: args = a filled _TrainMotionSampleArgs (the caller keeps its tensors alive)"""
    with torch.cuda.device(device):
        capi.check(capi.load().o3d_train_motion_sample(ctypes.addressof(args), torch.cuda.current_stream(device).cuda_stream),
                   "o3d_train_motion_sample")


# ---- the planned training epoch (csrc/train_batch.hip; sampler.py's build_planned is the caller) ------------------------------
TRAIN_DRAW_SIAMESE = capi.CONSTANTS["O3D_TRAIN_DRAW_SIAMESE"]
TRAIN_DRAW_MOTION = capi.CONSTANTS["O3D_TRAIN_DRAW_MOTION"]
TRAIN_DRAW_MOTION_AUG = capi.CONSTANTS["O3D_TRAIN_DRAW_MOTION_AUG"]


def train_draw(gt, rows, cand, J, seed, counter, degrees, num_candidates, mode, refs, first, offs, aug):
    """One o3d_train_draw launch (no sync): gt (R,15) float32 GPU = the box pool; rows (J,3 | J,2) and cand (J,) int32 GPU
    tensors, or addresses inside an uploaded chunk -> refs (2J,15), first (J,15) | None, offs (2J,4 | J,4), aug (2J,6) | None,
    float32 GPU tensors written in place"""
    _need_gpu(gt, "train_draw")
    assert gt.dtype == torch.float32 and gt.is_contiguous() and gt.dim() == 2 and gt.shape[1] == 15
    siamese = mode == TRAIN_DRAW_SIAMESE
    for t, numel in ((refs, 30 * J), (first, 15 * J if siamese else None), (offs, (8 if siamese else 4) * J),
                     (aug, 12 * J if mode == TRAIN_DRAW_MOTION_AUG else None)):
        if numel is not None:
            _need_gpu(t, "train_draw")
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= numel and t.device == gt.device
    for t, numel in ((rows, (3 if siamese else 2) * J), (cand, J)):
        assert not torch.is_tensor(t) or (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= numel)
    dev = gt.device
    with torch.cuda.device(dev):
        capi.check(capi.load().o3d_train_draw(
            gt.data_ptr(), gt.shape[0], _addr(rows), _addr(cand), int(J), _key_bits(seed), _key_bits(counter), int(bool(degrees)),
            int(num_candidates), int(mode), _addr(refs), _addr(first), _addr(offs), _addr(aug),
            torch.cuda.current_stream(dev).cuda_stream), "o3d_train_draw")
