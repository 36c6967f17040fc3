"""fp32 numpy restatement of the three kernels of open3dsot_amd/csrc/track.hip, in the kernels' stated operation order
(every numpy operation below is ONE fp32 operation on float32 arrays: no fused multiply-add, the order of the parentheses
is the order written at the head of track.hip).  The GPU tests compare the crop bit for bit against this; the CPU tests
compare this against the reference's own masks (tests/golden/ref_tracking.npz).  Test infrastructure only -- the product
has no CPU path.  tools/track_bench.py uses `crop` as the host crop a user had to write before the device loop existed."""
import numpy as np

SUBWINDOW, MODEL = 0, 1
f32 = np.float32


def crop_mask(points, box15, scale, offset, mode):
    """-> (keep (n,) bool, q (n,3) float32)"""
    p = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    b = np.asarray(box15, dtype=f32).reshape(15)
    scale, offset = f32(scale), f32(offset)
    dx, dy, dz = p[:, 0] - b[0], p[:, 1] - b[1], p[:, 2] - b[2]
    w, l, h = b[3], b[4], b[5]
    R = b[6:15]
    keep = np.ones(p.shape[0], bool)
    if mode == MODEL:
        s4, o2 = f32(4) * scale, f32(2) * offset
        L, W, H = (l * s4) * f32(0.5), (w * s4) * f32(0.5), (h * s4) * f32(0.5)
        e = [((np.abs(R[3 * i]) * L + np.abs(R[3 * i + 1]) * W) + np.abs(R[3 * i + 2]) * H) + o2 for i in range(3)]
        keep = (np.abs(dx) < e[0]) & (np.abs(dy) < e[1]) & (np.abs(dz) < e[2])
    qx = (R[0] * dx + R[3] * dy) + R[6] * dz
    qy = (R[1] * dx + R[4] * dy) + R[7] * dz
    qz = (R[2] * dx + R[5] * dy) + R[8] * dz
    hx, hy, hz = (l * scale) * f32(0.5) + offset, (w * scale) * f32(0.5) + offset, (h * scale) * f32(0.5) + offset
    keep = keep & (np.abs(qx) < hx) & (np.abs(qy) < hy) & (np.abs(qz) < hz)
    q = np.stack([qx, qy, qz], 1)
    assert q.dtype == f32
    return keep, q


def crop(points, box15, scale, offset, mode, capacity=None):
    """o3d_track_crop for one job -> (count, out): the survivors' q in their original order; with a capacity, `out` holds
    the first min(count, capacity) of them"""
    keep, q = crop_mask(points, box15, scale, offset, mode)
    out = q[keep]
    return int(keep.sum()), (out if capacity is None else out[:capacity])


def resample(src, idx, n, zero=False):
    """o3d_track_resample for one job"""
    if zero:
        return np.zeros((n, 3), f32)
    return np.asarray(src, f32)[np.asarray(idx)[:n]]


def limit_draw(seed, frame, comp):
    """the counter-based draw of track.hip (uint32 arithmetic) -> float32 in [-1, 1)"""
    m = 0xFFFFFFFF
    x = ((seed * 0x9E3779B1) & m) ^ ((frame * 0x85EBCA77 + comp * 0xC2B2AE3D + 0x27D4EB2F) & m)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & m
    x ^= x >> 16
    return f32(f32(x >> 8) * f32(2.0 / 16777216.0) - f32(1))


def offset_box(ref15, offset4, degrees, use_z, limit_box, seed=0, frame=0, yaw_state=None, rebase=False):
    """o3d_track_offset_box -> (box15 float32, new yaw_state | None): the arithmetic in double, rounded once, as the kernel"""
    ref = np.asarray(ref15, f32).reshape(15)
    off = np.asarray(offset4, f32).reshape(-1)[:4].copy()
    w, l, h = ref[3], ref[4], ref[5]
    if limit_box:
        if off[0] > w:
            off[0] = limit_draw(seed, frame, 0)
        if off[1] > min(l, f32(2)):
            off[1] = limit_draw(seed, frame, 1)
        if use_z and off[2] > h:
            off[2] = 0
    theta = float(off[3]) * (np.pi / 180.0) if degrees else float(off[3])
    chained = yaw_state is not None and not rebase

    def rz(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    if chained:
        R0 = np.asarray(yaw_state[:9], np.float64).reshape(3, 3)
        Rr = R0 @ rz(float(yaw_state[9]))
        yaw = float(yaw_state[9]) + theta
    else:
        R0 = ref[6:15].astype(np.float64).reshape(3, 3)
        Rr, yaw = R0, theta
    o = np.array([float(off[0]), float(off[1]), float(off[2]) if use_z else 0.0])
    yaw_f = f32(yaw)
    box = np.concatenate([ref[:3].astype(np.float64) + Rr @ o, [w, l, h],
                          (R0 @ rz(float(yaw_f) if yaw_state is not None else yaw)).reshape(-1)]).astype(f32)
    state = None
    if yaw_state is not None:
        state = np.concatenate([R0.reshape(-1), [yaw_f]]).astype(f32)
    return box, state


# ---- the cases of tests/golden/ref_tracking.npz (tests/golden/make_golden_tracking.py) -------------------------------------
# the evaluation keys of cfgs/BAT_Car.yaml :5-10,14,53-57 (P2B_Car.yaml has the same ones)
TEST_KEYS = dict(search_bb_scale=1.25, search_bb_offset=2, model_bb_scale=1.25, model_bb_offset=0, degrees=True, use_z=True,
                 limit_box=False, reference_BB="previous_result", shape_aggregation="firstandprevious", IoU_space=3,
                 up_axis=[0, 0, 1])
# case -> (model, overrides of TEST_KEYS)
CASES = {"bat_fap": ("BAT", {}), "p2b": ("P2B", {"limit_box": False}), "bat_first": ("BAT", {"shape_aggregation": "first"}),
         "bat_all": ("BAT", {"shape_aggregation": "all"})}
SEQ_FRAMES, SEQ_POINTS, FULL_POINTS = 8, 20000, 120000


def case_config(case):
    """the config dictionary of a case: the model keys of open3dsot_amd.trackers + the evaluation keys"""
    from open3dsot_amd import trackers
    name, over = CASES[case]
    cfg = dict(trackers.BAT_CAR if name == "BAT" else trackers.P2B_CAR)
    cfg.update(TEST_KEYS)
    cfg.update(over)
    return name, cfg


def init_weights(model):
    """The weights of the tracking fixture, storage-free: det_init.fill_state_dict_random(seed 0), then the rows of the two
    last layers that MOVE things -- the votes' xyz offsets (rpn.vote_layer, rows 0..2) and the proposals' (x, y, z, theta)
    (rpn.FC_proposal, rows 0..3) -- scaled by 0.05.  A He-initialised head moves the box by ~9 m per frame, off the target
    and into empty space within two frames; scaled, it moves it by decimetres, as a trained tracker does, so that every
    frame of the fixture has a populated search window.  The objectness row is left as drawn."""
    import det_init
    import torch
    det_init.fill_state_dict_random(model, seed=0)
    with torch.no_grad():
        for seq, rows in ((model.rpn.vote_layer, 3), (model.rpn.FC_proposal, 4)):
            last = [m for m in seq.modules() if isinstance(m, torch.nn.Conv1d)][-1]
            last.weight[:rows] *= 0.05
            last.bias[:rows] *= 0.05
    return model
