"""fp32 numpy restatement of o3d_track_motion_input (open3dsot_amd/csrc/track.hip), in the operation order written at the
head of that file: every numpy operation below is ONE fp32 operation on float32 arrays, no fused multiply-add.  The GPU
tests compare the kernel's xyz, time stamp and prior-targetness channels bit for bit against this; the CPU tests compare this
against the reference's own build_input_dict (tests/golden/ref_motion_tracking.npz, made by
tests/golden/make_golden_motion_tracking.py).  Also here: the fixture's case table, its weights and its hand-made input
cases, and `host_input`, the host form of build_input_dict that tools/track_bench.py times.  Test infrastructure only -- the
product has no CPU path."""
import numpy as np

import tracking_oracle as TO

f32 = np.float32
SX = np.array([1, 1, 1, 1, -1, -1, -1, -1], f32)        # Box.corners (datasets/data_classes.py:236-238)
SY = np.array([1, -1, -1, 1, 1, -1, -1, 1], f32)
SZ = np.array([1, 1, -1, -1, 1, 1, -1, -1], f32)


def motion_input(prev, cur, idx, N, wlh, first_frame, zero=(False, False), with_bc=True):
    """-> (points (2N,5) float32, candidate_bc (2N,9) float32 | None)"""
    wlh = np.asarray(wlh, f32).reshape(3)
    xyz = np.zeros((2 * N, 3), f32)
    for h, src in enumerate((prev, cur)):
        if zero[h]:
            continue
        src = np.asarray(src, f32).reshape(-1, 3)
        s = np.asarray(idx).reshape(-1)[h * N:(h + 1) * N].astype(np.int64)
        ok = (s >= 0) & (s < src.shape[0])                 # an index outside the source leaves a zero row
        rows = np.zeros((N, 3), f32)
        rows[ok] = src[s[ok]]
        xyz[h * N:(h + 1) * N] = rows
    pts = np.zeros((2 * N, 5), f32)
    pts[:, :3] = xyz
    pts[N:, 3], pts[N:, 4] = f32(0.1), f32(0.5)
    x, y, z = xyz[:N, 0], xyz[:N, 1], xyz[:N, 2]
    w, l, h = wlh
    hx, hy, hz = (l * f32(1.25)) * f32(0.5), (w * f32(1.25)) * f32(0.5), (h * f32(1.25)) * f32(0.5)
    inside = (np.abs(x) <= hx) & (np.abs(y) <= hy) & (np.abs(z) <= hz)
    pts[:N, 4] = np.where(inside, f32(1), f32(0)) if first_frame else np.where(inside, f32(0.8), f32(0.2))
    if not with_bc:
        return pts, None
    bc = np.zeros((2 * N, 9), f32)
    a, b, c = l * f32(0.5), w * f32(0.5), h * f32(0.5)
    bc[:N, 0] = np.sqrt((x * x + y * y) + z * z)
    for k in range(8):
        dx, dy, dz = x - SX[k] * a, y - SY[k] * b, z - SZ[k] * c
        bc[:N, 1 + k] = np.sqrt((dx * dx + dy * dy) + dz * dz)
    assert pts.dtype == f32 and bc.dtype == f32
    return pts, bc


def boxcloud64(xyz, wlh):
    """fp64: the distances of the rows to the centre and the eight corners of the canonical box"""
    w, l, h = np.asarray(wlh, np.float64)
    lm = np.concatenate([np.zeros((1, 3)), np.stack([SX * l / 2, SY * w / 2, SZ * h / 2], 1).astype(np.float64)], 0)
    return np.linalg.norm(np.asarray(xyz, np.float64)[:, None, :] - lm[None], axis=2)


def host_input(prev_frame, this_frame, box15, cfg, first_frame, with_bc=True):
    """MotionBaseModel.build_input_dict (models/base_model.py:255-304) on the host: the two crops (the fp32 restatement of
    generate_subwindow), the reference's index draws, and the channels above -> (points, candidate_bc | None, counts)"""
    from open3dsot_amd import tracking
    N = int(cfg["point_sample_size"])
    n_prev, prev = TO.crop(prev_frame, box15, cfg["bb_scale"], cfg["bb_offset"], TO.SUBWINDOW)
    n_this, cur = TO.crop(this_frame, box15, cfg["bb_scale"], cfg["bb_offset"], TO.SUBWINDOW)
    ip, it = tracking.draw_indices(n_prev, N), tracking.draw_indices(n_this, N)
    idx = np.concatenate([np.zeros(N, np.int64) if ip is None else ip, np.zeros(N, np.int64) if it is None else it])
    pts, bc = motion_input(prev, cur, idx, N, np.asarray(box15, f32)[3:6], first_frame, zero=(ip is None, it is None), with_bc=with_bc)
    return pts, bc, (n_prev, n_this)


# ---- the cases of tests/golden/ref_motion_tracking.npz (tests/golden/make_golden_motion_tracking.py) -----------------------
# the evaluation keys of cfgs/M2_track_kitti.yaml :5-8,10,32-34
TEST_KEYS = dict(bb_scale=1.25, bb_offset=2, point_sample_size=1024, degrees=False, use_z=True, limit_box=False, IoU_space=3,
                 up_axis=[0, 0, 1])
CASES = {"kitti": {}, "no_bc": {"box_aware": False}}
SEQ_FRAMES, SEQ_POINTS = TO.SEQ_FRAMES, TO.SEQ_POINTS
TIE = 2e-3                    # the TIE of tests/test_golden_m2track.py::replay_hard_masks
MAX_NEAR_TIES = 32
HEAD_SCALE = 0.005
SEG_BIAS_SHIFT = {True: -0.9, False: 1.0}      # box_aware -> added to the foreground logit's bias (seg_pointnet.fc.bias[1])
MIXED_FRAMES = 4                               # the generator wants both classes in the mask of at least 4 of the 7 frames


def case_config(case):
    """the config dictionary of a case: the model keys of open3dsot_amd.m2track + the evaluation keys"""
    from open3dsot_amd import m2track
    cfg = dict(m2track.M2_KITTI)
    cfg.update(TEST_KEYS)
    cfg.update(CASES[case])
    return cfg


def init_weights(model):
    """The weights of the motion-tracking fixture, storage-free: det_init.fill_by_module_type(seed 0) -- the streams of
    det_init.fill_state_dict_random (PCG64 seeded by (crc32(key), seed)), with a tensor's kind taken from the TYPE of the
    module that owns it -- then two adjustments.

    Why not fill_state_dict_random(seed 0): it recognises a BatchNorm by the `bn.` marker in its key, which the nn.Sequential
    stacks of M2-Track do not carry, and draws their gammas from N(0, 2); under it every point of every frame is background
    (logit margins ~100) and the network answers with the same four numbers at every frame.

    1. The LAST Linear of the three heads that move the box (motion_mlp, final_mlp, box_mlp) is scaled by HEAD_SCALE = 0.005,
       weight and bias.  Unscaled they answer with ~25 m and ~10 rad per frame, which carries the box into empty space at
       once; scaled, the box moves by about a decimetre and a few hundredths of a radian per frame, so that every frame's two
       windows stay populated (the reasoning of tracking_oracle.init_weights).
    2. The bias of the segmentation head's foreground logit (seg_pointnet.fc.bias[1]) is shifted by SEG_BIAS_SHIFT: -0.9 with
       box_aware, +1.0 without.  As drawn, the per-point margins l1 - l0 lie between about 0.2 and 2.5 on one side of zero --
       all foreground with candidate_bc, all background without -- so that the hard mask would be a constant; the shift
       moves zero into that range, and both classes occur.  The generator asserts it (MIXED_FRAMES) together with pairwise
       different estimation_boxes.  The motion-state head is left as drawn."""
    import det_init
    import torch
    det_init.fill_by_module_type(model, seed=0)
    with torch.no_grad():
        for name in ("motion_mlp", "final_mlp", "box_mlp"):
            last = getattr(model, name)[-1]
            assert isinstance(last, torch.nn.Linear) and last.out_features == 4
            last.weight *= HEAD_SCALE
            last.bias *= HEAD_SCALE
        model.seg_pointnet.fc.bias[1] += SEG_BIAS_SHIFT[bool(model.box_aware)]
    return model


# ---- the three input-only cases: hand-made frame pairs through the reference's build_input_dict alone ----------------------
# name -> (points kept in the previous window, in the current window, frame_id handed to build_input_dict)
INPUT_N = 256
INPUT_CASES = {"zero_fill": (2, 700, 2), "with_replacement": (100, 180, 1), "exact": (INPUT_N, INPUT_N, 2)}


def box_margin(q, half):
    """fp64, per row: min over the axes of (half extent - |coordinate|): > 0 inside, < 0 outside the box"""
    return (np.asarray(half, np.float64)[None] - np.abs(np.asarray(q, np.float64))).min(1)


def input_case_frames(name):
    """-> (prev_frame, this_frame, box15): two frames of synth.make_sequence thinned so that the window of the box holds exactly
    the case's number of points in each; points within 2e-3 m of a window plane or (in the box frame) of a face of the
    1.25-scaled box are dropped first, so that no decision of the case hangs on rounding"""
    from open3dsot_amd import synth
    n_prev, n_this, _ = INPUT_CASES[name]
    frames, gt = synth.make_sequence(40 + list(INPUT_CASES).index(name), 2, SEQ_POINTS)
    box = gt[0]
    out = []
    for f, n in zip(frames, (n_prev, n_this)):
        b = box.astype(np.float64)
        q = (f.astype(np.float64) - b[0:3]) @ b[6:15].reshape(3, 3)
        lwh = np.array([b[4], b[3], b[5]])
        m_win = box_margin(q, lwh * TEST_KEYS["bb_scale"] / 2 + TEST_KEYS["bb_offset"])
        m_box = box_margin(q, lwh * 1.25 / 2)
        f = f[(np.abs(m_win) > 2e-3) & (np.abs(m_box) > 2e-3)]
        keep, _ = TO.crop_mask(f, box, TEST_KEYS["bb_scale"], TEST_KEYS["bb_offset"], TO.SUBWINDOW)
        inside = np.flatnonzero(keep)
        assert inside.size >= n, (name, inside.size, n)
        drop = inside[n:]
        sel = np.ones(f.shape[0], bool)
        sel[drop] = False
        out.append(np.ascontiguousarray(f[sel]))
    return out[0], out[1], box
