"""A numpy restatement of the device rule of csrc/preload.hip (TEST ONLY), written from the rule, not from the kernel:

  bounds     the fp64 bounds of crop_pc_axis_aligned -- min / max over the eight corners of the fp64 box, -+ offset -- rounded
             directionally to float32: lo to the largest float32 <= it, hi to the smallest float32 >= it
  transform  camera mode: p'_i = float32(((T_i0*x + T_i1*y) + T_i2*z) + T_i3), every operation in fp64 on the float32 input
  test       lo < p < hi per axis, strictly, in float32
  order      the survivors keep the order of the frame

and of the frame plan of o3d_preload_scratch.  tests/test_kitti_reader_cpu.py shows that it reproduces every cloud of the
reference's kittiDataset bit for bit; tests/test_kitti_reader_gpu.py holds the kernels to it."""
import numpy as np

WG = 256
SIGNS = np.array([[1, 1, 1, 1, -1, -1, -1, -1], [1, -1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1, -1]], np.float64)


def f32_at_most(m):
    """the largest float32 <= the double m"""
    with np.errstate(over="ignore"):
        f = np.float32(m)
    return np.nextafter(f, np.float32(-np.inf)) if np.float64(f) > m else f


def f32_at_least(m):
    """the smallest float32 >= the double m"""
    with np.errstate(over="ignore"):
        f = np.float32(m)
    return np.nextafter(f, np.float32(np.inf)) if np.float64(f) < m else f


def bounds(box15, offset):
    """(6,) float32 [lo xyz | hi xyz] of the fp64 box; offset <= 0: no crop"""
    if offset <= 0:
        return np.array([-np.inf] * 3 + [np.inf] * 3, np.float32)
    b = np.asarray(box15, np.float64)
    w, l, h = b[3:6]
    corners = b[6:15].reshape(3, 3) @ (SIGNS * np.array([[l / 2], [w / 2], [h / 2]])) + b[0:3, None]
    lo, hi = corners.min(1) - offset, corners.max(1) + offset
    return np.array([f32_at_most(v) for v in lo] + [f32_at_least(v) for v in hi], np.float32)


def transform(raw, T):
    """raw (n,>=3) float32, T (3,4) fp64 | None -> (n,3) float32"""
    p = np.ascontiguousarray(raw[:, :3], np.float32)
    if T is None:
        return p
    x, y, z = (p[:, i].astype(np.float64) for i in range(3))
    T = np.asarray(T, np.float64)
    return np.stack([(((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]).astype(np.float32) for i in range(3)], 1)


def crop(raw, bnd, T=None):
    """the rows of transform(raw, T) strictly inside the float32 bounds bnd (6,), in order"""
    p = transform(raw, T)
    bnd = np.asarray(bnd, np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.ones(p.shape[0], bool)
        for a in range(3):
            keep &= (p[:, a] > bnd[a]) & (p[:, a] < bnd[3 + a])
    return p[keep]


def plan(n, boxes):
    """the frame plan: n, boxes = per record the points and the number of boxes -> (first box, workgroup start, scratch base)
    per record, the scratch length, the workgroups, B"""
    first, wg, base, b, w, s = [], [], [], 0, 0, 0
    for ni, ki in zip(n, boxes):
        first.append(b); wg.append(w); base.append(s)
        W = 0 if ki == 0 else max(1, -(-ni // WG))
        b, w, s = b + ki, w + W, s + W * ki
    return first, wg, base, s, w, b


def reader(annos, calibs, coordinate_mode, offset, read_bin):
    """the clouds of every tracklet frame by the device rule: annos / calibs = datasets.kitti_annotations' output, read_bin(scene,
    frame) -> (n,4) float32 | None (missing) -> a list (per tracklet) of lists of (n,3) float32"""
    out = []
    for a in annos:
        T = calibs[a["scene"]][:3] if coordinate_mode == "camera" else None
        clouds = []
        for frame, box in zip(a["frames"], a["boxes"]):
            raw = read_bin(a["scene"], int(frame))
            clouds.append(np.zeros((1, 3), np.float32) if raw is None else crop(raw, bounds(box, offset), T))
        out.append(clouds)
    return out
