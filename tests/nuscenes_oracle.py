"""A numpy restatement of the steps rule of csrc/preload.hip and of the NuScenes reader (TEST ONLY), written from the rule, not
from the kernel:

  step       on the float32 input (x, y, z) with M the (3,4) fp64 [R | t] of the step:
               r_i = float32((M_i0*x + M_i1*y) + M_i2*z)          every operation in fp64, this order, one rounding
               translate32 = 0:  p_i = float32(float64(r_i) + M_i3)   an fp64 sum, one more rounding
               translate32 = 1:  p_i = r_i + float32(M_i3)            an fp32 add
             p is the next step's input; any number of steps
  raw rows   row r is floats [r*row_floats, r*row_floats + 3) of the raw table, row_floats = 3 | 4 | 5
  bounds     kitti_oracle.bounds: the fp64 bounds of crop_pc_axis_aligned rounded directionally to float32
  test       lo < p < hi per axis, strictly, in float32; the survivors keep the order of the frame

tests/test_nuscenes_reader_cpu.py shows that with translate32 = 0 it reproduces every cloud of the reference's NuScenesDataset
(run under numpy >= 2) bit for bit; tests/test_nuscenes_reader_gpu.py holds the kernels and the reader to it."""
import numpy as np

import kitti_oracle as KO
from waymo_oracle import ref_clouds, rows  # noqa: F401  (the same fixture layout, the same raw table)


def chain(raw, steps, translate32=0):
    """raw (n,>=3) float32, steps (n_steps,3,4) | (n_steps,12) fp64 -> (n,3) float32"""
    p = np.ascontiguousarray(np.asarray(raw)[:, :3], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for M in np.asarray(steps, np.float64).reshape(-1, 3, 4):
            x, y, z = (p[:, i].astype(np.float64) for i in range(3))
            r = [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z).astype(np.float32) for i in range(3)]
            if translate32:
                p = np.stack([r[i] + np.float32(M[i, 3]) for i in range(3)], 1)
            else:
                p = np.stack([(r[i].astype(np.float64) + M[i, 3]).astype(np.float32) for i in range(3)], 1)
            assert p.dtype == np.float32
    return p


def crop(raw, bnd, steps, translate32=0):
    """the rows of chain(raw, steps) strictly inside the float32 bounds bnd (6,), in order"""
    return KO.crop(chain(raw, steps, translate32), bnd)


def crop_steps(raw, row_floats, records, bounds, steps, translate32=0):
    """The steps launches: records = [(first raw row, n, number of boxes)], bounds (B,6) float32 in record order, steps
    (F,n_steps,12) fp64 -> per box the (count,3) float32 survivors"""
    out, b = [], 0
    for (row0, n, nb), S in zip(records, steps):
        p = chain(rows(raw, row_floats, row0, n), S, translate32)
        for k in range(nb):
            out.append(KO.crop(p, bounds[b + k]))
        b += nb
    return out


def read_sweep(file):
    """(n,5) float32 of a .pcd.bin"""
    return np.fromfile(file, np.float32).reshape(-1, 5)


def reader(annos, files, steps, offset, read, translate32=0):
    """the clouds of every tracklet frame by the device rule: annos / files / steps = datasets.nuscenes_annotations' output,
    read(file) -> (n,5) float32 -> a list (per tracklet) of lists of (n,3) float32"""
    cache, out = {}, []
    for a in annos:
        clouds = []
        for f, box in zip(a["frames"], a["boxes"]):
            if f not in cache:
                cache[f] = chain(read(files[f]), steps[f], translate32)
            clouds.append(KO.crop(cache[f], KO.bounds(box, offset)))
        out.append(clouds)
    return out


def case_name(category, offset, split, key_frame_only, min_points):
    return "%s.%d.%s.k%d.m%d" % (category, offset, split, int(key_frame_only), int(min_points))


def cases(ref):
    """(name, category, offset, split, key_frame_only, min_points) of every case of the fixture tests/golden/ref_nuscenes.npz"""
    out = []
    for k in ref.files:
        if k.endswith(".cloud_ids"):
            name = k[:-len(".cloud_ids")]
            c, o, s, kf, m = name.split(".")
            out.append((name, c, int(o), s, kf == "k1", int(m[1:])))
    return out
