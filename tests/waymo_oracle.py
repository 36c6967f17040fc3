"""A numpy restatement of the posed device rule of csrc/preload.hip and of the Waymo reader (TEST ONLY), written from the
rule, not from the kernel:

  pose       p'_i = float32(((T_i0*x + T_i1*y) + T_i2*z) + T_i3) with T the (3,4) fp64 pose of the point's frame record, every
             operation in fp64 on the float32 input, ONE rounding (kitti_oracle.transform: the camera-mode rule)
  raw rows   row r is floats [r*row_floats, r*row_floats + 3) of the raw table, row_floats = 3 | 4
  bounds     kitti_oracle.bounds: the fp64 bounds of crop_pc_axis_aligned rounded directionally to float32
  test       lo < p < hi per axis, strictly, in float32; the survivors keep the order of the frame

tests/test_waymo_reader_cpu.py shows that it reproduces every cloud of the reference's WaymoDataset bit for bit;
tests/test_waymo_reader_gpu.py holds the kernels and the reader to it."""
import numpy as np

import kitti_oracle as KO


def rows(raw, row_floats, row0, n):
    """rows [row0, row0 + n) of the flat float32 table `raw` -> (n,3)"""
    flat = np.asarray(raw, np.float32).reshape(-1)
    return flat[row0 * row_floats:(row0 + n) * row_floats].reshape(n, row_floats)[:, :3]


def crop_posed(raw, row_floats, records, bounds, poses):
    """The posed launches: records = [(first raw row, n, number of boxes)], bounds (B,6) float32 in record order, poses
    (F,3,4) fp64 -> per box the (count,3) float32 survivors"""
    out, b = [], 0
    for (row0, n, nb), T in zip(records, poses):
        p = rows(raw, row_floats, row0, n)
        for k in range(nb):
            out.append(KO.crop(p, bounds[b + k], T))
        b += nb
    return out


def reader(annos, files, poses, offset, read_points):
    """the clouds of every tracklet frame by the device rule: annos / files / poses = datasets.waymo_annotations' output,
    read_points(file) -> (n,3) float32 -> a list (per tracklet) of lists of (n,3) float32"""
    cache = {}
    out = []
    for a in annos:
        clouds = []
        for f, box in zip(a["frames"], a["boxes"]):
            if f not in cache:
                cache[f] = np.ascontiguousarray(read_points(files[f]), np.float32)
            clouds.append(KO.crop(cache[f], KO.bounds(box, offset), poses[f]))
        out.append(clouds)
    return out


def cases(ref):
    """(name, category, offset, split, tiny) of every case of the fixture tests/golden/ref_waymo.npz"""
    out = []
    for k in ref.files:
        if k.endswith(".cloud_ids"):
            name = k[:-len(".cloud_ids")]
            parts = name.split(".")
            out.append((name, parts[0], int(parts[1]), parts[2], len(parts) == 4))
    return out


def ref_clouds(ref, name):
    """the fixture's clouds of a case, cut into tracklets"""
    flat = [ref["cloud.%d" % i] for i in ref[name + ".cloud_ids"]]
    ends = np.cumsum(ref[name + ".lengths"])
    return [flat[a:b] for a, b in zip(np.concatenate([[0], ends[:-1]]), ends)]
