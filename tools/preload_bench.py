"""What reading a KITTI, a Waymo or a nuScenes tree into HBM costs with the device-side preload crop (open3dsot_amd/datasets.py, csrc/preload.hip),
against the host preload restated in numpy.  Not bench.py: that measures the training step on resident batches.

  python tools/preload_bench.py [--dataset kitti|waymo|nuscenes] [--scenes 2] [--frames 50] [--points 120000] [--tracklets 8]
                                [--offset 10] [--runs 7] [--chunk-frames 64] [--mode velodyne|camera] [--host-only]

Setup: a synthetic tree in a temporary directory -- `--scenes` scenes (0019, 0020: the split `test`) of `--frames`
velodyne files of `--points` points (uniform in 80 m x 80 m x 4 m), `--tracklets` Car tracklets per scene annotated in every
frame.  Every file is read once before anything is timed, so all timings are from the page cache.  Each figure is the median
of `--runs` runs with the smallest and the largest, one JSON line at the end:
  reader_s            KittiTracklets(...) end to end (host clock, ends in a device synchronise): parse, read, upload, crop
  read_s              the host's file reads into the pinned buffer (host clock), summed over the chunks
  (read_s .. scatter_ms are the reader's own chunks run stage by stage: the reader's items -- datasets.kitti_items,
   waymo_items, nuscenes_items -- cut by datasets.preload_chunks, the one cut rule, and made into PreloadChunks by the
   reader class; `chunks` is their number)
  upload_ms           the raw frames and the tables, host to device (HIP events)
  count_ms, scatter_ms  the count + scan launches and the scatter launch (HIP events); launch_GBps = the bytes the three
                      launches must move (the raw rows twice, the pool rows once) over count_ms + scatter_ms
  host_numpy_s        the YARDSTICK: this file's numpy restatement of the host preload (every distinct frame read once, one
                      axis-aligned crop per annotated object per frame, float32 coordinates against fp64 bounds) -- NOT the
                      reference itself, which also builds a pandas frame and Box / PointCloud objects per annotation
The clouds of the restatement and of the reader are compared bit for bit before the result is printed.

--dataset waymo: the tree is `--scenes` sequences of `--frames` lidar and annotation pickles ((n,3) float32 points, a pose of
kilometres per frame), `--tracklets` VEHICLE objects per sequence annotated in every frame; the reader is WaymoTracklets, the
launches are the posed pair (a pose per frame record, rows of three floats), and read_s is the pull of the items, which
unpickles, plus the copy into the pinned buffer (the bounds and the plan are outside it, as for KITTI).  The yardstick transforms with numpy's `dot`, as the reference does; the bit-for-bit comparison is
against the same restatement with the ordered fp64 sum (BLAS may sum in another order, which reaches a float32 coordinate only
at a rounding boundary), and `dot_clouds_differing` counts the clouds where the two restatements differ.

--dataset nuscenes: the tree is the nine JSON tables and `--scenes` scenes of `--frames` key-frame .pcd.bin sweeps ((n,5)
float32 rows: x y z intensity ring; an ego pose of hundreds of metres per sweep), `--tracklets` vehicle.car instances per scene
annotated in every sample; the reader is NuScenesTracklets (translate="float64"), the launches are the steps pair (two rounded
rigid steps per frame record, rows of five floats uploaded as they lie), and read_s is the readinto of the files.  raw_bytes
is what is uploaded (20 bytes a row); launch_bytes counts the 12 bytes a row that the launches ask for, twice, plus the pool
rows -- the memory system fetches whole lines, so the 8 bytes between are moved as well.  The yardstick does what the reference
does with numpy (`dot` for rotate, `points[i] + np.float64` for translate, under the installed numpy >= 2); the bit-for-bit
comparison is against the same restatement with the ordered fp64 sums, and `dot_clouds_differing` counts as for waymo.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_tree(root, scenes, frames, points, tracklets, seed=0):
    rng = np.random.default_rng(seed)
    a = 0.012
    T = np.hstack([np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]) @
                   np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]), [[-0.004], [-0.076], [-0.27]]])
    for sub in ("label_02", "calib"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    names = ["%04d" % (19 + s) for s in range(scenes)]
    for scene in names:
        os.makedirs(os.path.join(root, "velodyne", scene), exist_ok=True)
        with open(os.path.join(root, "calib", scene + ".txt"), "w") as f:
            f.write("Tr_velo_cam " + " ".join("%.12e" % v for v in T.reshape(-1)) + "\n")
        start = rng.uniform([-25.0, -25.0, -1.0], [25.0, 25.0, -0.6], size=(tracklets, 3))
        speed = rng.uniform(-0.3, 0.3, size=(tracklets, 3)) * [1.0, 1.0, 0.0]
        lines = []
        for frame in range(frames):
            for k in range(tracklets):
                cam = T[:, :3] @ (start[k] + frame * speed[k]) + T[:, 3]
                lines.append("%d %d Car 0 0 -1.500000 100.000000 150.000000 200.000000 250.000000 %.6f %.6f %.6f %.6f %.6f %.6f %.6f"
                             % (frame, k, 1.5, 1.6, 3.9, cam[0], cam[1] + 0.75, cam[2], 0.2 * k + 0.01 * frame))
            pts = np.empty((points, 4), np.float32)
            pts[:, :3] = rng.uniform([-40.0, -40.0, -2.5], [40.0, 40.0, 1.5], size=(points, 3))
            pts[:, 3] = rng.uniform(size=points)
            pts.tofile(os.path.join(root, "velodyne", scene, "%06d.bin" % frame))
        with open(os.path.join(root, "label_02", scene + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return "test" if scenes == 2 else "testtiny"


SIGNS = np.array([[1, 1, 1, 1, -1, -1, -1, -1], [1, -1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1, -1]], np.float64)


def crop(pc, box, offset):
    """the reference's axis-aligned preload crop of a (3,n) float32 cloud: strictly inside the box's corners -+ offset, the
    float32 coordinates against fp64 bounds; offset <= 0: the cloud itself"""
    if offset <= 0:
        return pc
    w, l, h = box[3:6]
    corners = box[6:15].reshape(3, 3) @ (SIGNS * np.array([[l / 2], [w / 2], [h / 2]])) + box[0:3, None]
    hi, lo = corners.max(1) + offset, corners.min(1) - offset
    return pc[:, (pc[0] < hi[0]) & (pc[0] > lo[0]) & (pc[1] < hi[1]) & (pc[1] > lo[1]) & (pc[2] < hi[2]) & (pc[2] > lo[2])]


def host_preload(D, root, split, mode, offset):
    """the host preload in numpy: -> a list (per tracklet) of lists of (n,3) float32"""
    annos, calibs = D.kitti_annotations(root, split, "Car", mode)
    cache, out = {}, []
    for a in annos:
        clouds = []
        for frame, box in zip(a["frames"], a["boxes"]):
            key = (a["scene"], int(frame))
            if key not in cache:
                pc = np.fromfile(os.path.join(root, "velodyne", key[0], "%06d.bin" % key[1]), np.float32).reshape(-1, 4).T[:3]
                if mode == "camera":
                    pc = pc.copy()
                    pc[:3] = calibs[key[0]].dot(np.vstack((pc, np.ones(pc.shape[1]))))[:3]
                cache[key] = pc
            clouds.append(crop(cache[key], box, offset))
        out.append(clouds)
    return out


def write_waymo_tree(D, root, scenes, frames, points, tracklets, seed=0):
    import pickle
    rng = np.random.default_rng(seed)
    for sub in ("lidar", "annos"):
        os.makedirs(os.path.join(root, "train", sub), exist_ok=True)
    infos = []
    for s in range(scenes):
        start = rng.uniform([-25.0, -25.0, -1.0], [25.0, 25.0, -0.6], size=(tracklets, 3))
        speed = rng.uniform(-0.3, 0.3, size=(tracklets, 3)) * [1.0, 1.0, 0.0]
        for frame in range(frames):
            yaw, pitch = 0.5 + s + 0.01 * frame, 0.02
            T = np.eye(4)
            T[:3, :3] = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]) @ \
                np.array([[np.cos(pitch), 0.0, np.sin(pitch)], [0.0, 1.0, 0.0], [-np.sin(pitch), 0.0, np.cos(pitch)]])
            T[:3, 3] = [2913.37 + 5000.0 * s + 1.5 * frame, -17842.61 - 0.8 * frame, 120.5]
            objects = [{"name": "s%d_%d" % (s, k), "label": 1,
                        "box": np.array(list(start[k] + frame * speed[k]) + [3.9, 1.6, 1.5, 0.0, 0.0, 0.2 * k + 0.01 * frame], np.float32)}
                       for k in range(tracklets)]
            name = "seq_%d_frame_%d.pkl" % (s, frame)
            pts = rng.uniform([-40.0, -40.0, -2.5], [40.0, 40.0, 1.5], size=(points, 3)).astype(np.float32)
            with open(os.path.join(root, "train", "lidar", name), "wb") as f:
                pickle.dump({"lidars": {"points_xyz": pts}}, f, protocol=4)
            with open(os.path.join(root, "train", "annos", name), "wb") as f:
                pickle.dump({"veh_to_global": T.reshape(-1), "objects": objects}, f, protocol=4)
            infos.append({"path": os.path.join(root, "train", "lidar", name), "anno_path": os.path.join("train", "annos", name)})
    with open(os.path.join(root, "infos_train_01sweeps_filter_zero_gt.pkl"), "wb") as f:
        pickle.dump(infos, f, protocol=4)
    D.generate_waymo_sot_infos(root, "VEHICLE", "train")
    return "train"


def host_preload_waymo(D, root, split, offset, ordered=False):
    """the host preload of WaymoDataset in numpy: -> a list (per tracklet) of lists of (3,n) float32"""
    annos, files, poses = D.waymo_annotations(root, split, "VEHICLE")
    cache, out = {}, []
    for a in annos:
        clouds = []
        for f, box in zip(a["frames"], a["boxes"]):
            if f not in cache:
                pc = D.waymo_points(files[f]).transpose((1, 0)).copy()
                if ordered:
                    x, y, z = (pc[i].astype(np.float64) for i in range(3))
                    T = poses[f]
                    for i in range(3):
                        pc[i] = ((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]
                else:
                    pc[:3] = poses[f].dot(np.vstack((pc, np.ones(pc.shape[1]))))
                cache[f] = pc
            clouds.append(crop(cache[f], box, offset))
        out.append(clouds)
    return out


def write_nuscenes_tree(root, scenes, frames, points, tracklets, version, seed=0):
    """the nine tables with the fields the reader looks at, and the sweeps -> the split table"""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, version), exist_ok=True)
    os.makedirs(os.path.join(root, "samples", "LIDAR_TOP"), exist_ok=True)

    def quat(yaw, pitch):
        cz, sz, cy, sy = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2)
        return [float(cz * cy), float(-sz * sy), float(cz * sy), float(sz * cy)]         # Rz(yaw) Ry(pitch)

    def matrix(q):
        w, x, y, z = q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    tables = {n: [] for n in ("category", "instance", "sample_annotation", "sample", "sample_data", "scene", "sensor", "calibrated_sensor",
                              "ego_pose")}
    tables["category"].append({"token": "cat_car", "name": "vehicle.car"})
    tables["sensor"].append({"token": "lidar", "channel": "LIDAR_TOP", "modality": "lidar"})
    cs = {"token": "cs", "sensor_token": "lidar", "rotation": quat(-1.57, 0.01), "translation": [0.94, 0.0, 1.84]}
    tables["calibrated_sensor"].append(cs)
    for s in range(scenes):
        tables["scene"].append({"token": "scene%d" % s, "name": "scene-%04d" % s})
        start = rng.uniform([-25.0, -25.0, -1.0], [25.0, 25.0, -0.6], size=(tracklets, 3))
        speed = rng.uniform(-0.3, 0.3, size=(tracklets, 3)) * [1.0, 1.0, 0.0]
        for k in range(tracklets):
            tables["instance"].append({"token": "inst%d_%d" % (s, k), "category_token": "cat_car", "first_annotation_token": "a%d_%d_0" % (s, k)})
        for frame in range(frames):
            ego = {"token": "ego%d_%d" % (s, frame), "rotation": quat(0.5 + s + 0.01 * frame, 0.02),
                   "translation": [411.3 + 600.0 * s + 1.5 * frame, 1180.9 - 0.8 * frame, 1.84]}
            file = "samples/LIDAR_TOP/s%d_%d.pcd.bin" % (s, frame)
            tables["ego_pose"].append(ego)
            tables["sample"].append({"token": "smp%d_%d" % (s, frame), "scene_token": "scene%d" % s})
            tables["sample_data"].append({"token": "sd%d_%d" % (s, frame), "sample_token": "smp%d_%d" % (s, frame), "ego_pose_token": ego["token"],
                                          "calibrated_sensor_token": "cs", "is_key_frame": True, "filename": file})
            for k in range(tracklets):
                local = start[k] + frame * speed[k]
                centre = matrix(ego["rotation"]) @ (matrix(cs["rotation"]) @ local + cs["translation"]) + ego["translation"]
                yaw = 0.2 * k + 0.01 * frame
                tables["sample_annotation"].append(
                    {"token": "a%d_%d_%d" % (s, k, frame), "sample_token": "smp%d_%d" % (s, frame), "instance_token": "inst%d_%d" % (s, k),
                     "translation": [float(v) for v in centre], "size": [1.6, 3.9, 1.5], "rotation": [float(np.cos(yaw / 2)), 0.0, 0.0, float(np.sin(yaw / 2))],
                     "next": "a%d_%d_%d" % (s, k, frame + 1) if frame + 1 < frames else "", "num_lidar_pts": 40})
            pts = np.empty((points, 5), np.float32)
            pts[:, :3] = rng.uniform([-40.0, -40.0, -2.5], [40.0, 40.0, 1.5], size=(points, 3))
            pts[:, 3] = rng.uniform(0, 255, size=points)
            pts[:, 4] = rng.integers(0, 32, size=points)
            pts.tofile(os.path.join(root, file))
    for name, rows in tables.items():
        with open(os.path.join(root, version, name + ".json"), "w") as f:
            json.dump(rows, f)
    return {"train": [sc["name"] for sc in tables["scene"]]}


def host_preload_nuscenes(D, root, version, splits, offset, ordered=False):
    """the host preload of NuScenesDataset in numpy: -> a list (per tracklet) of lists of (3,n) float32"""
    annos, files, steps = D.nuscenes_annotations(root, "train", "Car", version, scenes=splits)
    cache, out = {}, []
    for a in annos:
        clouds = []
        for f, box in zip(a["frames"], a["boxes"]):
            if f not in cache:
                pc = np.fromfile(os.path.join(root, files[f]), np.float32).reshape(-1, 5)[:, :4].T[:3]
                for M in steps[f].reshape(-1, 3, 4):
                    if ordered:
                        x, y, z = (pc[i].astype(np.float64) for i in range(3))
                        for i in range(3):
                            pc[i] = (M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z
                    else:
                        pc[:3] = np.dot(M[:, :3], pc[:3])
                    for i in range(3):
                        pc[i] = pc[i] + M[i, 3]                               # an np.float64 scalar: fp64 under numpy >= 2
                cache[f] = pc
            clouds.append(crop(cache[f], box, offset))
        out.append(clouds)
    return out


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def timed_pulls(items, tot):
    """`items`, with the time of every pull added to tot["read"]: a Waymo item unpickles its lidar file when it is pulled"""
    it = iter(items)
    while True:
        t0 = time.perf_counter()
        item = next(it, None)
        tot["read"] += time.perf_counter() - t0
        if item is None:
            return
        yield item


def staged(torch, D, reader, dev, items, args, raw_row_bytes, read_row_bytes):
    """The reader's own chunks (D.preload_chunks over the reader's items, made into PreloadChunks by the reader class), stage by
    stage -> the timing fields.  items() gives the items afresh for a run; a raw row is raw_row_bytes in the upload and
    read_row_bytes of it are what a launch asks for"""
    cols = {"read": [], "upload": [], "count": [], "scatter": []}
    for run in range(args.runs + 1):                                        # run 0 warms up
        tot = dict.fromkeys(cols, 0.0)
        raw_rows = pool_rows = chunks = 0
        pinned = None
        for ck in D.preload_chunks(timed_pulls(items(), tot), args.chunk_frames):
            c = reader.preload_chunk(ck, dev, pinned)
            pinned = c.pinned
            t0 = time.perf_counter()
            c.read()
            tot["read"] += time.perf_counter() - t0
            e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            with torch.cuda.device(dev):
                e[0].record(); c.upload(); e[1].record(); c.count(); e[2].record()
                c.read_back()
                e[3].record(); c.scatter(); e[4].record()
            torch.cuda.synchronize(dev)
            tot["upload"] += e[0].elapsed_time(e[1])
            tot["count"] += e[1].elapsed_time(e[2])
            tot["scatter"] += e[3].elapsed_time(e[4])
            raw_rows, pool_rows, chunks = raw_rows + c.raw_rows, pool_rows + c.pool.shape[0], chunks + 1
        if run:
            for k in cols:
                cols[k].append(tot[k])
    raw_bytes, pool_bytes = raw_row_bytes * raw_rows, 12 * pool_rows
    moved = 2 * read_row_bytes * raw_rows + pool_bytes
    return dict(read_s=stat(cols["read"]), upload_ms=stat(cols["upload"]), count_ms=stat(cols["count"]), scatter_ms=stat(cols["scatter"]),
                raw_bytes=raw_bytes, pool_bytes=pool_bytes, launch_bytes=moved,
                launch_GBps=stat([moved / ((a + b) * 1e-3) / 1e9 for a, b in zip(cols["count"], cols["scatter"])]),
                upload_GBps=stat([raw_bytes / (ms * 1e-3) / 1e9 for ms in cols["upload"]]), chunks=chunks)


# per dataset: (args, D, root) -> what the JSON line says of the setup beyond the sizes (head, mid), host(ordered) the numpy
# restatement (ordered=True: the fp64 sums in the device's order, what the clouds are compared against; by_dot: whether
# ordered=False is another restatement), make(device) the reader, items() its PreloadItems, row_bytes = the bytes of a raw
# row (uploaded, asked for by a launch)
def setup_kitti(args, D, root):
    split = write_tree(root, args.scenes, args.frames, args.points, args.tracklets)
    kw = dict(category_name="Car", coordinate_mode=args.mode, preload_offset=args.offset, chunk_frames=args.chunk_frames)
    annos, calibs = D.kitti_annotations(root, split, "Car", args.mode)
    return SimpleNamespace(head={}, mid={"mode": args.mode}, by_dot=False, row_bytes=(16, 16),
                           host=lambda ordered=False: host_preload(D, root, split, args.mode, args.offset),
                           make=lambda dev: D.KittiTracklets(root, split, device=dev, **kw),
                           items=lambda: D.kitti_items(root, annos, calibs, args.mode, args.offset)[0])


def setup_waymo(args, D, root):
    split = write_waymo_tree(D, root, args.scenes, args.frames, args.points, args.tracklets)
    kw = dict(category_name="VEHICLE", preload_offset=args.offset, chunk_frames=args.chunk_frames)
    annos, files, poses = D.waymo_annotations(root, split, "VEHICLE")
    return SimpleNamespace(head={"dataset": "waymo"}, mid={}, by_dot=True, row_bytes=(12, 12),
                           host=lambda ordered=False: host_preload_waymo(D, root, split, args.offset, ordered),
                           make=lambda dev: D.WaymoTracklets(root, split, device=dev, **kw),
                           items=lambda: D.waymo_items(annos, files, poses, args.offset))


def setup_nuscenes(args, D, root):
    version = "v1.0-trainval"
    assert int(np.__version__.split(".")[0]) >= 2, "the yardstick's translate is numpy's: the reader's default mode is that of numpy >= 2"
    splits = write_nuscenes_tree(root, args.scenes, args.frames, args.points, args.tracklets, version)
    kw = dict(category_name="Car", version=version, preload_offset=args.offset, scenes=splits, chunk_frames=args.chunk_frames)
    annos, files, steps = D.nuscenes_annotations(root, "train", "Car", version, scenes=splits)
    return SimpleNamespace(head={"dataset": "nuscenes"}, mid={}, by_dot=True, row_bytes=(20, 12),
                           host=lambda ordered=False: host_preload_nuscenes(D, root, version, splits, args.offset, ordered),
                           make=lambda dev: D.NuScenesTracklets(root, "train", device=dev, **kw),
                           items=lambda: D.nuscenes_items(root, annos, files, steps, args.offset))


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("frames", 50), ("points", 120000), ("tracklets", 8), ("runs", 7), ("chunk-frames", 64)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--offset", type=float, default=10.0)
    ap.add_argument("--scenes", type=int, choices=(1, 2), default=2)
    ap.add_argument("--mode", choices=("velodyne", "camera"), default="velodyne")
    ap.add_argument("--dataset", choices=("kitti", "waymo", "nuscenes"), default="kitti")
    ap.add_argument("--host-only", action="store_true", help="write the tree and time the numpy restatement only (no device)")
    args = ap.parse_args()
    assert args.runs >= 7 or args.host_only, "a median of at least 7 runs"
    import torch
    from open3dsot_amd import datasets as D
    if not args.host_only and not torch.cuda.is_available():
        raise SystemExit("preload_bench needs a GPU: the reader cannot be measured on the host")
    setup = {"kitti": setup_kitti, "waymo": setup_waymo, "nuscenes": setup_nuscenes}[args.dataset]
    with tempfile.TemporaryDirectory() as root:
        s = setup(args, D, root)
        host = s.host(ordered=True)                                         # reads every file once: the page cache is warm
        res = {"tool": "preload_bench", **s.head, "scenes": args.scenes, "frames": args.frames, "points": args.points,
               "tracklets_per_scene": args.tracklets, "preload_offset": args.offset, **s.mid, "crops": sum(len(c) for c in host)}
        if s.by_dot:
            res["dot_clouds_differing"] = sum(a.tobytes() != b.tobytes() for x, y in zip(host, s.host()) for a, b in zip(x, y))
        host_s = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            s.host()
            host_s.append(time.perf_counter() - t0)
        res["host_numpy_s"] = stat(host_s)
        if args.host_only:
            print(json.dumps(res))
            return
        dev = torch.device("cuda", 0)
        trk = s.make(dev)                                                   # warm-up: code objects, the allocator, pinned memory
        torch.cuda.synchronize(dev)
        for t, h in zip(trk, host):                                         # faster and different is not faster
            for g, c in zip(t.frames, h):
                c = np.ascontiguousarray(c.T, np.float32)
                assert tuple(g.shape) == c.shape and np.array_equal(g.cpu().numpy().view(np.int32), c.view(np.int32))
        reader_s = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            trk = s.make(dev)
            torch.cuda.synchronize(dev)
            reader_s.append(time.perf_counter() - t0)
        res.update(reader_s=stat(reader_s), **staged(torch, D, type(trk), dev, s.items, args, *s.row_bytes),
                   host_over_reader=statistics.median(host_s) / statistics.median(reader_s))
        print(json.dumps(res))


if __name__ == "__main__":
    main()
