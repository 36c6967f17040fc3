"""A small nuScenes tree written from a seed into a directory: the input of both tests/golden/make_golden_nuscenes.py (which
runs the reference's NuScenesDataset on it over tests/golden/nuscenes_standin.py) and the reader tests.  No sweep is
committed; build(dir) is deterministic.  numpy and json only.

Layout, as the devkit documents it and the reference's datasets/nuscenes_data.py reads it:
  <root>/<VERSION>/{category, instance, sample_annotation, sample, sample_data, scene, sensor, calibrated_sensor, ego_pose}.json
  <root>/samples/LIDAR_TOP/<scene>_<i>.pcd.bin     (n,5) float32: x y z intensity ring in the sensor frame
  <root>/splits.json                               SPLITS, for the reader's scenes= (the split lists live in the devkit)
Tables the reference never reads (attribute, visibility, log, map) are not written; files of other sensors and of sweeps that
are no key frames are named by sample_data but not written: nothing opens them.

Scenes: scene-0001 (5 samples) and scene-0002 (4) in `train`, scene-0003 (3) in `val`, scene-0004 (2) in no split: 14 key-frame
sweeps of 200 .. 600 points.  Every sample has, in this table order, a LIDAR_TOP sweep that is no key frame, its key-frame
LIDAR_TOP record, a key-frame CAM_FRONT and a key-frame RADAR_FRONT record and one more LIDAR_TOP sweep that is no key frame:
whoever ignores `is_key_frame` or the channel picks a wrong record (another file, another pose).  Every record has its own
ego pose (yaw, pitch and roll; a translation of 400 .. 2000 m); every scene its own calibrated sensors (yaw, pitch, roll too).
Instances per scene, in TRACKS' order (`at`: the samples they are annotated in, cut to the scene's length):
  car_a     vehicle.car                    every sample
  car_b     vehicle.car                    samples 1 ..          (shares its sweeps with car_a)
  ped_a     human.pedestrian.adult         samples 0 .. 2
  ped_c     human.pedestrian.child         samples 1 ..          (a second general class of `pedestrian`)
  bus       vehicle.bus.rigid              every sample
  barrier   movable_object.barrier         every sample          (`void / ignore`)
  car_none  vehicle.car                    every sample; its first annotation has num_lidar_pts 0, the others 7
  car_few   vehicle.car                    every sample; its first annotation has num_lidar_pts 3
  car_one   vehicle.car                    sample 2 only         (a tracklet of one annotation; not in the scenes of 2 samples)
No instance is a truck, a trailer, a bicycle or a motorcycle: `truck` is the class with no instance.
"""
import hashlib
import json
import math
import os

import numpy as np

VERSION = "v1.0-trainval"
SCENES = (("scene-0001", 5), ("scene-0002", 4), ("scene-0003", 3), ("scene-0004", 2))
SPLITS = {"train": ["scene-0001", "scene-0002"], "val": ["scene-0003"], "test": []}
CATEGORIES = ("animal", "human.pedestrian.adult", "human.pedestrian.child", "human.pedestrian.construction_worker",
              "human.pedestrian.personal_mobility", "human.pedestrian.police_officer", "human.pedestrian.stroller",
              "human.pedestrian.wheelchair", "movable_object.barrier", "movable_object.debris", "movable_object.pushable_pullable",
              "movable_object.trafficcone", "static_object.bicycle_rack", "vehicle.bicycle", "vehicle.bus.bendy", "vehicle.bus.rigid",
              "vehicle.car", "vehicle.construction", "vehicle.emergency.ambulance", "vehicle.emergency.police", "vehicle.motorcycle",
              "vehicle.trailer", "vehicle.truck")
SENSORS = (("LIDAR_TOP", "lidar"), ("CAM_FRONT", "camera"), ("RADAR_FRONT", "radar"))
# name, category, samples, size (w, l, h), num_lidar_pts of the first annotation
TRACKS = (("car_a", "vehicle.car", range(0, 9), (1.9, 4.6, 1.6), 40),
          ("car_b", "vehicle.car", range(1, 9), (1.8, 4.3, 1.5), 40),
          ("ped_a", "human.pedestrian.adult", range(0, 3), (0.7, 0.8, 1.75), 40),
          ("ped_c", "human.pedestrian.child", range(1, 9), (0.5, 0.5, 1.2), 40),
          ("bus", "vehicle.bus.rigid", range(0, 9), (2.9, 11.2, 3.4), 40),
          ("barrier", "movable_object.barrier", range(0, 9), (2.5, 0.6, 1.0), 40),
          ("car_none", "vehicle.car", range(0, 9), (1.9, 4.4, 1.7), 0),
          ("car_few", "vehicle.car", range(0, 9), (2.0, 4.8, 1.5), 3),
          ("car_one", "vehicle.car", range(2, 3), (1.8, 4.1, 1.4), 40))


def token(*parts):
    """a 32-digit token, as the tables carry them"""
    return hashlib.md5("/".join(str(p) for p in parts).encode()).hexdigest()


def quat(yaw, pitch, roll):
    """(w, x, y, z) of Rz(yaw) Ry(pitch) Rx(roll), as a list of floats"""
    def mul(a, b):
        return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]
    qz = [math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)]
    qy = [math.cos(pitch / 2), 0.0, math.sin(pitch / 2), 0.0]
    qx = [math.cos(roll / 2), math.sin(roll / 2), 0.0, 0.0]
    return mul(mul(qz, qy), qx)


def matrix(q):
    """the rotation matrix of the quaternion q, fp64 (used only to place the boxes where the points are)"""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def calibrated(s, channel):
    """rotation, translation of scene s's calibrated sensor on `channel`"""
    c = [n for n, _ in SENSORS].index(channel)
    return (quat(-1.5 + 0.02 * s + 0.7 * c, 0.011 - 0.004 * s + 0.1 * c, -0.007 + 0.003 * s),
            [0.94 + 0.01 * s + 0.5 * c, 0.02 * s - 0.3 * c, 1.84 - 0.01 * s])


def ego(s, i, k):
    """rotation, translation of the ego pose of record k (0 .. 4, the key-frame lidar record is 1) of sample i of scene s"""
    t = i + 0.1 * (k - 1)
    return (quat(0.5 + 1.3 * s + 0.06 * t, 0.02 - 0.007 * t, -0.015 + 0.006 * t + 0.01 * s),
            [411.3 + 380.0 * s + 6.1 * t, 1180.9 + 190.0 * s - 3.7 * t, 1.2 + 0.3 * s + 0.05 * t])


def local_centre(k, i, s):
    """the centre of track k's box in the sensor frame of sample i of scene s"""
    return np.array([-24.0 + 6.5 * k + 0.8 * i, 14.0 - 4.0 * k + 0.5 * i - s, -1.0 + 0.05 * k])


def _dump(root, name, rows):
    with open(os.path.join(root, VERSION, name + ".json"), "w") as f:
        json.dump(rows, f, indent=0)


def lidar_file(scene, i):
    return "samples/LIDAR_TOP/%s_%d.pcd.bin" % (scene, i)


def build(root, seed=0):
    """write the tree under `root` (created) -> root"""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, VERSION), exist_ok=True)
    os.makedirs(os.path.join(root, "samples", "LIDAR_TOP"), exist_ok=True)
    _dump(root, "category", [{"token": token("category", c), "name": c, "description": ""} for c in CATEGORIES])
    _dump(root, "sensor", [{"token": token("sensor", n), "channel": n, "modality": m} for n, m in SENSORS])
    scenes, samples, sample_data, calibs, egos, instances, annos = [], [], [], [], [], [], []
    for s, (scene, S) in enumerate(SCENES):
        stoks = [token("sample", scene, i) for i in range(S)]
        scenes.append({"token": token("scene", scene), "log_token": token("log", scene), "nbr_samples": S, "first_sample_token": stoks[0],
                       "last_sample_token": stoks[-1], "name": scene, "description": ""})
        for channel, _ in SENSORS:
            rot, tr = calibrated(s, channel)
            calibs.append({"token": token("calib", scene, channel), "sensor_token": token("sensor", channel), "translation": tr,
                           "rotation": rot, "camera_intrinsic": []})
        present = [(k, tr) for k, tr in enumerate(TRACKS) if any(i in tr[2] for i in range(S))]
        for i in range(S):
            samples.append({"token": stoks[i], "timestamp": 1532402927000000 + 1000000 * s + 500000 * i, "prev": stoks[i - 1] if i else "",
                            "next": stoks[i + 1] if i + 1 < S else "", "scene_token": token("scene", scene)})
            records = (("LIDAR_TOP", False, "sweeps/LIDAR_TOP/%s_%d_before.pcd.bin" % (scene, i)), ("LIDAR_TOP", True, lidar_file(scene, i)),
                       ("CAM_FRONT", True, "samples/CAM_FRONT/%s_%d.jpg" % (scene, i)),
                       ("RADAR_FRONT", True, "samples/RADAR_FRONT/%s_%d.pcd" % (scene, i)),
                       ("LIDAR_TOP", False, "sweeps/LIDAR_TOP/%s_%d_after.pcd.bin" % (scene, i)))
            for k, (channel, key, file) in enumerate(records):
                rot, tr = ego(s, i, k)
                egos.append({"token": token("ego", scene, i, k), "timestamp": samples[-1]["timestamp"] + 1000 * k, "rotation": rot,
                             "translation": tr})
                sample_data.append({"token": token("sample_data", scene, i, k), "sample_token": stoks[i], "ego_pose_token": egos[-1]["token"],
                                    "calibrated_sensor_token": token("calib", scene, channel), "timestamp": egos[-1]["timestamp"],
                                    "fileformat": file.rsplit(".", 1)[1], "is_key_frame": key, "height": 0, "width": 0, "filename": file,
                                    "prev": "", "next": ""})
            # the sweep: background, and a cluster around every annotated object (not the barrier's)
            near = [local_centre(k, i, s) for k, tr in present if i in tr[2] and tr[0] != "barrier"]
            n = int(rng.integers(200, 601))
            n_obj = min(n // 2, 30 * len(near))
            pts = np.empty((n, 5), np.float32)
            pts[:n - n_obj, :3] = rng.uniform([-40.0, -40.0, -2.5], [40.0, 40.0, 1.5], size=(n - n_obj, 3))
            for j in range(n_obj):
                pts[n - n_obj + j, :3] = near[j % len(near)] + rng.normal(scale=(1.2, 0.8, 0.5))
            pts[:, 3] = rng.uniform(0, 255, size=n)
            pts[:, 4] = rng.integers(0, 32, size=n)
            pts = pts[rng.permutation(n)]
            pts.tofile(os.path.join(root, lidar_file(scene, i)))
        for k, (name, category, at, size, first_pts) in present:
            at = [i for i in range(S) if i in at]
            atoks = [token("anno", scene, name, i) for i in at]
            instances.append({"token": token("instance", scene, name), "category_token": token("category", category),
                              "nbr_annotations": len(at), "first_annotation_token": atoks[0], "last_annotation_token": atoks[-1]})
            for j, i in enumerate(at):
                (crot, ctr), (erot, etr) = calibrated(s, "LIDAR_TOP"), ego(s, i, 1)
                centre = matrix(erot) @ (matrix(crot) @ local_centre(k, i, s) + np.array(ctr)) + np.array(etr)
                annos.append({"token": atoks[j], "sample_token": stoks[i], "instance_token": instances[-1]["token"],
                              "visibility_token": "4", "attribute_tokens": [], "translation": [float(v) for v in centre],
                              "size": list(size), "rotation": quat(0.3 * k - 0.05 * i + 0.9 * s, 0.0, 0.0),
                              "prev": atoks[j - 1] if j else "", "next": atoks[j + 1] if j + 1 < len(at) else "",
                              "num_lidar_pts": first_pts if j == 0 else 7 if name == "car_none" else 40, "num_radar_pts": 0})
    for name, rows in (("scene", scenes), ("sample", samples), ("sample_data", sample_data), ("calibrated_sensor", calibs), ("ego_pose", egos),
                       ("instance", instances), ("sample_annotation", annos)):
        _dump(root, name, rows)
    with open(os.path.join(root, "splits.json"), "w") as f:
        json.dump(SPLITS, f)
    return root


def sweeps():
    """the key-frame sweep files, relative to the tree, in table order"""
    return [lidar_file(scene, i) for scene, S in SCENES for i in range(S)]
