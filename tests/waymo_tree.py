"""A small Waymo SOT tree written from a seed into a directory: the input of both tests/golden/make_golden_waymo.py (which
runs the reference's WaymoDataset on it) and the reader tests.  No frame is committed; build(dir, generate) is deterministic.

Layout, as the reference's datasets/waymo_data.py and datasets/generate_waymo_sot.py read it:
  <root>/<split>/lidar/seq_<s>_frame_<f>.pkl   {'scene_name', 'frame_id', 'lidars': {'points_xyz': (n,3) float32}}
  <root>/<split>/annos/seq_<s>_frame_<f>.pkl   {'scene_name', 'frame_id', 'veh_to_global': (16,) float64,
                                                'objects': [{'id', 'name', 'label', 'box': (9,) float32, 'num_points'}]}
  <root>/infos_<split>_01sweeps_filter_zero_gt.pkl   [{'path': the lidar file, 'anno_path': the annos file relative to root}]
  <root>/sot_infos_<category>_<split>.pkl      written by `generate(root, CLASS, split)`: the reference's generate_waymo_data in
                                                the fixture generator, datasets.generate_waymo_sot_infos in the tests
'path' is absolute (the reference opens it as it stands) unless build(..., absolute=False), which writes it relative to root.
The reader derives the annos file by replacing EVERY `lidar` of that string, so `root` must not contain `lidar`.

split `train`: sequences 0 (6 frames) and 1 (5 frames) of 300 .. 2 000 points in the vehicle frame.  Per sequence s:
  s<s>_veh_a   VEHICLE     every frame
  s<s>_veh_b   VEHICLE     frames 0, 1, 4, (5)     (a gap; shares its frames with veh_a)
  s<s>_veh_far VEHICLE     frames 2, 3             (its box is 500 m from every point: it keeps nothing)
  s<s>_ped     PEDESTRIAN  frames 1 .. 4
  s<s>_cyc     CYCLIST     frames 0 .. 2
  s<s>_sign    SIGN        every frame             (no category of the reader)
Frame 4 of sequence 0 has 0 points.  Every frame has its own pose: yaw, a few degrees of pitch and roll, a translation of
1e3 .. 2e4 m, built as a product of three plane rotations in fp64 (orthonormal to 1e-15).
split `val`: sequence 2, two frames of 300 points with 51 VEHICLE objects each, all names distinct: 102 one-frame tracklets,
of which `tiny` keeps 100; one PEDESTRIAN and one CYCLIST over both frames.
"""
import math
import os
import pickle

import numpy as np

CLASSES = ("VEHICLE", "PEDESTRIAN", "CYCLIST")
LABEL = {"UNKNOWN": 0, "VEHICLE": 1, "PEDESTRIAN": 2, "SIGN": 3, "CYCLIST": 4}
TRAIN_FRAMES = {0: 6, 1: 5}
EMPTY = (0, 4)
TRACKS = (("veh_a", "VEHICLE", (0, 1, 2, 3, 4, 5)), ("veh_b", "VEHICLE", (0, 1, 4, 5)), ("veh_far", "VEHICLE", (2, 3)),
          ("ped", "PEDESTRIAN", (1, 2, 3, 4)), ("cyc", "CYCLIST", (0, 1, 2)), ("sign", "SIGN", (0, 1, 2, 3, 4, 5)))
LWH = {"VEHICLE": (4.6, 1.9, 1.6), "PEDESTRIAN": (0.8, 0.7, 1.75), "CYCLIST": (1.8, 0.7, 1.7), "SIGN": (0.1, 0.6, 0.6)}


def pose(seq, frame):
    """veh_to_global (4,4) fp64 of a frame"""
    yaw, pitch, roll = 0.6 + 1.1 * seq + 0.04 * frame, 0.03 - 0.01 * frame, -0.02 + 0.008 * frame + 0.01 * seq
    cz, sz, cy, sy, cx, sx = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    rot = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @ \
        np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    T = np.eye(4)
    T[:3, :3] = rot
    T[:3, 3] = [2913.37 + 5000.0 * seq + 7.3 * frame, -17842.61 + 900.0 * seq - 4.1 * frame, 1021.9 + 0.35 * frame]
    return T


def object_box(track, cls, seq, frame):
    """the (9,) float32 annotation in the vehicle frame: x y z length width height vx vy heading"""
    if track == "veh_far":
        centre = (500.0 + frame, 30.0, 0.4)
    else:
        k = [t[0] for t in TRACKS].index(track)
        centre = (6.0 + 5.0 * k + 0.7 * frame, -12.0 + 6.5 * k - 0.3 * frame + seq, 0.2 + 0.1 * k)
    return np.array(list(centre) + list(LWH[cls]) + [0.7, -0.3, 0.4 * ([t[0] for t in TRACKS].index(track)) - 0.09 * frame + 0.3 * seq],
                    np.float32)


def _dump(file, obj):
    with open(file, "wb") as f:
        pickle.dump(obj, f, protocol=4)


def _frame(root, split, seq, frame, n, objects, rng, absolute):
    name = "seq_%d_frame_%d.pkl" % (seq, frame)
    near = [o["box"][:3] for o in objects if o["box"][0] < 400.0 and o["label"] != LABEL["SIGN"]]
    n_obj = min(n, 120 * len(near))
    pts = np.empty((n, 3), np.float32)
    pts[:n - n_obj] = rng.uniform([-40.0, -40.0, -2.5], [40.0, 40.0, 1.5], size=(n - n_obj, 3))
    for i in range(n_obj):
        pts[n - n_obj + i] = near[i % len(near)] + rng.normal(scale=(1.2, 0.8, 0.5))
    pts = pts[rng.permutation(n)]
    rel = os.path.join(split, "lidar", name)
    _dump(os.path.join(root, rel), {"scene_name": "seq_%d" % seq, "frame_id": frame, "lidars": {"points_xyz": pts}})
    _dump(os.path.join(root, split, "annos", name),
          {"scene_name": "seq_%d" % seq, "frame_id": frame, "veh_to_global": pose(seq, frame).reshape(-1), "objects": objects})
    return {"path": os.path.join(root, rel) if absolute else rel, "anno_path": os.path.join(split, "annos", name),
            "token": name}


def build(root, generate, seed=0, absolute=True):
    """write the tree under `root` (created), then the sot_infos files with generate(root, CLASS, split); -> root"""
    assert "lidar" not in root, "the reader replaces every `lidar` of a frame's path"
    rng = np.random.default_rng(seed)
    for split in ("train", "val"):
        for sub in ("lidar", "annos"):
            os.makedirs(os.path.join(root, split, sub), exist_ok=True)
    infos = []
    for seq, frames in TRAIN_FRAMES.items():
        for frame in range(frames):
            objects = [{"id": i, "name": "s%d_%s" % (seq, track), "label": LABEL[cls], "box": object_box(track, cls, seq, frame),
                        "num_points": 40} for i, (track, cls, at) in enumerate(TRACKS) if frame in at]
            n = 0 if (seq, frame) == EMPTY else int(rng.integers(300, 2001))
            infos.append(_frame(root, "train", seq, frame, n, objects, rng, absolute))
    _dump(os.path.join(root, "infos_train_01sweeps_filter_zero_gt.pkl"), infos)
    infos = []
    for frame in range(2):
        objects = [{"id": i, "name": "v%d_%02d" % (frame, i), "label": LABEL["VEHICLE"], "num_points": 5,
                    "box": np.array([-35.0 + 1.4 * i, 20.0 - 0.8 * i + frame, 0.3, 4.4, 1.8, 1.5, 0.0, 0.0, 0.05 * i], np.float32)}
                   for i in range(51)]
        for i, cls in ((51, "PEDESTRIAN"), (52, "CYCLIST")):
            objects.append({"id": i, "name": "val_" + cls.lower(), "label": LABEL[cls], "num_points": 5,
                            "box": np.array([3.0 * (i - 50), -4.0 + frame, 0.2] + list(LWH[cls]) + [0.1, 0.0, 1.0 + frame], np.float32)})
        infos.append(_frame(root, "val", 2, frame, 300, objects, rng, absolute))
    _dump(os.path.join(root, "infos_val_01sweeps_filter_zero_gt.pkl"), infos)
    for split in ("train", "val"):
        for cls in CLASSES:
            generate(root, cls, split)
    return root
