"""A small KITTI tracking tree (velodyne/, label_02/, calib/) written from a seed into a directory: the input of both
tests/golden/make_golden_kitti.py (which runs the reference's kittiDataset on it) and the reader tests.  No frame is
committed; build(dir) is deterministic.

Two scenes, 0000 and 0019 (so that `traintiny` and `testtiny` each see one), FRAMES frames of POINTS points each.
Per scene the label file holds, in KITTI's order (by frame, then track id):
  track 0  Car         every frame
  track 1  Van         frames 0, 1, 2
  track 2  Pedestrian  frames 1 .. 4
  track 3  Car         frames 0, 1, 4, 5      (a gap in its frame numbers)
  track 4  Car         frames 2, 3            (its box is 500 m from every point)
  track 5  Misc        frames 3, 4            (kept only by the `anything else` branch of the category filter)
  track -1 DontCare    every frame
In scene 0000 the velodyne file of frame 3 is MISSING and that of frame 4 is EMPTY.  The calib file has a `P0:` line (3x4), a
9-value `R_rect` line (skipped by the reader's rule) and `Tr_velo_cam`.
"""
import math
import os

import numpy as np

SCENES = ("0000", "0019")
FRAMES = 6
POINTS = 3000
MISSING = ("0000", 3)
EMPTY = ("0000", 4)
TRACKS = ((0, "Car", (0, 1, 2, 3, 4, 5)), (1, "Van", (0, 1, 2)), (2, "Pedestrian", (1, 2, 3, 4)), (3, "Car", (0, 1, 4, 5)),
          (4, "Car", (2, 3)), (5, "Misc", (3, 4)))
WLH = {"Car": (1.6, 3.9, 1.5), "Van": (1.9, 5.1, 2.2), "Pedestrian": (0.6, 0.8, 1.7), "Misc": (1.2, 2.0, 1.4)}


def velo_to_cam(scene):
    """a rigid transform close to KITTI's: camera x = -velodyne y, y = -z, z = x, turned by a small angle, plus a lever arm"""
    a = 0.01 + 0.002 * int(scene)
    base = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    turn = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return np.hstack([base @ turn, np.array([[-0.004], [-0.076], [-0.27]])])


def object_velo(track, frame):
    """centre of the object in velodyne coordinates"""
    if track == 4:
        return np.array([500.0 + frame, 20.0, -0.8])
    return np.array([8.0 + 4.0 * track + 0.6 * frame, -9.0 + 4.5 * track - 0.2 * frame, -0.9 + 0.05 * track])


def build(root, seed=0):
    """write the tree under `root` (created); -> root"""
    rng = np.random.default_rng(seed)
    for sub in ("label_02", "calib"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for scene in SCENES:
        os.makedirs(os.path.join(root, "velodyne", scene), exist_ok=True)
        T = velo_to_cam(scene)
        with open(os.path.join(root, "calib", scene + ".txt"), "w") as f:
            f.write("P0: " + " ".join("%.12e" % v for v in np.arange(12.0)) + "\n")
            f.write("R_rect " + " ".join("%.12e" % v for v in np.eye(3).reshape(-1)) + "\n")
            f.write("Tr_velo_cam " + " ".join("%.12e" % v for v in T.reshape(-1)) + "\n")
            f.write("Tr_imu_velo " + " ".join("%.12e" % v for v in np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(-1)) + "\n")
        lines = []
        for frame in range(FRAMES):
            lines.append("%d -1 DontCare -1 -1 -10.000000 %.6f %.6f %.6f %.6f -1000.000000 -1000.000000 -1000.000000 "
                         "-10.000000 -1.000000 -1.000000 -1.000000" % (frame, 10.0 + frame, 20.0, 50.0 + frame, 60.0))
            centres = []
            for track, kind, frames in TRACKS:
                if frame not in frames:
                    continue
                w, l, h = WLH[kind]
                c = object_velo(track, frame)
                if track != 4:                    # the far box stays empty: no point is drawn around it
                    centres.append(c)
                cam = T[:, :3] @ c + T[:, 3]
                ry = 0.35 * track - 0.07 * frame + 0.1 * int(scene)
                lines.append("%d %d %s 0 0 %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f"
                             % (frame, track, kind, -1.5 + 0.1 * track, 100.0, 150.0, 200.0, 250.0, h, w, l, cam[0], cam[1] + h / 2,
                                cam[2], ry))
            n_obj = 150 * len(centres)
            pts = np.empty((POINTS, 4), np.float32)
            pts[:POINTS - n_obj, :3] = rng.uniform([-40.0, -40.0, -2.5], [40.0, 40.0, 1.5], size=(POINTS - n_obj, 3))
            for i, c in enumerate(centres):
                pts[POINTS - n_obj + 150 * i:POINTS - n_obj + 150 * (i + 1), :3] = c + rng.normal(scale=(1.5, 1.0, 0.5), size=(150, 3))
            pts[:, 3] = rng.uniform(size=POINTS)
            pts = pts[rng.permutation(POINTS)]
            file = os.path.join(root, "velodyne", scene, "%06d.bin" % frame)
            if (scene, frame) == MISSING:
                continue
            if (scene, frame) == EMPTY:
                pts = pts[:0]
            pts.tofile(file)
        with open(os.path.join(root, "label_02", scene + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return root
