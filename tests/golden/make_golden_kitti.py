"""Generate tests/golden/ref_kitti.npz by running the REFERENCE'S OWN kittiDataset on the tree of tests/kitti_tree.py.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_kitti.py
Reference code executed (read-only, from /root/reference, on the CPU): datasets/kitti.py (kittiDataset: _build_scene_list,
_build_tracklet_anno, _get_frame_from_anno, _read_calib_file), datasets/base_dataset.py, datasets/points_utils.py
(crop_pc_axis_aligned), datasets/data_classes.py (PointCloud, Box).  Stubbed: easydict, nuscenes, pomegranate; pyquaternion is
tests/golden/quat_standin.py; pandas and numpy are the installed ones.

Cases `<mode>.<offset>.<category>.<split>`: coordinate_mode velodyne | camera x preload_offset 10 | -1 x category Car | All |
Other (a name outside the reference's list: its `anything but DontCare` branch), all on `traintiny` (scene 0000, which holds
the missing and the empty velodyne file), and three of them on `testtiny` (scene 0019) as well.
Stored per case: lengths (tracklet lengths), frames (the frame numbers, concatenated), scenes / track_ids (per tracklet), boxes
(every box as its fp64 15-vector [centre | wlh | rotation row-major]) and cloud_ids: the index of every tracklet frame's cloud
among `cloud.<i>` ((n,3) float32, the reference's points transposed; equal clouds are stored once).  `scenes.<split string>`:
_build_scene_list of that string.
ASSERTED: two runs on two freshly written trees give byte-identical arrays; for the camera cases without crop, every cloud
equals the ordered fp64 sum float32(((T_i0*x + T_i1*y) + T_i2*z) + T_i3) of tests/kitti_oracle.py bit for bit, so the GPU
test may demand equality.
"""
import importlib.util
import itertools
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_io  # noqa: E402
import kitti_oracle as KO  # noqa: E402
import kitti_tree  # noqa: E402
import quat_standin  # noqa: E402


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class EasyDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


stub("easydict", EasyDict=EasyDict)
stub("nuscenes"); stub("nuscenes.utils", geometry_utils=None); stub("nuscenes.utils.geometry_utils")
stub("pomegranate", MultivariateGaussianDistribution=None, GeneralMixtureModel=None)
stub("pyquaternion", Quaternion=quat_standin.Quaternion)
dpkg = stub("datasets")
DC = load("datasets.data_classes", "datasets/data_classes.py")
PU = load("datasets.points_utils", "datasets/points_utils.py")
BD = load("datasets.base_dataset", "datasets/base_dataset.py")
dpkg.points_utils, dpkg.data_classes, dpkg.base_dataset = PU, DC, BD
KITTI = load("datasets.kitti", "datasets/kitti.py")

CASES = [(m, o, c, "traintiny") for m, o, c in itertools.product(("velodyne", "camera"), (10, -1), ("Car", "All", "Other"))]
CASES += [("velodyne", 10, "Car", "testtiny"), ("camera", 10, "All", "testtiny"), ("camera", -1, "Car", "testtiny")]
SPLITS = ("train", "traintiny", "TRAIN_tiny", "valid", "validtiny", "test", "testtiny", "tinytest", "trainval", "all", "", "tiny")


def case_name(mode, offset, category, split):
    return "%s.%d.%s.%s" % (mode, offset, category, split)


def run(tree):
    out, clouds = {}, {}
    for s in SPLITS:
        out["scenes." + s] = np.array(KITTI.kittiDataset._build_scene_list(s), dtype="U4")
    for mode, offset, category, split in CASES:
        ds = KITTI.kittiDataset(tree, split, category, coordinate_mode=mode, preload_offset=offset)
        lengths, frames, scenes, tracks, boxes, ids = [], [], [], [], [], []
        for k in range(ds.get_num_tracklets()):
            T = ds.get_num_frames_tracklet(k)
            got = ds.get_frames(k, list(range(T)))
            lengths.append(T)
            scenes.append(got[0]["meta"]["scene"])
            tracks.append(int(got[0]["meta"]["track_id"]))
            for fr in got:
                frames.append(int(fr["meta"]["frame"]))
                bb = fr["3d_bbox"]
                boxes.append(np.concatenate([bb.center, bb.wlh, bb.rotation_matrix.reshape(-1)]).astype(np.float64))
                pts = np.ascontiguousarray(np.asarray(fr["pc"].points).T, dtype=np.float32)
                assert pts.ndim == 2 and pts.shape[1] == 3
                if mode == "camera" and offset <= 0:
                    file = os.path.join(tree, "velodyne", scenes[-1], "%06d.bin" % frames[-1])
                    if os.path.exists(file):
                        raw = np.fromfile(file, np.float32).reshape(-1, 4)
                        want = KO.transform(raw, ds.calibs[scenes[-1]]["Tr_velo_cam"])
                        assert np.array_equal(want.view(np.int32), pts.view(np.int32)), (scenes[-1], frames[-1])
                ids.append(clouds.setdefault((pts.shape[0], pts.tobytes()), len(clouds)))
        k = case_name(mode, offset, category, split) + "."
        out[k + "lengths"] = np.array(lengths, np.int64)
        out[k + "frames"] = np.array(frames, np.int64)
        out[k + "scenes"] = np.array(scenes, dtype="U4")
        out[k + "track_ids"] = np.array(tracks, np.int64)
        out[k + "boxes"] = np.array(boxes, np.float64).reshape(-1, 15)
        out[k + "cloud_ids"] = np.array(ids, np.int64)
    for (n, raw), i in clouds.items():
        out["cloud.%d" % i] = np.frombuffer(raw, np.float32).reshape(n, 3)
    return out


def main():
    runs = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            runs.append(run(kitti_tree.build(os.path.join(d, "kitti"))))
    a, b = runs
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    written = fixture_io.save(os.path.join(ROOT, "tests", "golden", "ref_kitti.npz"), **a)
    print("wrote", [(os.path.basename(p), os.path.getsize(p)) for p in written], len(a), "arrays")


if __name__ == "__main__":
    main()
