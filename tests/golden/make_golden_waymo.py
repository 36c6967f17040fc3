"""Generate tests/golden/ref_waymo.npz by running the REFERENCE'S OWN WaymoDataset on the tree of tests/waymo_tree.py.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_waymo.py
Reference code executed (read-only, from /root/reference, on the CPU): datasets/waymo_data.py (WaymoDataset with preloading:
_build_tracklet_anno, _load_data, _get_frame_from_anno, veh_pos_to_transform), datasets/generate_waymo_sot.py
(generate_waymo_data, with the upper-case class as its __main__ calls it: it writes the tree's sot_infos files),
datasets/base_dataset.py, datasets/points_utils.py (crop_pc_axis_aligned), datasets/data_classes.py (PointCloud, Box).
Stubbed: easydict, nuscenes, pomegranate; pyquaternion is tests/golden/quat_standin.py -- the fixture is pinned on the
reference's code over that stand-in, not over pyquaternion; pandas, tqdm, torch and numpy are the installed ones.

Cases `<category>.<offset>.<split>`: VEHICLE | PEDESTRIAN | CYCLIST x preload_offset 10 | -1 on `train`, VEHICLE x 10 | -1 and
PEDESTRIAN x 10 on `val`, and `VEHICLE.10.val.tiny` (tiny=True: 100 of the 102 tracklets).
Stored per case: lengths (tracklet lengths), keys (the tracklet keys, in order), files (the 'PC' string of every tracklet
frame RELATIVE to the tree, concatenated), boxes (every box as its fp64 15-vector [centre | wlh | rotation row-major]) and
cloud_ids: the index of every tracklet frame's cloud among `cloud.<i>` ((n,3) float32, the reference's points transposed;
equal clouds are stored once).  `sot.<category>.<split>.keys / .lengths / .files / .boxes`: the sot_infos dicts that the
reference's generate_waymo_data wrote (the boxes as they lie in the file, before any swap).
ASSERTED: two runs on two freshly written trees give byte-identical arrays; every uncropped cloud (offset -1) equals the
ordered fp64 sum float32(((T_i0*x + T_i1*y) + T_i2*z) + T_i3) of tests/waymo_oracle.py bit for bit -- numpy's dot goes through
BLAS, whose summation order is not ours, so this is a property of the tree's points, checked here so that the GPU test may
demand equality.  The tree's seed is 0: no point of it fails the assertion.
"""
import importlib.util
import os
import pickle
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
import quat_standin  # noqa: E402
import waymo_tree  # noqa: E402


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
GEN = load("datasets.generate_waymo_sot", "datasets/generate_waymo_sot.py")
dpkg.points_utils, dpkg.data_classes, dpkg.base_dataset, dpkg.generate_waymo_sot = PU, DC, BD, GEN
WAYMO = load("datasets.waymo_data", "datasets/waymo_data.py")

CASES = [(c, o, "train", False) for c in waymo_tree.CLASSES for o in (10, -1)]
CASES += [("VEHICLE", 10, "val", False), ("VEHICLE", -1, "val", False), ("PEDESTRIAN", 10, "val", False), ("VEHICLE", 10, "val", True)]


def case_name(category, offset, split, tiny):
    return "%s.%d.%s" % (category, offset, split) + (".tiny" if tiny else "")


def run(tree):
    out, clouds = {}, {}
    rel = lambda f: os.path.relpath(f, tree)      # noqa: E731
    for split in ("train", "val"):
        for cls in waymo_tree.CLASSES:
            with open(os.path.join(tree, "sot_infos_%s_%s.pkl" % (cls.lower(), split)), "rb") as f:
                sot = pickle.load(f)
            k = "sot.%s.%s." % (cls, split)
            out[k + "keys"] = np.array(list(sot), dtype=np.str_)
            out[k + "lengths"] = np.array([len(v) for v in sot.values()], np.int64)
            out[k + "files"] = np.array([rel(a["PC"]) for v in sot.values() for a in v], dtype=np.str_)
            out[k + "boxes"] = np.array([a["Box"] for v in sot.values() for a in v], np.float32).reshape(-1, 9)
            assert all(a["Class"] == cls for v in sot.values() for a in v)
    for category, offset, split, tiny in CASES:
        ds = WAYMO.WaymoDataset(tree, split, category, preloading=True, preload_offset=offset, tiny=tiny)
        lengths, keys, files, boxes, ids = [], [], [], [], []
        with open(os.path.join(tree, "sot_infos_%s_%s.pkl" % (category.lower(), ds.split)), "rb") as f:
            names = list(pickle.load(f))
        for k in range(ds.get_num_tracklets()):
            T = ds.get_num_frames_tracklet(k)
            got = ds.get_frames(k, list(range(T)))
            lengths.append(T)
            keys.append(names[k])
            for fr in got:
                files.append(rel(fr["meta"]["PC"]))
                bb = fr["3d_bbox"]
                boxes.append(np.concatenate([bb.center, bb.wlh, bb.rotation_matrix.reshape(-1)]).astype(np.float64))
                pts = np.ascontiguousarray(np.asarray(fr["pc"].points).T, dtype=np.float32)
                assert pts.ndim == 2 and pts.shape[1] == 3 and fr["pc"].points.dtype == np.float32
                if offset <= 0:
                    with open(fr["meta"]["PC"], "rb") as f:
                        raw = pickle.load(f)["lidars"]["points_xyz"]
                    with open(fr["meta"]["PC"].replace("lidar", "annos"), "rb") as f:
                        pose = np.reshape(pickle.load(f)["veh_to_global"], [4, 4])
                    want = KO.transform(raw, WAYMO.WaymoDataset.veh_pos_to_transform(pose)[0][:3])
                    assert np.array_equal(want.view(np.int32), pts.view(np.int32)), (files[-1], "change the tree's seed")
                ids.append(clouds.setdefault((pts.shape[0], pts.tobytes()), len(clouds)))
        k = case_name(category, offset, split, tiny) + "."
        out[k + "lengths"] = np.array(lengths, np.int64)
        out[k + "keys"] = np.array(keys, dtype=np.str_)
        out[k + "files"] = np.array(files, dtype=np.str_)
        out[k + "boxes"] = np.array(boxes, np.float64).reshape(-1, 15)
        out[k + "cloud_ids"] = np.array(ids, np.int64)
    for (n, raw), i in clouds.items():
        out["cloud.%d" % i] = np.frombuffer(raw, np.float32).reshape(n, 3)
    return out


def main():
    runs = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            runs.append(run(waymo_tree.build(os.path.join(d, "waymo"), GEN.generate_waymo_data)))
    a, b = runs
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    written = fixture_io.save(os.path.join(ROOT, "tests", "golden", "ref_waymo.npz"), **a)
    print("wrote", [(os.path.basename(p), os.path.getsize(p)) for p in written], len(a), "arrays")


if __name__ == "__main__":
    main()
