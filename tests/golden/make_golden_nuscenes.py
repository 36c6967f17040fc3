"""Generate tests/golden/ref_nuscenes.npz by running the REFERENCE'S OWN NuScenesDataset on the tree of tests/nuscenes_tree.py.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_nuscenes.py
Reference code executed (read-only, from /root/reference, on the CPU): datasets/nuscenes_data.py (NuScenesDataset with
preloading: filter_instance, _build_tracklet_anno, _load_data, _get_frame_from_anno_data), datasets/base_dataset.py,
datasets/points_utils.py (crop_pc_axis_aligned), datasets/data_classes.py (PointCloud.rotate / translate, Box.corners).
Stubbed: easydict, pomegranate; pyquaternion is tests/golden/quat_standin.py and the devkit (`nuscenes`) is
tests/golden/nuscenes_standin.py, whose Box and LidarPointCloud are the classes of the reference's datasets/data_classes.py --
the fixture is pinned on the reference's code over those stand-ins, not over the devkit; scipy, torch and numpy are the
installed ones.  numpy must be >= 2: PointCloud.translate adds an np.float64 scalar to a float32 array, which numpy >= 2 does
in fp64 (rounded on assignment) and numpy < 2 in fp32 -- the fixture pins the first rule, asserted below.

Cases `<category>.<offset>.<split>.k<key_frame_only>.m<min_points>` (CASES): car, pedestrian, bus and truck (a class with no
instance); preload_offset 10 and -1; splits train and val; key_frame_only both ways; min_points 0, 1 and 5.
Stored per case: lengths (tracklet lengths), keys (the instance tokens, in order), files (the sweep's `filename` of every
tracklet frame, relative to the tree, concatenated), boxes (every box as its fp64 15-vector [centre | wlh | rotation
row-major]) and cloud_ids: the index of every tracklet frame's cloud among `cloud.<i>` ((n,3) float32, the reference's points
transposed; equal clouds are stored once).
ASSERTED: two runs on two freshly written trees give byte-identical arrays; the reference's tracking_to_general_class equals
datasets.NUSCENES_TRACKING_CLASSES; every uncropped cloud (offset -1) equals tests/nuscenes_oracle.py in float64 mode bit for
bit -- numpy's dot goes through BLAS, whose summation order is not ours, so this is a property of the tree's points, checked
here so that the GPU test may demand equality.  The tree's seed is 0: no point of it fails the assertion.
"""
import glob
import importlib.util
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
import nuscenes_oracle as NO  # noqa: E402
import nuscenes_standin  # noqa: E402
import nuscenes_tree  # noqa: E402
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


assert int(np.__version__.split(".")[0]) >= 2, "the fixture pins the translate rule of numpy >= 2"
stub("easydict", EasyDict=EasyDict)
stub("pomegranate", MultivariateGaussianDistribution=None, GeneralMixtureModel=None)
stub("pyquaternion", Quaternion=quat_standin.Quaternion)
dpkg = stub("datasets")
DC = load("datasets.data_classes", "datasets/data_classes.py")
LidarPointCloud, Box = nuscenes_standin.data_classes(DC)
nusc = stub("nuscenes")
nusc.nuscenes = stub("nuscenes.nuscenes", NuScenes=nuscenes_standin.NuScenes)
nusc.utils = stub("nuscenes.utils")
nusc.utils.geometry_utils = stub("nuscenes.utils.geometry_utils")
nusc.utils.data_classes = stub("nuscenes.utils.data_classes", LidarPointCloud=LidarPointCloud, Box=Box)
nusc.utils.splits = stub("nuscenes.utils.splits", create_splits_scenes=nuscenes_standin.splits(nuscenes_tree.SPLITS))
PU = load("datasets.points_utils", "datasets/points_utils.py")
BD = load("datasets.base_dataset", "datasets/base_dataset.py")
dpkg.points_utils, dpkg.data_classes, dpkg.base_dataset = PU, DC, BD
NUSC = load("datasets.nuscenes_data", "datasets/nuscenes_data.py")

# (category, preload_offset, split, key_frame_only, min_points)
CASES = [(c, o, "train", False, 0) for c in ("car", "pedestrian", "bus") for o in (10, -1)]
CASES += [("truck", 10, "train", False, 0), ("car", 10, "val", False, 0), ("car", -1, "val", False, 0), ("pedestrian", 10, "val", False, 0),
          ("car", 10, "train", True, 0), ("car", 10, "train", False, 1), ("car", 10, "train", False, 5), ("car", -1, "train", True, 5)]


def run(tree):
    from open3dsot_amd import datasets as D
    assert {k: list(v) for k, v in D.NUSCENES_TRACKING_CLASSES.items()} == NUSC.tracking_to_general_class
    assert list(D.NUSCENES_TRACKING_CLASSES) == list(NUSC.tracking_to_general_class)
    out, clouds = {}, {}
    for category, offset, split, key_only, min_points in CASES:
        # the reference's spelling of the class: any case (it lower-cases)
        ds = NUSC.NuScenesDataset(tree, split, category.capitalize(), version=nuscenes_tree.VERSION, preloading=True, preload_offset=offset,
                                  key_frame_only=key_only, min_points=min_points)
        for f in glob.glob(os.path.join(tree, "preload_nuscenes_*.dat")):      # its cache does not know key_frame_only: no reuse
            os.remove(f)
        lengths, keys, files, boxes, ids = [], [], [], [], []
        for k in range(ds.get_num_tracklets()):
            T = ds.get_num_frames_tracklet(k)
            got = ds.get_frames(k, list(range(T)))
            lengths.append(T)
            keys.append(ds.track_instances[k]["token"])
            for fr in got:
                sd = fr["meta"]["sample_data_lidar"]
                files.append(sd["filename"])
                bb = fr["3d_bbox"]
                boxes.append(np.concatenate([bb.center, bb.wlh, bb.rotation_matrix.reshape(-1)]).astype(np.float64))
                assert fr["pc"].points.dtype == np.float32 and fr["pc"].points.shape[0] == 3
                pts = np.ascontiguousarray(np.asarray(fr["pc"].points).T, dtype=np.float32)
                if offset <= 0:
                    cs = ds.nusc.get("calibrated_sensor", sd["calibrated_sensor_token"])
                    ego = ds.nusc.get("ego_pose", sd["ego_pose_token"])
                    steps = [np.hstack([quat_standin.Quaternion(r["rotation"]).rotation_matrix, np.array(r["translation"]).reshape(3, 1)])
                             for r in (cs, ego)]
                    want = NO.chain(NO.read_sweep(os.path.join(tree, sd["filename"])), steps, 0)
                    assert np.array_equal(want.view(np.int32), pts.view(np.int32)), (files[-1], "change the tree's seed")
                ids.append(clouds.setdefault((pts.shape[0], pts.tobytes()), len(clouds)))
        k = NO.case_name(category, offset, split, key_only, min_points) + "."
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
            runs.append(run(nuscenes_tree.build(os.path.join(d, "nuscenes"))))
    a, b = runs
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    written = fixture_io.save(os.path.join(ROOT, "tests", "golden", "ref_nuscenes.npz"), **a)
    print("wrote", [(os.path.basename(p), os.path.getsize(p)) for p in written], len(a), "arrays")


if __name__ == "__main__":
    main()
