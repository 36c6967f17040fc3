"""Generate tests/golden/ref_train_batches.npz by running the REFERENCE'S OWN siamese_processing on synthetic sequences.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_train_batches.py
Reference code executed (read-only, from /root/reference, on the CPU): datasets/sampler.py (siamese_processing),
datasets/points_utils.py (getOffsetBB, getModel, cropAndCenterPC, crop_pc_axis_aligned, generate_subwindow, transform_box,
get_in_box_mask, regularize_pc, get_point_to_box_distance), datasets/searchspace.py (KalmanFiltering), datasets/data_classes.py
(PointCloud, Box).  Stubbed: easydict, nuscenes, pomegranate; pyquaternion is tests/golden/quat_standin.py.  Hooked, to record
what the reference drew under np.random.seed(s): getOffsetBB (the two offsets and the boxes it returns), cropAndCenterPC /
generate_subwindow (the crop counts), regularize_pc (the indices).  Inputs: open3dsot_amd/synth.py::make_sequence (no frame is
stored).

Cases (the keys of CASES below), each the candidates 0..3 of two annotations (frames (0, 2, 3)
and (0, 5, 6)) of one sequence:
  bat     cfgs/BAT_Car.yaml (degrees, data_limit_box False, box_aware), 8 frames of 20 000 points
  p2b     the same without BoxCloud
  sparse  BAT on 4 000-point frames: both clouds are shorter than their sample size (the with-replacement route)
plus `far`: one candidate of the bat sequence whose boxes are moved 500 m, for which the reference raises its
AssertionError -- that fact is stored.

Stored per sample: the numpy seed, the two offsets, the three crop counts, idx_t, idx_s, every output, and the mask near_face.
Conditions searched for (sequence seeds and numpy seeds, from 0 upwards) and ASSERTED:
  * crop margin, the rule of make_golden_tracking.py: for each of the three crops, every point of its frame lies more than
    1e-3 m (fp64) inside the crop region or more than 1e-3 m outside it (min over the crop's inequalities of
    `bound - |coordinate|` is > 1e-3 or < -1e-3; for the model crop over the world-frame and box-frame inequalities together);
  * near_face marks the search rows whose fp64 distance to a face plane of the transformed search box is below 1e-4 m (any
    face plane, whichever side of the others the point is on): at most 16 of the 1 024 rows of a sample.
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REF)
import fixture_io  # noqa: E402
import quat_standin  # noqa: E402
import tracking_oracle as TO  # noqa: E402
from open3dsot_amd import sampler as S, synth  # noqa: E402


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
dpkg.points_utils, dpkg.data_classes = PU, DC
dpkg.searchspace = load("datasets.searchspace", "datasets/searchspace.py")
SAMPLER = load("datasets.sampler", "datasets/sampler.py")

CASES = {"bat": (dict(S.DATA_KEYS), 20000), "p2b": (dict(S.DATA_KEYS, box_aware=False), 20000), "sparse": (dict(S.DATA_KEYS), 4000)}
FRAMES = 8
ANNOS = ((0, 2, 3), (0, 5, 6))


def box_of(b15):
    b = np.asarray(b15, np.float64)
    return DC.Box(b[0:3], b[3:6], quat_standin.Quaternion(matrix=b[6:15].reshape(3, 3)))


def vec_of(box):
    return np.concatenate([box.center, box.wlh, box.rotation_matrix.reshape(-1)]).astype(np.float64)


def margins(points, b15, scale, offset, mode):
    """fp64: per point, min over the crop's inequalities of (bound - |coordinate|): > 0 inside, < 0 outside"""
    b = np.asarray(b15, np.float64)
    d = points.astype(np.float64) - b[0:3]
    w, l, h = b[3:6]
    R = b[6:15].reshape(3, 3)
    m = (np.array([l, w, h]) * scale / 2 + offset - np.abs(d @ R)).min(1)
    if mode == TO.MODEL:
        e = np.abs(R) @ (np.array([l, w, h]) * 4 * scale / 2) + 2 * offset
        m = np.minimum(m, (e - np.abs(d)).min(1))
    return m


def face_distances(points, b15):
    """fp64: per point, the smallest distance to any of the six face planes of the box (whichever side of the others)"""
    b = np.asarray(b15, np.float64)
    q = (points.astype(np.float64) - b[0:3]) @ b[6:15].reshape(3, 3)
    w, l, h = b[3:6]
    return np.abs(np.array([l, w, h]) / 2 - np.abs(q)).min(1)


def run_reference(frames, gt, sample, cfg, np_seed):
    """the reference's siamese_processing on one sample under np.random.seed(np_seed) -> (its dict, what the hooks recorded)"""
    f0, f1, f2, cand = sample
    rec = {"offsets": [], "boxes": [], "model_counts": [], "idx": []}
    gob, cac, subw, reg = PU.getOffsetBB, PU.cropAndCenterPC, PU.generate_subwindow, PU.regularize_pc

    def rec_gob(box, offset, **k):
        rec["offsets"].append(np.array(offset, np.float64))
        r = gob(box, offset, **k)
        rec["boxes"].append(vec_of(r))
        return r

    def rec_cac(PC, box, **k):
        r = cac(PC, box, **k)
        rec["model_counts"].append(r[0].nbr_points())
        return r

    def rec_subw(pc, bb, **k):
        r = subw(pc, bb, **k)
        rec["search_count"] = r.nbr_points()
        return r

    def rec_reg(points, size, **k):
        p, idx = reg(points, size, **k)
        rec["idx"].append(None if idx is None else np.asarray(idx).astype(np.int32))
        rec.setdefault("raw", []).append(np.asarray(p, np.float64))
        return p, idx
    data = {"candidate_id": cand}
    for name, f in (("first_frame", f0), ("template_frame", f1), ("search_frame", f2)):
        data[name] = {"pc": DC.PointCloud(frames[f].T.copy()), "3d_bbox": box_of(gt[f])}
    PU.getOffsetBB, PU.cropAndCenterPC, PU.generate_subwindow, PU.regularize_pc = rec_gob, rec_cac, rec_subw, rec_reg
    try:
        np.random.seed(np_seed)
        out = SAMPLER.siamese_processing(data, EasyDict(cfg))
    finally:
        PU.getOffsetBB, PU.cropAndCenterPC, PU.generate_subwindow, PU.regularize_pc = gob, cac, subw, reg
    return out, rec


def conditions(frames, gt, sample, cfg, rec):
    """-> (ok, near_face (N,) bool, the worst crop margin)"""
    f0, f1, f2, _ = sample
    template_bb, sample_bb = rec["boxes"]
    worst = min(np.abs(margins(frames[f0], gt[f0], cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)).min(),
                np.abs(margins(frames[f1], template_bb, cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)).min(),
                np.abs(margins(frames[f2], sample_bb, cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)).min())
    search_box = vec_of(PU.transform_box(box_of(gt[f2]), box_of(sample_bb)))
    near = face_distances(rec["raw"][1], search_box) < 1e-4
    return bool(worst > 1e-3 and near.sum() <= 16), near, float(worst)


def run_case(case, seq_seed):
    cfg, n_points = CASES[case]
    frames, gt = synth.make_sequence(seq_seed, FRAMES, n_points)
    out = {}
    samples = [(f0, f1, f2, cand) for f0, f1, f2 in ANNOS for cand in range(cfg["num_candidates"])]
    for s, sample in enumerate(samples):
        found = False
        for np_seed in range(64):
            try:
                res, rec = run_reference(frames, gt, sample, cfg, np_seed)
            except AssertionError:
                continue
            ok, near, worst = conditions(frames, gt, sample, cfg, rec)
            if ok:
                found = True
                break
            if sample[3] == 0:
                break                         # candidate 0 draws nothing: another numpy seed changes nothing
        if not found:
            return {}, False, "sample %d: no numpy seed meets the conditions" % s
        k = "%s.s%d." % (case, s)
        out[k + "np_seed"] = np.int64(np_seed)
        out[k + "offset_t"], out[k + "offset_s"] = rec["offsets"]
        out[k + "counts"] = np.array(rec["model_counts"] + [rec["search_count"]], np.int32)
        out[k + "idx_t"], out[k + "idx_s"] = rec["idx"]
        for name, v in res.items():
            out[k + name] = np.asarray(v, np.float32)
        out[k + "near_face"] = np.packbits(near)
        out[k + "worst_margin"] = np.float64(worst)
        assert near.sum() <= 16 and worst > 1e-3
    out[case + ".samples"] = np.array(samples, np.int64)
    out[case + ".seq_seed"] = np.int64(seq_seed)
    out[case + ".n_points"] = np.int64(n_points)
    return out, True, ""


def far_candidate(seq_seed):
    """candidate 1 of annotation (0, 2, 3) of the bat sequence with every box moved 500 m: the reference's assertion fires"""
    cfg, n_points = CASES["bat"]
    frames, gt = synth.make_sequence(seq_seed, FRAMES, n_points)
    gt = gt.copy()
    gt[:, 0] += 500.0
    raised = False
    try:
        run_reference(frames, gt, (0, 2, 3, 1), cfg, 0)
    except AssertionError:
        raised = True
    assert raised
    return {"far.raises": np.bool_(raised), "far.shift": np.float32(500.0), "far.sample": np.array([0, 2, 3, 1], np.int64)}


def main():
    out = {}
    for case in CASES:
        for seed in range(0, 64):
            arrays, ok, why = run_case(case, seed)
            print("%s: sequence seed %d: %s" % (case, seed, "kept" if ok else why + " -> next seed"), flush=True)
            if ok:
                break
        assert ok, case
        out.update(arrays)
    out.update(far_candidate(int(out["bat.seq_seed"])))
    written = fixture_io.save(os.path.join(ROOT, "tests", "golden", "ref_train_batches.npz"), **out)
    print("wrote", [(os.path.basename(p), os.path.getsize(p)) for p in written], len(out), "arrays")


if __name__ == "__main__":
    main()
