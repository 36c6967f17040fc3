"""Generate tests/golden/ref_tracking.npz by running the REFERENCE'S OWN tracking loop on synthetic sequences.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_tracking.py
Reference code executed (read-only, from /root/reference): datasets/points_utils.py (generate_subwindow, cropAndCenterPC,
getModel, crop_pc_axis_aligned, regularize_pc, get_point_to_box_distance, getOffsetBB), datasets/data_classes.py (PointCloud,
Box), models/base_model.py (MatchingBaseModel.evaluate_one_sequence / build_input_dict / generate_template /
generate_search_area / prepare_input, BaseModel.evaluate_one_sample), models/bat.py (BAT.prepare_input, forward),
models/p2b.py and what they construct -- on the CPU over oracle/ext_shim.py, weights from tests/golden/det_init.py, as
make_golden_trackers.py does.  Stubbed: pytorch_lightning, easydict, nuscenes; utils.metrics (estimateOverlap /
estimateAccuracy return constants: shapely is absent and the metrics are not pinned); pyquaternion is
tests/golden/quat_standin.py.  Inputs: open3dsot_amd/synth.py::make_sequence (no frame is stored).

Stored per case of tests/tracking_oracle.py::CASES (8 frames of 20 000 points), per frame t = 1..7: the reference box, the
crop counts (search, template cloud, the model crops made), the regularised template / search clouds, the template BoxCloud
(BAT), the (64,5) proposals, the chosen offset and the result box.  Plus one 120 000-point frame as its two reference masks,
bit-packed.

Conditions searched for (sequence seeds, from 0 upwards) and ASSERTED, so that fp32 can change neither a mask nor an argmax
on these inputs:
  * crop margin: for every crop of the run, every point lies more than 1e-3 m (fp64) inside the crop region or more than
    1e-3 m outside it, measured against the crop's planes (min over the inequalities of `bound - |coordinate|` is > 1e-3 or
    < -1e-3; for the model crop over the world-frame and the box-frame inequalities together);
  * the two highest objectness scores differ by more than 1e-3 at every frame.
Full-size frame: at most 8 points per crop within 1e-4 m of the crop boundary (they are left out of the comparison).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch.Tensor.cuda = lambda self, *a, **k: self
from oracle import ext_shim  # noqa: E402

ext_shim.install()
sys.path.insert(0, REF)
import det_init  # noqa: E402
import fixture_io  # noqa: E402
import quat_standin  # noqa: E402
import tracking_oracle as TO  # noqa: E402
from open3dsot_amd import synth  # noqa: E402


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


class _Dummy:
    def __init__(self, *a, **k):
        pass


class EasyDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class LightningModule(torch.nn.Module):
    global_step = 0
    device = torch.device("cpu")

    def save_hyperparameters(self, *a, **k):
        pass

    def log(self, *a, **k):
        pass


stub("pytorch_lightning", LightningModule=LightningModule)
stub("easydict", EasyDict=EasyDict)
stub("nuscenes"); stub("nuscenes.utils", geometry_utils=None); stub("nuscenes.utils.geometry_utils")
stub("pyquaternion", Quaternion=quat_standin.Quaternion)
stub("utils"); stub("utils.metrics", TorchSuccess=_Dummy, TorchPrecision=_Dummy, estimateOverlap=lambda *a, **k: 0.0,
                    estimateAccuracy=lambda *a, **k: 0.0)
dpkg = stub("datasets")
DC = load("datasets.data_classes", "datasets/data_classes.py")
PU = load("datasets.points_utils", "datasets/points_utils.py")
dpkg.points_utils, dpkg.data_classes = PU, DC
pkg = stub("models"); stub("models.backbone"); stub("models.head")
load("models.backbone.pointnet", "models/backbone/pointnet.py")
load("models.head.xcorr", "models/head/xcorr.py")
load("models.head.rpn", "models/head/rpn.py")
pkg.base_model = load("models.base_model", "models/base_model.py")
REF_MODEL = {"BAT": load("models.bat", "models/bat.py").BAT, "P2B": load("models.p2b", "models/p2b.py").P2B}

# ---- recording hooks on the reference's own functions ----------------------------------------------------------------------
REC = {"masks": []}
_crop_aa = PU.crop_pc_axis_aligned


def _rec_crop_aa(PC, box, offset=0, scale=1.0, return_mask=False):
    new_pc, close = _crop_aa(PC, box, offset=offset, scale=scale, return_mask=True)
    REC["masks"].append(close.copy())
    return (new_pc, close) if return_mask else new_pc


PU.crop_pc_axis_aligned = _rec_crop_aa


def ref_subwindow_mask(points, box, scale, offset):
    """the reference's generate_subwindow on (n,3) float32 points -> (its mask over the input, its output points (3,k))"""
    REC["masks"] = []
    out = PU.generate_subwindow(DC.PointCloud(points.T.copy()), box, scale=scale, offset=offset)
    (m,) = REC["masks"]
    return m, out.points


def ref_model_mask(points, box, scale, offset):
    """the reference's cropAndCenterPC -> (its mask over the input: the world-frame crop, then the box-frame crop of the
    survivors; its output points)"""
    REC["masks"] = []
    out, _ = PU.cropAndCenterPC(DC.PointCloud(points.T.copy()), box, offset=offset, scale=scale)
    m1, m2 = REC["masks"]
    m = np.zeros(points.shape[0], bool)
    m[np.flatnonzero(m1)[m2]] = True
    return m, out.points


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
    q = d @ R
    m = (np.array([l, w, h]) * scale / 2 + offset - np.abs(q)).min(1)
    if mode == TO.MODEL:
        e = np.abs(R) @ (np.array([l, w, h]) * 4 * scale / 2) + 2 * offset
        m = np.minimum(m, (e - np.abs(d)).min(1))
    return m


class Reject(Exception):
    """a generator condition failed: the run is abandoned and the next sequence seed tried"""


def run_case(case, seq_seed):
    """-> (arrays, ok): the reference run of one case on make_sequence(seq_seed); ok = the generator conditions hold"""
    name, cfg = TO.case_config(case)
    frames, gt = synth.make_sequence(seq_seed, TO.SEQ_FRAMES, TO.SEQ_POINTS)
    torch.manual_seed(0)
    # models/base_model.py:186 reads `config.hape_aggregation` (sic) on the way to its `previous` and `all` branches: without
    # that key both raise.  Giving the key the value of shape_aggregation lets the reference reach the branch it names.
    model = REF_MODEL[name](EasyDict(dict(cfg, hape_aggregation=cfg["shape_aggregation"])))
    # det_init's non-degenerate variant (under the cos/sin waves of fill_state_dict the 64 objectness scores agree to ~1e-7,
    # which no margin condition can separate), its box-moving rows scaled: tests/tracking_oracle.py::init_weights
    TO.init_weights(model)
    model.eval()
    sequence = [{"pc": DC.PointCloud(f.T.copy()), "3d_bbox": box_of(gt[t])} for t, f in enumerate(frames)]
    per = []
    cur = {}
    bid, fwd, prep, gob = model.build_input_dict, model.forward, model.prepare_input, PU.getOffsetBB
    subw, cac = PU.generate_subwindow, PU.cropAndCenterPC

    def rec_subw(pc, bb, scale, offset=2, oriented=True):
        r = subw(pc, bb, scale, offset=offset, oriented=oriented)
        cur["search_crop"] = (vec_of(bb), r.nbr_points())
        if np.abs(margins(frames[pc_frame[id(pc)]], vec_of(bb), scale, offset, TO.SUBWINDOW)).min() <= 1e-3:
            raise Reject("search crop margin, frame %d" % pc_frame[id(pc)])
        return r

    def rec_cac(PC, box, offset=0, scale=1.0, normalize=False):
        r = cac(PC, box, offset=offset, scale=scale, normalize=normalize)
        cur.setdefault("model_crops", []).append((id(PC), vec_of(box), r[0].nbr_points()))
        if np.abs(margins(frames[pc_frame[id(PC)]], vec_of(box), scale, offset, TO.MODEL)).min() <= 1e-3:
            raise Reject("model crop margin, frame %d" % pc_frame[id(PC)])
        return r

    def rec_prep(template_pc, search_pc, template_box, *a, **k):
        cur["n_template"], cur["n_search"] = template_pc.nbr_points(), search_pc.nbr_points()
        cur["canon"] = vec_of(template_box)
        return prep(template_pc, search_pc, template_box, *a, **k)

    def rec_bid(seq, frame_id, results_bbs, **k):
        cur.clear()
        data, ref_bb = bid(seq, frame_id, results_bbs, **k)
        cur["data"] = {kk: v.numpy().copy() for kk, v in data.items()}
        cur["ref"] = vec_of(ref_bb)
        return data, ref_bb

    def rec_fwd(d):
        r = fwd(d)
        cur["boxes"] = r["estimation_boxes"].detach().numpy().copy()[0]
        top = np.sort(cur["boxes"][:, 4])
        if top[-1] - top[-2] <= 1e-3:
            raise Reject("objectness gap %.2e" % (top[-1] - top[-2]))
        return r

    def rec_gob(box, offset, **k):
        cur["offset"] = np.asarray(offset, np.float32).copy()
        r = gob(box, offset, **k)
        cur["result"] = vec_of(r)
        per.append(dict(cur))
        return r
    model.build_input_dict, model.forward, model.prepare_input = rec_bid, rec_fwd, rec_prep
    PU.getOffsetBB, PU.generate_subwindow, PU.cropAndCenterPC = rec_gob, rec_subw, rec_cac
    pc_frame = {id(s["pc"]): t for t, s in enumerate(sequence)}
    try:
        with torch.no_grad():
            _, _, results = model.evaluate_one_sequence(sequence)
    except Reject as e:
        return {}, False, str(e), ""
    finally:
        PU.getOffsetBB, PU.generate_subwindow, PU.cropAndCenterPC = gob, subw, cac
    assert len(per) == TO.SEQ_FRAMES - 1
    ok, worst_margin, worst_gap = True, np.inf, np.inf
    out = {}
    for t, c in enumerate(per, start=1):
        b, n = c["search_crop"]
        m = margins(frames[t], b, cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)
        assert int((m > 0).sum()) == n, (case, t, "fp64 restatement of the search crop disagrees with the reference")
        worst_margin = min(worst_margin, np.abs(m).min())
        mc = []
        for pid, b, n in c["model_crops"]:
            m = margins(frames[pc_frame[pid]], b, cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)
            assert int((m > 0).sum()) == n, (case, t, "fp64 restatement of the model crop disagrees with the reference")
            worst_margin = min(worst_margin, np.abs(m).min())
            mc.append(n)
        s = np.sort(c["boxes"][:, 4])
        worst_gap = min(worst_gap, float(s[-1] - s[-2]))
        k = "%s.f%d." % (case, t)
        out[k + "ref_box"], out[k + "result_box"] = c["ref"], c["result"]
        out[k + "counts"] = np.array([c["n_search"], c["n_template"]], np.int64)
        out[k + "model_crop_counts"] = np.array(mc, np.int64)
        out[k + "template_points"] = c["data"]["template_points"][0]
        out[k + "search_points"] = c["data"]["search_points"][0]
        if "points2cc_dist_t" in c["data"]:
            out[k + "points2cc_dist_t"] = c["data"]["points2cc_dist_t"][0]
        out[k + "proposals"] = c["boxes"]
        out[k + "offset"] = c["offset"]
        out[k + "canonical_wlh"] = c["canon"][3:6]
    ok = worst_margin > 1e-3 and worst_gap > 1e-3
    out[case + ".seq_seed"] = np.int64(seq_seed)
    out[case + ".worst_margin"], out[case + ".worst_gap"] = np.float64(worst_margin), np.float64(worst_gap)
    return out, ok, worst_margin, worst_gap


def full_frame():
    """one 120 000-point frame: the reference's two masks, bit-packed, for the box of the frame"""
    for seed in range(100, 200):
        frames, gt = synth.make_sequence(seed, 1, TO.FULL_POINTS)
        box = box_of(gt[0])
        k = TO.TEST_KEYS
        ms, _ = ref_subwindow_mask(frames[0], box, k["search_bb_scale"], k["search_bb_offset"])
        mm, _ = ref_model_mask(frames[0], box, k["model_bb_scale"], k["model_bb_offset"])
        near_s = np.abs(margins(frames[0], vec_of(box), k["search_bb_scale"], k["search_bb_offset"], TO.SUBWINDOW)) <= 1e-4
        near_m = np.abs(margins(frames[0], vec_of(box), k["model_bb_scale"], k["model_bb_offset"], TO.MODEL)) <= 1e-4
        if near_s.sum() <= 8 and near_m.sum() <= 8:
            break
    assert near_s.sum() <= 8 and near_m.sum() <= 8
    print("full frame: seed %d, %d / %d points kept, %d / %d within 1e-4 m of the boundary" %
          (seed, ms.sum(), mm.sum(), near_s.sum(), near_m.sum()))
    return {"full.seq_seed": np.int64(seed), "full.n": np.int64(frames[0].shape[0]),
            "full.search_mask": np.packbits(ms), "full.model_mask": np.packbits(mm),
            "full.search_near": np.flatnonzero(near_s).astype(np.int64), "full.model_near": np.flatnonzero(near_m).astype(np.int64)}


def main():
    out = {}
    for case in TO.CASES:
        for seed in range(0, 256):
            arrays, ok, wm, wg = run_case(case, seed)
            print("%s: sequence seed %d:" % (case, seed), ("worst crop margin %.3e m, worst objectness gap %.3e -> kept" % (wm, wg))
                  if ok else "%s -> next seed" % wm, flush=True)
            if ok:
                break
        assert ok, case
        assert arrays[case + ".worst_margin"] > 1e-3 and arrays[case + ".worst_gap"] > 1e-3
        out.update(arrays)
    out.update(full_frame())
    written = fixture_io.save(os.path.join(ROOT, "tests", "golden", "ref_tracking.npz"), **out)
    print("wrote", [os.path.basename(p) for p in written], len(out), "arrays")


if __name__ == "__main__":
    main()
