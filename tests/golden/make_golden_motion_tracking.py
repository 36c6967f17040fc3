"""Generate tests/golden/ref_motion_tracking.npz by running the REFERENCE'S OWN motion-tracker frame loop on synthetic
sequences.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_motion_tracking.py
Reference code executed (read-only, from /root/reference): models/base_model.py (BaseModel.evaluate_one_sequence /
evaluate_one_sample, MotionBaseModel.build_input_dict), models/m2track.py (M2TRACK.forward), models/backbone/pointnet.py,
datasets/points_utils.py (generate_subwindow, transform_box, regularize_pc, get_point_to_box_distance, getOffsetBB and the
tensor box helpers), datasets/data_classes.py -- on the CPU, with the stubs of make_golden_tracking.py (imported for them; its
main() is not run, so ref_tracking.npz stays as it is) plus torchmetrics (Accuracy: never called at inference) and
nuscenes.utils.geometry_utils.points_in_box = tests/golden/points_in_box_standin.py.  Weights:
tests/motion_oracle.py::init_weights.  Inputs: open3dsot_amd/synth.py::make_sequence, 8 frames of 20 000 points (no frame is
stored).

Stored per case of tests/motion_oracle.py::CASES (the KITTI config; box_aware=False), per frame t = 1..7: the reference box,
the two crop counts (previous frame, current frame), `points` (2048,5), the first half of `candidate_bc` (1024,9; the second
half is zeros, asserted), `estimation_boxes` (4,), the result box, the segmentation hard mask (bit-packed) with its per-point
logit margin |l1 - l0|, the motion-state decision with its margin.  Per case: the number of segmentation decisions whose
margin is <= 2e-3 (`near_ties`).

Conditions searched for (sequence seeds, from 0 upwards) and ASSERTED:
  * crop planes: every point of both frames of every crop lies more than 1e-3 m (fp64) inside or outside the crop region,
    measured against the crop's planes (make_golden_tracking.py::margins);
  * prior-box faces: every resampled previous-frame row lies more than 1e-3 m inside or outside the 1.25-scaled canonical
    box, measured the same way (min over the axes of `half extent - |coordinate|`);
  * every crop holds at least 3 points;
  * the motion-state margin is above 2e-3 at every frame;
  * non-degeneracy: the segmentation mask holds both classes in at least 4 of the 7 frames, and the seven estimation_boxes
    differ pairwise by more than 1e-4 in some component (an untrained head is easily all foreground or all background:
    tests/motion_oracle.py::init_weights); the per-frame foreground counts are stored (`<case>.foreground_points`);
  * at most 32 of the 7 x 2048 = 14 336 segmentation decisions of a case have a margin of 2e-3 or less (the TIE of
    tests/test_golden_m2track.py::replay_hard_masks; ref_m2track_grad.npz shows a rate of 9e-4 at that margin: ~13 expected).

Three input-only cases (tests/motion_oracle.py::INPUT_CASES: a previous window of 2 points -> zero fill; windows with fewer
points than the sample size -> a draw with replacement; windows with exactly the sample size -> arange) go through the
reference's build_input_dict alone, at point_sample_size 256: `points`, the first half of `candidate_bc`, the counts.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_tracking as base  # noqa: E402  (installs the stubs, loads the reference modules; does not run main())
import points_in_box_standin  # noqa: E402
import motion_oracle as MO  # noqa: E402
from open3dsot_amd import synth  # noqa: E402

fixture_io, TO, PU, DC = base.fixture_io, base.TO, base.PU, base.DC
geo = sys.modules["nuscenes.utils.geometry_utils"]
geo.points_in_box = points_in_box_standin.points_in_box
sys.modules["nuscenes.utils"].geometry_utils = geo
base.pkg.base_model.geometry_utils = geo
base.stub("torchmetrics", Accuracy=base._Dummy)
MAX_SEEDS, CHUNK, WORKERS = 8192, 128, 8
REF_M2 = base.load("models.m2track", "models/m2track.py").M2TRACK


_MODELS = {}


def reference_model(cfg):
    """the reference's M2TRACK with the fixture's weights, in eval mode (one per configuration: the weights are storage-free)"""
    key = repr(sorted(cfg.items()))
    if key not in _MODELS:
        torch.manual_seed(0)
        _MODELS[key] = MO.init_weights(REF_M2(base.EasyDict(cfg))).eval()
    return _MODELS[key]


def prior_margin(points, wlh):
    """fp64: the rows' margins against the faces of the canonical box scaled by 1.25"""
    w, l, h = np.asarray(wlh, np.float64)
    return MO.box_margin(points[:, :3], np.array([l, w, h]) * 1.25 / 2)


class Tape:
    """records the two torch.argmax decisions of a forward with the margin |l1 - l0| of their logits"""

    def __enter__(self):
        self.real, self.rows = torch.argmax, []
        torch.argmax = self._rec
        return self

    def _rec(self, x, *a, **k):
        r = self.real(x, *a, **k)
        self.rows.append((r.numpy().copy(), (x.detach().select(1, 1) - x.detach().select(1, 0)).abs().numpy().copy()))
        return r

    def __exit__(self, *exc):
        torch.argmax = self.real
        return False


def run_case(case, seq_seed):
    """-> (arrays, reason | None): the reference run of one case on make_sequence(seq_seed); reason: the condition that failed"""
    cfg = MO.case_config(case)
    N = cfg["point_sample_size"]
    frames, gt = synth.make_sequence(seq_seed, MO.SEQ_FRAMES, MO.SEQ_POINTS)
    model = reference_model(cfg)
    sequence = [{"pc": DC.PointCloud(f.T.copy()), "3d_bbox": base.box_of(gt[t])} for t, f in enumerate(frames)]
    pc_frame = {id(s["pc"]): t for t, s in enumerate(sequence)}
    per, cur = [], {}
    bid, fwd, gob, subw = model.build_input_dict, model.forward, PU.getOffsetBB, PU.generate_subwindow

    def rec_subw(pc, bb, scale, offset=2, oriented=True):
        r = subw(pc, bb, scale, offset=offset, oriented=oriented)
        m = base.margins(frames[pc_frame[id(pc)]], base.vec_of(bb), scale, offset, TO.SUBWINDOW)
        if np.abs(m).min() <= 1e-3:
            raise base.Reject("crop plane margin %.2e, frame %d" % (np.abs(m).min(), pc_frame[id(pc)]))
        assert int((m > 0).sum()) == r.nbr_points(), "fp64 restatement of the crop disagrees with the reference"
        if r.nbr_points() < 3:
            raise base.Reject("a crop of %d points" % r.nbr_points())
        cur.setdefault("counts", []).append(r.nbr_points())
        cur["crop_margin"] = min(cur.get("crop_margin", np.inf), float(np.abs(m).min()))
        return r

    def rec_bid(seq, frame_id, results_bbs):
        cur.clear()
        data, ref_bb = bid(seq, frame_id, results_bbs)
        cur["data"] = {k: v.numpy().copy() for k, v in data.items()}
        cur["ref"] = base.vec_of(ref_bb)
        pm = np.abs(prior_margin(cur["data"]["points"][0, :N].astype(np.float64), cur["ref"][3:6])).min()
        if pm <= 1e-3:
            raise base.Reject("prior-box face margin %.2e" % pm)
        cur["prior_margin"] = float(pm)
        return data, ref_bb

    def rec_fwd(d):
        with Tape() as tape:
            r = fwd(d)
        (seg, seg_m), (mot, mot_m) = tape.rows
        assert seg.shape == (1, 1, 2 * N) and mot.shape == (1, 1)
        cur["seg"], cur["seg_margin"] = seg.reshape(-1).astype(np.uint8), seg_m.reshape(-1).astype(np.float32)
        cur["motion"], cur["motion_margin"] = np.int8(mot.reshape(-1)[0]), np.float32(mot_m.reshape(-1)[0])
        if cur["motion_margin"] <= MO.TIE:
            raise base.Reject("motion-state margin %.2e" % cur["motion_margin"])
        cur["est"] = r["estimation_boxes"].detach().numpy().copy()[0]
        return r

    def rec_gob(box, offset, **k):
        r = gob(box, offset, **k)
        cur["result"] = base.vec_of(r)
        per.append(dict(cur))
        return r
    model.build_input_dict, model.forward = rec_bid, rec_fwd
    PU.getOffsetBB, PU.generate_subwindow = rec_gob, rec_subw
    try:
        with torch.no_grad():
            model.evaluate_one_sequence(sequence)
    except base.Reject as e:
        return {}, str(e)
    finally:
        PU.getOffsetBB, PU.generate_subwindow = gob, subw
        del model.build_input_dict, model.forward          # the instance attributes: the class's methods are back
    assert len(per) == MO.SEQ_FRAMES - 1
    out, near = {}, 0
    for t, c in enumerate(per, start=1):
        k = "%s.f%d." % (case, t)
        out[k + "ref_box"], out[k + "result_box"] = c["ref"], c["result"]
        out[k + "counts"] = np.array(c["counts"], np.int64)
        out[k + "points"] = c["data"]["points"][0]
        if "candidate_bc" in c["data"]:
            bc = c["data"]["candidate_bc"]
            bc = bc[0] if bc.ndim == 3 else bc
            assert bc.shape == (2 * N, 9) and not bc[N:].any()
            out[k + "candidate_bc_prev"] = bc[:N]
        out[k + "estimation_boxes"] = c["est"]
        out[k + "seg_mask"], out[k + "seg_margin"] = np.packbits(c["seg"]), c["seg_margin"]
        out[k + "motion_state"], out[k + "motion_margin"] = c["motion"], c["motion_margin"]
        near += int((c["seg_margin"] <= MO.TIE).sum())
    if near > MO.MAX_NEAR_TIES:
        return {}, "%d near ties" % near
    out[case + ".seq_seed"], out[case + ".near_ties"] = np.int64(seq_seed), np.int64(near)
    ones = np.array([int(c["seg"].sum()) for c in per], np.int64)                                 # of 2048, per frame
    mixed = int(((ones > 0) & (ones < 2 * N)).sum())
    if mixed < MO.MIXED_FRAMES:
        return {}, "both classes in %d frames only (foreground %s)" % (mixed, ones.tolist())
    ests = np.stack([c["est"] for c in per])
    apart = min(float(np.abs(ests[i] - ests[j]).max()) for i in range(len(per)) for j in range(i))
    if apart <= 1e-4:
        return {}, "two frames with the same estimation_boxes"
    out[case + ".foreground_points"], out[case + ".mixed_frames"] = ones, np.int64(mixed)
    out[case + ".estimation_apart"] = np.float64(apart)
    print("   foreground points per frame:", ones.tolist())
    out[case + ".worst_crop_margin"] = np.float64(min(c["crop_margin"] for c in per))
    out[case + ".worst_prior_margin"] = np.float64(min(c["prior_margin"] for c in per))
    out[case + ".worst_motion_margin"] = np.float64(min(float(c["motion_margin"]) for c in per))
    moves = [np.abs(c["est"]).tolist() for c in per]
    print("   |estimation_boxes| per frame:", " ".join("(%.2f %.2f %.2f %.3f)" % tuple(m) for m in moves))
    print("   counts:", [c["counts"] for c in per])
    return out, None


def input_cases():
    out = {}
    cfg = dict(MO.case_config("kitti"), point_sample_size=MO.INPUT_N)
    model = reference_model(cfg)
    for name, (n_prev, n_this, frame_id) in MO.INPUT_CASES.items():
        prev, this, box = MO.input_case_frames(name)
        b = base.box_of(box)
        sequence = [None] * (frame_id - 1) + [{"pc": DC.PointCloud(prev.T.copy()), "3d_bbox": b},
                                              {"pc": DC.PointCloud(this.T.copy()), "3d_bbox": b}]
        counts = []
        subw = PU.generate_subwindow

        def rec_subw(pc, bb, scale, offset=2, oriented=True):
            r = subw(pc, bb, scale, offset=offset, oriented=oriented)
            counts.append(r.nbr_points())
            return r
        PU.generate_subwindow = rec_subw
        try:
            data, _ = model.build_input_dict(sequence, frame_id, [b] * frame_id)
        finally:
            PU.generate_subwindow = subw
        assert counts == [n_prev, n_this], (name, counts)
        pts = data["points"].numpy()[0]
        assert np.abs(prior_margin(pts[:MO.INPUT_N].astype(np.float64), box[3:6])).min() > 1e-3 or n_prev <= 2
        bc = data["candidate_bc"].numpy()
        bc = bc[0] if bc.ndim == 3 else bc
        assert not bc[MO.INPUT_N:].any()
        k = "in.%s." % name
        out[k + "counts"], out[k + "points"], out[k + "candidate_bc_prev"] = np.array(counts, np.int64), pts, bc[:MO.INPUT_N]
        print("input case %s: counts %s, frame_id %d, mask values %s" % (name, counts, frame_id, np.unique(pts[:MO.INPUT_N, 4])))
    return out


def _try(args):
    torch.set_num_threads(1)
    return (args[1],) + run_case(*args)


def main():
    import multiprocessing
    out = {}
    pool = multiprocessing.get_context("fork").Pool(WORKERS)
    for case in MO.CASES:
        why = "no seed tried"
        for first in range(0, MAX_SEEDS, CHUNK):             # in order: the smallest seed that passes, however many workers
            for seed, arrays, why in pool.map(_try, [(case, s) for s in range(first, first + CHUNK)]):
                print("%s: sequence seed %d: %s" % (case, seed, "kept" if why is None else why + " -> next seed"), flush=True)
                if why is None:
                    break
            if why is None:
                break
        assert why is None, case
        assert arrays[case + ".mixed_frames"] >= MO.MIXED_FRAMES and arrays[case + ".estimation_apart"] > 1e-4
        assert arrays[case + ".worst_crop_margin"] > 1e-3 and arrays[case + ".worst_prior_margin"] > 1e-3
        assert arrays[case + ".worst_motion_margin"] > MO.TIE and arrays[case + ".near_ties"] <= MO.MAX_NEAR_TIES
        print("%s: %d near ties, worst margins: crop %.2e prior %.2e motion %.2e" % (
            case, arrays[case + ".near_ties"], arrays[case + ".worst_crop_margin"], arrays[case + ".worst_prior_margin"],
            arrays[case + ".worst_motion_margin"]))
        out.update(arrays)
    pool.close()
    out.update(input_cases())
    written = fixture_io.save(os.path.join(HERE, "ref_motion_tracking.npz"), **out)
    print("wrote", [os.path.basename(p) for p in written], len(out), "arrays")


if __name__ == "__main__":
    main()
