"""Generate tests/golden/ref_multi_tracking.npz: the REFERENCE'S OWN tracking loop, once per target, on the shared frames
of a scene with several targets.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_multi_tracking.py
The reference code executed, the stubs and the recording hooks are those of make_golden_tracking.py (imported, not
restated: importing that module installs them).  Inputs: open3dsot_amd/synth.py::make_scene(seed, 6, 20 000, 3) -- three
targets in frames of 60 000 points; no frame is stored.  Model: the `bat_fap` case of tests/tracking_oracle.py (BAT,
shape_aggregation firstandprevious) with tracking_oracle.init_weights.  The reference's evaluate_one_sequence runs once per
target over the same frames, with that target's box in frame 0.

Stored per target k and frame t = 1..5 under "t<k>.f<t>.": what ref_tracking.npz stores per frame (reference box, crop
counts, regularised clouds, BoxCloud, proposals, chosen offset, result box); per target "t<k>.worst_margin" and
"t<k>.worst_gap"; "scene_seed", "n_targets", "n_frames", "n_points".

Conditions searched for (scene seeds, from 0 upwards) and ASSERTED for every target and frame, as in make_golden_tracking.py:
  * every point lies more than 1e-3 m (fp64) from every plane of every crop of the run;
  * the two highest objectness scores differ by more than 1e-3.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_tracking as G  # noqa: E402  (installs the stubs, loads the reference's modules)

TO, PU, DC, synth, fixture_io = G.TO, G.PU, G.DC, G.synth, G.fixture_io
CASE, N_TARGETS, N_FRAMES, N_POINTS = "bat_fap", 3, 6, 20000


def run_target(frames, gt, cfg, name):
    """The reference run for one target (gt (T,15): its boxes; only gt[0] steers the run) on the shared frames ->
    (per-frame records, reject reason | None); the hooks of make_golden_tracking.run_case, on given frames."""
    torch.manual_seed(0)
    model = G.REF_MODEL[name](G.EasyDict(dict(cfg, hape_aggregation=cfg["shape_aggregation"])))
    TO.init_weights(model)
    model.eval()
    sequence = [{"pc": DC.PointCloud(f.T.copy()), "3d_bbox": G.box_of(gt[t])} for t, f in enumerate(frames)]
    pc_frame = {id(s["pc"]): t for t, s in enumerate(sequence)}
    per, cur = [], {}
    bid, fwd, prep, gob = model.build_input_dict, model.forward, model.prepare_input, PU.getOffsetBB
    subw, cac = PU.generate_subwindow, PU.cropAndCenterPC

    def rec_subw(pc, bb, scale, offset=2, oriented=True):
        r = subw(pc, bb, scale, offset=offset, oriented=oriented)
        cur["search_crop"] = (G.vec_of(bb), r.nbr_points())
        if np.abs(G.margins(frames[pc_frame[id(pc)]], G.vec_of(bb), scale, offset, TO.SUBWINDOW)).min() <= 1e-3:
            raise G.Reject("search crop margin, frame %d" % pc_frame[id(pc)])
        return r

    def rec_cac(PC, box, offset=0, scale=1.0, normalize=False):
        r = cac(PC, box, offset=offset, scale=scale, normalize=normalize)
        cur.setdefault("model_crops", []).append((id(PC), G.vec_of(box), r[0].nbr_points()))
        if np.abs(G.margins(frames[pc_frame[id(PC)]], G.vec_of(box), scale, offset, TO.MODEL)).min() <= 1e-3:
            raise G.Reject("model crop margin, frame %d" % pc_frame[id(PC)])
        return r

    def rec_prep(template_pc, search_pc, template_box, *a, **k):
        cur["n_template"], cur["n_search"] = template_pc.nbr_points(), search_pc.nbr_points()
        cur["canon"] = G.vec_of(template_box)
        return prep(template_pc, search_pc, template_box, *a, **k)

    def rec_bid(seq, frame_id, results_bbs, **k):
        cur.clear()
        data, ref_bb = bid(seq, frame_id, results_bbs, **k)
        cur["data"] = {kk: v.numpy().copy() for kk, v in data.items()}
        cur["ref"] = G.vec_of(ref_bb)
        return data, ref_bb

    def rec_fwd(d):
        r = fwd(d)
        cur["boxes"] = r["estimation_boxes"].detach().numpy().copy()[0]
        top = np.sort(cur["boxes"][:, 4])
        if top[-1] - top[-2] <= 1e-3:
            raise G.Reject("objectness gap %.2e" % (top[-1] - top[-2]))
        return r

    def rec_gob(box, offset, **k):
        cur["offset"] = np.asarray(offset, np.float32).copy()
        r = gob(box, offset, **k)
        cur["result"] = G.vec_of(r)
        per.append(dict(cur))
        return r
    model.build_input_dict, model.forward, model.prepare_input = rec_bid, rec_fwd, rec_prep
    PU.getOffsetBB, PU.generate_subwindow, PU.cropAndCenterPC = rec_gob, rec_subw, rec_cac
    try:
        with torch.no_grad():
            model.evaluate_one_sequence(sequence)
    except G.Reject as e:
        return [], str(e)
    finally:
        PU.getOffsetBB, PU.generate_subwindow, PU.cropAndCenterPC = gob, subw, cac
    assert len(per) == len(frames) - 1
    for c in per:
        c["model_crops"] = [(pc_frame[pid], b, n) for pid, b, n in c["model_crops"]]
    return per, None


def run_scene(seed):
    """-> (arrays, reject reason | None)"""
    name, cfg = TO.case_config(CASE)
    frames, gt = synth.make_scene(seed, N_FRAMES, N_POINTS, N_TARGETS)
    # the crops of frame 1 depend on the given boxes alone: test their margins before any network runs
    for k in range(N_TARGETS):
        if np.abs(G.margins(frames[1], gt[0, k], cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)).min() <= 1e-3:
            return {}, "target %d: search crop margin, frame 1" % k
        if np.abs(G.margins(frames[0], gt[0, k], cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)).min() <= 1e-3:
            return {}, "target %d: model crop margin, frame 0" % k
    out = {}
    for k in range(N_TARGETS):
        per, why = run_target(frames, gt[:, k], cfg, name)
        if why is not None:
            return {}, "target %d: %s" % (k, why)
        worst_margin, worst_gap = np.inf, np.inf
        for t, c in enumerate(per, start=1):
            b, n = c["search_crop"]
            m = G.margins(frames[t], b, cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)
            assert int((m > 0).sum()) == n, (k, t, "fp64 restatement of the search crop disagrees with the reference")
            worst_margin = min(worst_margin, np.abs(m).min())
            mc = []
            for tf, b, n in c["model_crops"]:
                m = G.margins(frames[tf], b, cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)
                assert int((m > 0).sum()) == n, (k, t, "fp64 restatement of the model crop disagrees with the reference")
                worst_margin = min(worst_margin, np.abs(m).min())
                mc.append(n)
            s = np.sort(c["boxes"][:, 4])
            worst_gap = min(worst_gap, float(s[-1] - s[-2]))
            key = "t%d.f%d." % (k, t)
            out[key + "ref_box"], out[key + "result_box"] = c["ref"], c["result"]
            out[key + "counts"] = np.array([c["n_search"], c["n_template"]], np.int64)
            out[key + "model_crop_counts"] = np.array(mc, np.int64)
            out[key + "template_points"] = c["data"]["template_points"][0]
            out[key + "search_points"] = c["data"]["search_points"][0]
            out[key + "points2cc_dist_t"] = c["data"]["points2cc_dist_t"][0]
            out[key + "proposals"] = c["boxes"]
            out[key + "offset"] = c["offset"]
            out[key + "canonical_wlh"] = c["canon"][3:6]
        if not (worst_margin > 1e-3 and worst_gap > 1e-3):
            return {}, "target %d: worst margin %.3e, worst gap %.3e" % (k, worst_margin, worst_gap)
        out["t%d.worst_margin" % k], out["t%d.worst_gap" % k] = np.float64(worst_margin), np.float64(worst_gap)
    out["scene_seed"] = np.int64(seed)
    out["n_targets"], out["n_frames"], out["n_points"] = np.int64(N_TARGETS), np.int64(N_FRAMES), np.int64(N_POINTS)
    return out, None


def main():
    for seed in range(0, 512):
        arrays, why = run_scene(seed)
        if why is None:
            print("scene seed %d: kept; per target worst crop margin [m] %s, worst objectness gap %s" % (
                seed, " ".join("%.3e" % arrays["t%d.worst_margin" % k] for k in range(N_TARGETS)),
                " ".join("%.3e" % arrays["t%d.worst_gap" % k] for k in range(N_TARGETS))), flush=True)
            break
        print("scene seed %d: %s -> next seed" % (seed, why), flush=True)
    assert why is None, "no scene seed below 512 meets the conditions"
    for k in range(N_TARGETS):
        assert arrays["t%d.worst_margin" % k] > 1e-3 and arrays["t%d.worst_gap" % k] > 1e-3
    written = fixture_io.save(os.path.join(G.ROOT, "tests", "golden", "ref_multi_tracking.npz"), **arrays)
    print("wrote", [os.path.basename(p) for p in written], len(arrays), "arrays")


if __name__ == "__main__":
    main()
