"""The C entries of every tracker of open3dsot_amd/tracking.py, call by call.

    python tools/tracker_trace.py [--root DIR] [--out FILE] [--json FILE]

Every C call of the trackers passes through `capi.check(rc, what)`.  The tool wraps that function and runs fourteen small
configurations (CONFIGS) on one synthetic scene.  Per tracker and per public call (init / begin, every update() / step(), the
retire / enroll events) it prints the ordered list of C entries, the call's host-stop count (the calls that
tests/test_free_running_tracking_gpu.py::host_stops counts) and the tracker's lane_uploads / uploads / crop_calls counters where
the class has them; after the run a sha256 of the bytes of results() and, where the class has them, of counts() and events().
Two commits whose trackers make the same C calls in the same order, stop the host as often, upload as often and compute the same
boxes give byte-identical output, so a refactor of the host side is checked with `diff` (profiles/tracker_trace.txt: copy this
file onto a checkout of another commit, or point --root at one, to repeat it).  The forward runs as a HIP graph (use_graph=True):
its entries show in the first update(), which runs it twice (warm-up and capture), and in no later one.

--json: the entry lists, host stops and counters without the digests (tests/golden/tracker_launches.json is the parent's; the
digests compare two runs of one session on one GPU and are no portable constant).

Shapes: 5 frames of 2048 points per target, K = 3 targets, L = 2 lanes over 3 tracklets of 3, 5 and 2 frames (4 steps: lane 0
starts a second tracklet at step 2 and idles at step 3; chunks of 2 steps, so the epoch uploads twice), capacities of 4096,
sampling="device" wherever a class takes it.  The scene runs retire slot 1 and enroll slot 2 in front of frame 3 (slot 1 stays
retired: its row of ref_boxes is ignored from then on) and have a sixth frame, the only one without a lane-table event.  The
managed runs start with 2 of 3 slots taken and see 4 detections per frame (the 3 targets and a box far away), none at frame 2.
"""
import argparse
import hashlib
import json
import os
import sys

FRAMES, POINTS, K, LANES, CAP, SEED = 5, 2048, 3, 2, 4096, 7
SCENE_FRAMES = FRAMES + 1     # a scene's lane table changes at frames 1 and 2, at the enroll's frame 3 and at frame 4: 5 has no event
TRACKLETS = (3, 5, 2)         # with 3, 4, 2 the two lanes end together; the fifth frame leaves lane 0 idle at the last step
CROPS = ("o3d_track_crop", "o3d_track_crop_multi", "o3d_track_crop_groups")
BOX_UPDATES = ("o3d_track_offset_box", "o3d_track_offset_box_multi", "o3d_track_offset_box_lanes")
COUNTERS = ("lane_uploads", "uploads", "crop_calls")
# name -> (model, loop, sampling); the models are those of models()
CONFIGS = {
    "sequence_reference": ("bat", "single", "reference"), "sequence_device": ("bat", "single", "device"),
    "motion_sequence_reference": ("motion", "single", "reference"), "motion_sequence_device": ("motion", "single", "device"),
    "multi_target": ("bat", "multi", "reference"), "multi_motion": ("motion", "multi", "reference"),
    "lanes": ("bat", "lanes", "device"), "motion_lanes": ("motion", "lanes", "device"),
    "scene": ("bat", "scene", "device"), "motion_scene": ("motion", "scene", "device"),
    "managed_scene": ("bat", "managed", "device"), "managed_motion_scene": ("motion", "managed", "device"),
    "scene_first": ("bat_first", "scene", "device"), "scene_previous_gt": ("bat_previous_gt", "scene", "device"),
}
FREE_LOOPS = ("lanes", "scene", "managed")          # with a leading axis and no host stop per frame


def _paths(root):
    root = os.path.abspath(root)
    for p in (os.path.join(root, "tests", "golden"), os.path.join(root, "tests"), root):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    return root


class Recorder:
    """capi.check wrapped: every entry name goes to the call that is open"""

    def __init__(self, capi):
        self.capi, self.orig, self.open = capi, capi.check, None

        def check(rc, what):
            if self.open is not None:
                self.open.append(str(what))
            return self.orig(rc, what)
        capi.check = check

    def close(self):
        self.capi.check = self.orig


def models(dev):
    """the four models of CONFIGS, with the weights of the tracking tests"""
    import motion_oracle as MO
    import tracking_oracle as TO
    from open3dsot_amd import m2track, trackers
    out = {}
    for name, over in (("bat", {}), ("bat_first", {"shape_aggregation": "first"}), ("bat_previous_gt", {"reference_BB": "previous_gt"})):
        cfg = TO.case_config("bat_fap")[1]
        cfg.update(over)
        out[name] = TO.init_weights(trackers.get_model("BAT")(trackers.make_config(cfg))).to(dev).eval()
    out["motion"] = MO.init_weights(m2track.M2TRACK(**MO.case_config("kitti"))).to(dev).eval()
    return out


def _capacities(motion):
    return dict(capacity=CAP) if motion else dict(search_capacity=CAP, model_capacity=CAP)


def _digest(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_config(name, model, dev, rec, stops):
    """-> {"calls": [{"call", "entries", "host_stops", counters...}], "digests": {...}}"""
    import numpy as np
    import torch
    from open3dsot_amd import synth, tracking
    kind, loop, sampling = CONFIGS[name]
    motion = kind == "motion"
    calls = []

    def call(label, fn, *a, **k):
        rec.open = entries = []
        with stops() as s:
            out = fn(*a, **k)
        rec.open = None
        row = {"call": label, "entries": entries, "host_stops": len(s.calls)}
        row.update({c: int(getattr(trk, c)) for c in COUNTERS if hasattr(trk, c)})
        calls.append(row)
        return out

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    kw = dict(seed=2, use_graph=True, **_capacities(motion))
    if loop == "single":
        frames, gt = synth.make_sequence(SEED, FRAMES, POINTS)
        frames = [up(f) for f in frames]
        trk = tracking.tracker_for(model, sampling=sampling, **kw)
        call("init", trk.init, frames[0], gt[0])
        for t in range(1, FRAMES):
            call("update %d" % t, trk.update, frames[t])
    elif loop == "lanes":
        tracklets = []
        for j, n in enumerate(TRACKLETS):
            frames, gt = synth.make_sequence(SEED + j, n, POINTS)
            tracklets.append(([up(f) for f in frames], up(gt)))
        trk = tracking.lane_tracker_for(model, LANES, plan_steps=2, sampling=sampling, **kw)
        steps = call("begin", trk.begin, tracklets)
        for s in range(steps):
            call("step %d" % s, trk.step)
    else:
        frames, gt = synth.make_scene(SEED, SCENE_FRAMES if loop == "scene" else FRAMES, POINTS, K)
        frames, gt_dev = [up(f) for f in frames], up(gt)
        if loop == "multi":
            trk = tracking.multi_tracker_for(model, K, **kw)
        elif loop == "scene":
            trk = tracking.scene_tracker_for(model, K, sampling=sampling, **kw)
        else:
            trk = tracking.managed_scene_tracker_for(model, K, sampling=sampling, manage=dict(max_misses=1, max_dist=3.0), **kw)
        call("init", trk.init, frames[0], gt[0, :2] if loop == "managed" else gt[0])
        by_gt = getattr(trk, "needs_ref_box", False)
        for t in range(1, len(frames)):
            if loop == "scene" and t == 3:
                call("retire", trk.retire, 1)
                call("enroll", trk.enroll, 2, gt[2, 2])
            if loop == "managed":
                far = np.array(gt[t, :1], np.float32)
                far[0, 0] += 500.0
                dets = None if t == 2 else up(np.concatenate([gt[t], far], 0))
                call("update %d" % t, trk.update, frames[t], dets)
            elif by_gt:
                call("update %d" % t, trk.update, frames[t], gt_dev[t - 1])
            else:
                call("update %d" % t, trk.update, frames[t])
    torch.cuda.synchronize()
    on_lanes = loop == "lanes"
    digests = {"results": _digest(trk.boxes.cpu().numpy() if on_lanes else trk.results())}
    if trk.free_running:
        digests["counts"] = _digest(trk.counts_log.cpu().numpy() if on_lanes else trk.counts())
    if hasattr(trk, "events"):
        digests["events"] = _digest(*trk.events())
    return {"calls": calls, "digests": digests}


def run(root=None, only=None):
    """Run CONFIGS (or the names in `only`) on the package under `root` (default: this file's checkout) -> {name: run_config}"""
    _paths(root or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import pytest
    import torch
    import test_free_running_tracking_gpu as FR
    from open3dsot_amd import capi
    dev = torch.device("cuda", 0)
    held = models(dev)
    rec = Recorder(capi)
    try:
        return {name: run_config(name, held[CONFIGS[name][0]], dev, rec, lambda: FR.host_stops(pytest.MonkeyPatch()))
                for name in CONFIGS if only is None or name in only}
    finally:
        rec.close()


def launches(result):
    """what tests/golden/tracker_launches.json holds: the calls without the digests"""
    return {name: r["calls"] for name, r in result.items()}


def text(result):
    lines = []
    for name, r in result.items():
        lines.append("# %s: %s" % (name, " ".join(CONFIGS[name])))
        for row in r["calls"]:
            lines.append("%s: %s" % (row["call"], " ".join(row["entries"]) or "-"))
            lines.append("  " + " ".join("%s=%d" % (k, v) for k, v in row.items() if k not in ("call", "entries")))
        for k, v in r["digests"].items():
            lines.append("sha256 %s %s" % (k, v))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="the checkout whose package is traced (default: this file's)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    result = run(a.root)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in launches(result).items()) + "\n}\n")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text(result))
    else:
        sys.stdout.write(text(result))


if __name__ == "__main__":
    main()
