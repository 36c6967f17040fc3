"""ms per tracked frame of a whole sequence: the device-resident loop (open3dsot_amd/tracking.py) against the loop a user
had to write before it existed, on the same box in the same run.  Not bench.py: that measures the network alone.

  python tools/track_bench.py [--frames 200] [--points 120000] [--model BAT]

Both loops track the same synth.make_sequence with a random-init model in eval mode and start from the frames resident in
HBM (device loop) / in host memory (host loop: where a dataset reader leaves them).
  device loop   SequenceTracker.update per frame; one 8-byte read-back per frame, the boxes never leave the device
  host loop     the numpy crops (tests/tracking_oracle.py, the fp32 restatement of the reference's generate_subwindow /
                cropAndCenterPC) -> upload -> model.prepare_input (BAT; P2B: regularize_pc) -> model.evaluate_one_sample
                -> read back the (4,) offset -> getOffsetBB's algebra in numpy
Prints one JSON line with both figures and their ratio.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracking_oracle as TO  # noqa: E402
from open3dsot_amd import points_utils as PU, synth, trackers, tracking  # noqa: E402


def host_loop(model, cfg, frames, box0, dev):
    """frames: host arrays.  shape_aggregation firstandprevious, reference_BB previous_result."""
    boxes = [np.asarray(box0, np.float32)]
    first = TO.crop(frames[0], boxes[0], cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)[1]
    canon = (np.zeros(3, np.float32), boxes[0][3:6], np.eye(3, dtype=np.float32))
    for t in range(1, len(frames)):
        search = TO.crop(frames[t], boxes[-1], cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)[1]
        prev = TO.crop(frames[t - 1], boxes[-1], cfg["model_bb_scale"], cfg["model_bb_offset"], TO.MODEL)[1]
        tpl = np.concatenate([first, prev], 0)
        tp, sp = torch.from_numpy(tpl).to(dev), torch.from_numpy(search).to(dev)
        if hasattr(model, "prepare_input"):
            data = model.prepare_input(tp, sp, canon)
        else:
            data = {"template_points": PU.regularize_pc(tp, cfg["template_size"], seed=1)[0][None],
                    "search_points": PU.regularize_pc(sp, cfg["search_size"], seed=1)[0][None]}
        with torch.no_grad():
            best, _ = model.evaluate_one_sample(data)
        off = best[0].cpu().numpy()                                     # the read-back (a sync)
        boxes.append(TO.offset_box(boxes[-1], off, cfg["degrees"], cfg["use_z"], cfg["limit_box"])[0])
    return np.stack(boxes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--model", default="BAT")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench.py needs a GPU: the HIP library is the only compute path (no CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    cfg = dict(trackers.BAT_CAR if args.model.upper() == "BAT" else trackers.P2B_CAR)
    cfg.update(TO.TEST_KEYS)
    model = trackers.get_model(args.model)(trackers.make_config(cfg)).to(dev).eval()
    frames, gt = synth.make_sequence(args.seed, args.frames, args.points)
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    warm = min(20, args.frames)

    trk = tracking.SequenceTracker(model)
    trk.init(dframes[0], gt[0])
    for t in range(1, warm):                                            # capture + warm-up
        trk.update(dframes[t])
    torch.cuda.synchronize()
    trk.init(dframes[0], gt[0])
    t0 = time.perf_counter()
    for t in range(1, args.frames):
        trk.update(dframes[t])
    dev_boxes = trk.results()                                           # the one read-back of the boxes (a sync)
    dev_ms = (time.perf_counter() - t0) / (args.frames - 1) * 1e3

    host_loop(model, cfg, frames[:warm], gt[0], dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_boxes = host_loop(model, cfg, frames, gt[0], dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) / (args.frames - 1) * 1e3

    # the forward alone on the tracker's own static inputs, for scale (what bench.py --infer times)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        trk._network()
    torch.cuda.synchronize()
    fwd_ms = (time.perf_counter() - t0) / 200 * 1e3
    print(json.dumps({
        "workload": "%s tracking a %d-frame, %d-point synthetic sequence (random-init weights, eval, fp32)" % (args.model.upper(), args.frames, args.points),
        "device_loop_ms_per_frame": round(dev_ms, 4), "host_loop_ms_per_frame": round(host_ms, 4),
        "host_over_device": round(host_ms / dev_ms, 2), "forward_replay_ms": round(fwd_ms, 4),
        "front_end_ms_per_frame": round(dev_ms - fwd_ms, 4), "hip_graph": trk.graph is not None,
        "largest_box_difference_between_the_loops": float(np.abs(dev_boxes - host_boxes).max())}))


if __name__ == "__main__":
    main()
