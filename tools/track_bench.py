"""ms per tracked frame of a whole sequence: the device-resident loop (open3dsot_amd/tracking.py) against the loop a user
had to write before it existed, on the same box in the same run.  Not bench.py: that measures the network alone.

  python tools/track_bench.py [--frames 200] [--points 120000] [--model BAT | P2B | M2TRACK]
  python tools/track_bench.py --targets K [--frames 200] [--points 120000] [--model BAT | P2B | M2TRACK]

Both loops track the same synth.make_sequence with a random-init model in eval mode and start from the frames resident in
HBM (device loop) / in host memory (host loop: where a dataset reader leaves them).
  device loop   SequenceTracker.update per frame; one 8-byte read-back per frame, the boxes never leave the device
  host loop     the numpy crops (tests/tracking_oracle.py, the fp32 restatement of the reference's generate_subwindow /
                cropAndCenterPC) -> upload -> model.prepare_input (BAT; P2B: regularize_pc) -> model.evaluate_one_sample
                -> read back the (4,) offset -> getOffsetBB's algebra in numpy
  --model M2TRACK: the device loop is MotionSequenceTracker.update; the host loop is MotionBaseModel.build_input_dict
                restated in numpy (tests/motion_oracle.py::host_input: two crops, two index draws, time stamp, prior-targetness
                mask, candidate BoxCloud) -> upload -> model.evaluate_one_sample -> read back -> getOffsetBB in numpy
Prints one JSON line with both figures and their ratio.

--targets K: K targets in the same frames (synth.make_scene, --points after merging): tracking.MultiTargetTracker, one batched
loop, against K SequenceTrackers run one after another over the same frames in the same process.  Both start from the
frames resident in HBM.  Prints one JSON line: ms per frame of both, targets x frames per second, their ratio and the
largest difference between the boxes of the two (batch-K against batch-1 forward, compounding over the sequence).
--targets K --model M2TRACK: tracking.MultiMotionTracker against K MotionSequenceTrackers run in turn, the same way, with the
same keys.

--sampling device: the free-running loop (tracking.tracker_for(model, sampling="device"): counts and index draws stay on the
device, update() only enqueues a frame) against the same tracker class with sampling="reference" (numpy's draw, one host sync
per frame), on the same frames and the same model (fixture weights, so that the box stays near its target), both from the
frames resident in HBM, each timed from the first update() to the read-back of its boxes, --repeats times in turn.  Prints one
JSON line: frames/s of both (median, smallest and largest run), their ratio, the crop counts of the last frame and overflow()
of the free-running loop.

--sampling table: the same measurement with a third loop in the rotation, sampling="table" (the free-running loop on the
reference's own indices, read from tracking.draw_table): frames/s of all three, table over device and over reference, the
build time and the bytes of the draw tables (built once, before the timed runs), and whether the table loop's boxes equal the
reference loop's in bits.  A scratch tracker is created and warmed before the three (first_capture: the first tracker of a
process is the slow one, whatever its mode).

--targets K --sampling device | table [--model M2TRACK]: the K targets of one live scene free-running
(tracking.scene_tracker_for(model, K, sampling=...): SceneTracker / MotionSceneTracker, no host stop per frame) against the
K-target loop of sampling="reference" (MultiTargetTracker / MultiMotionTracker: 2K counts read back, 2K numpy draws and two
uploads per frame) on the same synth.make_scene and the same model (fixture weights), both from frames resident in HBM, each
timed from its first update() to the read-back of its boxes, --repeats times in turn; a scratch tracker is created and warmed
before the two (first_capture).  Prints one JSON line: ms per frame of both (median, smallest and largest run), targets x
frames per second, their ratio, overflow() of the scene tracker, whether each loop replays a graph, the host time per update()
of both (the time until update() returns: the free-running loop only enqueues), and with "table" whether the two loops' boxes
are equal in bits.

--lanes L: the test epoch on L lanes (tracking.lane_tracker_for(model, L): --tracklets tracklets of --frames frames each, L at a
time in one free-running loop) against the sequential epoch of evaluate(..., sampling="device") (one free-running tracker, one
tracklet after the other) on the same tracklets, the same model (fixture weights) and the same SuccessPrecision scoring, both
from frames resident in HBM and both with their tracker and its captured graph reused, each timed from its first enqueue to
the read-back of the metric, --repeats times in turn.  The tracklets are --distinct different synth sequences used in
rotation.  Prints one JSON line: tracklet-frames/s of both (median, smallest and largest run), their ratio, the schedule's
steps and idle-lane share, overflow() and the batch-L forward replay.  With --sampling table a second lane tracker with
sampling="table" joins the rotation: tracklet-frames/s of both lane epochs and their ratio.

--targets K --manage D [--sampling device | table] [--model M2TRACK]: the managed scene tracker
(tracking.managed_scene_tracker_for(model, K): the slots' lifecycle as two device launches per frame) with D
device-resident detections per frame (the ground truth of the first min(D, K) targets, then boxes far away) against the plain
scene tracker at the same K, on the same scene, model and sampling ("table" unless given), both timed as above, --repeats times
in turn.  Prints one JSON line: ms per frame of both and their ratio, the device time of the two management launches (200 calls
between two events: o3d_scene_pair_scores alone, then both) and of the frame's crop call with and without the model-crop group
(the managed tracker always makes it), the managed tracker's final status and whether both replay a graph.  With --mot the
tracked run is then scored as multi-object tracking against the K ground-truth objects (tracker.score_mot, DESIGN.md section
12k): the device time of score_mot over all frames and of o3d_scene_pair_scores_frames and o3d_scene_mot_walk alone, each run
between two events (median, smallest, largest of 15), and the CLEAR-MOT numbers of the run.  --assignment optimal [--cost overlap]
 adds, in the same process beside the greedy run: a second managed tracker that matches by the optimal
assignment, timed in turn with the other two, its o3d_scene_manage_assign launch, with --mot the walk and score_mot under the
optimal rule, the path steps the Python restatement (tests/assign_oracle.py) counts on the read-back matrices, and one
o3d_scene_assign call at K = D = 64 with every pair tied, timed once after one warm-up call.
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))      # det_init, for motion_oracle.init_weights
import assign_oracle as AO  # noqa: E402
import motion_oracle as MO  # noqa: E402
import tracking_oracle as TO  # noqa: E402
from open3dsot_amd import m2track, points_utils as PU, synth, trackers, tracking  # noqa: E402


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


def motion_host_loop(model, cfg, frames, box0, dev):
    """frames: host arrays.  The motion tracker's loop with build_input_dict on the host."""
    boxes = [np.asarray(box0, np.float32)]
    for t in range(1, len(frames)):
        pts, bc, _ = MO.host_input(frames[t - 1], frames[t], boxes[-1], cfg, t == 1, with_bc=cfg["box_aware"])
        data = {"points": torch.from_numpy(pts).to(dev)[None]}
        if bc is not None:
            data["candidate_bc"] = torch.from_numpy(bc).to(dev)[None]
        off = model.evaluate_one_sample(data)[0].cpu().numpy()           # the read-back (a sync)
        boxes.append(TO.offset_box(boxes[-1], off, cfg["degrees"], cfg["use_z"], cfg["limit_box"])[0])
    return np.stack(boxes)


def motion_model(dev):
    """-> (model, cfg): the fixture's weights (tests/motion_oracle.py::init_weights) with the three box-moving heads scaled by a
    further 0.02: a He-initialised head answers with metres per frame, and even the fixture's decimetre per frame lifts the box
    off the ground within 25 frames, after which the loops would crop empty space and zero-fill their inputs"""
    cfg = MO.case_config("kitti")
    model = MO.init_weights(m2track.M2TRACK(**cfg))
    with torch.no_grad():
        for name in ("motion_mlp", "final_mlp", "box_mlp"):
            getattr(model, name)[-1].weight *= 0.02
            getattr(model, name)[-1].bias *= 0.02
    return model.to(dev).eval(), cfg


def multi_target_main(args, dev):
    K = args.targets
    if args.model.upper() == "M2TRACK":
        model, cfg = motion_model(dev)
        Multi, Single = tracking.MultiMotionTracker, tracking.MotionSequenceTracker
    else:
        cfg = dict(trackers.BAT_CAR if args.model.upper() == "BAT" else trackers.P2B_CAR)
        cfg.update(TO.TEST_KEYS)
        # the tracking fixture's weights: a He-initialised head moves every box by metres per frame, off its target
        model = TO.init_weights(trackers.get_model(args.model)(trackers.make_config(cfg))).to(dev).eval()
        Multi, Single = tracking.MultiTargetTracker, tracking.SequenceTracker
    frames, gt = synth.make_scene(args.seed, args.frames, max(args.points // K, 1024), K)
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    warm = min(20, args.frames)

    def run_multi(n):
        for t in range(1, n):
            multi.update(dframes[t])
        return multi.results()                                          # the one read-back of the boxes (a sync)

    def run_singles(n):
        out = []
        for k, s in enumerate(singles):                                 # one target after another
            s.init(dframes[0], gt[0, k])
            for t in range(1, n):
                s.update(dframes[t])
            out.append(s.results())
        return np.stack(out, 1)

    multi = Multi(model, K)
    multi.init(dframes[0], gt[0])
    run_multi(warm)                                                     # capture + warm-up
    torch.cuda.synchronize()
    multi.init(dframes[0], gt[0])
    t0 = time.perf_counter()
    multi_boxes = run_multi(args.frames)
    multi_ms = (time.perf_counter() - t0) / (args.frames - 1) * 1e3

    singles = [Single(model) for _ in range(K)]
    run_singles(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    single_boxes = run_singles(args.frames)
    single_ms = (time.perf_counter() - t0) / (args.frames - 1) * 1e3

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        multi._network()
    torch.cuda.synchronize()
    fwd_ms = (time.perf_counter() - t0) / 200 * 1e3
    diff = np.abs(multi_boxes - single_boxes).reshape(args.frames, -1).max(1)
    print(json.dumps({
        "workload": "%s tracking %d targets through a %d-frame, %d-point synthetic scene (fixture weights, eval, fp32)" % (
            args.model.upper(), K, args.frames, int(frames[0].shape[0])),
        "targets": K, "batched_loop_ms_per_frame": round(multi_ms, 4), "sequential_loops_ms_per_frame": round(single_ms, 4),
        "one_sequential_loop_ms_per_frame": round(single_ms / K, 4), "sequential_over_batched": round(single_ms / multi_ms, 2),
        "batched_target_frames_per_s": round(K * 1e3 / multi_ms, 1), "sequential_target_frames_per_s": round(K * 1e3 / single_ms, 1),
        "batched_forward_replay_ms": round(fwd_ms, 4), "batched_front_end_ms_per_frame": round(multi_ms - fwd_ms, 4),
        "hip_graph": multi.graph is not None, "crop_calls": multi.crop_calls,
        "largest_box_difference_frame_1": float(diff[1]), "largest_box_difference": float(diff.max())}))


def first_capture(model, dframes, box0):
    """The first tracker of a process replays its captured forward 6-9 % slower than every tracker created after it, whichever
    sampling mode it runs (measured in both creation orders).  Where --sampling table compares the two
    free-running modes, a scratch tracker takes that place before the timed ones are created -> the tracker, for the caller to
    keep alive (its buffers stay where they are)."""
    scratch = tracking.tracker_for(model)
    scratch.init(dframes[0], box0)
    for t in range(1, min(5, len(dframes))):
        scratch.update(dframes[t])
    torch.cuda.synchronize()
    return scratch


def sampling_main(args, dev):
    if args.model.upper() == "M2TRACK":
        model, cfg = motion_model(dev)
    else:
        cfg = dict(trackers.BAT_CAR if args.model.upper() == "BAT" else trackers.P2B_CAR)
        cfg.update(TO.TEST_KEYS)
        model = TO.init_weights(trackers.get_model(args.model)(trackers.make_config(cfg))).to(dev).eval()
    frames, gt = synth.make_sequence(args.seed, args.frames, args.points)
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    warm = min(20, args.frames)
    modes = ("device", "table", "reference") if args.sampling == "table" else ("device", "reference")
    trks, times, boxes, tables = {}, {m: [] for m in modes}, {}, {}
    scratch = first_capture(model, dframes, gt[0]) if args.sampling == "table" else None      # noqa: F841  (kept alive)
    for m in modes:
        if m == "table":                                                # the tables are built here, once: timed on their own
            tracking.clear_draw_tables()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        trks[m] = tracking.tracker_for(model, sampling=m)
        if m == "table":
            torch.cuda.synchronize()
            held = list(tracking._DRAW_TABLES.values())
            tables = {"draw_tables_build_s": round(time.perf_counter() - t0, 3), "draw_tables_shapes": [list(t.shape) for t in held],
                      "draw_tables_bytes": int(sum(t.numel() * t.element_size() for t in held))}
        trks[m].init(dframes[0], gt[0])
        for t in range(1, warm):                                        # capture + warm-up
            trks[m].update(dframes[t])
    torch.cuda.synchronize()
    for _ in range(args.repeats):                                       # the two loops in turn: what disturbs one disturbs the other
        for m in modes:
            trk = trks[m]
            trk.init(dframes[0], gt[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(1, args.frames):
                trk.update(dframes[t])
            boxes[m] = trk.results()                                    # the one read-back of the boxes (a sync)
            times[m].append(time.perf_counter() - t0)
    fps = {m: sorted((args.frames - 1) / dt for dt in times[m]) for m in modes}
    mid = {m: fps[m][len(fps[m]) // 2] for m in modes}
    free, ref = trks["device"], trks["reference"]
    if "table" in modes:
        tab = trks["table"]
        tables.update({
            "table_sampling_frames_per_s": round(mid["table"], 1),
            "table_sampling_frames_per_s_min_max": [round(fps["table"][0], 1), round(fps["table"][-1], 1)],
            "table_sampling_ms_per_frame": round(1e3 / mid["table"], 4),
            "table_over_device": round(mid["table"] / mid["device"], 3), "table_over_reference": round(mid["table"] / mid["reference"], 3),
            "table_sampling_overflow": list(tab.overflow()), "table_sampling_hip_graph": tab.graph is not None,
            "table_boxes_equal_reference_boxes_in_bits": bool(np.array_equal(boxes["table"].view(np.int32), boxes["reference"].view(np.int32)))})
    print(json.dumps({
        "workload": "%s tracking a %d-frame, %d-point synthetic sequence (fixture weights, eval, fp32), median of %d runs, the %d "
                    "loops in turn" % (args.model.upper(), args.frames, args.points, args.repeats, len(modes)),
        "device_sampling_frames_per_s": round(mid["device"], 1), "reference_sampling_frames_per_s": round(mid["reference"], 1),
        "device_over_reference": round(mid["device"] / mid["reference"], 3),
        "device_sampling_frames_per_s_min_max": [round(fps["device"][0], 1), round(fps["device"][-1], 1)],
        "reference_sampling_frames_per_s_min_max": [round(fps["reference"][0], 1), round(fps["reference"][-1], 1)],
        "device_sampling_ms_per_frame": round(1e3 / mid["device"], 4), "reference_sampling_ms_per_frame": round(1e3 / mid["reference"], 4),
        "hip_graph": [free.graph is not None, ref.graph is not None],
        "device_sampling_counts_last_frame": free.counts()[-1].tolist(), "device_sampling_overflow": list(free.overflow()),
        "reference_sampling_counts_last_frame": [int(v) if v is not None else -1 for v in ref.log[-1][:2]],
        "largest_centre_distance_between_the_two_trajectories": float(
            np.linalg.norm(boxes["device"][:, :3] - boxes["reference"][:, :3], axis=1).max()), **tables}))


def scene_main(args, dev):
    """--targets K --sampling device | table: the free-running K-target loop against the reference-sampling K-target loop"""
    K = args.targets
    if args.model.upper() == "M2TRACK":
        model, cfg = motion_model(dev)
    else:
        cfg = dict(trackers.BAT_CAR if args.model.upper() == "BAT" else trackers.P2B_CAR)
        cfg.update(TO.TEST_KEYS)
        model = TO.init_weights(trackers.get_model(args.model)(trackers.make_config(cfg))).to(dev).eval()
    frames, gt = synth.make_scene(args.seed, args.frames, max(args.points // K, 1024), K)
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    warm = min(20, args.frames)
    scratch = first_capture(model, dframes, gt[0, 0])      # noqa: F841  (kept alive: the first tracker of a process is the slow one)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trks = {"scene": tracking.scene_tracker_for(model, K, sampling=args.sampling)}      # "table": the draw tables are built here
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    trks["reference"] = tracking.multi_tracker_for(model, K)
    for trk in trks.values():
        trk.init(dframes[0], gt[0])
        for t in range(1, warm):                                        # capture + warm-up
            trk.update(dframes[t])
    torch.cuda.synchronize()
    times, host, boxes = {m: [] for m in trks}, {m: [] for m in trks}, {}
    for _ in range(args.repeats):                                       # the two loops in turn: what disturbs one disturbs the other
        for m, trk in trks.items():
            trk.init(dframes[0], gt[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(1, args.frames):
                trk.update(dframes[t])
            t1 = time.perf_counter()                                    # every update() has returned
            boxes[m] = trk.results()                                    # the one read-back of the boxes (a sync)
            times[m].append(time.perf_counter() - t0)
            host[m].append(t1 - t0)
    n = args.frames - 1
    ms = {m: sorted(1e3 * dt / n for dt in times[m]) for m in trks}
    mid = {m: ms[m][len(ms[m]) // 2] for m in trks}
    host_mid = {m: sorted(1e3 * dt / n for dt in host[m])[len(host[m]) // 2] for m in trks}
    scn, ref = trks["scene"], trks["reference"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        scn._network()
    torch.cuda.synchronize()
    fwd_ms = (time.perf_counter() - t0) / 200 * 1e3
    print(json.dumps({
        "workload": "%s tracking %d targets through a %d-frame, %d-point synthetic scene (fixture weights, eval, fp32), median of %d "
                    "runs, the two loops in turn" % (args.model.upper(), K, args.frames, int(frames[0].shape[0]), args.repeats),
        "targets": K, "sampling": args.sampling,
        "scene_ms_per_frame": round(mid["scene"], 4), "reference_ms_per_frame": round(mid["reference"], 4),
        "scene_ms_per_frame_min_max": [round(ms["scene"][0], 4), round(ms["scene"][-1], 4)],
        "reference_ms_per_frame_min_max": [round(ms["reference"][0], 4), round(ms["reference"][-1], 4)],
        "scene_target_frames_per_s": round(K * 1e3 / mid["scene"], 1), "reference_target_frames_per_s": round(K * 1e3 / mid["reference"], 1),
        "scene_over_reference": round(mid["reference"] / mid["scene"], 3),
        "scene_host_ms_per_update": round(host_mid["scene"], 4), "reference_host_ms_per_update": round(host_mid["reference"], 4),
        "batch_K_forward_replay_ms": round(fwd_ms, 4),
        "hip_graph": [scn.graph is not None, ref.graph is not None], "scene_overflow": list(scn.overflow()),
        "scene_overflow_targets": int(scn.overflow(per_target=True).any(1).sum()), "scene_lane_table_uploads_per_run": scn.lane_uploads,
        "scene_tracker_build_s": round(build_s, 3),
        "scene_boxes_equal_reference_boxes_in_bits": bool(np.array_equal(boxes["scene"].view(np.int32), boxes["reference"].view(np.int32))),
        "largest_centre_distance_between_the_two_trajectories": float(
            np.linalg.norm(boxes["scene"][..., :3] - boxes["reference"][..., :3], axis=-1).max())}))


def device_ms(fn, n=200):
    """ms per call of fn between two events on the current stream, after 10 calls of warm-up"""
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def manage_main(args, dev):
    """--targets K --manage D: the managed scene tracker with D device detections per frame against the plain scene tracker"""
    K, D = args.targets, args.manage
    sampling = args.sampling if args.sampling in tracking.FREE_RUNNING else "table"
    motion = args.model.upper() == "M2TRACK"
    if motion:
        model, cfg = motion_model(dev)
    else:
        cfg = dict(trackers.BAT_CAR if args.model.upper() == "BAT" else trackers.P2B_CAR)
        cfg.update(TO.TEST_KEYS)
        model = TO.init_weights(trackers.get_model(args.model)(trackers.make_config(cfg))).to(dev).eval()
    frames, gt = synth.make_scene(args.seed, args.frames, max(args.points // K, 1024), K)
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    far = np.tile(gt[:, :1], (1, max(D - K, 0), 1))                    # detections that match nothing: 10 km away, 10 m apart
    far[:, :, 0] += 1e4 + 10.0 * np.arange(far.shape[1])[None, :]
    dets = [torch.from_numpy(np.ascontiguousarray(np.concatenate([gt[t, :min(D, K)], far[t]], 0))).to(dev) for t in range(args.frames)]
    n_det = torch.tensor([D], dtype=torch.int32, device=dev)
    warm = min(20, args.frames)
    scratch = first_capture(model, dframes, gt[0, 0])      # noqa: F841  (kept alive: the first tracker of a process is the slow one)
    trks = {"managed": tracking.managed_scene_tracker_for(model, K, sampling=sampling, manage=dict(max_detections=max(D, 1))),
            "scene": tracking.scene_tracker_for(model, K, sampling=sampling)}
    optimal = args.assignment == "optimal"
    if optimal:
        rule = dict(assignment="optimal", cost=args.cost)
        trks["managed_optimal"] = tracking.managed_scene_tracker_for(model, K, sampling=sampling, manage=dict(max_detections=max(D, 1), **rule))

    def run(m, n):
        trk = trks[m]
        trk.init(dframes[0], gt[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(1, n):
            if m != "scene":
                trk.update(dframes[t], dets[t], n_det)
            else:
                trk.update(dframes[t])
        t1 = time.perf_counter()
        trk.results()                                                   # the one read-back of the boxes (a sync)
        return time.perf_counter() - t0, t1 - t0
    for m in trks:
        run(m, warm)                                                    # capture + warm-up
    times, host = {m: [] for m in trks}, {m: [] for m in trks}
    for _ in range(args.repeats):                                       # the two loops in turn: what disturbs one disturbs the other
        for m in trks:
            dt, dh = run(m, args.frames)
            times[m].append(dt)
            host[m].append(dh)
    n = args.frames - 1
    ms = {m: sorted(1e3 * dt / n for dt in times[m]) for m in trks}
    mid = {m: ms[m][len(ms[m]) // 2] for m in trks}
    host_mid = {m: sorted(1e3 * dt / n for dt in host[m])[len(host[m]) // 2] for m in trks}
    man, scn = trks["managed"], trks["scene"]
    status, next_id, dropped = man.status(), int(man.next_id), int(man.events()[2][-1])      # before the timing calls below
    last = dets[args.frames - 1]
    ov, di = (man._pairs[i, :K * D].view(K, D) for i in (0, 1))
    scores_ms = device_ms(lambda: PU.scene_pair_scores(man.cur, man.active, last, n_det, man.score_dim, man.score_up, out=(ov, di)))
    bank_next = None if motion else man.bank_state[man.t & 1]
    both_ms = device_ms(lambda: man._manage(last, n_det, 1 if motion else 0, bank_next, None if motion else man.aggregation))
    pts, prev = dframes[-1], dframes[-2]
    crop_both_ms = device_ms(lambda: man._crop_scene([prev, pts] if motion else [pts, prev]))
    crop_one_ms = crop_both_ms if motion else device_ms(lambda: man._crop_scene([pts, None]))
    mot = mot_timing(man, gt, dev) if args.mot else {}
    if optimal:
        mot.update(optimal_timing(trks["managed_optimal"], last, n_det, motion, gt, dev, rule, scores_ms, mid, ms, args.mot))
    print(json.dumps({
        "workload": "%s tracking %d targets through a %d-frame, %d-point synthetic scene with %d device detections per frame (fixture "
                    "weights, eval, fp32), median of %d runs, the two loops in turn" % (args.model.upper(), K, args.frames,
                                                                                        int(frames[0].shape[0]), D, args.repeats),
        "targets": K, "detections": D, "sampling": sampling,
        "managed_ms_per_frame": round(mid["managed"], 4), "scene_ms_per_frame": round(mid["scene"], 4),
        "managed_ms_per_frame_min_max": [round(ms["managed"][0], 4), round(ms["managed"][-1], 4)],
        "scene_ms_per_frame_min_max": [round(ms["scene"][0], 4), round(ms["scene"][-1], 4)],
        "managed_over_scene": round(mid["managed"] / mid["scene"], 4),
        "managed_host_ms_per_update": round(host_mid["managed"], 4), "scene_host_ms_per_update": round(host_mid["scene"], 4),
        "pair_scores_launch_device_ms": round(scores_ms, 5), "manage_launch_device_ms": round(both_ms - scores_ms, 5),
        "management_device_ms_per_frame": round(both_ms, 5), "management_share_of_scene_frame": round(both_ms / mid["scene"], 4),
        "crop_call_device_ms_both_groups": round(crop_both_ms, 5), "crop_call_device_ms_search_group_only": round(crop_one_ms, 5),
        "hip_graph": [man.graph is not None, scn.graph is not None],
        "managed_active_slots": int(status["active"].sum()), "managed_next_id": next_id,
        "managed_dropped_detections_last_frame": dropped, "managed_overflow": list(man.overflow()),
        "scene_overflow": list(scn.overflow()), **mot}))


def optimal_timing(man, last, n_det, motion, gt, dev, rule, scores_ms, mid, ms, with_mot):
    """--assignment optimal: the second managed tracker's figures, keys prefixed optimal_; the path steps of the last frame's
    match and (--mot) of every frame of the walk, counted by tests/assign_oracle.py on the read-back matrices; the tied call"""
    K, D = man.K, last.shape[0]
    ov, di = (man._pairs[i, :K * D].view(K, D) for i in (0, 1))
    bank_next = None if motion else man.bank_state[man.t & 1]
    active = man.active.cpu().numpy()                                   # before the timing calls below
    PU.scene_pair_scores(man.cur, man.active, last, n_det, man.score_dim, man.score_up, out=(ov, di))
    stats = {}
    AO.assign(ov.cpu().numpy(), di.cpu().numpy(), active, int(n_det), man.manage["min_iou"], man.manage["max_dist"], stats=stats, **rule)
    both_ms = device_ms(lambda: man._manage(last, n_det, 1 if motion else 0, bank_next, None if motion else man.aggregation))
    out = {"optimal_rule": rule, "optimal_managed_ms_per_frame": round(mid["managed_optimal"], 4),
           "optimal_managed_ms_per_frame_min_max": [round(ms["managed_optimal"][0], 4), round(ms["managed_optimal"][-1], 4)],
           "optimal_manage_launch_device_ms": round(both_ms - scores_ms, 5),
           "optimal_management_share_of_scene_frame": round(both_ms / mid["scene"], 4),
           "optimal_manage_path_steps_last_frame": stats["steps"], "optimal_hip_graph": man.graph is not None}
    if with_mot:
        res = mot_timing(man, gt, dev, rule=rule)
        out.update({"optimal_" + k: v for k, v in res.items()})
    n = 64                                                              # every pair tied: row r takes r + 1 steps
    tied = (torch.zeros((n, n), device=dev), torch.ones((n, n), device=dev))
    PU.scene_assign(*tied, **rule)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = PU.scene_assign(*tied, **rule)
    b.record()
    b.synchronize()
    steps = n * (n + 1) // 2
    out.update({"assign_tied_64_device_ms_once": round(a.elapsed_time(b), 5), "assign_tied_64_path_steps": steps,
                "assign_tied_64_us_per_step": round(1e3 * a.elapsed_time(b) / steps, 4), "assign_tied_64_summary": res[2].tolist()})
    return out


def mot_timing(man, gt, dev, runs=15, rule=None):
    """--mot: score the managed run that was just tracked as multi-object tracking, G = K ground-truth
    objects over all its frames: the device time of score_mot (both launches and the torch reductions of ClearMOT.update) and of
    each launch alone, every run between two events of its own, median and range of `runs` runs after 3 of warm-up"""
    from open3dsot_amd import metrics as MT
    T, K = man.t, man.K
    g_dev = torch.from_numpy(np.ascontiguousarray(gt[:T], dtype=np.float32)).to(dev)
    v_dev = torch.ones((T, K), dtype=torch.int32, device=dev)
    boxes, ids = man.boxes[:T], man.ids_log[:T]
    rule = dict(rule or {})                                             # {}: the greedy walk
    m = MT.ClearMOT(K, dev, dim=man.score_dim, up_axis=(0, 0, 1) if man.score_up == 2 else (0, -1, 0), **rule)
    assert m.chunk_frames(K) >= T, "the separate launches below time one chunk"
    ov, di = PU.scene_pair_scores_frames(g_dev, v_dev, boxes, ids, m.dim, m.up)
    rows = PU.scene_mot_walk(ov, di, v_dev, ids, m.state[0], m.state[1], m.state[2], m.min_iou, m.max_dist, **rule)
    steps = {}
    if rule:                                                            # the path steps of the walk, counted by the restatement
        stats = {}
        AO.mot_walk(ov.cpu().numpy(), di.cpu().numpy(), v_dev.cpu().numpy(), ids.cpu().numpy(), None, m.min_iou, m.max_dist, stats=stats, **rule)
        steps = {"mot_walk_path_steps_per_frame": round(stats["steps"] / T, 2)}

    def timed(fn):
        ms = []
        for i in range(runs + 3):
            m.reset()                                                   # every run walks from the empty state
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= 3:
                ms.append(a.elapsed_time(b))
        ms.sort()
        return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]
    whole = timed(lambda: man.score_mot(g_dev, v_dev, metrics=m))
    res = m.compute()
    scores = timed(lambda: PU.scene_pair_scores_frames(g_dev, v_dev, boxes, ids, m.dim, m.up, out=(ov, di)))
    walk = timed(lambda: PU.scene_mot_walk(ov, di, v_dev, ids, m.state[0], m.state[1], m.state[2], m.min_iou, m.max_dist, out=rows, **rule))
    return {"mot_frames": T, "mot_objects": K, "mot_gates": [m.min_iou, m.max_dist], "mot_runs": runs,
            "score_mot_device_ms_median_min_max": whole, "pair_scores_frames_device_ms_median_min_max": scores,
            "mot_walk_device_ms_median_min_max": walk, "mot_walk_ms_per_frame": round(walk[0] / T, 5),
            "mot": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in res.items()}, **steps}


def lanes_main(args, dev):
    from open3dsot_amd import metrics as MT
    L = args.lanes
    if args.model.upper() == "M2TRACK":
        model, cfg = motion_model(dev)
    else:
        cfg = dict(trackers.BAT_CAR if args.model.upper() == "BAT" else trackers.P2B_CAR)
        cfg.update(TO.TEST_KEYS)
        model = TO.init_weights(trackers.get_model(args.model)(trackers.make_config(cfg))).to(dev).eval()
    distinct = []
    for j in range(min(args.distinct, args.tracklets)):
        frames, gt = synth.make_sequence(args.seed + j, args.frames, args.points)
        distinct.append(([torch.from_numpy(f).to(dev) for f in frames], torch.from_numpy(gt).to(dev)))
    tracklets = [distinct[j % len(distinct)] for j in range(args.tracklets)]
    tracked = args.tracklets * (args.frames - 1)
    scratch = first_capture(model, distinct[0][0], distinct[0][1][0]) if args.sampling == "table" else None      # noqa: F841  (kept alive)
    lane, one = tracking.lane_tracker_for(model, L), tracking.tracker_for(model, sampling="device")
    results = {}

    def run_lanes():
        m = MT.SuccessPrecision(device=dev)
        lane.run(tracklets)
        lane.score(metrics=m)
        return m.compute()                                              # the one read-back (a sync)

    def run_sequential():
        m = MT.SuccessPrecision(device=dev)
        for frames, gt in tracklets:
            tracking.evaluate_sequence(model, frames, gt, tracker=one, metrics=m)
        return m.compute()

    loops = {"lanes": run_lanes, "sequential": run_sequential}
    warm = [distinct[0]] * min(2 * L, args.tracklets)
    lane.run(warm)                                                      # capture + warm-up
    extra = {}
    if args.sampling == "table":                                        # a second lane epoch, on the reference's indices
        lane_tab = tracking.lane_tracker_for(model, L, sampling="table")

        def run_lanes_table():
            m = MT.SuccessPrecision(device=dev)
            lane_tab.run(tracklets)
            lane_tab.score(metrics=m)
            return m.compute()
        loops = {"lanes": run_lanes, "lanes_table": run_lanes_table, "sequential": run_sequential}
        lane_tab.run(warm)
    tracking.evaluate_sequence(model, *distinct[0], tracker=one)
    torch.cuda.synchronize()
    times = {k: [] for k in loops}
    for _ in range(args.repeats):                                       # the two epochs in turn: what disturbs one disturbs the other
        for k, loop in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[k] = loop()
            times[k].append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        lane._network()
    torch.cuda.synchronize()
    fwd_ms = (time.perf_counter() - t0) / 200 * 1e3
    fps = {k: sorted(tracked / dt for dt in times[k]) for k in loops}
    mid = {k: fps[k][len(fps[k]) // 2] for k in loops}
    idle = float((lane.schedule[0] < 0).mean())
    if args.sampling == "table":
        extra = {"lanes_table_tracklet_frames_per_s": round(mid["lanes_table"], 1),
                 "lanes_table_tracklet_frames_per_s_min_max": [round(fps["lanes_table"][0], 1), round(fps["lanes_table"][-1], 1)],
                 "lanes_table_over_lanes": round(mid["lanes_table"] / mid["lanes"], 3), "lanes_table_overflow": list(lane_tab.overflow()),
                 "lanes_table_hip_graph": lane_tab.graph is not None}
    print(json.dumps({
        "workload": "%s test epoch: %d tracklets of %d frames of %d points (%d distinct synthetic sequences, fixture weights, eval, "
                    "fp32), median of %d runs, the %d epochs in turn" % (args.model.upper(), args.tracklets, args.frames, args.points,
                                                                         len(distinct), args.repeats, len(loops)),
        "lanes": L, "steps": int(lane.steps), "idle_lane_share": round(idle, 4), "chunk_uploads": lane.uploads,
        "lanes_tracklet_frames_per_s": round(mid["lanes"], 1), "sequential_tracklet_frames_per_s": round(mid["sequential"], 1),
        "lanes_over_sequential": round(mid["lanes"] / mid["sequential"], 3),
        "lanes_tracklet_frames_per_s_min_max": [round(fps["lanes"][0], 1), round(fps["lanes"][-1], 1)],
        "sequential_tracklet_frames_per_s_min_max": [round(fps["sequential"][0], 1), round(fps["sequential"][-1], 1)],
        "lanes_ms_per_step": round(1e3 * tracked / mid["lanes"] / max(lane.steps, 1), 4),
        "sequential_ms_per_frame": round(1e3 / mid["sequential"], 4), "batch_L_forward_replay_ms": round(fwd_ms, 4),
        "hip_graph": [lane.graph is not None, one.graph is not None], "lanes_overflow": list(lane.overflow()),
        "success_precision": {k: [round(float(v["success"]), 3), round(float(v["precision"]), 3)] for k, v in results.items()},
        "scored_frames": [int(v["frames"]) for v in results.values()], **extra}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--model", default="BAT")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--targets", type=int, default=0, help="K > 0: the batched K-target loop against K single-target trackers in turn")
    ap.add_argument("--sampling", default="reference", choices=tracking.SAMPLING,
                    help="device: the free-running loop against the reference-sampling loop, frames/s of both; table: the "
                         "free-running loop on the reference's indices as a third loop (with --lanes: a second lane epoch)")
    ap.add_argument("--repeats", type=int, default=15, help="--sampling device, --lanes: timed runs per loop (the median is reported)")
    ap.add_argument("--lanes", type=int, default=0, help="L > 0: the test epoch on L lanes against the sequential free-running epoch")
    ap.add_argument("--manage", type=int, default=0, help="with --targets K: D > 0 device detections per frame, the managed scene "
                                                          "tracker against the plain one")
    ap.add_argument("--mot", action="store_true", help="with --manage: time score_mot (ClearMOT) on the tracked run, and its two "
                                                       "launches alone, each between two events, 15 runs")
    ap.add_argument("--assignment", default="greedy", choices=sorted(PU.ASSIGNMENTS),
                    help="with --manage: optimal adds a managed tracker, its launches and (--mot) its walk under the optimal assignment")
    ap.add_argument("--cost", default="distance", choices=sorted(PU.ASSIGN_COSTS), help="--assignment optimal: the integer cost")
    ap.add_argument("--tracklets", type=int, default=64, help="--lanes: tracklets of the epoch, --frames frames each")
    ap.add_argument("--distinct", type=int, default=8, help="--lanes: different synthetic sequences, used in rotation")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench.py needs a GPU: the HIP library is the only compute path (no CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    if args.lanes > 0:
        if args.targets > 0 or args.frames < 2:
            raise SystemExit("--lanes times the test epoch: no --targets, at least 2 frames per tracklet")
        return lanes_main(args, dev)
    if args.manage > 0:
        if args.targets < 1 or args.frames < 3:
            raise SystemExit("--manage D times the managed scene tracker: it needs --targets K and at least 3 frames")
        return manage_main(args, dev)
    if args.targets > 0:
        if args.sampling in tracking.FREE_RUNNING:
            if args.frames < 2:
                raise SystemExit("--targets K --sampling %s times a scene: at least 2 frames" % args.sampling)
            return scene_main(args, dev)
        return multi_target_main(args, dev)
    if args.sampling in tracking.FREE_RUNNING:
        return sampling_main(args, dev)
    motion = args.model.upper() == "M2TRACK"
    if motion:
        model, cfg = motion_model(dev)
        loop = motion_host_loop
    else:
        cfg = dict(trackers.BAT_CAR if args.model.upper() == "BAT" else trackers.P2B_CAR)
        cfg.update(TO.TEST_KEYS)
        model = trackers.get_model(args.model)(trackers.make_config(cfg)).to(dev).eval()
        loop = host_loop
    frames, gt = synth.make_sequence(args.seed, args.frames, args.points)
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    warm = min(20, args.frames)

    trk = tracking.tracker_for(model)
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

    loop(model, cfg, frames[:warm], gt[0], dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_boxes = loop(model, cfg, frames, gt[0], dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) / (args.frames - 1) * 1e3

    # the forward alone on the tracker's own static inputs, for scale (what bench.py --infer times)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        trk._network()
    torch.cuda.synchronize()
    fwd_ms = (time.perf_counter() - t0) / 200 * 1e3
    extra = {}
    if motion:      # what the untrained segmentation head made of the last frame: the stages behind it run on the masked points
        with torch.no_grad():
            seg = model(trk.inputs)["seg_logits"][0]
        extra = {"foreground_points_last_frame": int((seg[1] > seg[0]).sum()), "points_per_frame": int(seg.shape[1]),
                 "crop_counts_last_frame": list(trk.log[-1])}
    print(json.dumps({
        "workload": "%s tracking a %d-frame, %d-point synthetic sequence (%s weights, eval, fp32)" % (
            args.model.upper(), args.frames, args.points, "random-init, box-moving heads scaled" if motion else "random-init"),
        "device_loop_ms_per_frame": round(dev_ms, 4), "host_loop_ms_per_frame": round(host_ms, 4),
        "host_over_device": round(host_ms / dev_ms, 2), "forward_replay_ms": round(fwd_ms, 4),
        "front_end_ms_per_frame": round(dev_ms - fwd_ms, 4), "hip_graph": trk.graph is not None,
        "largest_box_difference_between_the_loops": float(np.abs(dev_boxes - host_boxes).max()), **extra}))


if __name__ == "__main__":
    main()
