"""What deterministic mode (fused.set_deterministic) costs, measured against the default mode in the same process.

  python tools/deterministic_cost.py [--models BAT,P2B] [--batch 48] [--template 512] [--search 1024] [--steps 40]
                                     [--repeats 7] [--out FILE]

Per model:
  step     two captured trainers on the same seeded model and the same resident batches, one captured with the mode on and one
           with it off; blocks of --steps replayed steps (host clock around a block that ends in a device synchronise),
           the two alternated --repeats times: median and range of the blocks' ms per step.
  launches eager steps with every fused launch bracketed by HIP events (gemm._PROF), the mode flipped between steps: the
           `group_reduce` calls (index build + list sums, one per set abstraction that has them, in backward order) of the ordered
           entry against the default pair, median and range over the steps.
Prints one JSON line; --out also writes the table as text.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med_range(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(model_name, a):
    from open3dsot_amd import dist as D, fused, gemm, synth, trackers
    dev = torch.device("cuda", 0)
    pool = [synth.to_torch(synth.make_batch(7000 + i * a.batch, a.batch, a.template, a.search), dev) for i in range(4)]
    trainers = {}
    for det in (False, True):
        fused.set_deterministic(det)
        torch.manual_seed(1234)
        model = trackers.get_model(model_name)().to(dev).train()
        tr = D.DataParallelStep(model, world=1, graph=True, graph_warmup=2, require_graph=True)
        for i in range(8):
            tr.step(pool[i % 4])
        torch.cuda.synchronize()
        assert tr.graph is not None
        trainers[det] = (tr, [tr.make_batch(b) for b in pool])
    blocks = {False: [], True: []}
    for _ in range(a.repeats):
        for det in (False, True):
            fused.set_deterministic(det)
            tr, flat = trainers[det]
            tr.step(flat[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                tr.step(flat[i % 4])
            torch.cuda.synchronize()
            blocks[det].append((time.perf_counter() - t0) * 1e3 / a.steps)
    # the launches, eagerly, on a third model
    fused.set_deterministic(False)
    torch.manual_seed(1234)
    model = trackers.get_model(model_name)().to(dev).train()
    calls = {False: [], True: []}
    for rep in range(2 + 2 * a.repeats):
        det = bool(rep % 2)
        fused.set_deterministic(det)
        gemm._PROF["events"], gemm._PROF["on"] = [], rep >= 2           # (the first step of each mode: warm-up)
        try:
            model.zero_grad(set_to_none=True)
            loss, _ = model.training_loss(pool[rep % 4])
            loss.backward()
            torch.cuda.synchronize()
        finally:
            gemm._PROF["on"] = False
        ms = [e0.elapsed_time(e1) for name, _, e0, e1, _ in gemm._PROF["events"] if name == "group_reduce"]
        if ms:
            calls[det].append(ms)
    gemm._PROF["events"] = []
    fused.set_deterministic(False)
    n = len(calls[False][0])
    launches = [{"call": i, "default_ms": med_range([c[i] for c in calls[False]]),
                 "ordered_ms": med_range([c[i] for c in calls[True]])} for i in range(n)]
    return {"model": model_name, "batch": a.batch, "template": a.template, "search": a.search, "steps_per_block": a.steps,
            "blocks": a.repeats, "step_ms_default": med_range(blocks[False]), "step_ms_deterministic": med_range(blocks[True]),
            "group_reduce_calls_in_backward_order": launches}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--models", default="BAT,P2B")
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--template", type=int, default=512)
    ap.add_argument("--search", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing is measured on the host"
    res = [measure(m, a) for m in a.models.split(",")]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/deterministic_cost.py: %s, one process, blocks alternated\n" % torch.cuda.get_device_name(0))
            for r in res:
                f.write("%s batch %d, %d/%d points, %d blocks of %d replayed steps per mode\n" % (
                    r["model"], r["batch"], r["template"], r["search"], r["blocks"], r["steps_per_block"]))
                for k, lab in (("step_ms_default", "default"), ("step_ms_deterministic", "deterministic")):
                    f.write("  step, %-13s median %.4f ms  (min %.4f, max %.4f)\n" % (lab, r[k]["median"], r[k]["min"], r[k]["max"]))
                for c in r["group_reduce_calls_in_backward_order"]:
                    f.write("  group_reduce call %d (index build + list sums, HIP events, eager): default %.4f ms (%.4f..%.4f), "
                            "ordered %.4f ms (%.4f..%.4f)\n" % (
                                c["call"], c["default_ms"]["median"], c["default_ms"]["min"], c["default_ms"]["max"],
                                c["ordered_ms"]["median"], c["ordered_ms"]["min"], c["ordered_ms"]["max"]))


if __name__ == "__main__":
    main()
