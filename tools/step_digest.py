"""SHA-256 digests of a seeded training run: the handle for comparing two checkouts, or two runs, BY EQUALITY.

  python tools/step_digest.py --model {BAT,P2B,M2TRACK} --batch B --template M --search N --steps S [--graph] [--deterministic]

A seeded model, a DataParallelStep (its own optimizer: Adam) and S synth batches (synth.make_batch(1000 + i*B, B, M, N);
M2TRACK: synth.make_motion_batch(1000 + i*B, B, N), --template is not used); S steps, one batch each.  One JSON line:
  losses   the digest of every step's loss
  grads    the digest of every parameter's gradient after the last step, in named_parameters order ("none": no gradient)
  state    the digest of every parameter and buffer after the last step
  all      one digest over all of the above, in that order
  graph    whether the last step was a replayed HIP graph (--graph: two eager steps, then capture and replay; a failed
           capture is an error)
Each digest is over the raw bytes of the tensor.  With --deterministic (fused.set_deterministic(True)) two runs print the same
line; without it the layer-0 list sums' LDS atomics usually make them differ.  Reads nothing outside the repository.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digest(t):
    if t is None:
        return "none"
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(model_name, batch, template, search, steps, graph=False, deterministic=False, seed=1234):
    from open3dsot_amd import dist as D, fused, synth, trackers
    dev = torch.device("cuda", 0)
    was = fused.deterministic_enabled()
    fused.set_deterministic(deterministic)
    try:
        torch.manual_seed(seed)
        if model_name == "M2TRACK":
            from open3dsot_amd import m2track
            model = m2track.M2TRACK().to(dev).train()
            batches = [synth.to_torch(synth.make_motion_batch(1000 + i * batch, batch, search), dev) for i in range(steps)]
        else:
            model = trackers.get_model(model_name)().to(dev).train()
            batches = [synth.to_torch(synth.make_batch(1000 + i * batch, batch, template, search), dev) for i in range(steps)]
        trainer = D.DataParallelStep(model, world=1, graph=graph, graph_warmup=min(2, max(steps - 1, 0)), require_graph=graph)
        losses = [digest(trainer.step(b)) for b in batches]
        torch.cuda.synchronize()
        out = {"model": model_name, "batch": batch, "template": template, "search": search, "steps": steps,
               "deterministic": bool(deterministic), "graph": trainer.graph is not None, "losses": losses,
               "grads": {k: digest(p.grad) for k, p in model.named_parameters()},
               "state": {k: digest(v) for k, v in list(model.named_parameters()) + list(model.named_buffers())}}
    finally:
        fused.set_deterministic(was)
    h = hashlib.sha256()
    for d in out["losses"] + list(out["grads"].values()) + list(out["state"].values()):
        h.update(d.encode())
    out["all"] = h.hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="BAT", choices=["BAT", "P2B", "M2TRACK"])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--template", type=int, default=256)
    ap.add_argument("--search", type=int, default=512)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--deterministic", action="store_true")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    print(json.dumps(run(a.model, a.batch, a.template, a.search, a.steps, a.graph, a.deterministic), sort_keys=True))


if __name__ == "__main__":
    main()
