"""One line per kernel launch of a tracker's eager training step (forward + backward) and eval forward.

    python tools/launch_trace.py --model BAT|P2B|M2TRACK --shape small|bench [--root DIR] [--out FILE] [--save FILE.pt]

Every launch of the fused operators goes through `_call(name, flops, fn, *args, dims=)`.  The tool wraps that function in
every loaded module that holds a reference to it and prints, per launch: the launch name, the C entry, the FLOP figure
(for the compact layout's (per-column, meta, ldp) tuple: the per-column factor and ldp), `dims` (in the form
`fused.profile_step` reads: a false third entry is no third entry), every scalar argument
(as `fn.argtypes` classifies them) and, for each pointer argument, only whether it is NULL (`0`) or not (`p`).  Two
commits that make the same launches with the same shapes, entries and roofline accounting give byte-identical output, so
a refactor of the host side is checked with `diff` (profiles/launch_trace.txt holds the six configurations: copy this
file onto a checkout of another commit, or point --root at one, to repeat it).

--shape small: the smallest batch tests/test_model_gpu.py runs for the tracker, stepped as that suite steps it (training_loss,
then a plain backward); bench: the default shape of bench.py, stepped as bench.py's eager step does (DataParallelStep: the
backward inside the deferred weight-gradient scope).  Three pairs of 256 / 512 points are NOT a shape for that scope: the
template half of conv_final (96 columns) runs on torch ops, and `fused_heads._submit_jobs` rules out a parameter shared
between a deferred stack and a torch op.
--save: the seeded training step's loss, end points, parameter gradients and running statistics as a torch file.
"""
import argparse
import ctypes
import os
import sys


def _fmt(v):
    return repr(float(v)) if isinstance(v, float) else str(v)


def _line(name, flops, fn, args, dims):
    if isinstance(flops, tuple):
        fl = "percol=%s ldp=%d" % (_fmt(float(flops[0])), flops[2])
    else:
        fl = _fmt(float(flops))
    out = []
    for t, a in zip(fn.argtypes, args):
        if t is ctypes.c_void_p:
            out.append("p" if a else "0")
        elif t in (ctypes.c_float, ctypes.c_double):
            out.append(_fmt(float(a)))
        else:
            out.append(str(int(a)))
    if dims is not None:      # as `fused.profile_step` reads it: (Cin, Cout) and a third entry only when it is true
        dims = tuple(dims[:2]) + ((True,) if len(dims) > 2 and dims[2] else ())
    return "%s %s flops=%s dims=%s args=%s" % (name, fn.__name__, fl, dims, ",".join(out))


def install(sink):
    """wrap `_call` wherever a loaded module of the package holds it; sink(line) receives every launch"""
    from open3dsot_amd import fused
    orig = fused._call

    def traced(name, flops, fn, *args, dims=None):
        sink(_line(name, flops, fn, args, dims))
        return orig(name, flops, fn, *args, dims=dims)
    for mod in list(sys.modules.values()):
        if getattr(mod, "__name__", "").startswith("open3dsot_amd") and getattr(mod, "_call", None) is orig:
            mod._call = traced


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, choices=["BAT", "P2B", "M2TRACK"])
    ap.add_argument("--shape", required=True, choices=["small", "bench"])
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                    help="the checkout whose package is traced (default: this file's)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--save", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from open3dsot_amd import dist as D, fused_heads, fused_pointwise, fused_rows, fused_xcorr, synth, trackers  # noqa: F401
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    if a.model == "M2TRACK":
        from open3dsot_amd import m2track
        model = m2track.M2TRACK().to(dev).train()
        host = synth.make_motion_batch(3, 16, 256) if a.shape == "small" else synth.make_motion_batch(0, 48, 1024)
    else:
        model = trackers.get_model(a.model)().to(dev).train()
        host = synth.make_batch(300, 3, 256, 512) if a.shape == "small" else synth.make_batch(0, 48, 512, 1024)
    batch = synth.to_torch(host, dev)
    trainer = D.DataParallelStep(model, world=1, graph=False) if a.shape == "bench" else None
    lines, ends = [], []
    install(lines.append)
    model.register_forward_hook(lambda mod, inp, out: ends.append(out))      # the end points of both forwards
    lines.append("# %s %s: training step" % (a.model, a.shape))
    if trainer is not None:
        loss = trainer._forward_backward(batch)
    else:
        loss, _ = model.training_loss(batch)
        loss.backward()
    torch.cuda.synchronize()
    saved = {"loss": loss.detach().cpu()}
    saved.update({"grad." + k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None})
    saved.update({"stat." + k: v.detach().cpu() for k, v in model.state_dict().items() if "running" in k or "tracked" in k})
    lines.append("# %s %s: eval forward" % (a.model, a.shape))
    model.eval()
    with torch.no_grad():
        keep = ("points", "candidate_bc") if a.model == "M2TRACK" else None
        model({k: v for k, v in batch.items() if keep is None or k in keep})
    torch.cuda.synchronize()
    if a.save:
        for tag, out in zip(("train", "eval"), ends):
            saved.update({"%s.%s" % (tag, k): v.detach().cpu() for k, v in out.items() if isinstance(v, torch.Tensor)})
        torch.save(saved, a.save)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
