"""Train a tracker from the command line: a thin front of open3dsot_amd.training.fit (the reference's main.py).

  python tools/train.py --model BAT --epoch 2 --batch_size 8                        synthetic tracklets (synth.make_sequence)
  python tools/train.py --model M2TRACK --path /data/kitti --epoch 60 --batch_size 100 --log_dir runs/m2
  python tools/train.py --model BAT --path /data/kitti --checkpoint runs/bat/last.ckpt --epoch 60

--epoch, --batch_size, --save_top_k, --check_val_every_n_epoch, --checkpoint and --log_dir are main.py's arguments; --set
key=value overrides a key of the model's config (lr, wd, optimizer, lr_decay_step, gradient_clip_val, template_size, ...).
With --path the tracklets are datasets.KittiTracklets(path, --train_split / --val_split, --category); without it --tracklets
synthetic sequences of --frames frames are made, the last --val_tracklets of them held out for validation.
Prints the history as one JSON document.
"""
import argparse
import ast
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open3dsot_amd import m2track, sampler, synth, trackers, training  # noqa: E402


def parse_overrides(pairs):
    out = {}
    for pair in pairs:
        key, _, value = pair.partition("=")
        if not key or not _:
            raise SystemExit("--set takes key=value, got %r" % pair)
        try:
            out[key] = ast.literal_eval(value)
        except (ValueError, SyntaxError):
            out[key] = value
    return out


def make_model(name, overrides):
    if name.upper() == "M2TRACK":
        return m2track.M2TRACK(**overrides)
    base = {"BAT": trackers.BAT_CAR, "P2B": trackers.P2B_CAR}[name.upper()]
    return trackers.get_model(name.upper())(trackers.make_config(base, **overrides))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="BAT", choices=["BAT", "P2B", "M2TRACK"])
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--epoch", type=int, default=2)
    ap.add_argument("--save_top_k", type=int, default=-1)
    ap.add_argument("--check_val_every_n_epoch", type=int, default=1)
    ap.add_argument("--checkpoint", default=None, help="resume from this checkpoint (or start from its weights)")
    ap.add_argument("--log_dir", default=None, help="where last.ckpt and the epoch files go (default: nothing is written)")
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE", help="override a config key")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--path", default=None, help="KITTI tracking root (velodyne/, label_02/, calib/)")
    ap.add_argument("--train_split", default="train")
    ap.add_argument("--val_split", default="valid")
    ap.add_argument("--category", default="Car")
    ap.add_argument("--tracklets", type=int, default=4)
    ap.add_argument("--val_tracklets", type=int, default=1)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/train.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    model = make_model(args.model, parse_overrides(args.set)).to(dev).train()
    if args.path is not None:
        from open3dsot_amd import datasets
        train = datasets.KittiTracklets(args.path, args.train_split, category_name=args.category, device=dev)
        val = datasets.KittiTracklets(args.path, args.val_split, category_name=args.category, device=dev)
    else:
        if not 0 <= args.val_tracklets < args.tracklets:
            raise SystemExit("--val_tracklets must be below --tracklets")
        seqs = [synth.make_sequence(1000 * args.seed + i, args.frames, args.points) for i in range(args.tracklets)]
        cut = args.tracklets - args.val_tracklets
        train = sampler.DeviceTracklets([s[0] for s in seqs[:cut]], [s[1] for s in seqs[:cut]], device=dev)
        val = sampler.DeviceTracklets([s[0] for s in seqs[cut:]], [s[1] for s in seqs[cut:]], device=dev) if cut < len(seqs) else None
    history = training.fit(model, train, val, epochs=args.epoch, batch_size=args.batch_size, seed=args.seed,
                           check_val_every_n_epoch=args.check_val_every_n_epoch, ckpt_dir=args.log_dir,
                           save_top_k=args.save_top_k, resume=args.checkpoint)
    print(json.dumps({"model": args.model, "epochs": args.epoch, "batch_size": args.batch_size, "history": history}))


if __name__ == "__main__":
    main()
