#!/usr/bin/env python
"""GPU diagnostic (round 6): M2-Track gradient at the benchmarked batch (48 x 2 048 points) against the reference's fp64
gradient (tests/golden/ref_m2track_grad.npz) with the product's test hooks switched one at a time -- which component carries
the 2.7e-2 the pinned-gradient test found (48 x 512 points: 4.5e-3)?"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import test_golden_m2track as T
from open3dsot_amd import backbone, box_utils, fused_loss, fused_pointwise, fused_rows, m2track, nn_blocks

gold = T.fixture_io.load(os.path.join(ROOT, "tests/golden/ref_m2track.npz"))
gold48 = T.fixture_io.load(os.path.join(ROOT, "tests/golden/ref_m2track_b48.npz"))
goldg = T.fixture_io.load(os.path.join(ROOT, "tests/golden/ref_m2track_grad.npz"))


def run(tag, label, dev="cuda"):
    net = m2track.M2TRACK()
    net.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd.")}, strict=True)
    net = net.to(dev).train()
    b = {k: v.to(dev) for k, v in T.grad_fixture_batch(tag, gold, gold48, goldg).items()}
    with T.replay_hard_masks(goldg, tag):
        ld = net.compute_loss(b, net(b))
    ld["loss_total"].backward()
    rows = []
    try:
        T.assert_grads_within_fp64_yardstick({k: p.grad for k, p in net.named_parameters()}, goldg, tag, rows)
    except AssertionError:
        pass
    errs = {r[0]: r[1] for r in rows}
    print("%-10s %-34s whole %.2e | box_mlp.0.weight %.2e | seg.seq_per_point.0.0.weight %.2e | mini_pointnet.features.0.weight %.2e | loss %.6f"
          % (tag, label, errs["WHOLE"], errs["box_mlp.0.weight"], errs["seg_pointnet.seq_per_point.0.0.weight"],
             errs["mini_pointnet.features.0.weight"], float(ld["loss_total"])), flush=True)


import contextlib, io
for tag in ("b48", "b48x2048"):
    with contextlib.redirect_stdout(io.StringIO()) as _:
        pass
    run(tag, "default")
    fused_loss.set_fused_loss(False); run(tag, "fused loss off"); fused_loss.set_fused_loss(True)
    fused_rows.set_fused_rows(False); run(tag, "fused rows off"); fused_rows.set_fused_rows(True)
    backbone.set_cloud_bias(False); run(tag, "cloud bias off"); backbone.set_cloud_bias(True)
    fused_pointwise._POOLED_GMAX["on"] = False; run(tag, "pooled gmax off"); fused_pointwise._POOLED_GMAX["on"] = True
    backbone.set_fused_pointwise(False); run(tag, "fused pointwise off (torch GPU)"); backbone.set_fused_pointwise(True)
    nn_blocks.set_flat_pointwise(False); run(tag, "module path (torch GPU)"); nn_blocks.set_flat_pointwise(True)
