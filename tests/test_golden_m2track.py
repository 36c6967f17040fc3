"""M2-Track against the reference's own code: tests/golden/ref_m2track.npz is
produced by tests/golden/make_golden_m2track.py, which runs /root/reference/models/m2track.py (forward and
compute_loss), models/backbone/pointnet.py and the tensor helpers of datasets/points_utils.py.  The
product's mirror (open3dsot_amd/m2track.py, backbone.py, box_utils.py) loads the reference state_dict
with strict=True and must reproduce outputs, losses and BatchNorm running statistics, on the module-by-
module path and on the flat-GEMM path of the per-point stacks."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fixture_io  # noqa: E402
TOL = dict(rtol=2e-4, atol=2e-5)


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_m2track.npz"))


def build(gold, train):
    from open3dsot_amd import m2track
    net = m2track.M2TRACK()
    sd = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd.")}
    net.load_state_dict(sd, strict=True)
    return net.train(train)


def batch(gold):
    return {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("in.")}


@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_m2track_matches_reference(gold, mode, flat):
    from open3dsot_amd import nn_blocks
    was = nn_blocks._FLAT["on"]
    nn_blocks.set_flat_pointwise(flat)
    try:
        net = build(gold, mode == "train")
        b = batch(gold)
        out = net(b)
        ld = net.compute_loss(b, out)
    finally:
        nn_blocks.set_flat_pointwise(was)
    # the heads run BatchNorm1d over a batch of 8 samples: a 1e-7 change of the pooled features (the flat
    # path sums in GEMM order) moves a normalised value by 1e-4; the module-by-module path is bitwise
    # the reference's arithmetic and keeps the tight tolerance
    tol = dict(rtol=2e-3, atol=5e-4) if flat else TOL
    for k in out:
        np.testing.assert_allclose(out[k].detach().numpy(), gold["%s.out.%s" % (mode, k)], err_msg=k, **tol)
    for k in ld:
        assert abs(float(ld[k]) - float(gold["%s.loss.%s" % (mode, k)])) < (1e-3 if flat else 2e-4) * (1 + abs(float(ld[k]))), k
    if mode == "train":
        for k, v in net.state_dict().items():
            if "running" in k:
                np.testing.assert_allclose(v.numpy(), gold["train.sd_after." + k], rtol=1e-4, atol=1e-5, err_msg=k)


def test_box_helpers_match_reference(gold):
    from open3dsot_amd import box_utils
    pts, ref, off = (torch.from_numpy(gold["box.in." + k]) for k in ("pts", "ref", "off"))
    keep = pts.clone()
    np.testing.assert_allclose(box_utils.get_offset_points_tensor(pts, ref, off).numpy(), gold["box.offset_points"], **TOL)
    np.testing.assert_allclose(box_utils.get_offset_box_tensor(ref, off).numpy(), gold["box.offset_box"], **TOL)
    np.testing.assert_allclose(box_utils.remove_transform_points_tensor(pts, ref).numpy(), gold["box.remove_transform"], **TOL)
    assert torch.equal(pts, keep)        # unlike the reference, the inputs are not modified in place


def test_m2track_backward_and_synthetic_contract():
    from open3dsot_amd import m2track, synth
    torch.manual_seed(0)
    net = m2track.M2TRACK().train()
    b = synth.to_torch(synth.make_motion_batch(0, 3, 64))
    assert b["points"].shape == (3, 128, 5) and b["candidate_bc"].shape == (3, 128, 9) and b["seg_label"].dtype == torch.int64
    loss, ld = net.training_loss(b)
    loss.backward()
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


def test_batched_loss_equals_the_term_by_term_reference_form():
    """M2TRACK.compute_loss (four stacked (centre, angle) pairs, one dot product for the total) against
    compute_loss_reference (models/m2track.py:153-231 term by term), batch 48, every configuration switch: each entry of
    the dict and every gradient to fp32 rounding"""
    import itertools
    import torch
    from open3dsot_amd import m2track, synth
    batch = synth.to_torch(synth.make_motion_batch(11, 48, 256))
    for cls, second, prev in itertools.product([True, False], repeat=3):
        torch.manual_seed(3)
        model = m2track.M2TRACK(use_motion_cls=cls, use_second_stage=second, use_prev_refinement=prev).train()
        out = model(batch)
        new, ref = model.compute_loss(batch, out), model.compute_loss_reference(batch, out)
        assert set(new) == set(ref)
        for k in ref:
            assert abs(float(new[k].detach()) - float(ref[k].detach())) <= 2e-6 * (1 + abs(float(ref[k].detach()))), (k, cls, second, prev)
        params = [p for p in model.parameters()]
        gn = torch.autograd.grad(new["loss_total"], params, retain_graph=True, allow_unused=True)
        gr = torch.autograd.grad(ref["loss_total"], params, allow_unused=True)
        gmax = max(float(b.abs().max()) for b in gr if b is not None)     # biases in front of a BatchNorm: true gradient 0, computed noise
        for a, b in zip(gn, gr):
            assert (a is None) == (b is None)
            if a is not None:
                assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-6 * gmax


def test_rotz_as_one_gemm_is_the_stacked_matrix_bit_for_bit():
    import torch
    from open3dsot_amd import box_utils
    t = torch.linspace(-7.0, 7.0, 97, requires_grad=True)
    a, b = box_utils.rotz_batch_tensor(t), box_utils.rotz_batch_tensor_stacked(t)
    assert a.shape == (97, 3, 3) and torch.equal(a, b)
    g = torch.randn(97, 3, 3, generator=torch.Generator().manual_seed(0))
    ga, = torch.autograd.grad(a, t, g)
    gb, = torch.autograd.grad(b, t, g)
    assert float((ga - gb).abs().max()) <= 1e-6
    assert torch.equal(box_utils.rotz_batch_tensor(t.detach().double()), box_utils.rotz_batch_tensor_stacked(t.detach().double()))


@pytest.fixture(scope="module")
def gold64():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_m2track_f64.npz"))


def scale_err(a, b):
    """max |a - b| relative to the scale of b (b: the fp64 truth)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def assert_within_fp64_yardstick(out, ld, sd_after, ref32, gold64, tag, mode, report=None):
    """The reference's own M2TRACK evaluated in DOUBLE precision (hard-mask decisions replayed from its fp32 run:
    tests/golden/make_golden_m2track.py, third fixture) is the truth; the reference's own fp32 run's distance to it is the
    yardstick.  Every output / loss term / running statistic of the run under test must be within
    max(1e-4 (1e-5 for the running statistics), 3 x yardstick) of the truth, relative to the tensor's scale -- the rule
    tests/test_golden_trackers_b8.py holds BAT / P2B to, instead of a bare tolerance."""
    pre = "%s.%s." % (tag, mode)
    rows = []
    for k, v in out.items():
        truth = gold64[pre + "out." + k]
        err, yard = scale_err(v.detach().cpu().numpy(), truth), scale_err(ref32["%s.out.%s" % (mode, k)], truth)
        rows.append(("out." + k, err, yard, max(1e-4, 3 * yard)))
    for k, v in ld.items():
        truth = float(gold64[pre + "loss." + k])
        err = abs(float(v) - truth) / (1 + abs(truth))
        yard = abs(float(ref32["%s.loss.%s" % (mode, k)]) - truth) / (1 + abs(truth))
        rows.append(("loss." + k, err, yard, max(1e-4, 3 * yard)))
    for k, v in (sd_after or {}).items():
        if "running" in k:
            truth = gold64["%s.train.sd_after.%s" % (tag, k)]
            err, yard = scale_err(v.cpu().numpy(), truth), scale_err(ref32["train.sd_after." + k], truth)
            rows.append(("sd." + k, err, yard, max(1e-5, 3 * yard)))
    if report is not None:
        report.extend(rows)
    bad = [r for r in rows if not r[1] <= r[3]]
    assert not bad, ["%s: err %.2e, reference fp32 vs fp64 %.2e, bound %.2e" % r for r in bad]
    return rows


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("tag", ["b8", "b48"])
def test_m2track_flat_path_within_the_references_fp64_yardstick(gold, gold48, gold64, tag, mode):
    """CPU twin of tests/test_golden_m2track_gpu.py::test_gpu_m2track_within_the_references_fp64_yardstick: the flat-GEMM
    host path (torch ops) against the double-precision evaluation of the reference's own model"""
    assert int(gold64["%s.%s.fp64_would_flip" % (tag, mode)].sum()) == 0      # no hard-mask decision near a tie in the fixtures
    net = build(gold, mode == "train")
    ref32 = gold if tag == "b8" else gold48
    b = batch(ref32)
    out = net(b)
    ld = net.compute_loss(b, out)
    if tag == "b48" and mode == "eval":        # the batch-48 fixture keeps three eval outputs only
        out = {k: v for k, v in out.items() if "eval.out." + k in ref32.files}
    rows = assert_within_fp64_yardstick(out, ld, net.state_dict() if mode == "train" else None, ref32, gold64, tag, mode)
    worst = max(rows, key=lambda r: r[1] / r[3])
    print("%s %s worst: %s err %.2e (reference fp32: %.2e, bound %.2e)" % ((tag, mode) + worst))


def assert_grads_within_fp64_yardstick(named_grads, goldg, tag, report=None):
    """tests/golden/ref_m2track_grad.npz (generator: tests/golden/make_golden_m2track_grad.py): the gradient of the reference's
    own M2TRACK loss (models/m2track.py:73-231) evaluated in DOUBLE precision, hard masks replayed, with the reference's own
    fp32 gradient's distance to it stored per key.  Every parameter's gradient of the run under test must be within
    max(2e-2, 3 x that yardstick) of the truth in relative L2 -- the rule tests/test_golden_trackers_b8.py holds BAT / P2B
    to -- and so must the whole vector.  Keys whose true gradient is below 1e-6 of the whole norm (biases in front of a
    BatchNorm: true gradient 0) only enter the whole-vector bound.  Tensors above 40 000 elements are stored as the
    deterministic sample flat[::stride]; the whole-vector error weighs a sampled key's squared error by its stride."""
    gn = float(goldg[tag + ".gradnorm64"])
    keys = sorted(k[len(tag) + 8:] for k in goldg.files if k.startswith(tag + ".grad64."))
    assert set(keys) == set(named_grads), sorted(set(keys) ^ set(named_grads))
    rows, whole = [], 0.0
    for k in keys:
        stride = int(goldg["%s.stride.%s" % (tag, k)])
        truth = goldg["%s.grad64.%s" % (tag, k)].astype(np.float64)
        got = named_grads[k].detach().cpu().double().flatten()[::stride].numpy()
        assert got.shape == truth.shape, (k, got.shape, truth.shape)
        d2 = float(((got - truth) ** 2).sum())
        whole += stride * d2
        if float(goldg["%s.norm64.%s" % (tag, k)]) <= 1e-6 * gn:
            continue
        yard = float(goldg["%s.ref32err.%s" % (tag, k)])
        rows.append((k, d2 ** 0.5 / float(np.linalg.norm(truth)), yard, max(2e-2, 3 * yard)))
    yard = float(goldg[tag + ".ref32err_whole"])
    rows.append(("WHOLE", whole ** 0.5 / gn, yard, max(2e-2, 3 * yard)))
    if report is not None:
        report.extend(rows)
    bad = [r for r in rows if not r[1] <= r[3]]
    for r in bad:
        print("   BAD %-50s err %.3e | reference fp32 vs fp64 %.3e | bound %.3e" % r)
    assert not bad, ["%s: err %.2e, reference fp32 vs fp64 %.2e, bound %.2e" % r for r in bad]
    return rows


@pytest.fixture(scope="module")
def goldg():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_m2track_grad.npz"))


class replay_hard_masks:
    """Context manager: the two hard-mask decisions of an M2-Track forward (torch.argmax of the segmentation logits per point
    and of the motion-state logits per cloud, models/m2track.py:95,113) are REPLAYED from the reference's fp32 run stored in
    ref_m2track_grad.npz, exactly as the fixture's generator replays them into the reference's fp64 run: the gradient of the
    run under test is then the gradient of the SAME graph.  A decision of the run under test that differs from the stored
    one is only legitimate where the reference's own fp64 logits are within rounding of a tie: `flips` lists
    (which, how many differ, largest fp64 margin among them) and __exit__ asserts that margin <= TIE."""
    TIE = 2e-3

    def __init__(self, goldg, tag):
        self.g, self.tag, self.flips, self.calls = goldg, tag, [], 0

    def __enter__(self):
        self.real = torch.argmax
        torch.argmax = self._replay
        return self

    def _replay(self, x, *a, **k):
        mine = self.real(x, *a, **k)
        which = ("seg", "motion")[self.calls]
        self.calls += 1
        if which == "seg":
            bits = np.unpackbits(self.g[self.tag + ".mask.seg"])[:mine.numel()]
            margin = self.g[self.tag + ".margin.seg"].astype(np.float32)
        else:
            bits, margin = self.g[self.tag + ".mask.motion"], self.g[self.tag + ".margin.motion"]
        theirs = torch.from_numpy(bits.astype(np.int64)).reshape(mine.shape).to(mine.device)
        differ = (mine != theirs).reshape(-1).cpu().numpy()
        self.flips.append((which, int(differ.sum()), float(margin[differ].max()) if differ.any() else 0.0))
        return theirs

    def __exit__(self, *exc):
        torch.argmax = self.real
        if exc[0] is None:
            assert self.calls == 2, self.calls
            assert all(m <= self.TIE for _, _, m in self.flips), ("a hard-mask decision differs from the reference's away from a tie", self.flips)
        return False


def row_relu_flips(net, b, goldg, tag):
    """The ROUTING through the ReLUs behind the heads' Linear -> BatchNorm1d rows (122 880 units at batch 48) is discrete.  A
    second forward of `net` with the row stacks as the torch modules they are (fused_rows off; hooks on every nn.ReLU fed a
    2-D tensor) is compared with the reference's fp64 inputs of the same ReLUs stored in ref_m2track_grad.npz:
    -> [(module, units routed the other way, largest |z_fp64| / rms(z) among them)] for the modules with at least one."""
    from open3dsot_amd import fused_rows
    got, hooks = {}, []
    for name, mod in net.named_modules():
        if isinstance(mod, torch.nn.ReLU):
            def rec(m, inp, out, _n=name):
                if inp[0].dim() == 2:
                    got[_n] = inp[0].detach().cpu().numpy()
            hooks.append(mod.register_forward_hook(rec))
    was = fused_rows._ON["on"]
    fused_rows.set_fused_rows(False)
    try:
        with torch.no_grad(), replay_hard_masks(goldg, tag):
            net(b)
    finally:
        fused_rows.set_fused_rows(was)
        for h in hooks:
            h.remove()
    want = {k[len(tag) + 6:]: goldg[k] for k in goldg.files if k.startswith(tag + ".relu.")}
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    flips = []
    for name, z in want.items():
        differ = (got[name] > 0) != (z > 0)
        if differ.any():
            flips.append((name, int(differ.sum()), float(np.abs(z[differ]).max() / np.sqrt((z.astype(np.float64) ** 2).mean()))))
    return flips


def assert_gradient_direction(named_grads, goldg, tag, cos_min=0.995, ratio_tol=3e-2):
    """the loose, routing-tolerant form of assert_grads_within_fp64_yardstick: per key the DIRECTION and the NORM of the
    gradient (a mis-wired or mis-scaled gradient is off by tens of percent; one re-routed near-tie ReLU unit moves a key by
    a few percent: cos 0.9993 on the worst key of the case that motivated this, profiles/r06_m2track_gradient_pin.txt)"""
    gn = float(goldg[tag + ".gradnorm64"])
    rows = []
    for k in sorted(k[len(tag) + 8:] for k in goldg.files if k.startswith(tag + ".grad64.")):
        if float(goldg["%s.norm64.%s" % (tag, k)]) <= 1e-6 * gn:
            continue
        stride = int(goldg["%s.stride.%s" % (tag, k)])
        truth = goldg["%s.grad64.%s" % (tag, k)].astype(np.float64)
        got = named_grads[k].detach().cpu().double().flatten()[::stride].numpy()
        cos = float(got @ truth / (np.linalg.norm(got) * np.linalg.norm(truth)))
        rows.append((k, cos, float(np.linalg.norm(got) / np.linalg.norm(truth))))
    bad = [r for r in rows if not (r[1] >= cos_min and abs(r[2] - 1) <= ratio_tol)]
    assert not bad, bad
    return rows


def grad_fixture_batch(tag, gold, gold48, goldg):
    """inputs of a tag of ref_m2track_grad.npz: the stored ones of the two older fixtures, or (benchmarked batch, 48 x 2 048
    points: not stored) regenerated from open3dsot_amd/synth.py and checked against the digest the generator stored"""
    if tag != "b48x2048":
        return batch(gold if tag == "b8" else gold48)
    import hashlib
    from open3dsot_amd import synth
    bt = synth.make_motion_batch(211, 48, point_sample_size=1024)
    h = hashlib.sha256()
    for k in sorted(bt):
        h.update(k.encode())
        h.update(np.ascontiguousarray(bt[k]).tobytes())
    assert h.digest() == goldg[tag + ".in_sha256"].tobytes(), "synth.make_motion_batch(211, 48, 1024) is not the generator's batch"
    return synth.to_torch(bt)


@pytest.mark.parametrize("tag", ["b8", "b48", "b48x2048"])
def test_m2track_flat_path_gradients_within_the_references_fp64_yardstick(gold, gold48, goldg, tag):
    """CPU twin of tests/test_golden_m2track_gpu.py::test_gpu_m2track_gradients_...: the host mirror's autograd gradient of
    loss_total against the reference model's own fp64 gradient, per parameter"""
    net = build(gold, True)
    b = grad_fixture_batch(tag, gold, gold48, goldg)
    with replay_hard_masks(goldg, tag) as rp:
        ld = net.compute_loss(b, net(b))
    print("hard-mask decisions differing from the reference's fp32 run (replayed):", rp.flips)
    assert abs(float(ld["loss_total"].detach()) - float(goldg[tag + ".loss64"])) <= 1e-4 * (1 + float(goldg[tag + ".loss64"]))
    ld["loss_total"].backward()
    rows = assert_grads_within_fp64_yardstick({k: p.grad for k, p in net.named_parameters()}, goldg, tag)
    worst = max(rows, key=lambda r: r[1] / r[3])
    print("%s gradients, %d keys, worst: %s err %.2e (reference fp32: %.2e, bound %.2e); whole %.2e"
          % ((tag, len(rows)) + worst + (rows[-1][1],)))


@pytest.fixture(scope="module")
def gold48():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_m2track_b48.npz"))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_m2track_matches_reference_at_batch48(gold, gold48, mode):
    """the reference model (state dict of ref_m2track.npz) on 48 frame pairs -- the benchmarked batch, where the heads'
    BatchNorm1d over the batch is well conditioned: every loss term of the flat-GEMM path within 1e-4"""
    net = build(gold, mode == "train")
    b = batch(gold48)
    out = net(b)
    ld = net.compute_loss(b, out)
    for k in ld:
        want = float(gold48["%s.loss.%s" % (mode, k)])
        assert abs(float(ld[k]) - want) <= 1e-4 * (1 + abs(want)), (k, float(ld[k]), want)
    for k in ("estimation_boxes", "motion_cls", "estimation_boxes_prev"):
        np.testing.assert_allclose(out[k].detach().numpy(), gold48["%s.out.%s" % (mode, k)], err_msg=k, rtol=1e-3, atol=2e-4)
    if mode == "train":
        for k, v in net.state_dict().items():
            if "running" in k:
                np.testing.assert_allclose(v.numpy(), gold48["train.sd_after." + k], rtol=1e-4, atol=1e-5, err_msg=k)


def test_motion_merge_closed_form_backward_equals_autograd_of_the_reference_chain():
    """csrc/boxcloud.hip::motion_merge_bwd_kernel does not differentiate the reference's chain step by step: z rotations commute,
    so the previous frame's half collapses to Rz(-prev_t)(x - prev_c) and the current half is Rz(-aux_t)(x - aux_c); four
    per-cloud sums and the chain through aux = prev (+) motion give both gradients.  The same closed form in torch (fp64, CPU)
    against autograd of get_offset_box_tensor / get_offset_points_tensor / remove_transform_points_tensor
    (datasets/points_utils.py:390-452 as mirrored in open3dsot_amd/box_utils.py): 1e-12."""
    from open3dsot_amd import box_utils
    g = torch.Generator().manual_seed(3)
    B, N = 6, 64
    pts = torch.randn(B, 4, N, generator=g, dtype=torch.float64) * 2
    prev = (torch.randn(B, 4, generator=g, dtype=torch.float64) * 0.7).requires_grad_()
    mo = (torch.randn(B, 4, generator=g, dtype=torch.float64) * 0.5).requires_grad_()
    gm = torch.randn(B, 3, N, generator=g, dtype=torch.float64)
    ga = torch.randn(B, 4, generator=g, dtype=torch.float64)
    merged, aux = box_utils.motion_merge_reference(pts, prev, mo)
    ((merged * gm).sum() + (aux * ga).sum()).backward()

    def rot(t, x, y):                 # Rz(t) (x, y)
        c, s = torch.cos(t), torch.sin(t)
        return c * x - s * y, s * x + c * y

    with torch.no_grad():
        pc, pt, mc, mt = prev[:, :3], prev[:, 3], mo[:, :3], mo[:, 3]
        ax, ay = rot(pt, mc[:, 0], mc[:, 1])
        ac = torch.stack([ax + pc[:, 0], ay + pc[:, 1], mc[:, 2] + pc[:, 2]], 1)
        at = pt + mt
        # forward identity: the previous half never sees the motion
        h = N // 2
        y0 = rot(-pt[:, None], pts[:, 0, :h] - pc[:, 0:1], pts[:, 1, :h] - pc[:, 1:2])
        assert float((merged[:, 0, :h] - y0[0]).abs().max()) < 1e-12 and float((merged[:, 1, :h] - y0[1]).abs().max()) < 1e-12
        sums = []
        for (c, t, sl) in ((pc, pt, slice(0, h)), (ac, at, slice(h, N))):
            dx, dy = pts[:, 0, sl] - c[:, 0:1], pts[:, 1, sl] - c[:, 1:2]
            cs, sn = torch.cos(t)[:, None], torch.sin(t)[:, None]
            tx, ty = -sn * dx + cs * dy, -cs * dx - sn * dy          # d/dtheta of Rz(-theta)(d)
            S = gm[:, :, sl].sum(2)
            T = (gm[:, 0, sl] * tx + gm[:, 1, sl] * ty).sum(1)
            sums.append((S, T))
        (S0, T0), (S1, T1) = sums
        gpx, gpy = rot(pt, -S0[:, 0], -S0[:, 1])
        gax, gay = rot(at, -S1[:, 0], -S1[:, 1])
        gac = torch.stack([gax, gay, -S1[:, 2]], 1) + ga[:, :3]
        gat = T1 + ga[:, 3]
        gmx, gmy = rot(-pt, gac[:, 0], gac[:, 1])
        g_motion = torch.stack([gmx, gmy, gac[:, 2], gat], 1)
        dax = -torch.sin(pt) * mc[:, 0] - torch.cos(pt) * mc[:, 1]
        day = torch.cos(pt) * mc[:, 0] - torch.sin(pt) * mc[:, 1]
        g_prev = torch.stack([gpx + gac[:, 0], gpy + gac[:, 1], -S0[:, 2] + gac[:, 2], T0 + gat + gac[:, 0] * dax + gac[:, 1] * day], 1)
    assert float((g_motion - mo.grad).abs().max()) < 1e-12 * (1 + float(mo.grad.abs().max()))
    assert float((g_prev - prev.grad).abs().max()) < 1e-12 * (1 + float(prev.grad.abs().max()))


FLAG_VARIANTS = {
    "plain": dict(box_aware=False, use_motion_cls=False, use_second_stage=False, use_prev_refinement=False),
    "no_bc": dict(box_aware=False, use_motion_cls=True, use_second_stage=True, use_prev_refinement=True),
    "no_cls_no_prev": dict(box_aware=True, use_motion_cls=False, use_second_stage=True, use_prev_refinement=False),
    "one_stage": dict(box_aware=True, use_motion_cls=True, use_second_stage=False, use_prev_refinement=True),
}


def build_variant(name):
    """the mirror with the variant's flags and the storage-free weights the generator gave the reference's class"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from det_init import fill_by_module_type
    from open3dsot_amd import m2track
    torch.manual_seed(5)
    return fill_by_module_type(m2track.M2TRACK(**FLAG_VARIANTS[name]), seed=17)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", sorted(FLAG_VARIANTS))
def test_m2track_flag_variants_match_the_reference_class(name, mode):
    """tests/golden/ref_m2track_flags.npz: the reference's own M2TRACK built with box_aware / use_motion_cls /
    use_second_stage / use_prev_refinement switched (models/m2track.py:22-71), forward and compute_loss -- the mirror has the
    same parameters (count), the same output keys, outputs and loss terms (module-by-module path: the reference's arithmetic)"""
    from open3dsot_amd import nn_blocks
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ref_m2track_flags.npz"))
    net = build_variant(name).train(mode == "train")
    assert sum(p.numel() for p in net.parameters()) == int(gold[name + ".nparams"])
    b = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("in.")}
    was = nn_blocks._FLAT["on"]
    nn_blocks.set_flat_pointwise(False)
    try:
        out = net(b)
        ld = net.compute_loss(b, out)
    finally:
        nn_blocks.set_flat_pointwise(was)
    pre = "%s.%s." % (name, mode)
    want_out = {k[len(pre) + 4:] for k in gold.files if k.startswith(pre + "out.")}
    want_loss = {k[len(pre) + 5:] for k in gold.files if k.startswith(pre + "loss.")}
    assert set(out) == want_out and set(ld) == want_loss, (sorted(out), sorted(want_out), sorted(ld), sorted(want_loss))
    for k in out:
        np.testing.assert_allclose(out[k].detach().numpy(), gold[pre + "out." + k], err_msg=k, **TOL)
    for k in ld:
        assert abs(float(ld[k]) - float(gold[pre + "loss." + k])) < 2e-4 * (1 + abs(float(ld[k]))), (k, float(ld[k]))


def test_m2_loss_closed_form_gradients_equal_autograd_of_compute_loss_reference():
    """csrc/loss.hip::m2_loss_grads_kernel writes the gradients of the weighted total in closed form (softmax - one-hot for the
    two cross entropies, clamp(d, -1, 1) for smooth-L1, cos(t) * clamp(sin t - sin t*) for the angle terms, the motion pair over
    state / (sum state + 1e-6)).  The same formulas in torch (fp64, CPU) against autograd of M2TRACK.compute_loss_reference
    (models/m2track.py:153-231 restated term by term): 1e-12."""
    from open3dsot_amd import m2track
    g = torch.Generator().manual_seed(8)
    B, N, K = 6, 32, 9
    model = m2track.M2TRACK()
    c = model.config
    f64 = torch.float64
    box = torch.randn(B, 4, generator=g, dtype=f64)
    out = {"seg_logits": torch.randn(B, 2, N, generator=g, dtype=f64) * 2, "pred_bc": torch.randn(B, N, K, generator=g, dtype=f64) * 1.5,
           "motion_cls": torch.randn(B, 2, generator=g, dtype=f64), "motion_pred": torch.randn(B, 4, generator=g, dtype=f64) * 1.5,
           "aux_estimation_boxes": box + torch.randn(B, 4, generator=g, dtype=f64) * 0.8,
           "estimation_boxes": box + torch.randn(B, 4, generator=g, dtype=f64) * 1.5,
           "estimation_boxes_prev": torch.randn(B, 4, generator=g, dtype=f64) * 1.2}
    out = {k: v.requires_grad_() for k, v in out.items()}
    data = {"seg_label": (torch.rand(B, N, generator=g) < 0.3).long(), "prev_bc": torch.randn(B, N // 2, K, generator=g, dtype=f64),
            "this_bc": torch.randn(B, N // 2, K, generator=g, dtype=f64), "motion_state_label": (torch.rand(B, generator=g) < 0.5).long(),
            "motion_label": torch.randn(B, 4, generator=g, dtype=f64), "box_label": box,
            "box_label_prev": torch.randn(B, 4, generator=g, dtype=f64)}
    model.compute_loss_reference(data, out)["loss_total"].backward()
    with torch.no_grad():
        def sl1g(d):
            return d.clamp(-1, 1)

        def box_grad(pred, lab, wrow):              # wrow (B,): weight of every sample's (centre mean over 3, angle) pair
            gcen = c.center_weight * wrow[:, None] / 3.0 * sl1g(pred[:, :3] - lab[:, :3])
            gang = c.angle_weight * wrow * torch.cos(pred[:, 3]) * sl1g(torch.sin(pred[:, 3]) - torch.sin(lab[:, 3]))
            return torch.cat([gcen, gang[:, None]], 1)
        even = torch.full((B,), 1.0 / B, dtype=f64)
        st = data["motion_state_label"].to(f64)
        # (the reference adds 1e-6 to the INTEGER sum of the state labels: the denominator is a float32 -- models/m2track.py:199)
        moving = st / (data["motion_state_label"].sum() + 1e-6)
        cw = torch.tensor([0.5, 2.0], dtype=f64)[data["seg_label"]]                        # (B,N)
        p = torch.softmax(out["seg_logits"], 1)
        onehot = torch.nn.functional.one_hot(data["seg_label"], 2).permute(0, 2, 1).to(f64)
        g_seg = c.seg_weight * cw[:, None, :] / cw.sum() * (p - onehot)
        pm = torch.softmax(out["motion_cls"], 1)
        g_mcls = c.motion_cls_seg_weight / B * (pm - torch.nn.functional.one_hot(data["motion_state_label"], 2).to(f64))
        bc_label = torch.cat([data["prev_bc"], data["this_bc"]], 1)
        g_bc = c.bc_weight / (B * N * K) * sl1g(out["pred_bc"] - bc_label)
        want = {"seg_logits": g_seg, "motion_cls": g_mcls, "pred_bc": g_bc,
                "motion_pred": box_grad(out["motion_pred"], data["motion_label"], moving),
                "aux_estimation_boxes": box_grad(out["aux_estimation_boxes"], box, even),
                "estimation_boxes": box_grad(out["estimation_boxes"], box, even),
                "estimation_boxes_prev": box_grad(out["estimation_boxes_prev"], data["box_label_prev"], even)}
    for k, w in want.items():
        err = float((out[k].grad - w).abs().max())
        assert err < 1e-12 * (1 + float(w.abs().max())), (k, err)
