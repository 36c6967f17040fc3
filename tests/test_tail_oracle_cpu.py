"""tests/tail_oracle.py without a GPU:
  * every function against what the project treats as specification, in fp64 to 1e-12: trackers.{BAT,P2B}.compute_loss and
    M2TRACK.compute_loss_reference (all 16 flag combinations) under autograd, torch.optim.Adam over 3 steps, box_utils'
    motion_merge_reference and get_offset_box_tensor_reference under autograd, the three torch lines of the vote head's glue,
    numpy.argmax;
  * the bounds of tests/test_tail_kernels_gpu.py on its own input sets: the oracle's formulas evaluated in numpy float32 stay
    within them (ratio <= 1), no proposal's distance sits within 1e-5 of a threshold, and on the exact leg float32 gives the
    fp64 value bit for bit (every product and partial sum is representable), fl(1/3) included;
  * refusals: one per clause of the `if` at the top of the ten entry points, each O3D_EINVAL before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

import tail_oracle as O
from test_rows_kernels_gpu import Randn, compare

TOL = 1e-12
EINVAL = -1
FLOOR = 2.0 ** -126 / O.E24


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.abs(a - b).max(initial=0.0) <= TOL * (1 + np.abs(b).max(initial=0.0))


def t64(a, grad=False):
    return torch.from_numpy(np.array(a, np.float64)).requires_grad_(grad)


def within(name, got, ref, ref_abs, n):
    ref_abs = np.asarray(ref_abs, np.float64) + 0.0 * np.asarray(ref, np.float64)
    compare(name, np.asarray(got, np.float64), ref, np.where(ref_abs > 0, ref_abs + FLOOR, 0.0), n, False, {})


# ---- ties to the specification -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from open3dsot_amd import m2track, trackers
    return trackers.BAT(), trackers.P2B(), m2track.M2TRACK()


@pytest.fixture
def all_double(monkeypatch):
    """The loss specifications hold two casts that are no-ops in fp32 production but round a denominator to fp32 when the
    inputs are fp64: `(dist < 0.3).float()` and `integer count + 1e-6` (the default dtype).  Here both give fp64, so that the
    specification is evaluated in fp64 throughout."""
    monkeypatch.setattr(torch.Tensor, "float", lambda self: self.double())
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


@pytest.mark.parametrize("case", O.TRACK_ROUNDED + O.TRACK_EXACT[:3], ids=str)
@pytest.mark.parametrize("with_bc", (True, False), ids=("BAT", "P2B"))
def test_track_loss_matches_compute_loss_under_autograd(models, all_double, case, with_bc):
    seed, shape, kind = case
    if shape[0] * shape[1] > 20000:
        shape = (7, 64, 64, 9)
    i = O.track_inputs(Randn(seed) if seed < 1000 else O.Dyadic(seed), *shape, kind=kind)
    model = models[0] if with_bc else models[1]
    cla, vote, boxes, bcp = t64(i.cla, True), t64(i.vote, True), t64(i.boxes, True), t64(i.bc_pred, True)
    data = {"seg_label": t64(i.seg), "box_label": t64(i.box_label), "points2cc_dist_s": t64(i.bc_label)}
    out = {"estimation_boxes": boxes, "estimation_cla": cla, "center_xyz": t64(i.centers), "vote_xyz": vote, "pred_search_bc": bcp}
    ld = model.compute_loss(data, out)
    w = O.TRACK_W
    total = (ld["loss_objective"] * w[0] + ld["loss_box"] * w[1] + ld["loss_seg"] * w[2] + ld["loss_vote"] * w[3] +
             (ld["loss_bc"] * w[4] if with_bc else 0.0))
    total.backward()
    r = O.track_loss(*O.track_args(i, with_bc), w)
    want = [total, ld["loss_objective"], ld["loss_box"], ld["loss_seg"], ld["loss_vote"], ld["loss_bc"] if with_bc else torch.zeros(())]
    assert close(r.losses, [float(x.detach()) for x in want])
    assert close(r.g_cla, cla.grad.numpy()) and close(r.g_vote, vote.grad.numpy()) and close(r.g_boxes, boxes.grad.numpy())
    if with_bc:
        assert close(r.g_bc, bcp.grad.numpy())
    else:
        assert r.g_bc is None and bcp.grad is None


@pytest.mark.parametrize("kind", ("plain", "still"))
@pytest.mark.parametrize("flags", O.M2_FLAGS, ids=lambda f: "bc%d_cls%d_est%d_prev%d" % f)
def test_m2track_loss_matches_compute_loss_reference_under_autograd(models, all_double, flags, kind):
    from types import SimpleNamespace
    model = models[2]
    bc, cls, est, prev = flags
    model.box_aware, model.use_motion_cls, model.use_second_stage, model.use_prev_refinement = map(bool, flags)
    w = O.M2_W
    model.config = SimpleNamespace(center_weight=w[0], angle_weight=w[1], seg_weight=w[2], bc_weight=w[3], motion_cls_seg_weight=w[4])
    B, N, K = 5, 6, 9
    full = O.m2_inputs(Randn(77 + sum(flags)), B, N, K, (1, 1, 1, 1), kind)
    i = O.m2_inputs(Randn(77 + sum(flags)), B, N, K, flags, kind)
    leaf = {k: t64(getattr(full, k), True) for k in ("seg_logits", "bc_pred", "motion_cls", "motion", "aux", "est", "prev")}
    data = {"box_label": t64(i.box_lab), "box_label_prev": t64(i.prev_lab), "motion_label": t64(i.motion_lab),
            "motion_state_label": torch.from_numpy(full.state), "seg_label": torch.from_numpy(i.seg_label),
            "prev_bc": t64(full.bc_a), "this_bc": t64(full.bc_b)}
    out = {"aux_estimation_boxes": leaf["aux"], "motion_pred": leaf["motion"], "seg_logits": leaf["seg_logits"],
           "motion_cls": leaf["motion_cls"], "estimation_boxes": leaf["est"], "estimation_boxes_prev": leaf["prev"],
           "pred_bc": leaf["bc_pred"]}
    ld = model.compute_loss_reference(data, out)
    ld["loss_total"].backward()
    r = O.m2track_loss(*O.m2_args(i), w)
    names = ("loss_total", "loss_motion_cls", "loss_center", "loss_angle", "loss_center_prev", "loss_angle_prev", "loss_seg",
             "loss_center_aux", "loss_center_motion", "loss_angle_aux", "loss_angle_motion", "loss_bc")
    assert close(r.losses, [float(ld[n]) if n in ld else 0.0 for n in names])
    on = {"g_seg": 1, "g_bc": bc, "g_mcls": cls, "g_motion": 1, "g_aux": 1, "g_est": est, "g_prev": prev}
    src = {"g_seg": "seg_logits", "g_bc": "bc_pred", "g_mcls": "motion_cls", "g_motion": "motion", "g_aux": "aux", "g_est": "est",
           "g_prev": "prev"}
    for g in O.M2_GRADS:
        if on[g]:
            assert close(getattr(r, g), leaf[src[g]].grad.numpy()), g
        else:
            assert getattr(r, g) is None and leaf[src[g]].grad is None, g


@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_adam_step_matches_torch_adam_over_three_steps(wd):
    draw = Randn(5)
    h = O.ADAM_ROUNDED
    p = torch.nn.Parameter(t64(draw.val((300,))))
    opt = torch.optim.Adam([p], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=wd)
    pn, m, v = p.detach().numpy().copy(), np.zeros(300), np.zeros(300)
    for t in (1, 2, 3):
        g = draw.val((300,))
        p.grad = t64(g)
        opt.step()
        r = O.adam_step(pn, m, v, g, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, 1 - h["beta1"] ** t, 1 - h["beta2"] ** t)
        pn, m, v = r.p, r.m, r.v
        state = opt.state[p]
        assert close(pn, p.detach().numpy()) and close(m, state["exp_avg"].numpy()) and close(v, state["exp_avg_sq"].numpy())


@pytest.mark.parametrize("with_prev", (True, False))
@pytest.mark.parametrize("with_gaux", (True, False))
@pytest.mark.parametrize("N", (2, 6, 258))
def test_motion_merge_matches_the_reference_chain_under_autograd(N, with_gaux, with_prev):
    from open3dsot_amd import box_utils
    i = O.merge_inputs(Randn(9 + N), 3, N)
    prev, motion = (t64(i.prev, True) if with_prev else None), t64(i.motion, True)
    merged, aux = box_utils.motion_merge_reference(t64(i.pts), prev, motion)
    loss = (merged * t64(i.g)).sum() + ((aux * t64(i.g_aux)).sum() if with_gaux else 0.0)
    loss.backward()
    f = O.motion_merge_fwd(i.pts, i.prev if with_prev else None, i.motion)
    assert close(f.merged, merged.detach().numpy()) and close(f.aux, aux.detach().numpy())
    b = O.motion_merge_bwd(i.pts, i.prev if with_prev else None, i.motion, i.g, i.g_aux if with_gaux else None)
    assert close(b.g_motion, motion.grad.numpy())
    if with_prev:
        assert close(b.g_prev, prev.grad.numpy())
    assert (f.merged_abs >= np.abs(f.merged) * (1 - 1e-12)).all() and (b.g_motion_abs >= np.abs(b.g_motion) * (1 - 1e-12)).all()
    assert (b.g_prev_abs >= np.abs(b.g_prev) * (1 - 1e-12)).all()


def test_offset_box_matches_the_reference_under_autograd():
    from open3dsot_amd import box_utils
    i = O.offset_inputs(Randn(11), 65)
    ref, off = t64(i.ref, True), t64(i.off, True)
    box = box_utils.get_offset_box_tensor_reference(ref, off)
    (box * t64(i.g)).sum().backward()
    assert close(O.offset_box(i.ref, i.off).box, box.detach().numpy())
    b = O.offset_box_bwd(i.ref, i.off, i.g)
    assert close(b.g_ref, ref.grad.numpy()) and close(b.g_off, off.grad.numpy())


@pytest.mark.parametrize("shape", O.RPN_SHAPES, ids=str)
def test_rpn_glue_matches_sigmoid_transpose_cat(shape):
    B, N, f = shape
    draw = Randn(13 + N)
    cla, vote = t64(draw.val((B, 1, N)), True), t64(draw.val((B, 3 + f, N)), True)
    score = torch.sigmoid(cla)
    vote_xyz = vote[:, 0:3, :].transpose(1, 2).contiguous()
    vote_feature = torch.cat((score, vote[:, 3:, :]), dim=1)
    r = O.rpn_votes_fwd(cla.detach().numpy()[:, 0], vote.detach().numpy())
    assert close(r.score, score.detach().numpy()[:, 0]) and close(r.vote_xyz, vote_xyz.detach().numpy())
    assert close(r.vote_feature, vote_feature.detach().numpy())
    dvf, dvx = draw.val((B, 1 + f, N)), draw.val((B, 3, N))
    ((vote_feature * t64(dvf)).sum() + (vote_xyz * t64(dvx).transpose(1, 2)).sum()).backward()
    b = O.rpn_votes_bwd(r.score, dvf, dvx, f)
    assert close(b.dcla, cla.grad.numpy()[:, 0])
    assert close(b.dvote, vote.grad.permute(1, 0, 2).reshape(3 + f, B * N).numpy())
    z = O.rpn_votes_bwd(r.score, None, None, f)
    assert not z.dcla.any() and not z.dvote.any()
    P = N
    off, ctr = t64(draw.val((B, 5, P))), t64(draw.val((B, P, 3)))
    boxes = torch.cat((off[:, 0:3, :] + ctr.transpose(1, 2), off[:, 3:5, :]), dim=1).transpose(1, 2)
    assert close(O.box_assemble(off.numpy(), ctr.numpy()).boxes, boxes.numpy())


@pytest.mark.parametrize("kind", O.BEST_KINDS)
def test_best_proposal_is_numpy_argmax(kind):
    for B in O.BEST_B:
        for P in O.BEST_P:
            draw = O.Dyadic(7000 + 10 * B + P)
            boxes = draw.val((B, P, 5), 0.125, 8.0)
            boxes[:, :, 4] = O.best_scores(kind, B, P, draw)
            r = O.best_proposal(boxes)
            idx = boxes[:, :, 4].argmax(1)
            assert np.array_equal(r.idx, idx) and np.array_equal(r.out, boxes[np.arange(B), idx, :4])
    if kind == "lane_rounds":
        assert (idx == 3).all()
    if kind == "zeros":
        assert (idx == 200 // 3).all()


# ---- the bounds, on the GPU file's own input sets ---------------------------------------------------------------------------
def test_the_gpu_file_runs_the_tabled_cases():
    import test_tail_kernels_gpu as K
    assert K.U_MEASURED.keys() == O.U.keys()
    assert O.TRACK_SCRATCH == 512 and O.M2_SCRATCH == 1024
    assert [c[1] for c in O.TRACK_ROUNDED[:5]] == O.TRACK_SHAPES == [c[1] for c in O.TRACK_EXACT]
    assert {c[2] for c in O.TRACK_ROUNDED} == set(O.TRACK_KINDS)
    assert [c[2] for c in O.M2_ROUNDED[4:20]] == O.M2_FLAGS == [c[2] for c in O.M2_EXACT[4:20]]
    assert O.M2_ROUNDED[20][1] == (2, 7, 0) and [c[3] for c in O.M2_ROUNDED[21:23]] == ["still", "labels"]
    # the second round of every loop and its tail
    assert O.TRACK_SHAPES[3][0] * O.TRACK_SHAPES[3][1] > O.LG * O.LT > O.TRACK_SHAPES[3][0] * O.TRACK_SHAPES[3][2]
    assert min(O.TRACK_SHAPES[4][0] * O.TRACK_SHAPES[4][1], O.TRACK_SHAPES[4][0] * O.TRACK_SHAPES[4][2]) > O.LG * O.LT
    assert O.M2_SHAPES[2][0] > O.LG and O.M2_SHAPES[2][1] > O.LT and O.M2_SHAPES[3][0] > O.LT


def _draw(seed):
    return Randn(seed) if seed < 1000 else O.Dyadic(seed)


@pytest.mark.parametrize("case", O.TRACK_ROUNDED + O.TRACK_EXACT, ids=str)
def test_track_loss_float32_stays_within_the_bounds_and_no_decision_sits_on_an_edge(case):
    seed, shape, kind = case
    draw = _draw(seed)
    i = O.track_inputs(draw, *shape, kind=kind)
    d = O.track_dist(i.centers, i.box_label)
    assert np.abs(d - 0.3).min() >= 1e-5 and np.abs(d - 0.6).min() >= 1e-5
    for with_bc in (True, False):
        a = O.track_args(i, with_bc)
        r = O.track_loss(*a, O.TRACK_W)
        with O.precision(np.float32):
            s = O.track_sums(*a)
            f = O.track_finish(r.sums, shape[0] * shape[1], shape[0] * shape[2], O.TRACK_W, with_bc)
            g = O.track_grads(*a, O.TRACK_W, r.sums)
        assert s.sums.dtype == np.float32 and g.g_vote.dtype == np.float32
        assert np.array_equal(s.sums[:3], r.sums[:3])
        for j in range(8):
            within("sum", s.sums[j], r.sums[j], r.sums_abs[j], r.sums_n[j])
            if draw.exact and j in (0, 1, 2, 4, 5, 7):
                assert s.sums[j] == r.sums[j] and r.sums_abs[j] / O.track_spacing(i)[j] < O.TWO24, (j, s.sums[j], r.sums[j])
        for j in range(6):
            within("loss", f.losses[j], r.losses[j], r.losses_abs[j], r.losses_n[j])
        for name in ("g_cla", "g_vote", "g_boxes") + (("g_bc",) if with_bc else ()):
            within(name, getattr(g, name), getattr(r, name), getattr(r, name + "_abs"), getattr(r, name + "_n"))
    if draw.exact:
        # the kernel multiplies by fl(1/3) where the oracle divides by 3: v = 3 sl1(d) comes back as sl1(d) either way
        v = O.sl1(i.vote - i.box_label[:, None, :3]).sum(-1)
        assert np.array_equal(np.float32(v) * np.float32(1.0 / 3.0), (v / 3.0).astype(np.float32))
        assert np.array_equal((v / 3.0).astype(np.float32).astype(np.float64), v / 3.0)
        mags = np.abs(i.vote - i.box_label[:, None, :3])
        assert (np.abs(mags[mags != 1.0] - 1.0) >= 1e-5).all()


@pytest.mark.parametrize("case", O.M2_ROUNDED + O.M2_EXACT + O.M2_EXACT_GRADS, ids=str)
def test_m2track_loss_float32_stays_within_the_bounds(case):
    seed, shape, flags, kind = case
    draw = _draw(seed)
    w = O.M2_W_EXACT if case in O.M2_EXACT_GRADS else O.M2_W
    i = O.m2_inputs(draw, *shape, flags, kind)
    a = O.m2_args(i)
    r = O.m2track_loss(*a, w)
    with O.precision(np.float32):
        s = O.m2_sums(*a)
        f = O.m2_finish(r.sums, *shape, w, i.bc_pred is not None, i.motion_cls is not None, i.state is not None, i.est is not None,
                        i.prev is not None)
        g = O.m2_grads(*a, w, r.sums)
    for j in range(13):
        within("sum", s.sums[j], r.sums[j], r.sums_abs[j], r.sums_n[j])
        if draw.exact and j not in (1, 12):
            assert s.sums[j] == r.sums[j] and r.sums_abs[j] / O.m2_spacing(i)[j] < O.TWO24, (j, s.sums[j], r.sums[j])
    for j in range(12):
        within("loss", f.losses[j], r.losses[j], r.losses_abs[j], r.losses_n[j])
    for name in O.M2_GRADS:
        if getattr(r, name) is not None:
            within(name, getattr(g, name), getattr(r, name), getattr(r, name + "_abs"), getattr(r, name + "_n"))
    if case in O.M2_EXACT_GRADS:
        B = shape[0]
        assert np.array_equal(g.g_bc, r.g_bc)
        for name in ("g_motion", "g_aux", "g_est", "g_prev"):
            assert np.array_equal(getattr(g, name)[:, :3], getattr(r, name)[:, :3]) and not getattr(r, name)[:, 3].any()
        # the kernel's order for g_motion: ((w_center * 1) * (1 / B)) * fl(1/3) is w_center / (3 B) exactly
        c = np.float32(w[0]) * np.float32(1.0) * (np.float32(1.0) / np.float32(B)) * np.float32(1.0 / 3.0)
        assert float(c) == w[0] / (3.0 * B) and float(np.float32(w[0]) / (np.float32(3.0) * np.float32(B))) == w[0] / (3.0 * B)
    if draw.exact:
        v = O.sl1(i.motion[:, :3] - i.motion_lab[:, :3]).sum(-1)
        assert np.array_equal(np.float32(v) * np.float32(1.0 / 3.0), (v / 3.0).astype(np.float32))


@pytest.mark.parametrize("wd", (0.0, 0.125))
def test_adam_exact_leg_is_exact_in_float32(wd):
    import test_tail_kernels_gpu as K
    for p, m, v, g in K.adam_exact_jobs(wd):
        r = O.adam_step(p, m, v, g, wd=wd, **O.ADAM_EXACT)
        with O.precision(np.float32):
            s = O.adam_step(p, m, v, g, wd=wd, **O.ADAM_EXACT)
        assert s.p.dtype == np.float32 and np.isfinite(r.p).all()
        assert np.array_equal(s.p, r.p) and np.array_equal(s.m, r.m) and np.array_equal(s.v, r.v)
        root = np.sqrt(r.v)
        assert np.array_equal(root, np.round(root * 2) / 2) and (np.log2(root) % 1 == 0).all()       # a power of two


@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_adam_rounded_leg_float32_stays_within_the_bounds(wd):
    h = O.ADAM_ROUNDED
    for k, n in enumerate(O.ADAM_JOBS):
        p, m, v, g = (O.f32(x) for x in O.adam_inputs(Randn(600 + k), n, k))
        assert (np.abs(g[g != 0]) >= 1e-15).all() and (np.abs(g) <= 1e15).all() and (v[n // 8:] >= 1e-31).all()
        r = O.adam_moments(m, v, g, p, h["beta1"], h["beta2"], wd)
        u = O.adam_update(p, r.m, r.v, h["lr"], h["eps"], 0.5, 1e-3)
        with O.precision(np.float32):
            s = O.adam_moments(m, v, g, p, h["beta1"], h["beta2"], wd)
            su = O.adam_update(p, r.m, r.v, h["lr"], h["eps"], 0.5, 1e-3)
        within("m", s.m, r.m, r.m_abs, r.m_n), within("v", s.v, r.v, r.v_abs, r.v_n), within("p", su.p, u.p, u.p_abs, u.p_n)
        if wd == 0.0:
            assert np.array_equal(u.p[:n // 8], p[:n // 8])


@pytest.mark.parametrize("exact", (True, False))
@pytest.mark.parametrize("N", O.MERGE_N)
def test_motion_merge_float32_stays_within_the_bounds(N, exact):
    for B in O.MERGE_B:
        i = O.merge_inputs(O.Dyadic(900 + N + B) if exact else Randn(900 + N + B), B, N, zero_angles=exact)
        for prev in (i.prev, None):
            f, b = O.motion_merge_fwd(i.pts, prev, i.motion), O.motion_merge_bwd(i.pts, prev, i.motion, i.g, i.g_aux)
            with O.precision(np.float32):
                f32, b32 = O.motion_merge_fwd(i.pts, prev, i.motion), O.motion_merge_bwd(i.pts, prev, i.motion, i.g, i.g_aux)
            if exact:
                assert np.array_equal(f32.merged, f.merged) and np.array_equal(f32.aux, f.aux)
                assert np.array_equal(b32.g_motion, b.g_motion) and np.array_equal(b32.g_prev, b.g_prev)
            else:
                within("merged", f32.merged, f.merged, f.merged_abs, f.merged_n), within("aux", f32.aux, f.aux, f.aux_abs, f.aux_n)
                within("g_motion", b32.g_motion, b.g_motion, b.g_motion_abs, b.g_motion_n)
                within("g_prev", b32.g_prev, b.g_prev, b.g_prev_abs, b.g_prev_n)


@pytest.mark.parametrize("exact", (True, False))
def test_offset_box_and_glue_float32_stay_within_the_bounds(exact):
    for B in O.OFFSET_B:
        i = O.offset_inputs(O.Dyadic(980 + B) if exact else Randn(980 + B), B, zero_angles=exact)
        f, b = O.offset_box(i.ref, i.off), O.offset_box_bwd(i.ref, i.off, i.g)
        with O.precision(np.float32):
            f32, b32 = O.offset_box(i.ref, i.off), O.offset_box_bwd(i.ref, i.off, i.g)
        if exact:
            assert np.array_equal(f32.box, f.box) and np.array_equal(b32.g_ref, b.g_ref) and np.array_equal(b32.g_off, b.g_off)
        else:
            within("box", f32.box, f.box, f.box_abs, f.box_n)
            within("g_ref", b32.g_ref, b.g_ref, b.g_ref_abs, b.g_ref_n), within("g_off", b32.g_off, b.g_off, b.g_off_abs, b.g_off_n)
    draw = Randn(821)
    cla, dvf = 2.0 * draw.val((3, 100)), draw.val((3, 5, 100))
    r = O.rpn_votes_fwd(cla, draw.val((3, 7, 100)))
    s = O.f32(r.score)
    b = O.rpn_votes_bwd(s, dvf, None, 4)
    with O.precision(np.float32):
        r32, b32 = O.rpn_votes_fwd(cla, draw.val((3, 7, 100))), O.rpn_votes_bwd(s, dvf, None, 4)
    within("score", r32.score, r.score, r.score_abs, r.score_n), within("dcla", b32.dcla, b.dcla, b.dcla_abs, b.dcla_n)


# ---- refusals -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi
    return capi.load()


def refused(fn, valid, bad):
    """every (index, value) of `bad` put into the valid argument list in turn -> O3D_EINVAL (nothing is launched: the pointers
    are host memory that no kernel may see)"""
    for idx, value in bad:
        args = list(valid)
        for k, v in zip(idx if isinstance(idx, tuple) else (idx,), value if isinstance(idx, tuple) else (value,)):
            args[k] = v
        assert fn(*args) == EINVAL, (fn.__name__, idx, value)


def test_tail_entry_points_refuse_each_clause_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # o3d_track_loss: 0..7 cla seg vote box_label centers boxes bc_pred bc_label | 8..11 B N P K | 12..16 weights |
    # 17 scratch 18 losses | 19..22 g_cla g_vote g_boxes g_bc | 23 stream
    valid = [p] * 8 + [2, 8, 4, 9] + [1.0] * 5 + [p, p] + [p] * 4 + [None]
    refused(lib.o3d_track_loss, valid, [(k, None) for k in (0, 1, 2, 3, 4, 5, 17, 18)] + [(8, 0), (9, 0), (10, 0), (7, None), (11, 0),
                                                                                         (20, None), (21, None), (22, None)])
    # o3d_m2track_loss: 0 seg_logits 1 seg_label 2 bc_pred 3 bc_a 4 bc_b 5 motion_cls 6 state 7 motion 8 motion_lab 9 aux 10 est
    # 11 prev 12 box_lab 13 prev_lab | 14..16 B N K | 17..23 weights | 24 scratch 25 losses | 26..32 g_seg g_bc g_mcls g_motion
    # g_aux g_est g_prev | 33 stream
    valid = [p] * 14 + [2, 8, 9] + [1.0] * 5 + [0.5, 2.0] + [p, p] + [p] * 7 + [None]
    refused(lib.o3d_m2track_loss, valid, [(k, None) for k in (0, 1, 7, 8, 9, 12, 24, 25)] + [(14, 0), (15, 0), (4, None), (16, 0),
            (6, None), (13, None), (29, None), (30, None), (27, None), (28, None), (31, None), (32, None)])
    # o3d_adam_step: jobs njobs params exp_avg exp_avg_sq | lr beta1 beta2 eps wd bc1 bc2 | stream
    valid = [p, 1, p, p, p, 1e-3, 0.5, 0.999, 1e-6, 0.0, 0.5, 1e-3, None]
    refused(lib.o3d_adam_step, valid, [(0, None), (1, 0), (2, None), (3, None), (4, None), (11, 0.0)])
    refused(lib.o3d_best_proposal, [p, 1, 64, p, p, None], [(3, None), (2, 0)])
    # o3d_rpn_votes_fwd: cla sb sn vote sb sc sn | B N f | score vote_xyz vote_feature | stream
    valid = [p, 8, 1, p, 40, 8, 1, 2, 8, 2, p, p, p, None]
    refused(lib.o3d_rpn_votes_fwd, valid, [(0, None), (3, None), (10, None), (11, None), (12, None), (7, 0), (8, 0), (9, 0)])
    # o3d_rpn_votes_bwd: score | dvf sb sc sn | dvx sb sc sn | B N f | dcla dvote | stream
    valid = [p, p, 24, 8, 1, p, 24, 8, 1, 2, 8, 2, p, p, None]
    refused(lib.o3d_rpn_votes_bwd, valid, [(0, None), (12, None), (13, None), (9, 0), (10, 0), (11, 0)])
    # o3d_box_assemble: offsets sb sc sn centers B P boxes stream
    valid = [p, 40, 8, 1, p, 2, 8, p, None]
    refused(lib.o3d_box_assemble, valid, [(0, None), (4, None), (7, None), (5, 0), (6, 0)])
    # o3d_motion_merge_fwd: pts bstride cstride prev motion B N merged aux stream
    valid = [p, 32, 8, p, p, 1, 8, p, p, None]
    refused(lib.o3d_motion_merge_fwd, valid, [(4, None), (7, None), (8, None), (5, 0), (6, 0)])
    # o3d_motion_merge_bwd: pts bstride cstride prev motion B N g_merged g_aux g_prev g_motion stream
    valid = [p, 32, 8, p, p, 1, 8, p, p, p, p, None]
    refused(lib.o3d_motion_merge_bwd, valid, [(0, None), (4, None), (7, None), (10, None), (5, 0), (6, 0), (6, 7)])
    # o3d_offset_box: ref off B box g_box g_ref g_off stream
    refused(lib.o3d_offset_box, [p, p, 1, p, None, None, None, None], [(0, None), (1, None), (2, 0)])
    assert not any(buf), "a refused call wrote through a pointer"
