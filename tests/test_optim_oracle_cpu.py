"""tests/optim_oracle.py tied to torch (clip_grad_norm_ and torch.optim.SGD in fp64), its exact-leg inputs shown exact in
float32, its rounded-leg bounds shown to hold for a float32 restatement of the kernel, the refusals of the three entry points
of csrc/optim.hip (the library loads without a GPU), and the host-side pieces of open3dsot_amd/training.py."""
import ctypes

import numpy as np
import pytest
import torch

import optim_oracle as O
import tail_oracle as T
from test_rows_kernels_gpu import Randn
from test_tail_oracle_cpu import refused, within


def _tensors(arrays, dtype=torch.float64):
    return [torch.tensor(np.asarray(a, np.float64), dtype=dtype) for a in arrays]


# ---- ties to torch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", (1e-3, 0.5, 7.0, 1e30))
@pytest.mark.parametrize("kind", ("exact", "rounded", "zeros"))
def test_norm_and_coefficient_match_clip_grad_norm(kind, max_norm):
    grads = {"exact": O.norm_exact_grads, "rounded": O.norm_rounded_grads,
             "zeros": lambda: [np.zeros(n) for n in T.ADAM_JOBS]}[kind]()
    r = O.grad_norm(grads, max_norm)
    ps = [torch.zeros(len(g), dtype=torch.float64, requires_grad=True) for g in grads]
    for p, g in zip(ps, _tensors(grads)):
        p.grad = g.clone()
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    assert abs(total - r.norm) <= 1e-12 * r.norm and r.terms == sum(T.ADAM_JOBS)
    for p, g in zip(ps, grads):        # what clip_grad_norm_ left in .grad is g * coefficient
        want = np.asarray(g, np.float64) * r.coef
        assert np.allclose(p.grad.numpy(), want, rtol=1e-12, atol=0.0)
    if kind == "zeros":
        assert r.norm == 0.0 and r.coef == 1.0
    if max_norm == 1e30:
        assert r.coef == 1.0
    if kind == "exact":
        assert r.S == float(sum((np.asarray(g) ** 2).sum() for g in grads)) and r.S * 64 == int(r.S * 64) < 2 ** 53


@pytest.mark.parametrize("clip", (None, 0.75))
@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_sgd_matches_torch_sgd_over_three_steps(wd, clip):
    h = O.SGD_ROUNDED
    draw = Randn(41)
    p0 = draw.val((300,))
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([p], lr=h["lr"], momentum=h["momentum"], weight_decay=wd)
    pn, buf = p0.copy(), np.zeros(300)
    for t in range(3):
        g = draw.val((300,))
        p.grad = torch.tensor(g, dtype=torch.float64)
        scale = None
        if clip is not None:
            scale = O.grad_norm([g], clip).coef
            assert scale < 1.0
            torch.nn.utils.clip_grad_norm_([p], clip)
        opt.step()
        r = O.sgd_step(pn, buf, g, h["lr"], h["momentum"], wd, scale)
        pn, buf = r.p, r.buf
        assert np.allclose(pn, p.detach().numpy(), rtol=1e-12, atol=1e-15)
        assert np.allclose(buf, opt.state[p]["momentum_buffer"].numpy(), rtol=1e-12, atol=1e-15)


# ---- the legs of tests/test_optim_kernels_gpu.py ----------------------------------------------------------------------------
@pytest.mark.parametrize("wd", (0.0, 0.125))
def test_sgd_exact_leg_is_exact_in_float32(wd):
    h = O.SGD_EXACT
    for (p, buf, g), (_, _, g2) in zip(O.sgd_exact_jobs(wd), O.sgd_exact_jobs(wd, 1)):
        for grad in (g, g2):                                # two steps, the second on the first's results
            r = O.sgd_step(p, buf, grad, wd=wd, scale=O.SGD_EXACT_SCALE, **h)
            with T.precision(np.float32):
                s = O.sgd_step(p, buf, grad, wd=wd, scale=O.SGD_EXACT_SCALE, **h)
            k = O.sgd_step_f32(p, buf, grad, wd=wd, scale=O.SGD_EXACT_SCALE, **h)
            assert s.p.dtype == np.float32 and np.isfinite(r.p).all()
            assert np.array_equal(s.p, r.p) and np.array_equal(s.buf, r.buf)
            assert np.array_equal(k.p, r.p) and np.array_equal(k.buf, r.buf)
            p, buf = r.p, r.buf


@pytest.mark.parametrize("scale", (None, O.SGD_ROUNDED_SCALE))
@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_sgd_rounded_leg_float32_stays_within_the_bounds(wd, scale):
    h = O.SGD_ROUNDED
    for k, n in enumerate(T.ADAM_JOBS):
        p, buf, _, g = (T.f32(x) for x in T.adam_inputs(Randn(600 + k), n, k))
        for t in range(2):
            r = O.sgd_buf(p, buf, g, h["momentum"], wd, scale)
            s = O.sgd_step_f32(p, buf, g, h["lr"], h["momentum"], wd, scale)
            within("sgd.buf", s.buf, r.buf, r.buf_abs, r.buf_n)
            u = O.sgd_update(p, s.buf, h["lr"])
            within("sgd.p", s.p, u.p, u.p_abs, u.p_n)
            p, buf = s.p.astype(np.float64), s.buf.astype(np.float64)
            g = T.f32(T.adam_inputs(Randn(650 + k), n, k)[3])


def test_norm_rounded_inputs_stay_in_range():
    grads = O.norm_rounded_grads()
    for g in grads:
        assert (np.abs(g[g != 0]) >= 1e-15).all() and (np.abs(g) <= 1e15).all()
    r = O.grad_norm(grads, 1.0)
    # n terms of double accumulation: n * 2^-53 relative, against the float's 2^-24 half-ulp
    assert r.terms * 2.0 ** -53 < 2.0 ** -24 / 1024 and 1e-30 < r.coef < 1.0 and np.isfinite(np.float32(r.norm))


# ---- refusals -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi
    return capi.load()


def test_optim_entry_points_refuse_each_clause_before_any_launch(lib):
    from open3dsot_amd import capi
    assert capi.CONSTANTS["O3D_NORM_SLICES"] == O.NORM_SLICES
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # o3d_grad_norm: jobs njobs max_norm partials out stream
    refused(lib.o3d_grad_norm, [p, 1, 1.0, p, p, None],
            [(0, None), (1, 0), (1, -1), (2, 0.0), (2, -1.0), (2, float("nan")), (3, None), (4, None)])
    # o3d_adam_step_scaled: jobs njobs params exp_avg exp_avg_sq | lr beta1 beta2 eps wd bc1 bc2 | grad_scale stream
    valid = [p, 1, p, p, p, 1e-3, 0.5, 0.999, 1e-6, 0.0, 0.5, 1e-3, p, None]
    refused(lib.o3d_adam_step_scaled, valid, [(0, None), (1, 0), (2, None), (3, None), (4, None), (10, 0.0), (11, 0.0), (12, None)])
    # o3d_sgd_step: jobs njobs params momentum_buf | lr momentum wd | grad_scale (nullable) stream
    valid = [p, 1, p, p, 1e-3, 0.9, 0.0, None, None]
    refused(lib.o3d_sgd_step, valid, [(0, None), (1, 0), (2, None), (3, None), (4, -1.0), (4, float("nan")), (5, -0.1), (6, -1e-3)])
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_double: "d"}
    assert "".join(kinds[a] for a in capi.SIGNATURES["o3d_grad_norm"]) == "pidppp"
    assert "".join(kinds[a] for a in capi.SIGNATURES["o3d_adam_step_scaled"]) == "pipppdddddddpp"
    assert "".join(kinds[a] for a in capi.SIGNATURES["o3d_sgd_step"]) == "pippdddpp"


# ---- make_sgd and the configs on the CPU ----------------------------------------------------------------------------------------
def test_make_sgd_on_cpu_parameters_is_torch_sgd():
    from open3dsot_amd import m2track, optim, trackers
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.make_sgd([p], 0.1, 0.01)
    assert type(opt) is torch.optim.SGD and opt.defaults["momentum"] == 0.9 and opt.defaults["weight_decay"] == 0.01
    for model in (trackers.BAT(trackers.make_config(trackers.BAT_CAR, optimizer="sgd")),
                  m2track.M2TRACK(optimizer="SGD")):
        assert type(model.configure_optimizers()["optimizer"]) is torch.optim.SGD
    assert type(m2track.M2TRACK().configure_optimizers()["optimizer"]) is torch.optim.Adam


# ---- the host pieces of training.py -----------------------------------------------------------------------------------------
def test_validation_epochs():
    from open3dsot_amd import training as TR
    assert [e for e in range(7) if TR.validates_after(e, 1)] == list(range(7))
    assert [e for e in range(7) if TR.validates_after(e, 3)] == [2, 5]
    assert [e for e in range(3) if TR.validates_after(e, 5)] == []
    with pytest.raises(ValueError):
        TR.validates_after(0, 0)


def test_top_k_bookkeeping():
    from open3dsot_amd import training as TR
    scores = [0.3, 0.5, 0.5, 0.1, 0.9, None, float("nan")]

    def run(k):
        kept, on_disk = [], set()
        for e, s in enumerate(scores):
            kept, save, drop = TR.top_k_update(kept, "e%d" % e, s, k)
            if save:
                on_disk.add("e%d" % e)
            assert set(drop) <= on_disk
            on_disk -= set(drop)
            assert on_disk == {n for _, n in kept}
        return kept
    assert run(0) == []
    assert [n for _, n in run(-1)] == ["e%d" % e for e in range(7)]                 # keeps all, validated or not
    assert run(1) == [[0.9, "e4"]]
    assert run(2) == [[0.9, "e4"], [0.5, "e1"]]                                     # the tie at 0.5: the older file stays
    assert run(3) == [[0.9, "e4"], [0.5, "e1"], [0.5, "e2"]]
    kept, save, drop = TR.top_k_update([[0.5, "a"]], "b", 0.5, 1)                    # not strictly better: not saved
    assert (kept, save, drop) == ([[0.5, "a"]], False, [])
    assert TR.checkpoint_name(3, 120) == "epoch=3-step=120.ckpt"


def test_checkpoint_files_hold_plain_data_and_weights_only_files_load(tmp_path):
    from open3dsot_amd import training as TR
    assert TR._plain({"a": (1, 2.0, "x", None, True), "t": torch.ones(2)})["a"] == [1, 2.0, "x", None, True]
    with pytest.raises(TypeError):
        TR._plain({"a": object()})
    torch.save({"state_dict": {"w": torch.arange(3.0)}}, tmp_path / "bare.ckpt")
    c = TR.load_checkpoint(tmp_path / "bare.ckpt")
    assert set(TR.CKPT_KEYS) <= set(c) and c["epoch"] == 0 and c["global_step"] == 0 and c["optimizer_states"] == []
    assert torch.equal(c["state_dict"]["w"], torch.arange(3.0)) and c["sampler"] is None
    torch.save({"weights": 1}, tmp_path / "bad.ckpt")
    with pytest.raises(ValueError, match="state_dict"):
        TR.load_checkpoint(tmp_path / "bad.ckpt")
