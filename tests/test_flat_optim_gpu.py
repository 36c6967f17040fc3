"""optim.FlatSGD, the flat optimizers' grad_clip, and dist.DataParallelStep(grad_clip=...).

FlatSGD against an fp64 twin under torch.optim.SGD (+ clip_grad_norm_): the yardstick is torch's OWN fp32 SGD (same inputs, on
the GPU) against that twin; FlatSGD may err up to twice that -- one rounding may differ per operation (torch multiplies and
adds, the kernel fuses) -- never by a figure taken from FlatSGD itself.  Both errors are printed (DESIGN.md has a run's)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = (1, 257, 8193)
LR, MOMENTUM, CLIP = 0.05, 0.9, 40.0


class Three(torch.nn.Module):
    def __init__(self, seed=3, dtype=torch.float32):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a, self.b, self.c = (torch.nn.Parameter(torch.randn(n, generator=g).to(DEV, dtype)) for n in SIZES)
        self.c.data = self.c.data.view(3, 2731)          # a matrix: the views keep their shape


def grads_of(step, dtype=torch.float32):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(n, generator=g).to(DEV, dtype) for n in SIZES]


def run(opt_of, dtype, clip, steps=3, start=0):
    model = Three(dtype=dtype)
    opt = opt_of(model)
    drive(model, opt, clip, range(start, start + steps))
    return model, opt


def drive(model, opt, clip, steps):
    for t in steps:
        for p, g in zip(model.parameters(), grads_of(t, next(model.parameters()).dtype)):
            p.grad = g.view_as(p).clone()
        if clip is not None and not hasattr(opt, "last_grad_norm"):
            torch.nn.utils.clip_grad_norm_(list(model.parameters()), clip)
        opt.step()
    torch.cuda.synchronize()


def worst(model, twin):
    return max(float((p.detach().double() - q.detach()).abs().max()) for p, q in zip(model.parameters(), twin.parameters()))


@pytest.mark.parametrize("clip", (None, CLIP), ids=("noclip", "clip"))
@pytest.mark.parametrize("wd", (0.0, 1e-2))
def test_flat_sgd_against_an_fp64_twin(wd, clip):
    from open3dsot_amd import optim
    twin, _ = run(lambda m: torch.optim.SGD(m.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=wd), torch.float64, clip)
    ref, _ = run(lambda m: torch.optim.SGD(m.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=wd), torch.float32, clip)
    flat, opt = run(lambda m: optim.FlatSGD(m.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=wd, grad_clip=clip),
                    torch.float32, clip)
    assert isinstance(opt, optim.FlatSGD) and flat.c.shape == (3, 2731)
    e_torch, e_flat = worst(ref, twin), worst(flat, twin)
    print("FlatSGD wd=%g clip=%s, 3 steps: max |p - fp64 twin| %.3e (torch.optim.SGD fp32: %.3e)" % (wd, clip, e_flat, e_torch))
    assert e_torch > 0 and e_flat <= 2 * e_torch
    if clip is not None:
        norm = float(torch.cat([g.double() for g in grads_of(2)]).norm())
        assert norm > clip                                             # the last step did clip
        assert abs(float(opt.last_grad_norm()) - norm) <= 2e-7 * norm
        assert abs(float(opt.last_clip_coef()) - clip / (norm + 1e-6)) <= 2e-7
        for p, g in zip(flat.parameters(), grads_of(2)):               # unlike torch: p.grad is left unclipped
            assert torch.equal(p.grad, g.view_as(p))
    else:
        assert opt.last_grad_norm() is None and opt._norm is None      # no launch, no allocation


def test_flat_sgd_state_dict_round_trip_through_torch_sgd():
    from open3dsot_amd import optim
    kw = dict(lr=LR, momentum=MOMENTUM, weight_decay=1e-2)
    a, opt_a = run(lambda m: optim.FlatSGD(m.parameters(), **kw), torch.float32, None, steps=2)
    sd = opt_a.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2] and all(list(s) == ["momentum_buffer"] for s in sd["state"].values())
    assert sd["state"][2]["momentum_buffer"].shape == (3, 2731)
    mid = copy.deepcopy(a)
    opt_t = torch.optim.SGD(mid.parameters(), lr=1.0)
    opt_t.load_state_dict(copy.deepcopy(sd))
    assert opt_t.param_groups[0]["lr"] == LR and opt_t.param_groups[0]["momentum"] == MOMENTUM
    b = copy.deepcopy(a)
    opt_b = optim.FlatSGD(b.parameters(), lr=1.0, momentum=0.0)
    opt_b.load_state_dict(copy.deepcopy(opt_t.state_dict()))
    for p in b.parameters():                                          # the buffers went back into the flat buffer
        off, n = opt_b._offsets[p]
        assert opt_b.state[p]["momentum_buffer"].data_ptr() == opt_b._buf.data_ptr() + 4 * off
    drive(a, opt_a, None, [2])
    drive(b, opt_b, None, [2])
    drive(mid, opt_t, None, [2])
    for p, q, r in zip(a.parameters(), b.parameters(), mid.parameters()):
        assert torch.equal(p, q)
        assert torch.allclose(p, r, rtol=1e-5, atol=1e-6)             # torch's own step from the same state: the same update
    # a torch.optim.SGD checkpoint taken before its first step: no buffers -> zeros
    c = Three()
    opt_c = optim.FlatSGD(c.parameters(), **kw)
    opt_c._buf.fill_(7.0)
    opt_c.load_state_dict(torch.optim.SGD(Three().parameters(), **kw).state_dict())
    assert float(opt_c._buf.abs().max()) == 0.0


def test_grad_clip_unset_leaves_flat_adam_bit_equal():
    from open3dsot_amd import optim
    kw = dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-6, weight_decay=1e-2)
    a, opt_a = run(lambda m: optim.FlatAdam(m.parameters(), **kw), torch.float32, None)
    b, opt_b = run(lambda m: optim.FlatAdam(m.parameters(), grad_clip=None, **kw), torch.float32, None)
    c, opt_c = run(lambda m: optim.FlatAdam(m.parameters(), grad_clip=0, **kw), torch.float32, None)
    d, opt_d = run(lambda m: optim.FlatAdam(m.parameters(), grad_clip=1e30, **kw), torch.float32, None)    # coefficient 1.0f
    for p, q, r, s in zip(a.parameters(), b.parameters(), c.parameters(), d.parameters()):
        assert torch.equal(p, q) and torch.equal(p, r) and torch.equal(p, s)
    for o in (opt_a, opt_b, opt_c):
        assert o.last_grad_norm() is None and o._norm is None
    assert float(opt_d.last_clip_coef()) == 1.0 and "grad_clip" not in opt_d.state_dict()["param_groups"][0]
    # settable afterwards: the clipped Adam step is Adam on g * coefficient
    e, opt_e = run(lambda m: optim.FlatAdam(m.parameters(), **kw), torch.float32, None, steps=2)
    opt_e.grad_clip = CLIP
    drive(e, opt_e, None, [2])
    f, opt_f = run(lambda m: torch.optim.Adam(m.parameters(), **kw), torch.float64, None, steps=2)
    drive(f, opt_f, CLIP, [2])
    assert float(opt_e.last_clip_coef()) < 1.0
    assert worst(e, f) < 1e-5 and worst(e, f) < 0.05 * worst(a, f)    # far closer to the clipped twin than the unclipped run is


def test_rehomed_parameter_raises():
    from open3dsot_amd import optim
    model = Three()
    first = optim.FlatSGD(model.parameters(), lr=LR)
    optim.FlatSGD(model.parameters(), lr=LR)                          # re-homes every parameter
    for p, g in zip(model.parameters(), grads_of(0)):
        p.grad = g.view_as(p)
    with pytest.raises(RuntimeError, match="FlatSGD: a parameter no longer lives"):
        first.step()
    with pytest.raises(ValueError, match="fp32 CUDA parameters only"):
        optim.FlatSGD([torch.nn.Parameter(torch.zeros(3))], lr=LR)
    assert isinstance(optim.make_sgd(Three().parameters(), LR, 0.0), optim.FlatSGD)
    optim.set_flat_adam(False)
    try:
        assert type(optim.make_sgd(Three().parameters(), LR, 0.0)) is torch.optim.SGD
    finally:
        optim.set_flat_adam(True)


def test_data_parallel_step_clips_the_update():
    """BAT at batch 2, graph on, SGD: the first step's parameter delta is -lr * g * coefficient, so with c = half the gradient
    norm it equals the unclipped twin's delta times last_clip_coef() -- to the run-to-run rounding of two trainers (the per-
    parameter rule of tests/test_model_gpu.py::test_*_graph_replay: max-norm difference below 5e-3 of the parameter's scale,
    parameters whose delta is below 1e-4 of the largest one only required to stay below 1e-3 of it).  lr = 1: the delta is
    read as p_after - p_before, whose rounding is half an ulp of p -- at the config's lr 1e-3 that alone is percents of the
    delta of a BatchNorm weight (p = 1, g of order 1e-3).  Deterministic mode, at the shape it is tested at: the two trainers
    then see the same gradient bits, and what is left is the rounding of the two updates."""
    from open3dsot_amd import dist as D, fused, optim, synth, trackers
    batch = synth.to_torch(synth.make_batch(5, 2, 256, 512), DEV)
    fused.set_deterministic(True)
    try:
        _clipped_delta_equals_scaled_delta(D, optim, trackers, batch)
    finally:
        fused.set_deterministic(False)


def _clipped_delta_equals_scaled_delta(D, optim, trackers, batch):

    def one(clip):
        torch.manual_seed(31)
        model = trackers.BAT(trackers.make_config(trackers.BAT_CAR, optimizer="sgd", lr=1.0)).to(DEV).train()
        before = [p.detach().clone() for p in model.parameters()]
        trainer = D.DataParallelStep(model, world=1, graph=True, graph_warmup=0, require_graph=True, grad_clip=clip)
        assert isinstance(trainer.optimizer, optim.FlatSGD) and trainer.optimizer.grad_clip == clip
        trainer.step(batch)
        torch.cuda.synchronize()
        assert trainer.graph is not None
        delta = [p.detach() - q for p, q in zip(model.parameters(), before)]
        norm = float(torch.cat([p.grad.double().flatten() for p in model.parameters() if p.grad is not None]).norm())
        return trainer, delta, norm

    plain, d0, norm = one(None)
    assert plain.optimizer.last_grad_norm() is None
    clipped, d1, _ = one(0.5 * norm)
    coef = float(clipped.optimizer.last_clip_coef())
    assert abs(float(clipped.optimizer.last_grad_norm()) - norm) < 5e-3 * norm and abs(coef - 0.5) < 5e-3
    top = max(float(d.abs().max()) for d in d0) * coef
    assert top > 0
    worst_err = 0.0
    for a, b in zip(d1, d0):
        want = b * coef
        scale = float(want.abs().max())
        if scale < 1e-4 * top:
            assert float(a.abs().max()) < 1e-3 * top
            continue
        err = float((a - want).abs().max()) / scale
        worst_err = max(worst_err, err)
        assert err < 5e-3, err
    print("DataParallelStep(grad_clip): coefficient %.6f, worst per-parameter delta difference %.1e" % (coef, worst_err))


def test_data_parallel_step_clips_other_optimizers_with_torch():
    from open3dsot_amd import dist as D, synth, trackers
    batch = synth.to_torch(synth.make_batch(5, 2, 256, 512), DEV)
    torch.manual_seed(31)
    model = trackers.BAT().to(DEV).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    trainer = D.DataParallelStep(model, optimizer=opt, world=1, grad_clip=1e-3)
    trainer.step(batch)
    norm = float(torch.cat([p.grad.flatten() for p in model.parameters() if p.grad is not None]).norm())
    assert abs(norm - 1e-3) < 1e-5                                     # clip_grad_norm_ scaled p.grad itself
