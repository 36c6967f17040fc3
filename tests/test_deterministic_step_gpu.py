"""Deterministic mode (fused.set_deterministic): the training step as a function of its inputs, bit for bit.

Three runs from the same seeded state -- a fresh model and optimizer each, the same batch -- give byte-identical loss,
gradients, BatchNorm buffers and parameters after Adam, eagerly and as a replayed HIP graph.  The run count is three: this
is no hunt for a rare difference.  Nothing is asserted about the default mode; what two default runs differ by is printed.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    from open3dsot_amd import fused
    yield
    fused.set_deterministic(False)


def make(model_name):
    from open3dsot_amd import synth, trackers
    torch.manual_seed(31)
    if model_name == "M2TRACK":
        from open3dsot_amd import m2track
        return m2track.M2TRACK().to(DEV).train(), synth.to_torch(synth.make_motion_batch(5, 2, 512), DEV)
    return trackers.get_model(model_name)().to(DEV).train(), synth.to_torch(synth.make_batch(5, 2, 256, 512), DEV)


def one_run(model_name, graph):
    """a fresh seeded model + its own optimizer (Adam), steps on one batch until the asked-for kind of step has run once after the
    first -> {name: bytes} of the LAST step's loss, gradients, and the buffers / parameters it leaves"""
    from open3dsot_amd import dist as D
    model, batch = make(model_name)
    trainer = D.DataParallelStep(model, world=1, graph=graph, graph_warmup=1, require_graph=graph)
    trainer.step(batch)                 # eager
    loss = trainer.step(batch)          # eager, or captured here and replayed
    torch.cuda.synchronize()
    assert (trainer.graph is not None) == graph, trainer.graph_error
    out = {"loss": loss}
    out.update({"grad:" + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
    out.update({"buffer:" + k: b for k, b in model.named_buffers()})
    out.update({"param:" + k: p for k, p in model.named_parameters()})
    assert any(k.startswith("grad:") for k in out) and any("running_mean" in k for k in out)
    return {k: v.detach().cpu().contiguous().numpy().tobytes() for k, v in out.items()}, \
        {k: v.detach().float().cpu() for k, v in out.items() if k.startswith("grad:")}


def differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if a[k] != b[k]]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "replay"])
@pytest.mark.parametrize("model_name", ["BAT", "P2B", "M2TRACK"])
def test_three_runs_are_byte_identical(model_name, graph):
    from open3dsot_amd import fused
    fused.set_deterministic(True)
    runs = [one_run(model_name, graph)[0] for _ in range(3)]
    for r in runs[1:]:
        bad = differing(runs[0], r)
        assert not bad, (model_name, graph, len(bad), bad[:6])


@pytest.mark.parametrize("model_name", ["BAT", "P2B"])
def test_eager_step_and_its_replay_agree_byte_for_byte(model_name):
    """the captured step launches the kernels of the eager one on the same inputs: in deterministic mode the two agree bit for bit
    (measured on the first run)"""
    from open3dsot_amd import fused
    fused.set_deterministic(True)
    bad = differing(one_run(model_name, False)[0], one_run(model_name, True)[0])
    print("deterministic eager vs replay, %s: %d tensors differ %s" % (model_name, len(bad), bad[:6]))
    assert not bad


def test_default_mode_difference_is_printed():
    """MEASURED, not asserted: the largest gradient difference between two default-mode runs, in the second step (LDS float
    atomics in the layer-0 list sums; the Adam update between the two steps normalises the first step's rounding noise to +-lr)"""
    from open3dsot_amd import fused
    assert not fused.deterministic_enabled()
    (_, g0), (_, g1) = one_run("BAT", False), one_run("BAT", False)
    worst = max(float((g0[k] - g1[k]).abs().max()) for k in g0)
    top = max(float(g0[k].abs().max()) for k in g0)
    print("default mode, BAT 2 x 256/512, second step: largest gradient difference between two runs %.3e (largest gradient %.3e)"
          % (worst, top))


def test_flip_after_capture_raises():
    from open3dsot_amd import dist as D, fused
    model, batch = make("BAT")
    trainer = D.DataParallelStep(model, world=1, graph=True, graph_warmup=0, require_graph=True)
    trainer.step(batch)
    assert trainer.graph is not None
    fused.set_deterministic(True)
    with pytest.raises(RuntimeError, match="build a new trainer"):
        trainer.step(batch)
    fused.set_deterministic(False)
    trainer.step(batch)                 # back in the mode it was captured in: runs


def test_cold_scatter_operators_refuse_the_mode():
    from open3dsot_amd import fused, ops
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(2, 4, 32, generator=g).to(DEV).requires_grad_(True)
    idx = torch.randint(0, 32, (2, 8, 4), generator=g, dtype=torch.int32).to(DEV)
    idx1 = torch.randint(0, 32, (2, 8), generator=g, dtype=torch.int32).to(DEV)
    idx3 = torch.randint(0, 32, (2, 8, 3), generator=g, dtype=torch.int32).to(DEV)
    w3 = torch.rand(2, 8, 3, generator=g).to(DEV)
    calls = {"GroupingOperation": lambda: ops.grouping_operation(feats, idx),
             "GatherOperation": lambda: ops.gather_operation(feats, idx1),
             "ThreeInterpolate": lambda: ops.three_interpolate(feats, idx3, w3)}
    for name, call in calls.items():
        feats.grad = None
        call().sum().backward()         # off: as before
        assert feats.grad is not None and bool(torch.isfinite(feats.grad).all())
        fused.set_deterministic(True)
        try:
            out = call()                # forward is unaffected
            with pytest.raises(RuntimeError, match=name + ".*float atomics"):
                out.sum().backward()
        finally:
            fused.set_deterministic(False)


def test_mode_refuses_the_atomic_fallback():
    """set_reduce_gather(False) forces the LDS-atomic kernel: with the mode on that is an error naming the shape, not a fallback"""
    from open3dsot_amd import fused
    model, batch = make("BAT")
    fused.set_deterministic(True)
    fused.set_reduce_gather(False)
    try:
        loss, _ = model.training_loss(batch)
        with pytest.raises(RuntimeError, match=r"deterministic mode.*spanmax.*set_reduce_gather\(False\)"):
            loss.backward()
    finally:
        fused.set_reduce_gather(True)
