"""The launches of csrc/optim.hip through the C ABI with raw pointers, against tests/optim_oracle.py (tied to torch by
tests/test_optim_oracle_cpu.py): o3d_grad_norm, o3d_adam_step_scaled, o3d_sgd_step.  Method, job layout and guards are those
of tests/test_tail_kernels_gpu.py's o3d_adam_step section: the jobs of tail_oracle.ADAM_JOBS (1, 255, 256, 257, 8192, 8193,
20000 elements) lie out of order in the flat buffers with gaps of sentinels that must come back untouched, the gradients at
odd element offsets of a NaN-filled buffer.  e = 2^-24.

o3d_grad_norm, EXACT leg: g = +-2^k (k in [-3, 3]) or 0 -- every square and every sum of squares is exact in double, so the
partials read back sum to S exactly whatever the order, and out[0] is float32(sqrt(S)) up to 1 float ulp (the fp64 square root
and the cast round once each).  ROUNDED leg: |g| in [1e-15, 1e15]; double accumulation over n <= 4e4 terms errs by n * 2^-53
relative, far below 2^-24, so out[0] and out[1] lie within 1 float ulp of the oracle's fp64 value rounded to float32 -- a
derived bound, not a measured one.  Coefficient: norm <= max_norm gives exactly 1.0f; all-zero gradients give norm 0, scale 1.

o3d_adam_step_scaled: bit-equal to o3d_adam_step at *grad_scale = 1.0f, and at 0.5f bit-equal to o3d_adam_step on pre-halved
gradients (a halving is exact), on the rounded leg's inputs with eps and weight decay on.

o3d_sgd_step, EXACT leg: lr, momentum, wd, scale powers of two, inputs like adam_exact_jobs: bit for bit over two steps.
ROUNDED leg: lr 1e-3, momentum 0.9, two steps, |err| <= (n + 8) e sum|t_i| with n counted from the four stated operations
(optim_oracle's docstring): buf 5, p 2 against the update computed in fp64 from the STORED buffer.
"""
import numpy as np
import pytest
import torch

import optim_oracle as O
import tail_oracle as T
from test_pointwise_kernels_gpu import SENT, TAIL, Randn, dev, host, lib, outbuf, st, untouched  # noqa: F401
from test_tail_kernels_gpu import AdamRun, adam_exact_jobs, bits, cmp

pytestmark = pytest.mark.gpu

DSENT = -7.0e300


def ulps32(got, want):
    want = np.float32(want)
    return abs(float(np.float32(got)) - float(want)) / O.ulp32(want) if want != 0 else (0.0 if got == 0 else np.inf)


# ---- o3d_grad_norm --------------------------------------------------------------------------------------------------------
class NormRun(AdamRun):
    """AdamRun's gradient buffer and job table (P, M, V stay sentinels: the norm writes none of them)"""

    def __init__(self, grads):
        z = [np.zeros(len(g)) for g in grads]
        super().__init__([(a, a, a, g) for a, g in zip(z, grads)])
        for b in (self.P, self.M, self.V):
            b.fill_(SENT)
        self.count = len(grads) * O.NORM_SLICES
        self.partials = torch.full((self.count + TAIL,), DSENT, dtype=torch.float64, device="cuda")
        self.outf, self.out = outbuf((2,))

    def norm(self, lib, max_norm):
        self.partials.fill_(DSENT)
        assert lib.o3d_grad_norm(self.tab.data_ptr(), len(self.sizes), max_norm, self.partials.data_ptr(), self.out.data_ptr(),
                                 st()) == 0
        torch.cuda.synchronize()
        for b in (self.P, self.M, self.V, self.outf[2:]):
            assert untouched(b), "the norm wrote into a parameter buffer or beyond out[1]"
        assert bool((self.partials[self.count:] == DSENT).all()), "write beyond the partials"
        part = self.partials[:self.count].cpu().numpy()
        assert (part != DSENT).all() and np.isfinite(part).all(), "a partial was not written"
        o = self.out.cpu().numpy()
        return part.reshape(len(self.sizes), O.NORM_SLICES), o[0], o[1]


@pytest.fixture(scope="module")
def exact_run():
    grads = O.norm_exact_grads()
    return grads, NormRun(grads)


def test_grad_norm_exact(lib, exact_run):
    grads, run = exact_run
    r = O.grad_norm(grads, 4.0)
    part, nrm, coef = run.norm(lib, 4.0)
    for j, g in enumerate(grads):                 # per job: its slices add up to the job's sum exactly, empty slices are 0
        assert part[j].sum() == float((np.asarray(g) ** 2).sum())
        used = -(-len(g) // 256)
        assert (part[j, used:] == 0).all()
    assert part.sum() == r.S and r.norm > 4.0
    assert ulps32(nrm, r.norm) <= 1 and ulps32(coef, r.coef) <= 1 and 0 < coef < 1


def test_grad_norm_below_max_norm_and_zero_gradients(lib, exact_run):
    grads, run = exact_run
    r = O.grad_norm(grads, 1e6)
    _, nrm, coef = run.norm(lib, 1e6)
    assert r.norm < 1e6 and bits(coef) == bits(1.0) and ulps32(nrm, r.norm) <= 1
    zeros = NormRun([np.zeros(n) for n in T.ADAM_JOBS])
    part, nrm, coef = zeros.norm(lib, 1.0)
    assert (part == 0).all() and bits(nrm) == bits(0.0) and bits(coef) == bits(1.0)


@pytest.mark.parametrize("max_norm", (1.0, 3e14))
def test_grad_norm_rounded(lib, max_norm):
    grads = O.norm_rounded_grads()
    r = O.grad_norm(grads, max_norm)
    assert r.norm > max_norm
    run = NormRun(grads)
    part, nrm, coef = run.norm(lib, max_norm)
    print("grad_norm rounded: norm %.9g (oracle %.17g) %.2f ulp, coef %.9g (oracle %.17g) %.2f ulp, fp64 sum of partials off by %.3g"
          % (nrm, r.norm, ulps32(nrm, r.norm), coef, r.coef, ulps32(coef, r.coef), abs(part.sum() - r.S) / r.S))
    assert ulps32(nrm, r.norm) <= 1 and ulps32(coef, r.coef) <= 1


def test_grad_norm_refuses_before_any_launch(lib, exact_run):
    _, run = exact_run
    run.partials.fill_(DSENT)
    run.out.fill_(SENT)
    for max_norm in (0.0, -1.0):
        assert lib.o3d_grad_norm(run.tab.data_ptr(), len(run.sizes), max_norm, run.partials.data_ptr(), run.out.data_ptr(), st()) == -1
    assert lib.o3d_grad_norm(run.tab.data_ptr(), len(run.sizes), 1.0, None, run.out.data_ptr(), st()) == -1
    torch.cuda.synchronize()
    assert untouched(run.outf) and bool((run.partials == DSENT).all())


# ---- o3d_adam_step_scaled -------------------------------------------------------------------------------------------------
def adam_scaled(run, lib, scale, lr, beta1, beta2, eps, wd, bc1, bc2):
    s = torch.tensor([scale], dtype=torch.float32, device="cuda")
    assert lib.o3d_adam_step_scaled(run.tab.data_ptr(), len(run.sizes), run.P.data_ptr(), run.M.data_ptr(), run.V.data_ptr(),
                                    lr, beta1, beta2, eps, wd, bc1, bc2, s.data_ptr(), st()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("scale", (1.0, 0.5))
@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_adam_step_scaled_is_adam_step_on_scaled_gradients(lib, wd, scale):
    h = T.ADAM_ROUNDED
    jobs = [T.adam_inputs(Randn(600 + k), n, k) for k, n in enumerate(T.ADAM_JOBS)]
    pre = [(p, m, v, T.f32(g) * scale) for p, m, v, g in jobs]            # a halving of a float in [1e-15, 1e15] is exact
    assert all(np.array_equal(T.f32(j[3]), j[3]) for j in pre)
    ref, run = AdamRun(pre), AdamRun(jobs)
    for t in (1, 2):
        bc1, bc2 = 1 - h["beta1"] ** t, 1 - h["beta2"] ** t
        ref.step(lib, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, bc1, bc2)
        adam_scaled(run, lib, scale, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, bc1, bc2)
        run.read()                                 # the gaps and the tails
        for a, b in ((ref.P, run.P), (ref.M, run.M), (ref.V, run.V)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "o3d_adam_step_scaled differs from o3d_adam_step"
        grads = [T.f32(T.adam_inputs(Randn(650 + k), n, k)[3]) for k, n in enumerate(T.ADAM_JOBS)]
        ref.set_grads([g * scale for g in grads])
        run.set_grads(grads)


def test_adam_step_scaled_exact_inputs_match_the_oracle(lib):
    """the exact leg of o3d_adam_step at scale 0.5 on doubled gradients: the oracle's values, bit for bit"""
    jobs = adam_exact_jobs(0.0)
    run = AdamRun([(p, m, v, 2.0 * g) for p, m, v, g in jobs])
    adam_scaled(run, lib, 0.5, wd=0.0, **T.ADAM_EXACT)
    for (p, m, v, g), (gp, gm, gv) in zip(jobs, run.read()):
        r = T.adam_step(p, m, v, g, wd=0.0, **T.ADAM_EXACT)
        cmp("adam_scaled.m", gm, r.m, None, None, True)
        cmp("adam_scaled.v", gv, r.v, None, None, True)
        cmp("adam_scaled.p", gp, r.p, None, None, True)


# ---- o3d_sgd_step ---------------------------------------------------------------------------------------------------------
class SgdRun(AdamRun):
    """P = the parameters, M = the momentum buffer; V keeps what it was given and must come back unchanged"""

    def __init__(self, jobs):
        super().__init__([(p, buf, np.full(len(p), 0.5), g) for p, buf, g in jobs])

    def sgd(self, lib, lr, momentum, wd, scale):
        s = None if scale is None else torch.tensor([scale], dtype=torch.float32, device="cuda")
        assert lib.o3d_sgd_step(self.tab.data_ptr(), len(self.sizes), self.P.data_ptr(), self.M.data_ptr(), lr, momentum, wd,
                                None if s is None else s.data_ptr(), st()) == 0
        torch.cuda.synchronize()
        got = self.read()
        assert all((v == 0.5).all() for _, _, v in got)
        return [(p, b) for p, b, _ in got]


@pytest.mark.parametrize("wd", (0.0, 0.125))
def test_sgd_step_exact_two_steps(lib, wd):
    jobs = O.sgd_exact_jobs(wd)
    run = SgdRun(jobs)
    state = [(p, buf) for p, buf, _ in jobs]
    grads = [g for _, _, g in jobs]
    for t in range(2):
        got = run.sgd(lib, wd=wd, scale=O.SGD_EXACT_SCALE, **O.SGD_EXACT)
        for (p, buf), g, (gp, gb) in zip(state, grads, got):
            r = O.sgd_step(p, buf, g, wd=wd, scale=O.SGD_EXACT_SCALE, **O.SGD_EXACT)
            cmp("sgd.buf", gb, r.buf, None, None, True)
            cmp("sgd.p", gp, r.p, None, None, True)
        state = got
        grads = [g for _, _, g in O.sgd_exact_jobs(wd, 1)]
        run.set_grads(grads)


def test_sgd_step_zero_buffer_takes_the_gradient(lib):
    """torch's first-step rule: buf = g' exactly when the buffer is zero, and p = fma(-lr, g', p)"""
    jobs = [(p, np.zeros(len(p)), g) for p, _, _, g in (T.adam_inputs(Randn(600 + k), n, k) for k, n in enumerate(T.ADAM_JOBS))]
    run = SgdRun(jobs)
    for (p, _, g), (gp, gb) in zip(jobs, run.sgd(lib, 1e-3, 0.9, 0.0, None)):
        assert np.array_equal(bits(gb), bits(T.f32(g)))
        assert np.array_equal(bits(gp), bits(O.fma32(-np.float32(1e-3), T.f32(g), T.f32(p))))


@pytest.mark.parametrize("scale", (None, O.SGD_ROUNDED_SCALE))
@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_sgd_step_rounded_two_steps(lib, wd, scale):
    h = O.SGD_ROUNDED
    jobs = [(p, m, g) for p, m, _, g in (T.adam_inputs(Randn(600 + k), n, k) for k, n in enumerate(T.ADAM_JOBS))]
    run = SgdRun(jobs)
    state = [(T.f32(p), T.f32(buf)) for p, buf, _ in jobs]
    grads = [T.f32(g) for _, _, g in jobs]
    for t in range(2):
        got = run.sgd(lib, h["lr"], h["momentum"], wd, scale)
        for (p, buf), g, (gp, gb) in zip(state, grads, got):
            r = O.sgd_buf(p, buf, g, h["momentum"], wd, scale)
            cmp("sgd.buf", gb, r.buf, r.buf_abs, r.buf_n)
            u = O.sgd_update(p, gb, h["lr"])
            cmp("sgd.p", gp, u.p, u.p_abs, u.p_n)
        state = got
        grads = [T.f32(T.adam_inputs(Randn(650 + k), n, k)[3]) for k, n in enumerate(T.ADAM_JOBS)]
        run.set_grads(grads)
