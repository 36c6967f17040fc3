"""Plain numpy fp64 restatement of csrc/optim.hip -- no torch, no GPU: o3d_grad_norm (the total gradient norm and
torch.nn.utils.clip_grad_norm_'s coefficient) and o3d_sgd_step (torch.optim.SGD with momentum, dampening 0, no Nesterov).
o3d_adam_step_scaled has no formula of its own: it is tests/tail_oracle.py's adam_step on g * scale.  As in tail_oracle, next
to a value `x` stand `x_abs` = sum|t_i| of its terms and `x_n` = the roundings a value of the kernel passes through, the two
figures of |err| <= (n + 8) * 2^-24 * sum|t_i|.  tests/test_optim_oracle_cpu.py ties the formulas to torch.

Roundings of o3d_sgd_step, from the four stated operations (the kernel is built without contraction: nothing else rounds):
  buf   5: g * scale; fma(wd, p, .) and the float wd; fma(momentum, buf, .) and the float momentum.  The scale is a float in
           device memory and enters the oracle as that float: no rounding of its own.
  p     2, against the update computed in fp64 from the STORED buffer: the float lr, the fma.  sum|t| = |p| + |lr * buf|.
"""
import math

import numpy as np

import tail_oracle as T
from tail_oracle import Ref, f64

SGD_EXACT = dict(lr=2.0 ** -3, momentum=0.5)          # with scale 0.5 and wd in (0, 0.125): powers of two throughout
SGD_EXACT_SCALE = 0.5
SGD_ROUNDED = dict(lr=1e-3, momentum=0.9)
SGD_ROUNDED_SCALE = float(np.float32(0.37))
NORM_SLICES = 32                                       # O3D_NORM_SLICES of include/o3dsot.h (asserted by the CPU test)


def grad_norm(grads, max_norm):
    """-> S = sum g^2 (correctly rounded: math.fsum over the exact fp64 squares' nearest doubles), norm = sqrt(S),
    coef = min(1, max_norm / (norm + 1e-6)), all fp64"""
    S = math.fsum(float(x) for g in grads for x in (np.asarray(g, np.float64).reshape(-1) ** 2))
    norm = math.sqrt(S)
    c = max_norm / (norm + 1e-6)
    return Ref(S=S, norm=norm, coef=1.0 if c > 1.0 else c, terms=sum(int(np.size(g)) for g in grads))


def sgd_buf(p, buf, g, momentum, wd, scale=None):
    p, buf, g = map(f64, (p, buf, g))
    dt = T.DT[-1]
    gs = g if scale is None else g * dt(scale)
    ge = gs + dt(wd) * p if wd != 0 else gs
    b2 = dt(momentum) * buf + ge
    return Ref(buf=b2, buf_abs=np.abs(momentum * buf) + np.abs(gs) + np.abs(wd * p), buf_n=5)


def sgd_update(p, buf2, lr):
    p, buf2 = map(f64, (p, buf2))
    u = T.DT[-1](lr) * buf2
    return Ref(p=p - u, p_abs=np.abs(p) + np.abs(u), p_n=2)


def sgd_step(p, buf, g, lr, momentum, wd, scale=None):
    """torch.optim.SGD's update on g * scale: g' = g * scale; g' += wd * p; buf = momentum * buf + g'; p -= lr * buf"""
    r = sgd_buf(p, buf, g, momentum, wd, scale)
    r.__dict__.update(sgd_update(p, r.buf, lr).__dict__)
    return r


def fma32(a, b, c):
    """float32 fma of float32 operands: the product of two floats is exact in fp64; the fp64 sum is rounded once more to float
    (a double rounding that differs from the fused result only at a tie of the second rounding)"""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    return (a * b + c).astype(np.float32)


def sgd_step_f32(p, buf, g, lr, momentum, wd, scale=None):
    """the kernel's four operations in numpy float32, hyper-parameters rounded to float as the entry point does"""
    p, buf, g = (np.asarray(x, np.float32) for x in (p, buf, g))
    if scale is not None:
        g = g * np.float32(scale)
    if np.float32(wd) != 0:
        g = fma32(np.float32(wd), p, g)
    b2 = fma32(np.float32(momentum), buf, g)
    return Ref(buf=b2, p=fma32(-np.float32(lr), b2, p))


def sgd_exact_jobs(wd, step=0):
    """(p, buf, g) per job of T.ADAM_JOBS, built like tests/test_tail_kernels_gpu.py::adam_exact_jobs: g = +-2^k, buf and p
    dyadic, and with wd != 0 p a multiple of g / wd.  step 1: the gradients of the second step (p and buf are then the first
    step's results)"""
    jobs = []
    for k, n in enumerate(T.ADAM_JOBS):
        draw = T.Dyadic(8000 + 100 * step + k)
        e = np.abs(draw.val((n,), 1.0, 1.0 if wd else 3.0))
        g = T._signs(draw, (n,)) * 2.0 ** e
        buf = draw.val((n,), 0.25, 4.0)
        p = g / wd * T._pick(draw, (0.0, 1.0, 3.0), (n,)) if wd else draw.val((n,), 0.125, 4.0)
        jobs.append((p, buf, g))
    return jobs


def norm_exact_grads():
    """g = +-2^k, k in [-3, 3], a zero now and then: every square and every partial sum of squares is a multiple of 2^-6
    below 2^22, exact in double (and the norm's fp64 square root is the only rounding before the cast to float)"""
    out = []
    for k, n in enumerate(T.ADAM_JOBS):
        draw = T.Dyadic(8500 + k)
        g = T._signs(draw, (n,)) * 2.0 ** draw.val((n,), 1.0, 3.0)
        g[draw.val((n,), 1.0, 4.0) == 0] = 0.0
        out.append(g)
    return out


def norm_rounded_grads(seed=700):
    """T.adam_inputs' gradients: |g| in [1e-15, 1e15] on a log grid for the odd jobs, of order 1 for the even ones, zeros in
    front.  n = 37163 terms: double accumulation errs by at most n * 2^-53 relative, far below the float's 2^-24"""
    from test_rows_kernels_gpu import Randn
    return [T.f32(T.adam_inputs(Randn(seed + k), n, k)[3]) for k, n in enumerate(T.ADAM_JOBS)]


def ulp32(x):
    return float(np.spacing(np.abs(np.float32(x))))
