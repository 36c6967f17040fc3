"""o3d_sa_eval_fused (csrc/sa_eval.hip: the one kernel behind every eval-mode set abstraction) and o3d_bn_eval_consts
(csrc/heads.hip: the {mean, invstd, scale, shift} vectors every eval path consumes), called through the C ABI with raw
pointers against the numpy fp64 reference tests/sa_eval_oracle.py (tied to conv2d / batch_norm / amax on the grouped tensor
by tests/test_sa_eval_oracle_cpu.py).  Same method as tests/test_pointwise_kernels_gpu.py.  e = 2^-24.

o3d_sa_eval_fused
  EXACT leg: Z, W0, centres, W1, W2, scale and shift on dyadic grids: every product and partial sum of a correct kernel is
  exact in fp32 in any order (sum|terms| / spacing < 2^24 per layer, asserted before the launch and on the CPU), so every
  output element must EQUAL the oracle's.
  ROUNDED leg: torch.randn inputs against the bound propagated through the three layers (the recursion is written out in
  tests/sa_eval_oracle.py: each layer's own (K + 8) * e * sum|t| plus |W| . the previous layer's bound, scaled by |scale|;
  ReLU and max are 1-Lipschitz).  The worst err / bound is recorded per case.
  The cases reach what the documented contract allows and the workloads never ran: G = C0 / 8 in {1, 2, 3, 4, 5, 8} through
  the weight ring (clamped initial loads, the tail guard), 5 row tiles over 4 waves, every pool step (ns = 1 .. 32), a
  workgroup across a cloud boundary, centers NULL / ldw 3 / 19, pt_base > 0 with ld > N, ldz beyond the columns in use, the
  dynamic-LDS path.  Every Z column that no index names and every W0 column beyond 2 holds NaN: the output must be finite.
  The CPU file proves that every slot position decides some output, that outputs are > 0 and exactly 0, that padded balls
  repeat an index.
o3d_bn_eval_consts
  mean    = running_mean - conv_bias: two terms, (2 + 8) * e * (|running_mean| + |conv_bias|); conv_bias NULL: bit-equal.
  invstd  relative (3 + 8) * e: the add, the sqrt and the divide are three roundings.
  scale, shift vs fp64 over the kernel's OWN stored mean and invstd: 8 * e * sum|terms| (gamma * invstd; beta, mean * scale).
  Every one of the nrep copies is bit-identical to the first; the vector's tail is untouched.
GUARDS: every output has a 256-element sentinel tail.  When O3D_SA_EVAL_PINS names a file the worst ratios are written there
(profiles/sa_eval_kernel_pins.txt is such a run).
"""
import os

import numpy as np
import pytest
import torch

import sa_eval_oracle as O

pytestmark = pytest.mark.gpu

SENT = -7.0e37
TAIL = 256
EINVAL = -1
RATIOS = {}


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi
    return capi.load()


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_SA_EVAL_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound, rounded legs of tests/test_sa_eval_kernels_gpu.py; sa_eval: the bound propagated\n"
                    "# through the three layers (tests/sa_eval_oracle.py); bn_eval_consts: see that file's docstring;\n"
                    "# every ratio must be <= 1\n")
            for k in sorted(RATIOS):
                f.write("%-52s %.4f\n" % (k, RATIOS[k]))


def st():
    return torch.cuda.current_stream().cuda_stream


class Randn:
    """torch.randn fp32 values (handed to the oracle as the fp64 numbers they are)"""
    exact = False

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def val(self, shape, step=None, lim=None):
        return torch.randn(shape, generator=self.g, dtype=torch.float32).double().numpy()

    def coef(self, shape, zero=True):
        return self.val(shape)


def compare(kernel, got, ref, bound, exact, ratios=RATIOS):
    """exact: equality.  else |got - ref| <= bound at every element, the worst ratio recorded"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), kernel
    if exact:
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (kernel, len(bad), bad[:8].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        return
    bound = np.asarray(bound, np.float64) + 0.0 * ref
    err = np.abs(got - ref)
    assert (err[bound == 0] == 0).all(), kernel
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    ratios[kernel] = max(ratios.get(kernel, 0.0), ratio)
    print("rounded leg %s: worst err/bound %.4f" % (kernel, ratio))
    assert ratio <= 1.0, (kernel, ratio)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).cuda()


def outbuf(shape):
    n = int(np.prod(shape))
    flat = torch.full((n + TAIL,), SENT, dtype=torch.float32, device="cuda")
    return flat, flat[:n].view(shape)


def tail_intact(flat):
    assert bool((flat[-TAIL:] == SENT).all()), "write beyond the buffer"


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- o3d_sa_eval_fused -------------------------------------------------------------------------------------------------
def _sa(lib, k, draw):
    c = O.CASES[k]
    i = O.inputs(draw, c, k)
    Zh = i.Z.copy()
    Zh[:, ~i.used] = np.nan                                    # no index names these columns
    ldw = c.ldw or 3
    W0h = np.full((c.C0, ldw), np.nan)
    W0h[:, :3] = i.W0
    Z, W0, W1, W2 = dev(Zh), dev(W0h), dev(i.W1), dev(i.W2)
    v0, v1, v2 = dev(i.v0), dev(i.v1), dev(i.v2)
    assert all(t.data_ptr() % 16 == 0 for t in (W1, W2, v1, v2))
    for n, s in enumerate(i.sets):
        r = O.run(i, s)
        if draw.exact:
            O.assert_exact("sa.A0", r.T0), O.assert_exact("sa.A1", r.T1), O.assert_exact("sa.A2", r.T2)
        idx = torch.from_numpy(s.idx.astype(np.int32)).cuda()
        assert int(idx.max()) < O.N_POINTS <= s.ld and s.pt_base + s.B * s.ld <= i.ldz      # every read inside Z
        ctr = dev(s.centers) if s.centers is not None else None
        Of, out = outbuf((s.B, c.C2, s.npoint))
        rc = lib.o3d_sa_eval_fused(ptr(Z), i.ldz, ptr(idx), ptr(ctr), ptr(W0), ldw, ptr(v0), ptr(W1), ptr(v1), ptr(W2), ptr(v2),
                                   c.C0, c.C1, c.C2, s.B, s.npoint, s.ns, s.ld, s.pt_base, ptr(out), st())
        torch.cuda.synchronize()
        assert rc == 0
        tail_intact(Of)
        got = out.cpu().numpy().astype(np.float64)
        assert (got != np.float32(SENT)).all(), "an output element was not written"
        compare("sa_eval.%s%s" % (O.case_id(c), ".set%d" % n if c.second else ""), got, r.out, r.bound, draw.exact)
        assert (got >= 0).all() and not got[:, 1].any(), "the clamped channel"


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=[O.case_id(c) for c in O.CASES])
def test_sa_eval_exact(lib, k):
    _sa(lib, k, O.Dyadic(4000 + k))


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=[O.case_id(c) for c in O.CASES])
def test_sa_eval_rounded(lib, k):
    _sa(lib, k, Randn(83 + k))


def test_sa_eval_refusals(lib):
    """every one is rejected by the single `if` at the top of o3d_sa_eval_fused (csrc/sa_eval.hip), before the LDS attribute
    is set and before the launch; nothing is written"""
    z = torch.zeros(64 * 64 + 8, device="cuda")
    zi = torch.zeros(2048, dtype=torch.int32, device="cuda")
    Of, out = outbuf((1, 64, 64))
    p, pi = z.data_ptr(), zi.data_ptr()
    assert p % 16 == 0

    def call(C0=8, C1=32, C2=32, B=1, npoint=8, ns=4, centers=p, ldw=3, v1=p):
        return lib.o3d_sa_eval_fused(p, 64, pi, centers, p, ldw, p, p, v1, p, p, C0, C1, C2, B, npoint, ns, 32, 0, ptr(out), st())

    assert call(C0=12) == EINVAL                      # `C0 % 8`
    assert call(C1=48) == EINVAL                      # `C1 % 32`
    assert call(ns=3, npoint=32) == EINVAL            # `(ns & (ns - 1))`
    assert call(ns=64) == EINVAL                      # `ns > 32`
    assert call(npoint=12) == EINVAL                  # `slots % 32 != 0`: 1 * 12 * 4 = 48
    assert call(v1=p + 4) == EINVAL                   # `((uintptr_t)v1 & 15)`: read as float4
    assert call(ldw=2) == EINVAL                      # `(centers && (!W0 || ldw < 3))`
    # (a W1 / W2 off a 16-byte boundary is NOT refused: the trackers pass views of the optimizer's flat parameter buffer,
    #  tests/test_model_gpu.py::test_train_eval_train_eval_uses_fresh_batchnorm_constants; this file launches none)
    torch.cuda.synchronize()
    assert bool((Of == SENT).all())


# ---- o3d_bn_eval_consts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrep", O.BN_CONSTS_NREP)
@pytest.mark.parametrize("C", O.BN_CONSTS_C)
def test_bn_eval_consts(lib, C, nrep):
    d = Randn(97 + C)
    rm, rv, gamma, beta, bias = d.val((C,)), 0.5 + np.abs(d.val((C,))), d.val((C,)), d.val((C,)), d.val((C,))
    rv = rv.astype(np.float32).astype(np.float64)
    D = [dev(a) for a in (rm, rv, gamma, beta, bias)]
    for with_bias in (False, True):
        Vf, vec = outbuf((4, nrep, C))
        assert lib.o3d_bn_eval_consts(ptr(D[0]), ptr(D[1]), ptr(D[2]), ptr(D[3]), ptr(D[4]) if with_bias else None, O.EPS, C, nrep,
                                      ptr(vec), st()) == 0
        torch.cuda.synchronize()
        tail_intact(Vf)
        got = vec.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and (got == got[:, :1]).all(), "the nrep copies differ"
        mean, invstd, scale, shift = got[:, 0]
        want = O.bn_eval_consts(rm, rv, gamma, beta, bias if with_bias else None)[:, 0]
        if with_bias:
            compare("bn_eval_consts.mean", mean, want[0], (2 + 8) * O.E24 * (np.abs(rm) + np.abs(bias)), False)
        else:
            assert np.array_equal(mean, rm), "no conv_bias: mean != running_mean"
        compare("bn_eval_consts.invstd", invstd, want[1], (3 + 8) * O.E24 * want[1], False)
        s = O.scale_shift_of(mean, invstd, gamma, beta)
        compare("bn_eval_consts.scale", scale, s.scale, 8 * O.E24 * s.scale_abs, False)
        compare("bn_eval_consts.shift", shift, s.shift, 8 * O.E24 * s.shift_abs, False)


def test_bn_eval_consts_refusals(lib):
    """the single `if` at the top of o3d_bn_eval_consts (csrc/heads.hip)"""
    one = torch.ones(8, device="cuda")
    Vf, vec = outbuf((4, 1, 8))
    p = one.data_ptr()
    assert lib.o3d_bn_eval_consts(p, p, p, p, None, O.EPS, 0, 1, ptr(vec), st()) == EINVAL      # `C <= 0`
    assert lib.o3d_bn_eval_consts(p, p, p, p, None, O.EPS, 8, 0, ptr(vec), st()) == EINVAL      # `nrep <= 0`
    assert lib.o3d_bn_eval_consts(p, None, p, p, None, O.EPS, 8, 1, ptr(vec), st()) == EINVAL   # `!running_var`
    torch.cuda.synchronize()
    assert bool((Vf == SENT).all())
