"""The row stacks of csrc/rowmlp.hip (Linear -> BatchNorm1d over the rows -> ReLU on R <= 64 rows), called through the C ABI
with raw pointers, launch by launch, against the stage-wise numpy fp64 reference tests/rows_oracle.py (tied to
nn.Sequential(Linear, BatchNorm1d, ReLU) under autograd by tests/test_rows_oracle_cpu.py): o3d_row_mlp_fwd, o3d_row_mlp_bwd
(both gradient sources, input_mode), o3d_row_mlp_fwd_group, o3d_row_mlp_bwd_group, o3d_row_mlp_input_grad.  Same method as
tests/test_pointwise_kernels_gpu.py.  e = 2^-24 below.

EXACT leg: every input lies on a small dyadic grid, so every product and every partial sum of a correct kernel is exactly
representable in fp32 whatever its summation order (asserted before each launch and, without a GPU, by the CPU file), and
the comparison is EQUALITY: Z in the forward; dZ, db, dW, dgamma, dbeta and dX in the backward, whose Z, mean, invstd, gamma,
beta and g are inputs -- in eval mode (dZ = gamma * invstd * g) at every R, in training mode where 1 / R is a power of two.
Pre-activations planted exactly at 0 in live features have gradient 0: the mask is > 0.
ROUNDED leg: torch.randn inputs, |err| <= (n + 8) * e * sum|t_i| per output and per stage.

Forward bounds, each against fp64 over what the kernel itself stored (read back), so that no stage's bound carries another's:
  Z        vs the oracle on X, W, b: n = Cin + 1 terms (the products and the bias).
  mean     vs the fp64 mean of the stored Z: R terms z / R -> (R + 8) * e * sum|z| / R.
  invstd   vs 1 / sqrt(var + eps) of the stored Z, RELATIVE (R + 8) * e: the squared deviations are non-negative, so the R
           additions and the few roundings of a term cost at most (R + 5) * e relative in var, half of that in invstd; the
           kernel's mean differs from the fp64 mean by d <= (R + 8) * e * 16 std (the inputs keep |mean| <= 16 std per
           feature, asserted), which moves var by d^2: second order; rsqrt and one Newton step add a few ulp.
  Y        vs relu(z * sc + (beta - mean * sc)), sc = gamma * invstd, over the stored Z, mean, invstd: the kernel rounds sc,
           mean * sc, the inner and the outer fma -- four roundings of at most |z*sc| + |mean*sc| + |beta| each; bound
           8 * e * (|z*sc| + |mean*sc| + |beta|).  ReLU is 1-Lipschitz: no tie handling.  Without BatchNorm Y == Z bit for bit.
  running  vs (1 - m) * running + m * {stored mean, unbiased variance of the stored Z}: 8 * e * sum|terms|; the unbiased
           variance var * R / (R - 1) only when R > 1.  The kernel meets it because the cross-thread sum of a statistic adds
           its 32 partials in fp64 and rounds once (rows_sum): a thread's two squared deviations, the division by R, R / (R - 1)
           and the update are at most ~5 roundings of the variance term.  With that sum in fp32 (up to R roundings in var)
           the worst ratio was 1.23 at R = 64, Cin = 1024, where m * var dwarfs the running value.
In eval mode the running statistics are bit-unchanged and the stored mean is the running mean.

Backward: every stage against the oracle fed the inputs that were given; dW and db additionally against the oracle fed the
kernel's own stored dZ (n = R).  A gradient that is itself a sum (dZup . Wup, Cup terms) brings its own count and |terms|
into the stages behind it (rows_oracle.bn_bwd).  On the rounded leg the fp64 mask is the kernel's mask because no
pre-activation lies within rounding of 0 (asserted before the launch); the forward -> backward case needs no such margin:
it takes the mask from the forward's stored Y, at every element.

GUARDS: every output has a 256-element sentinel tail and two extra rows that must stay untouched, as must the pad columns
of a strided dX; X rows beyond R and the ldx padding hold NaN, and every output must be finite.  The worst err / bound per
kernel is printed and, when O3D_ROWS_PINS names a file, written there (profiles/rows_kernel_pins.txt is such a run).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import rows_oracle as O

pytestmark = pytest.mark.gpu

SENT = -7.0e37
TAIL = 256
EINVAL = -1
EXTRA_ROWS = 2
RATIOS = {}
E24 = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from open3dsot_amd import capi
    return capi.load()


@pytest.fixture(scope="module")
def structs():
    from open3dsot_amd import capi
    return capi.struct("o3d_row_fwd_args"), capi.struct("o3d_row_bwd_args")


@pytest.fixture(scope="module", autouse=True)
def _pins():
    yield
    path = os.environ.get("O3D_ROWS_PINS")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# worst |err| / bound per kernel and output, rounded legs of tests/test_rows_kernels_gpu.py;\n"
                    "# bound = (n + 8) * 2^-24 * sum|t_i| (invstd: relative (R + 8) * 2^-24); every ratio must be <= 1\n")
            for k in sorted(RATIOS):
                f.write("%-28s %.4f\n" % (k, RATIOS[k]))


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


def compare(kernel, got, ref, ref_abs, n, exact, ratios=RATIOS):
    """exact: equality.  else: |got - ref| <= (n + 8) * 2^-24 * sum|t_i| at every element, worst ratio recorded"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), kernel
    if exact:
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (kernel, len(bad), bad[:8].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        return
    bound = (np.asarray(n, np.float64) + 8) * E24 * np.asarray(ref_abs, np.float64) + 0.0 * ref
    err = np.abs(got - ref)
    assert (err[bound == 0] == 0).all(), kernel
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    ratios[kernel] = max(ratios.get(kernel, 0.0), ratio)
    print("rounded leg %s: worst err/bound %.4f" % (kernel, ratio))
    assert ratio <= 1.0, (kernel, ratio)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).cuda()


def dev_rows(A, pad=0, off=0):
    """A (R, K) as rows of stride K + pad inside a NaN-filled buffer of R + EXTRA_ROWS rows, the base `off` floats past a
    256-byte boundary -> (buffer to hold, pointer, row stride)"""
    R, K = A.shape
    ld = K + pad
    buf = torch.full((off + (R + EXTRA_ROWS) * ld + 4,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[off:off + R * ld].view(R, ld)[:, :K] = dev(A)
    return buf, buf.data_ptr() + 4 * off, ld


class Out:
    """an output (rows, cols; row stride ld >= cols) with EXTRA_ROWS more rows and a TAIL, all prefilled with the sentinel"""

    def __init__(self, rows, cols, ld=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.flat = torch.full(((rows + EXTRA_ROWS) * self.ld + TAIL,), SENT, dtype=torch.float32, device="cuda")

    @property
    def ptr(self):
        return self.flat.data_ptr()

    def host(self):
        """-> the (rows, cols) values, after checking that nothing else was written and everything written is finite"""
        a = self.flat.cpu().numpy()
        body = a[:self.rows * self.ld].reshape(self.rows, self.ld)
        assert (a[self.rows * self.ld:] == np.float32(SENT)).all(), "write beyond the output's rows"
        assert (body[:, self.cols:] == np.float32(SENT)).all(), "write into the pad columns"
        got = body[:, :self.cols].astype(np.float64)
        assert np.isfinite(got).all() and (got != np.float32(SENT)).all(), "an element was not written"
        return got

    def untouched(self):
        return bool((self.flat == SENT).all())


def optr(o):
    return None if o is None else o.ptr


def ptr(t):
    return None if t is None else t.data_ptr()


def f32(a):
    return None if a is None else np.asarray(a, np.float32).astype(np.float64)


# ---- o3d_row_mlp_fwd ---------------------------------------------------------------------------------------------------
class FwdRun:
    """device operands and outputs of one forward layer; args() is the C argument list, fields() the group job's"""

    def __init__(self, c, i):
        self.c, self.i = c, i
        self.Xb, self.Xp, self.ldx = dev_rows(i.X, c.pad, c.off)
        self.W, self.b = dev(i.W), None if i.b is None else dev(i.b)
        self.gamma, self.beta = (dev(i.gamma), dev(i.beta)) if c.bn else (None, None)
        run = c.bn and (c.running or not c.training)
        self.rm, self.rv = (Out(1, c.Cout), Out(1, c.Cout)) if run else (None, None)
        if run:
            self.rm.flat[:c.Cout], self.rv.flat[:c.Cout] = dev(i.rm), dev(i.rv)
        self.Z = Out(c.R, c.Cout) if "Z" in c.save else None
        self.mean = Out(1, c.Cout) if c.bn and "mean" in c.save else None
        self.invstd = Out(1, c.Cout) if c.bn and "invstd" in c.save else None
        self.Y = Out(c.R, c.Cout)

    def fields(self):
        c = self.c
        return (self.Xp, self.ldx, ptr(self.W), ptr(self.b), ptr(self.gamma), ptr(self.beta), optr(self.rm), optr(self.rv),
                O.MOMENTUM, O.EPS, c.training, int(c.relu), c.R, c.Cin, c.Cout, optr(self.Z), self.Y.ptr, optr(self.mean),
                optr(self.invstd))

    def launch(self, lib):
        assert lib.o3d_row_mlp_fwd(*self.fields(), st()) == 0
        torch.cuda.synchronize()

    def outputs(self):
        return [o.flat for o in (self.Y, self.Z, self.mean, self.invstd, self.rm, self.rv) if o is not None]


def check_fwd(k, run, draw):
    """every output of a finished forward launch that stored all of Z, mean, invstd against the oracle, stage by stage"""
    c, i = run.c, run.i
    ref = O.linear(i.X, i.W, i.b)
    Y, Zs = run.Y.host(), run.Z.host()
    compare(k + ".Z", Zs, ref.Z, ref.Z_abs, ref.n, draw.exact)
    if not c.bn:
        assert np.array_equal(Y, Zs), "no BatchNorm: Y != Z"
        return
    mean, invstd = run.mean.host()[0], run.invstd.host()[0]
    s = O.batch_stats(Zs)
    if c.training:
        compare(k + ".mean", mean, s.mean, s.mean_abs, c.R, False)
        want = O.invstd_of(s.var)
        compare(k + ".invstd", invstd, want, want, c.R, False)
    else:
        assert np.array_equal(run.rm.host()[0], f32(i.rm)) and np.array_equal(run.rv.host()[0], f32(i.rv)), \
            "eval mode changed the running statistics"
        assert np.array_equal(mean, f32(i.rm)), "eval mode: the stored mean is not the running mean"
        want = O.invstd_of(f32(i.rv))
        compare(k + ".invstd_eval", invstd, want, want, 3, False)      # add, rsqrt, Newton step: relative (3 + 8) * e
    a = O.bn_act(Zs, mean, invstd, i.gamma, i.beta, c.relu)
    compare(k + ".Y", Y, a.Y, a.Y_abs, 0, False)
    if c.relu:
        assert (Y >= 0).all()
    if c.training and run.rm is not None:
        u = O.running_update(f32(i.rm), f32(i.rv), mean, s.var, c.R)      # (the unbiased variance only when R > 1)
        compare(k + ".running_mean", run.rm.host()[0], u.rm, u.rm_abs, 0, False)
        compare(k + ".running_var", run.rv.host()[0], u.rv, u.rv_abs, 0, False)


ALL_SAVED = ("Z", "mean", "invstd")


def _fwd(lib, c, draw):
    """the case with everything stored, checked stage by stage; then the case as the table has it (optional outputs NULL):
    whatever it stores is bit-identical"""
    i = O.fwd_inputs(draw, c.R, c.Cin, c.Cout, c.bias, c.bn)
    ref = O.linear(i.X, i.W, i.b)
    if draw.exact:
        O.assert_exact("rows.Z", ref.Z_abs)
    if c.bn and c.training and c.R > 1:
        assert O.feature_spread(ref.Z) <= 16.0
    full = FwdRun(O._c(**dict(vars(c), save=ALL_SAVED)), i)
    full.launch(lib)
    check_fwd("row_fwd", full, draw)
    if tuple(c.save) != ALL_SAVED:
        part = FwdRun(c, i)
        part.launch(lib)
        for name in ("Y", "Z", "mean", "invstd", "rm", "rv"):
            o = getattr(part, name)
            if o is not None:
                assert torch.equal(o.flat, getattr(full, name).flat), name + " differs when an optional output is NULL"
    return full


@pytest.mark.parametrize("k", range(len(O.FWD_CASES)), ids=[O.case_id(c) for c in O.FWD_CASES])
def test_row_fwd_exact(lib, k):
    _fwd(lib, O.FWD_CASES[k], O.Dyadic(1000 + k))


@pytest.mark.parametrize("k", range(len(O.FWD_CASES)), ids=[O.case_id(c) for c in O.FWD_CASES])
def test_row_fwd_rounded(lib, k):
    _fwd(lib, O.FWD_CASES[k], Randn(31 + k))


def test_row_fwd_r1_training_keeps_the_biased_variance(lib):
    """R = 1 in training mode: var = 0, there is no unbiased estimate and nothing may be divided by R - 1 = 0: the running
    variance becomes (1 - m) * running_var + m * 0 (check_fwd, within its bound) and every output is finite"""
    _fwd(lib, O._c(R=1, Cin=72, Cout=8), Randn(77))


# ---- o3d_row_mlp_bwd ---------------------------------------------------------------------------------------------------
NULLABLE = ("dZ", "dW", "db", "dgamma", "dbeta")


class BwdRun:
    def __init__(self, c, i, null=()):
        self.c, self.i = c, i
        self.Xb, self.Xp, self.ldx = dev_rows(i.X, c.pad, c.off)
        self.Z = dev(i.Z)
        self.gamma, self.beta, self.mean, self.invstd = (dev(i.gamma), dev(i.beta), dev(i.mean), dev(i.invstd)) if c.bn else \
            (None,) * 4
        if c.cup:
            self.dZup, self.Wup, self.dYb, self.dYp, self.lddy = dev(i.dZup), dev(i.Wup), None, None, 0
        else:
            self.dZup = self.Wup = None
            self.dYb, self.dYp, self.lddy = dev_rows(i.g, c.lddy)
        self.dX = Out(c.R, c.C, c.C + O.LDDX_PAD) if c.input else None
        mk = lambda name, rows, cols: None if (name in null or c.input) else Out(rows, cols)      # noqa: E731
        self.dZ, self.dW, self.db = mk("dZ", c.R, c.C), mk("dW", c.C, c.Cin), mk("db", 1, c.C)
        self.dgamma = mk("dgamma", 1, c.C) if c.bn else None
        self.dbeta = mk("dbeta", 1, c.C) if c.bn else None

    def fields(self):
        c = self.c
        return (self.dYp, self.lddy, ptr(self.dZup), ptr(self.Wup), c.cup, int(c.input), optr(self.dX),
                c.C + O.LDDX_PAD if c.input else 0, ptr(self.Z), ptr(self.gamma), ptr(self.beta), ptr(self.mean),
                ptr(self.invstd), c.training, int(c.relu), self.Xp, self.ldx, c.R, c.Cin, c.C, optr(self.dZ), optr(self.dW),
                optr(self.db), optr(self.dgamma), optr(self.dbeta))

    def launch(self, lib):
        assert lib.o3d_row_mlp_bwd(*self.fields(), st()) == 0
        torch.cuda.synchronize()

    def outs(self):
        return {n: getattr(self, n) for n in NULLABLE + ("dX",) if getattr(self, n) is not None}


def check_bwd(k, run, draw):
    c, i = run.c, run.i
    ex = draw.exact
    if c.input:
        compare(k + ".dX", run.dX.host(), i.g, i.g_abs, i.g_n, ex)
        return
    r = O.backward(i.g, i.X, i.Z, i.mean, i.invstd, i.gamma, i.beta, c.relu, c.training, i.g_abs, i.g_n)
    got = {n: o.host() for n, o in run.outs().items()}
    if "dZ" in got:
        compare(k + ".dZ", got["dZ"], r.dZ, r.dZ_abs, r.dZ_n, ex)
        if c.bn and c.relu and not c.training:
            assert not got["dZ"][~r.mask].any(), "a gradient passed where the pre-activation is <= 0"
        w = O.wgrad(got["dZ"], i.X)           # dW / db over the kernel's own stored dZ
        if "dW" in got:
            compare(k + ".dW_of_dZ", got["dW"], w.dW, w.dW_abs, w.n, ex)
        if "db" in got:
            compare(k + ".db_of_dZ", got["db"][0], w.db, w.db_abs, w.n, ex)
    if "dW" in got:
        compare(k + ".dW", got["dW"], r.dW, r.dW_abs, r.dW_n, ex)
    if "db" in got:
        compare(k + ".db", got["db"][0], r.db, r.db_abs, r.dW_n, ex)
    if "dgamma" in got:
        compare(k + ".dgamma", got["dgamma"][0], r.dgamma, r.dgamma_abs, r.dgamma_n, ex)
    if "dbeta" in got:
        compare(k + ".dbeta", got["dbeta"][0], r.dbeta, r.dbeta_abs, r.dbeta_n, ex)
    if ex and i.planted is not None and "dZ" in got:
        row, feats = i.planted
        assert not r.mask[row, feats].any() if c.relu else True
        if c.relu and not c.training:
            assert (i.g[row, feats] != 0).all() and not got["dZ"][row, feats].any(), "gradient through a pre-activation of 0"


def bwd_pre(c, i, draw):
    """before the launch: exactness of the exact leg, the mask margin of the rounded leg"""
    if draw.exact:
        if c.input:
            O.assert_exact("rows.dX", i.g_abs)
            return
        r = O.backward(i.g, i.X, i.Z, i.mean, i.invstd, i.gamma, i.beta, c.relu, c.training, i.g_abs, i.g_n)
        e = O.exact_suffix(c)
        O.assert_exact("rows.g", i.g_abs), O.assert_exact("rows.dZ" + e, r.dZ_abs)
        O.assert_exact("rows.dW" + e, r.dW_abs), O.assert_exact("rows.db" + e, r.db_abs)
        if c.bn:
            O.assert_exact("rows.dbeta", r.dbeta_abs), O.assert_exact("rows.dgamma", r.dgamma_abs)
    elif not c.input:
        assert O.mask_margin(i, c.relu) > 16 * E24, "a pre-activation within rounding of 0: choose another seed"


def _bwd(lib, c, draw, null=()):
    i = O.bwd_inputs(draw, c)
    bwd_pre(c, i, draw)
    run = BwdRun(c, i, null)
    run.launch(lib)
    check_bwd("row_bwd", run, draw)
    return run


EXACT_BWD = [k for k, c in enumerate(O.BWD_CASES) if O.exact_ok(c)]


@pytest.mark.parametrize("k", EXACT_BWD, ids=[O.case_id(O.BWD_CASES[k]) for k in EXACT_BWD])
def test_row_bwd_exact(lib, k):
    _bwd(lib, O.BWD_CASES[k], O.Dyadic(2000 + EXACT_BWD.index(k)))


@pytest.mark.parametrize("k", range(len(O.BWD_CASES)), ids=[O.case_id(c) for c in O.BWD_CASES])
def test_row_bwd_rounded(lib, k):
    _bwd(lib, O.BWD_CASES[k], Randn(41 + k))


@pytest.mark.parametrize("k", (0, 2))
def test_row_bwd_each_output_null_in_turn(lib, k):
    """dZ, dW, db, dgamma, dbeta NULL in turn: the others are bit-identical to the launch that had them all"""
    c = O.BWD_CASES[k]
    full = _bwd(lib, c, Randn(41 + k))
    for name in NULLABLE:
        run = _bwd(lib, c, Randn(41 + k), null=(name,))
        assert getattr(run, name) is None
        for n, o in run.outs().items():
            assert torch.equal(o.flat, getattr(full, n).flat), (name, n)


def test_row_fwd_then_bwd_masks_on_the_stored_output(lib):
    """The forward (training mode, ReLU) stores Z, mean, invstd and Y; the backward recomputes y from them and promises the
    mask of the stored Y bit for bit.  dZ shows the mask at an element when the backward runs in EVAL mode on those stored
    constants (dZ = gamma * invstd * g * mask; in training mode dZ carries the batch terms at masked elements too):
    dZ == 0 exactly where Y == 0 and dZ != 0 where Y > 0 and g != 0, at every element."""
    cf = O._c(R=64, Cin=72, Cout=128)
    fwd = _fwd(lib, cf, Randn(53))
    Y = fwd.Y.host()
    assert (Y == 0).any() and (Y > 0).any()
    c = O._c(R=64, Cin=72, C=128, training=0)
    i = O.bwd_inputs(Randn(54), c)
    i.X, i.gamma, i.beta = fwd.i.X, fwd.i.gamma, fwd.i.beta
    i.Z, i.mean, i.invstd = fwd.Z.host(), fwd.mean.host()[0], fwd.invstd.host()[0]
    assert (i.gamma != 0).all() and (i.g != 0).all()
    run = BwdRun(c, i)
    run.launch(lib)
    dZ = run.dZ.host()
    assert not dZ[Y == 0].any(), "gradient passed where the forward clamped"
    assert (dZ[Y > 0] != 0).all(), "gradient dropped where the forward passed"
    # and the stages, with the forward's own mask in the oracle
    r = O.bn_bwd(i.g, i.Z, i.mean, i.invstd, i.gamma, i.beta, True, False, mask=Y > 0)
    compare("row_bwd.dZ", dZ, r.dZ, r.dZ_abs, r.dZ_n, False)
    compare("row_bwd.dbeta", run.dbeta.host()[0], r.dbeta, r.dbeta_abs, r.dbeta_n, False)
    compare("row_bwd.dgamma", run.dgamma.host()[0], r.dgamma, r.dgamma_abs, r.dgamma_n, False)
    # the same in training mode: the mask shows in dbeta = sum g * mask, a sum of the unmasked g alone
    c = O._c(R=64, Cin=72, C=128)
    run = BwdRun(c, i)
    run.launch(lib)
    r = O.bn_bwd(i.g, i.Z, i.mean, i.invstd, i.gamma, i.beta, True, True, mask=Y > 0)
    compare("row_bwd.dbeta", run.dbeta.host()[0], r.dbeta, r.dbeta_abs, r.dbeta_n, False)
    compare("row_bwd.dZ", run.dZ.host(), r.dZ, r.dZ_abs, r.dZ_n, False)


# ---- groups ------------------------------------------------------------------------------------------------------------
def _jobs(struct, runs):
    jobs = (struct * len(runs))()
    for j, r in enumerate(runs):
        jobs[j] = struct(*r.fields())
    return jobs


@pytest.mark.parametrize("njobs", (1, 4))
@pytest.mark.parametrize("exact", (True, False))
def test_row_fwd_group(lib, structs, njobs, exact):
    """jobs of unequal widths (the workgroups of a narrower job beyond its Cout return at once): every job bit-identical
    to its single launch, which is checked against the oracle"""
    widths = O.GROUP_WIDTHS[:njobs]
    mk = lambda C: O.Dyadic(1100 + C) if exact else Randn(61 + C)      # noqa: E731
    cs = [O._c(R=O.GROUP_R, Cin=O.GROUP_CIN, Cout=C) for C in widths]
    ins = [O.fwd_inputs(mk(c.Cout), c.R, c.Cin, c.Cout) for c in cs]
    if exact:
        for i in ins:
            O.assert_exact("rows.Z", O.linear(i.X, i.W, i.b).Z_abs)
    single, grouped = [FwdRun(c, i) for c, i in zip(cs, ins)], [FwdRun(c, i) for c, i in zip(cs, ins)]
    for r in single:
        r.launch(lib)
        check_fwd("row_fwd", r, mk(0))
    jobs = _jobs(structs[0], grouped)
    assert lib.o3d_row_mlp_fwd_group(ctypes.addressof(jobs), njobs, st()) == 0
    torch.cuda.synchronize()
    for a, b in zip(single, grouped):
        for x, y in zip(a.outputs(), b.outputs()):
            assert torch.equal(x, y), "a job of the group differs from its single launch"


@pytest.mark.parametrize("njobs", (1, 4))
@pytest.mark.parametrize("exact", (True, False))
def test_row_bwd_group(lib, structs, njobs, exact):
    widths = O.GROUP_WIDTHS[:njobs]
    mk = lambda C: O.Dyadic(2100 + C) if exact else Randn(67 + C)      # noqa: E731
    cs = [O._c(R=O.GROUP_R, Cin=O.GROUP_CIN, C=C, training=0 if exact else 1) for C in widths]
    ins = [O.bwd_inputs(mk(c.C), c) for c in cs]
    for c, i in zip(cs, ins):
        bwd_pre(c, i, mk(0))
    single, grouped = [BwdRun(c, i) for c, i in zip(cs, ins)], [BwdRun(c, i) for c, i in zip(cs, ins)]
    for r in single:
        r.launch(lib)
        check_bwd("row_bwd", r, mk(0))
    jobs = _jobs(structs[1], grouped)
    assert lib.o3d_row_mlp_bwd_group(ctypes.addressof(jobs), njobs, st()) == 0
    torch.cuda.synchronize()
    for a, b in zip(single, grouped):
        for n, o in a.outs().items():
            assert torch.equal(o.flat, b.outs()[n].flat), "a job of the group differs from its single launch: " + n


@pytest.mark.parametrize("nsrc", (1, 2, 4))
@pytest.mark.parametrize("exact", (True, False))
def test_row_input_grad(lib, structs, nsrc, exact):
    """dX (R, C; row stride C + 5) = the sum over nsrc sources of unequal Cup, in fp64 within (sum Cup + 8) * e * sum|t| and
    on the exact leg to equality; R, C, dX, lddx come from jobs[0]: jobs[1..] carry garbage sizes and NULLs there"""
    draw = O.Dyadic(3000) if exact else Randn(71)
    srcs = O.input_grad_sources(draw, nsrc)
    r = O.input_grad(srcs)
    if exact:
        O.assert_exact("rows.dX", r.dX_abs)
    R, C = O.INPUT_GRAD_R, O.INPUT_GRAD_C
    held = [(dev(d), dev(w)) for d, w in srcs]
    dX = Out(R, C, C + O.LDDX_PAD)
    Bwd = structs[1]
    jobs = (Bwd * nsrc)()
    for j, (d, w) in enumerate(held):
        a = Bwd()
        a.dZup, a.Wup, a.Cup = d.data_ptr(), w.data_ptr(), d.shape[1]
        if j == 0:
            a.R, a.C, a.dX, a.lddx = R, C, dX.ptr, C + O.LDDX_PAD
        else:
            a.R, a.C, a.dX, a.lddx, a.Cin, a.ldx, a.lddy = 9999, -3, None, 1, -7, 12345, -1
        jobs[j] = a
    assert lib.o3d_row_mlp_input_grad(ctypes.addressof(jobs), nsrc, st()) == 0
    torch.cuda.synchronize()
    compare("row_input_grad.dX", dX.host(), r.dX, r.dX_abs, r.n, exact)


# ---- refusals: each is rejected on the host before any launch (csrc/rowmlp.hip) ------------------------------------------
def test_row_refusals(lib, structs):
    Fwd, Bwd = structs
    z = torch.zeros(66 * 1100, device="cuda")
    outs = [Out(66, 128) for _ in range(6)]
    p = z.data_ptr()
    o = [x.ptr for x in outs]

    def fwd(R=8, Cin=16, Cout=8, ldx=None):
        return (p, Cin if ldx is None else ldx, p, p, p, p, o[0], o[1], 0.1, 1e-5, 1, 1, R, Cin, Cout, o[2], o[3], o[4], o[5])

    def bwd(R=8, C=8, Cin=16, dY=p, lddy=None, Cup=0, input_mode=0, gamma=p, relu=1):
        return (dY, C if lddy is None else lddy, None if dY else p, None if dY else p, Cup, input_mode,
                o[5] if input_mode else None, C, p, gamma, p, p, p, 1, relu, p, Cin, R, Cin, C, o[0], o[1], o[2], o[3], o[4])

    s = st()
    # R = 65 > RM_RMAX: the first `if` of o3d_row_mlp_fwd / o3d_row_mlp_bwd, row_fwd_ok / row_bwd_ok in the group entries
    assert lib.o3d_row_mlp_fwd(*fwd(R=65), s) == EINVAL
    assert lib.o3d_row_mlp_bwd(*bwd(R=65), s) == EINVAL
    # Cin = 1025 > RM_KMAX (the LDS weight slice): the first `if` of o3d_row_mlp_fwd, row_fwd_ok
    assert lib.o3d_row_mlp_fwd(*fwd(Cin=1025), s) == EINVAL
    # Cup = 1025 > RM_KMAX: the first `if` of o3d_row_mlp_bwd (the !dY branch), row_bwd_ok
    assert lib.o3d_row_mlp_bwd(*bwd(dY=None, Cup=1025), s) == EINVAL
    # relu without gamma: the `else if` of o3d_row_mlp_bwd, the last clause of row_bwd_ok
    assert lib.o3d_row_mlp_bwd(*bwd(gamma=None, relu=1), s) == EINVAL
    # lddy < C: the first `if` of o3d_row_mlp_bwd, row_bwd_ok
    assert lib.o3d_row_mlp_bwd(*bwd(lddy=7), s) == EINVAL
    # 5 jobs > RM_GROUP: the first line of each group entry, before a job is read
    fj, bj = (Fwd * 5)(*[Fwd(*fwd()) for _ in range(5)]), (Bwd * 5)(*[Bwd(*bwd()) for _ in range(5)])
    assert lib.o3d_row_mlp_fwd_group(ctypes.addressof(fj), 5, s) == EINVAL
    assert lib.o3d_row_mlp_bwd_group(ctypes.addressof(bj), 5, s) == EINVAL
    ij = (Bwd * 5)(*[Bwd(*bwd(dY=None, Cup=8, input_mode=1)) for _ in range(5)])
    assert lib.o3d_row_mlp_input_grad(ctypes.addressof(ij), 5, s) == EINVAL
    # a refused job inside a group refuses the launch: row_fwd_ok / row_bwd_ok in the loop over the jobs
    fj = (Fwd * 2)(Fwd(*fwd()), Fwd(*fwd(R=65)))
    assert lib.o3d_row_mlp_fwd_group(ctypes.addressof(fj), 2, s) == EINVAL
    # input_mode inside a bwd group: `|| jobs[j].input_mode` in the loop of o3d_row_mlp_bwd_group
    bj = (Bwd * 2)(Bwd(*bwd()), Bwd(*bwd(dY=None, Cup=8, input_mode=1)))
    assert lib.o3d_row_mlp_bwd_group(ctypes.addressof(bj), 2, s) == EINVAL
    # Cup = 1025 in a source of o3d_row_mlp_input_grad: row_bwd_ok on the patched job
    ij = (Bwd * 2)(Bwd(*bwd(dY=None, Cup=8, input_mode=1)), Bwd(*bwd(dY=None, Cup=1025, input_mode=1)))
    assert lib.o3d_row_mlp_input_grad(ctypes.addressof(ij), 2, s) == EINVAL
    torch.cuda.synchronize()
    assert all(x.untouched() for x in outs)
