"""Plain numpy fp64 reference of the row stacks of csrc/rowmlp.hip, written from what include/o3dsot.h documents for
o3d_row_mlp_fwd, o3d_row_mlp_bwd (both gradient sources, input_mode), o3d_row_mlp_fwd_group, o3d_row_mlp_bwd_group and
o3d_row_mlp_input_grad.  It imports nothing of the package under test.  Shared by tests/test_rows_oracle_cpu.py (which ties
the composed stages to nn.Sequential(Linear, BatchNorm1d, ReLU) in fp64 under autograd) and tests/test_rows_kernels_gpu.py
(which pins every entry point to it, launch by launch).

STAGE-WISE: every stage takes its inputs as arguments, so that the GPU file can feed it the kernel's own stored
intermediates (the stored Z for the statistics, the stored dZ for dW / db).  As in the other oracles every stage takes the
fp32 inputs as the fp64 numbers they are and returns a Ref: per output the value, *_abs = the same sum over the absolute
values of every product that enters a term, and *_n = the number of terms -- the yardsticks of the exactness condition
(sum|terms| / spacing < 2^24) and of the rounding bound (n + 8) * 2^-24 * sum|terms| (tests/compact_oracle.py).

  linear          Z (R, Cout) = X . W^T + b                                   n = Cin + 1
  batch_stats     mean, biased var of a Z over its rows                        n = R
  bn_act          Y = act(z * sc + (beta - mean * sc)), sc = gamma * invstd    Y_abs = |z*sc| + |mean*sc| + |beta|
  running_update  (1 - m) * running + m * {mean, var * R / (R - 1) if R > 1}   *_abs = the two |terms|
  source_up       g (R, C) = dZup (R, Cup) . Wup (Cup, C)                      n = Cup
  bn_bwd          mask = y > 0 (STRICT; y as bn_act, or a mask that is given), gm = g * mask, dbeta = sum gm,
                  dgamma = sum gm * xhat, xhat = (z - mean) * invstd,
                  dZ = sc * (gm - dbeta / R - xhat * dgamma / R) in training, sc * gm in eval; no BatchNorm: dZ = g
  wgrad           dW (C, Cin) = dZ^T . X, db (C) = sum over the rows of dZ     n = R
  input_grad      dX = sum over the sources of dZup_j . Wup_j                  n = sum Cup_j

The case tables of tests/test_rows_kernels_gpu.py and the input grids of its exact legs live here too, so that the CPU file
proves the exactness condition of every exact case without a GPU.
"""
from types import SimpleNamespace as Ref

import numpy as np

import compact_oracle as CO
from compact_oracle import Dyadic, TWO24  # noqa: F401  (re-exported for the tests)

f64 = lambda a: np.asarray(a, np.float64)      # noqa: E731
EPS = float(np.float32(1e-5))
MOMENTUM = float(np.float32(0.1))

# grid spacing of the terms of every exactly compared output (products of the input steps of fwd_inputs / bwd_inputs)
SPACING = {"rows.Z": 1.0 / 8, "rows.g": 1.0 / 4, "rows.dbeta": 1.0 / 4, "rows.dgamma": 1.0 / 16, "rows.dZ": 2.0 ** -15,
           "rows.dW": 2.0 ** -16, "rows.db": 2.0 ** -15, "rows.dX": 1.0 / 4,
           # eval mode and no BatchNorm: dZ = gamma * invstd * g, no division by R
           "rows.dZ.eval": 1.0 / 16, "rows.dW.eval": 1.0 / 32, "rows.db.eval": 1.0 / 16}
CO.SPACING.update(SPACING)
assert_exact = CO.assert_exact


# ---- forward stages ------------------------------------------------------------------------------------------------------
def linear(X, W, b=None):
    X, W = f64(X), f64(W)
    Z, Za = X @ W.T, np.abs(X) @ np.abs(W).T
    if b is not None:
        Z, Za = Z + f64(b)[None, :], Za + np.abs(f64(b))[None, :]
    return Ref(Z=Z, Z_abs=Za, n=X.shape[1] + 1)


def batch_stats(Z):
    """-> Ref(mean, mean_abs = sum|z| / R, var (biased), n = R)"""
    Z = f64(Z)
    mean = Z.mean(0)
    return Ref(mean=mean, mean_abs=np.abs(Z).mean(0), var=((Z - mean[None, :]) ** 2).mean(0), n=Z.shape[0])


def invstd_of(var, eps=EPS):
    return 1.0 / np.sqrt(f64(var) + eps)


def bn_act(Z, mean=None, invstd=None, gamma=None, beta=None, relu=False):
    """gamma None: no BatchNorm, Y = Z (and no ReLU: the stacks have none without a BatchNorm)"""
    Z = f64(Z)
    if gamma is None:
        assert not relu
        return Ref(Y=Z.copy(), Y_abs=np.abs(Z), pre=Z.copy())
    sc = (f64(gamma) * f64(invstd))[None, :]
    mu, bt = f64(mean)[None, :], f64(beta)[None, :]
    pre = Z * sc + (bt - mu * sc)
    return Ref(Y=np.maximum(pre, 0.0) if relu else pre, Y_abs=np.abs(Z * sc) + np.abs(mu * sc) + np.abs(bt) + 0.0 * Z, pre=pre)


def running_update(rm, rv, mean, var, R, momentum=MOMENTUM):
    """torch's update: the UNBIASED variance var * R / (R - 1) when R > 1, the biased one at R = 1"""
    unb = f64(var) * R / (R - 1) if R > 1 else f64(var)
    m = momentum
    return Ref(rm=(1 - m) * f64(rm) + m * f64(mean), rm_abs=np.abs((1 - m) * f64(rm)) + np.abs(m * f64(mean)),
               rv=(1 - m) * f64(rv) + m * unb, rv_abs=np.abs((1 - m) * f64(rv)) + np.abs(m * unb))


def forward(X, W, b, gamma, beta, rm, rv, training, relu, eps=EPS, momentum=MOMENTUM):
    """the composed layer, as o3d_row_mlp_fwd documents it -> Ref(Z, Y, mean, invstd, rm, rv (after the call))"""
    z = linear(X, W, b)
    if gamma is None:
        return Ref(Z=z.Z, Y=bn_act(z.Z).Y, mean=None, invstd=None, rm=rm, rv=rv)
    if training:
        s = batch_stats(z.Z)
        mean, invstd = s.mean, invstd_of(s.var, eps)
        if rm is not None:
            u = running_update(rm, rv, s.mean, s.var, z.Z.shape[0], momentum)
            rm, rv = u.rm, u.rv
    else:
        mean, invstd = f64(rm), invstd_of(rv, eps)
    return Ref(Z=z.Z, Y=bn_act(z.Z, mean, invstd, gamma, beta, relu).Y, mean=mean, invstd=invstd, rm=rm, rv=rv)


# ---- backward stages -----------------------------------------------------------------------------------------------------
def source_up(dZup, Wup):
    dZup, Wup = f64(dZup), f64(Wup)
    return Ref(g=dZup @ Wup, g_abs=np.abs(dZup) @ np.abs(Wup), n=dZup.shape[1])


def input_grad(sources):
    """sources: [(dZup_j (R, Cup_j), Wup_j (Cup_j, C))] -> Ref(dX, dX_abs, n = sum Cup_j)"""
    ups = [source_up(d, w) for d, w in sources]
    return Ref(dX=sum(u.g for u in ups), dX_abs=sum(u.g_abs for u in ups), n=sum(u.n for u in ups))


def bn_bwd(g, Z=None, mean=None, invstd=None, gamma=None, beta=None, relu=False, training=True, mask=None, g_abs=None,
           g_n=1):
    """g: the gradient of the layer's output, with its own |terms| and term count when it is itself a sum (source_up).
    -> Ref(mask, dZ, dZ_abs, dZ_n, dgamma, dgamma_abs, dgamma_n, dbeta, dbeta_abs, dbeta_n)
    term counts: dbeta = R sums of a g; dgamma two more roundings (xhat); dZ in training takes dgamma's chain, xhat * dgamma
    / R, the two subtractions and the scale: R + 4 beyond g's own count (the + 8 of the bound covers the rest)."""
    g = f64(g)
    ga = np.abs(g) if g_abs is None else f64(g_abs)
    R = g.shape[0]
    if gamma is None:
        assert not relu
        return Ref(mask=np.ones(g.shape, bool), dZ=g.copy(), dZ_abs=ga.copy(), dZ_n=g_n, dgamma=None, dbeta=None)
    Z, mu, istd, gm_, bt = f64(Z), f64(mean)[None, :], f64(invstd)[None, :], f64(gamma)[None, :], f64(beta)[None, :]
    sc = gm_ * istd
    if mask is None:
        mask = (Z * sc + (bt - mu * sc) > 0) if relu else np.ones(g.shape, bool)
    gm, gma = np.where(mask, g, 0.0), np.where(mask, ga, 0.0)
    xh, xha = (Z - mu) * istd, (np.abs(Z) + np.abs(mu)) * np.abs(istd)
    r = Ref(mask=mask, dbeta=gm.sum(0), dbeta_abs=gma.sum(0), dbeta_n=g_n + R, dgamma=(gm * xh).sum(0),
            dgamma_abs=(gma * xha).sum(0), dgamma_n=g_n + R + 2)
    if training:
        r.dZ = sc * (gm - r.dbeta[None, :] / R - xh * r.dgamma[None, :] / R)
        r.dZ_abs = np.abs(sc) * (gma + r.dbeta_abs[None, :] / R + xha * r.dgamma_abs[None, :] / R)
        r.dZ_n = g_n + R + 4
    else:
        r.dZ, r.dZ_abs, r.dZ_n = sc * gm, np.abs(sc) * gma, g_n + 2
    return r


def wgrad(dZ, X):
    dZ, X = f64(dZ), f64(X)
    return Ref(dW=dZ.T @ X, dW_abs=np.abs(dZ).T @ np.abs(X), db=dZ.sum(0), db_abs=np.abs(dZ).sum(0), n=dZ.shape[0])


def backward(g, X, Z, mean, invstd, gamma, beta, relu, training, g_abs=None, g_n=1):
    """the composed layer backward, as o3d_row_mlp_bwd documents it"""
    r = bn_bwd(g, Z, mean, invstd, gamma, beta, relu, training, g_abs=g_abs, g_n=g_n)
    w = wgrad(r.dZ, X)
    r.dW, r.db = w.dW, w.db
    # dW / db of the composition: the |terms| go through dZ's own |terms|
    r.dW_abs, r.db_abs, r.dW_n = r.dZ_abs.T @ np.abs(f64(X)), r.dZ_abs.sum(0), r.dZ_n + w.n
    return r


# ---- case tables of tests/test_rows_kernels_gpu.py -----------------------------------------------------------------------
def _c(**kw):
    d = dict(pad=0, off=0, bias=True, bn=True, relu=True, training=1, save=("Z", "mean", "invstd"), running=True, lddy=0,
             cup=0, input=False)
    d.update(kw)
    return Ref(**d)


# forward: X (R, Cin) with row stride Cin + pad, its base `off` floats past a 16-byte boundary; save: the optional outputs
# that are given; running: running_mean / running_var given (always in eval mode)
FWD_CASES = [
    _c(R=1, Cin=72, Cout=8, training=0),                                   # the per-frame tracker
    _c(R=5, Cin=3, Cout=4),
    _c(R=31, Cin=70, Cout=9, bias=False),                                  # K % 4 != 0: the scalar loop
    _c(R=32, Cin=72, Cout=40, pad=3, running=False),                       # K % 4 == 0, lda % 4 != 0: the scalar loop
    _c(R=33, Cin=72, Cout=40, off=1, relu=False),                          # K % 4 == 0, base off 16 bytes: the scalar loop
    _c(R=48, Cin=260, Cout=128, bn=False, relu=False, save=("Z",)),
    _c(R=64, Cin=1024, Cout=128, save=()),                                 # the LDS slice full; nothing saved
    _c(R=64, Cin=72, Cout=9, training=0, bias=False, save=("mean", "invstd")),
]

# backward: gradient source dY (R, C; row stride C + lddy) or, cup > 0, dZup (R, cup) . Wup (cup, C); X as in the forward
# cases.  The exact leg runs where every intermediate of a correct kernel is representable: eval mode (and no BatchNorm)
# at every R, training mode where 1 / R is a power of two.
BWD_CASES = [
    _c(R=32, Cin=72, C=40),
    _c(R=64, Cin=260, C=128, lddy=5),                                      # two passes of the dW loop, the last partial
    _c(R=64, Cin=70, C=9, cup=4),
    _c(R=32, Cin=3, C=8, cup=9, relu=False),
    _c(R=5, Cin=72, C=4, pad=3, cup=128, training=0),
    _c(R=31, Cin=1024, C=40, cup=1024, training=0),
    _c(R=33, Cin=72, C=9, off=1),
    _c(R=48, Cin=260, C=128, bn=False, relu=False),
    _c(R=1, Cin=72, C=8, training=0),
    _c(R=48, Cin=70, C=40, lddy=5),
    _c(R=5, Cin=3, C=4, cup=4),
    _c(R=33, Cin=72, C=9, cup=128, input=True),                            # input_mode: dX (R, C; row stride C + 5)
    _c(R=64, Cin=72, C=128, cup=1024, input=True),
]
LDDX_PAD = 5
GROUP_WIDTHS = (4, 40, 128, 9)          # the jobs of a group launch: unequal, the widest neither first nor last
GROUP_R, GROUP_CIN = 48, 72
INPUT_GRAD_CUPS = (4, 9, 128, 1024)     # the sources of o3d_row_mlp_input_grad: the first 1, 2 and all 4 of them
INPUT_GRAD_R, INPUT_GRAD_C = 33, 40


def exact_ok(c):
    return (not c.bn) or (not c.training) or c.R in (32, 64) or c.input


def exact_suffix(c):
    """which SPACING entries a backward case's dZ / dW / db lie on"""
    return "" if (c.bn and c.training) else ".eval"


def case_id(c):
    return "R%d-Cin%d-C%d%s" % (c.R, c.Cin, getattr(c, "Cout", None) or c.C,
                                 "".join("-" + k for k, on in (("pad", c.pad), ("off", c.off), ("nobias", not c.bias),
                                                               ("nobn", not c.bn), ("norelu", c.bn and not c.relu),
                                                               ("eval", c.bn and not c.training), ("lddy", c.lddy),
                                                               ("cup%d" % c.cup, c.cup), ("input", c.input)) if on))


# ---- inputs: dyadic grids (Dyadic draw) or randn (the GPU file's Randn draw) ---------------------------------------------
def pow2(draw, shape, choices=(1.0, 0.5)):
    """exact leg: powers of two (an invstd); rounded leg: positive values around 1"""
    if draw.exact:
        return draw.rng.choice(np.array(choices), size=shape)
    return 0.5 + np.abs(draw.val(shape))


def fwd_inputs(draw, R, Cin, Cout, bias=True, bn=True):
    """the running variance is positive; |mean| <= 16 std per feature holds by construction on randn inputs and is asserted
    (feature_spread) by the CPU file and before each launch"""
    return Ref(X=draw.val((R, Cin), 0.25, 2.0), W=draw.coef((Cout, Cin)), b=draw.val((Cout,), 0.25, 1.0) if bias else None,
               gamma=draw.coef((Cout,), zero=False) if bn else None, beta=draw.val((Cout,), 0.25, 0.5) if bn else None,
               rm=draw.val((Cout,), 0.25, 0.5) if bn else None, rv=pow2(draw, (Cout,), (1.0, 0.25, 4.0)) if bn else None)


def feature_spread(Z):
    """worst |mean| / std over the features that vary (the invstd bound assumes <= 16)"""
    s = batch_stats(Z)
    live = s.var > 0
    return float((np.abs(s.mean[live]) / np.sqrt(s.var[live])).max()) if live.any() else 0.0


def bwd_inputs(draw, c):
    """Z, mean, invstd, gamma, beta and the gradient source are INPUTS of the backward: the exact leg supplies them on
    dyadic grids.  Exact leg: in every second feature beta = 0 and row min(1, R - 1) of Z sits on the mean, so the
    pre-activation there is exactly 0 -- its gradient must be 0 (the mask is > 0) although g there is not."""
    R, C, Cin = c.R, c.C, c.Cin
    i = Ref(X=draw.val((R, Cin), 0.5, 1.0), Z=draw.val((R, C), 0.5, 1.0), mean=draw.val((C,), 0.5, 0.5),
            invstd=pow2(draw, (C,)), gamma=draw.coef((C,), zero=False), beta=draw.val((C,), 0.25, 0.5), planted=None)
    if c.cup:
        i.dZup, i.Wup = draw.val((R, c.cup), 0.5, 1.0), draw.coef((c.cup, C))
        s = source_up(i.dZup, i.Wup)
        i.g, i.g_abs, i.g_n = s.g, s.g_abs, s.n
    else:
        i.g = draw.val((R, C), 0.5, 1.0)
        i.g_abs, i.g_n = np.abs(i.g), 1
    if draw.exact and c.bn:
        row, feats = min(1, R - 1), np.arange(0, C, 2)
        i.beta[feats] = 0.0
        i.Z[row, feats] = i.mean[feats]
        if not c.cup:
            i.g[row, feats] = 1.0
            i.g_abs = np.abs(i.g)
        i.planted = (row, feats)
    if not c.bn:
        i.gamma = i.beta = i.mean = i.invstd = None
    return i


def mask_margin(i, relu):
    """rounded leg: the smallest |pre-activation| / its |terms| -- the fp64 mask is the kernel's mask as long as no
    pre-activation lies within rounding (8 * 2^-24 of its terms) of 0"""
    if i.gamma is None or not relu:
        return np.inf
    a = bn_act(i.Z, i.mean, i.invstd, i.gamma, i.beta, True)
    live = a.Y_abs > 0
    return float((np.abs(a.pre[live]) / a.Y_abs[live]).min())


def exact_preconditions():
    """the exactness condition of every exact-leg input set of tests/test_rows_kernels_gpu.py -> [(name, worst)]"""
    seen = []

    def ok(name, abs_sum):
        seen.append((name, assert_exact(name, abs_sum)))

    for k, c in enumerate(FWD_CASES):
        i = fwd_inputs(Dyadic(1000 + k), c.R, c.Cin, c.Cout, c.bias, c.bn)
        ok("rows.Z", linear(i.X, i.W, i.b).Z_abs)
    for Cout in GROUP_WIDTHS:
        i = fwd_inputs(Dyadic(1100 + Cout), GROUP_R, GROUP_CIN, Cout)
        ok("rows.Z", linear(i.X, i.W, i.b).Z_abs)
    cases = [c for c in BWD_CASES if exact_ok(c)]
    cases += [_c(R=GROUP_R, Cin=GROUP_CIN, C=C, training=0) for C in GROUP_WIDTHS]
    for k, c in enumerate(cases):
        i = bwd_inputs(Dyadic(2000 + k), c)
        if c.input:
            ok("rows.dX", i.g_abs)
            continue
        r = backward(i.g, i.X, i.Z, i.mean, i.invstd, i.gamma, i.beta, c.relu, c.training, i.g_abs, i.g_n)
        e = exact_suffix(c)
        ok("rows.g", i.g_abs), ok("rows.dZ" + e, r.dZ_abs), ok("rows.dW" + e, r.dW_abs), ok("rows.db" + e, r.db_abs)
        if c.bn:
            ok("rows.dbeta", r.dbeta_abs), ok("rows.dgamma", r.dgamma_abs)
    srcs = input_grad_sources(Dyadic(3000), len(INPUT_GRAD_CUPS))
    ok("rows.dX", input_grad(srcs).dX_abs)
    return seen


def input_grad_sources(draw, n):
    return [(draw.val((INPUT_GRAD_R, cup), 0.5, 1.0), draw.coef((cup, INPUT_GRAD_C))) for cup in INPUT_GRAD_CUPS[:n]]
