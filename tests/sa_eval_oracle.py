"""Plain numpy fp64 reference of the eval-mode set abstraction o3d_sa_eval_fused (csrc/sa_eval.hip), written from the comment
above that entry point, and of o3d_bn_eval_consts (csrc/heads.hip), written from include/o3dsot.h.  It imports nothing of
the package under test.  Shared by tests/test_sa_eval_oracle_cpu.py (which ties it to F.conv2d / F.batch_norm(training=False)
/ amax on the grouped tensor in fp64) and tests/test_sa_eval_kernels_gpu.py (which pins both entry points to it).

  Y0[c, (b,j,k)] = Z[c, pt_base + b*ld + idx[b,j,k]] - W0[c, 0:3] . centers[b*np + j]          (centers None: no centre term)
  A_l = relu(scale_l * (W_l . A_{l-1}) + shift_l),  l = 1, 2;   A_0 = relu(scale_0 * Y0 + shift_0)
  out[b, c, j] = max over the ns slots k of A_2[c, (b,j,k)];    v_l (4, C_l) = {mean, invstd, scale, shift}

ERROR BOUND, propagated through the layers (e = 2^-24; T_l = the sum of the absolute values of every term of a layer's
pre-activation; b_l = a bound on |kernel's A_l - A_l|, per channel and slot):
  T_0 = |scale_0| * (|z| + sum_i |W0[c,i] * centre_i|) + |shift_0|        b_0 = (5 + 8) * e * T_0   (z, three products, shift)
  T_l = |scale_l| * (|W_l| . (|A_{l-1}| + b_{l-1})) + |shift_l|           b_l = (K_l + 8) * e * T_l + |scale_l| * (|W_l| . b_{l-1})
a layer contributes its own (K + 8) * e * sum|t| and passes on the previous layer's bound through |W|, both scaled by
|scale|; ReLU and max are 1-Lipschitz, so the pooled output's bound is the largest b_2 among the ball's slots.
The exactness condition of the exact leg is sum|terms| / spacing < 2^24 on T_0, T_1, T_2 (tests/compact_oracle.py).

The case table of the GPU file and its inputs live here, so that the CPU file proves the exactness condition and the input
conditions of every case without a GPU.
"""
from types import SimpleNamespace as Ref

import numpy as np

import compact_oracle as CO
from compact_oracle import Dyadic, TWO24  # noqa: F401  (re-exported for the tests)

f64 = lambda a: np.asarray(a, np.float64)      # noqa: E731
E24 = 2.0 ** -24
EPS = float(np.float32(1e-5))

SPACING = {"sa.A0": 1.0 / 8, "sa.A1": 1.0 / 32, "sa.A2": 1.0 / 128}
CO.SPACING.update(SPACING)
assert_exact = CO.assert_exact


def bn_eval_consts(rm, rv, gamma, beta, conv_bias=None, eps=EPS, nrep=1):
    """vec (4, nrep, C) = {mean, invstd, scale, shift}: mean = running_mean - conv_bias, invstd = 1 / sqrt(running_var + eps),
    scale = gamma * invstd, shift = beta - mean * scale; every one of the nrep copies the same"""
    mean = f64(rm) - (f64(conv_bias) if conv_bias is not None else 0.0)
    invstd = 1.0 / np.sqrt(f64(rv) + eps)
    scale = f64(gamma) * invstd
    v = np.stack([mean, invstd, scale, f64(beta) - mean * scale])
    return np.repeat(v[:, None, :], nrep, 1)


def scale_shift_of(mean, invstd, gamma, beta):
    """scale and shift from a GIVEN (the kernel's stored) mean and invstd, with the |terms| of the shift"""
    scale = f64(gamma) * f64(invstd)
    return Ref(scale=scale, scale_abs=np.abs(scale), shift=f64(beta) - f64(mean) * scale,
               shift_abs=np.abs(f64(beta)) + np.abs(f64(mean) * scale))


def gather(Z, idx, centers, W0, B, npoint, ns, ld, pt_base):
    """-> Y0 (C0, slots), its |terms|, gp (slots,) the Z column of every slot"""
    idx = np.asarray(idx, np.int64).reshape(B, npoint, ns)
    gp = (pt_base + np.arange(B)[:, None, None] * ld + idx).reshape(-1)
    Z = f64(Z)
    Y0, Ya = Z[:, gp], np.abs(Z[:, gp])
    if centers is not None:
        c = np.repeat(f64(centers).reshape(B * npoint, 3), ns, 0).T          # (3, slots)
        w = f64(W0)[:, :3]
        Y0, Ya = Y0 - w @ c, Ya + np.abs(w) @ np.abs(c)
    return Y0, Ya, gp


def sa_eval(Z, idx, centers, W0, v0, W1, v1, W2, v2, B, npoint, ns, ld, pt_base):
    """-> Ref(out (B, C2, np), bound (B, C2, np), A0, A1, A2 (C_l, slots), T0, T1, T2, arg (B, C2, np) first maximising slot,
    nmax (B, C2, np) the number of slots that attain the maximum)"""
    Y0, Ya, _ = gather(Z, idx, centers, W0, B, npoint, ns, ld, pt_base)
    sc, sh = f64(v0)[2][:, None], f64(v0)[3][:, None]
    T = [np.abs(sc) * Ya + np.abs(sh)]
    A = [np.maximum(sc * Y0 + sh, 0.0)]
    b = [(5 + 8) * E24 * T[0]]
    for W, v in ((W1, v1), (W2, v2)):
        W, sc, sh = f64(W), f64(v)[2][:, None], f64(v)[3][:, None]
        K = W.shape[1]
        T.append(np.abs(sc) * (np.abs(W) @ (np.abs(A[-1]) + b[-1])) + np.abs(sh))
        b.append((K + 8) * E24 * T[-1] + np.abs(sc) * (np.abs(W) @ b[-1]))
        A.append(np.maximum(sc * (W @ A[-1]) + sh, 0.0))
    C2 = A[2].shape[0]
    a3 = A[2].reshape(C2, B, npoint, ns)
    out = a3.max(3)
    return Ref(out=out.transpose(1, 0, 2), bound=b[2].reshape(C2, B, npoint, ns).max(3).transpose(1, 0, 2), A0=A[0], A1=A[1],
               A2=A[2], T0=T[0], T1=T[1], T2=T[2], arg=a3.argmax(3).transpose(1, 0, 2),
               nmax=(a3 == out[..., None]).sum(3).transpose(1, 0, 2))


# ---- case table of tests/test_sa_eval_kernels_gpu.py ---------------------------------------------------------------------
def _c(C0, C1, C2, B, npoint, ns, ldw=3, second=False, ldz_pad=0):
    """ldw: 0 = centers NULL, else the row stride of W0 (columns beyond 2 hold NaN on the device); second: a second set of
    clouds behind the first in the same Z (pt_base > 0, ld > N), as the two-set modules launch; ldz_pad: Z columns beyond
    the ones in use"""
    return Ref(C0=C0, C1=C1, C2=C2, B=B, npoint=npoint, ns=ns, ldw=ldw, second=second, ldz_pad=ldz_pad)


CASES = [
    _c(8, 32, 32, 1, 64, 1),                   # G = K / 8 = 1: the three initial loads of the weight ring all clamped
    _c(16, 32, 32, 1, 64, 2, ldw=0),           # G = 2; no centres
    _c(24, 32, 32, 2, 12, 4, ldw=19),          # G = 3; workgroup 1 of 3 straddles the cloud boundary
    _c(32, 32, 96, 1, 16, 8, ldz_pad=5),       # G = 4
    _c(40, 32, 32, 1, 16, 16, ldw=19),         # G = 5: G % 4 != 0, the tail guard g + u < G
    _c(64, 32, 160, 1, 16, 32),                # G = 8; C2 = 160: 5 row tiles over 4 waves
    _c(32, 160, 160, 2, 8, 4, second=True, ldz_pad=3),       # C1 = 160 (G = 20 in layer 2); two sets sharing one Z
    _c(16, 64, 32, 1, 8, 4),                   # C1 = 64: two row tiles in layer 1, G = 8 in layer 2
    _c(256, 256, 32, 1, 4, 8),                 # 66560 bytes of LDS: the dynamic path above 48 KB
]
N_POINTS = 40                                  # points per cloud; the second set has ld = N_POINTS + 7 columns per cloud
BN_CONSTS_C, BN_CONSTS_NREP = (1, 255, 256, 257), (1, 3)


def case_id(c):
    return "C%d-%d-%d-B%d-np%d-ns%d%s" % (c.C0, c.C1, c.C2, c.B, c.npoint, c.ns, ("-nocentre" if not c.ldw else "-ldw%d" % c.ldw) +
                                          ("-two" if c.second else "") + ("-ldz+%d" % c.ldz_pad if c.ldz_pad else ""))


def ball_idx(rng, B, npoint, ns, N):
    """(B, npoint, ns) as ball_query pads: the first cnt slots distinct points, the rest copies of the first hit; every
    third ball is full, ball 1 holds a single point"""
    idx = np.zeros((B, npoint, ns), np.int64)
    for b in range(B):
        for j in range(npoint):
            cnt = ns if j % 3 == 0 else 1 if j == 1 else rng.randint(1, ns + 1)
            hit = rng.permutation(N)[:cnt]
            idx[b, j, :cnt], idx[b, j, cnt:] = hit, hit[0]
    return idx


def layer_consts(draw, C):
    """v (4, C): scale on the coefficient grid (never 0), shift on the 1/4 grid; mean and invstd (rows 0, 1) play no part in
    the fused kernel's formula: values that would show if they did"""
    v = np.full((4, C), 12345.0)
    v[2], v[3] = draw.coef((C,), zero=False), draw.val((C,), 0.25, 0.5)
    return v


def inputs(draw, c, seed):
    """-> Ref(Z (C0, ldz), sets = [Ref(idx, centers, B, npoint, ns, ld, pt_base)], W0 (C0, ldw or 3), v0, W1, v1, W2, v2, ldz,
    used (ldz,) bool: the Z columns some index names).  Channel 1 of the last layer has a shift below every pre-activation:
    its pooled output is exactly 0 in every ball (all slots clamped)."""
    rng = np.random.RandomState(seed)
    N = N_POINTS
    lds = [N] + ([N + 7] if c.second else [])
    ldz = c.B * sum(lds) + c.ldz_pad
    i = Ref(Z=draw.val((c.C0, ldz), 0.5, 1.0), W0=draw.coef((c.C0, 3)), v0=layer_consts(draw, c.C0),
            W1=draw.coef((c.C1, c.C0)), v1=layer_consts(draw, c.C1), W2=draw.coef((c.C2, c.C1)), v2=layer_consts(draw, c.C2),
            ldz=ldz, sets=[], used=np.zeros(ldz, bool))
    base = 0
    for ld in lds:
        s = Ref(idx=ball_idx(rng, c.B, c.npoint, c.ns, N), centers=draw.val((c.B * c.npoint, 3), 0.5, 1.0) if c.ldw else None,
                B=c.B, npoint=c.npoint, ns=c.ns, ld=ld, pt_base=base)
        i.used[(base + np.arange(c.B)[:, None, None] * ld + s.idx).reshape(-1)] = True
        i.sets.append(s)
        base += c.B * ld
    worst = 0.0
    for s in i.sets:
        r = run(i, s)
        worst = max(worst, float(r.T2[1].max()))
    i.v2[3, 1] = -float(np.ceil(worst + 1.0))        # (an integer: on every grid)
    return i


def run(i, s):
    return sa_eval(i.Z, s.idx, s.centers, i.W0, i.v0, i.W1, i.v1, i.W2, i.v2, s.B, s.npoint, s.ns, s.ld, s.pt_base)


def input_conditions(i, s, r):
    """what a case's inputs must provide for the pins to see a wrong pool or a wrong slot, from the oracle alone
    -> dict of the measured figures (asserted by the CPU file)"""
    ns = s.ns
    unique = (r.nmax == 1) & (r.out > 0)
    pos = np.unique(r.arg[unique])
    idx = s.idx.reshape(-1, ns)
    padded = np.array([len(np.unique(row)) < ns for row in idx])
    dup_ok = all((row[1:] == row[0]).any() for row in idx[padded]) if ns > 1 else True
    return dict(unique_positions=len(pos), ns=ns, positive=float((r.out > 0).mean()), zeros=int((r.out == 0).sum()),
                padded_balls=int(padded.sum()), padded_have_duplicate=bool(dup_ok))


def exact_preconditions():
    seen = []
    for k, c in enumerate(CASES):
        i = inputs(Dyadic(4000 + k), c, k)
        for s in i.sets:
            r = run(i, s)
            for name, T in (("sa.A0", r.T0), ("sa.A1", r.T1), ("sa.A2", r.T2)):
                seen.append((name, assert_exact(name, T)))
    return seen
