"""Plain numpy reference of the glue in front of the GEMMs -- o3d_sample_query (csrc/index_ops.hip: its centres; the ball
query itself is oracle.ops.ball_query on them), o3d_gather_rows2, o3d_pack_rows / o3d_pack_rows_ld, o3d_prep_weights
(csrc/heads.hip) and o3d_cosine_sim_fwd / o3d_cosine_sim_bwd (csrc/xcorr.hip) -- written from include/o3dsot.h.  It imports
nothing of the package under test.  Everything but the cosine map moves values without arithmetic: those references are
copies, compared for equality.  The cosine map is fp64 and follows the kernel's rule: a norm clamped at 1e-8 is a constant,
with no gradient through it.  Shared by tests/test_glue_oracle_cpu.py and tests/test_glue_kernels_gpu.py.

Bounds of the cosine map, u = 2^-24, a sum of n products bounded by (n + 8) u sum|t_i| as everywhere in these pins; the
library is built without fast-math, so hipcc's fp32 division and square root are correctly rounded (the div_scale / div_fmas /
div_fixup and the corrected v_sqrt sequences are what the compiler emits for csrc/xcorr.hip) and each adds one rounding:
  tn, sn   sqrt halves the relative error of the sum of squares, plus its own rounding:  ((f + 8) / 2 + 1) u |tn|
  sim      over the STORED norms: the dot product, the product sn * tn, the quotient:    ((f + 8) sum|t s| + 2 |dot|) u / (sn tn)
  dt, ds   over the fp32 inputs of the backward (dsim, sim, tn, sn, t, s), with A_i = sum_j dsim sim (n = N), a_i = A_i / tn_i^2
           (the square and the quotient: two roundings), G = dsim / (tn sn) (two roundings):
           dt[c,i] = sum_j G s - t a_i:  u [ (N + 8 + 2 + 1) sum_j|G s| + |t| ((N + 8) sum_j|dsim sim| + 2 |A_i|) / tn_i^2 + 2 |t a_i| ]
           (the last 2: the product t * a_i and the final subtraction), and ds likewise with the roles of (i, M) and (j, N) swapped.
"""
from types import SimpleNamespace as Ref

import numpy as np

U = 2.0 ** -24
EPS = float(np.float32(1e-8))          # CS_EPS as the kernel holds it


def f64(a):
    return np.asarray(a, np.float64)


# ---- o3d_sample_query ------------------------------------------------------------------------------------------------------
def sample_centres(xyz, sidx, npoint):
    """xyz (B, N, 3) float32, sidx (B, npoint) or None (the first npoint points) -> (B, npoint, 3) float32, bit for bit"""
    xyz = np.asarray(xyz, np.float32)
    B = xyz.shape[0]
    if sidx is None:
        return xyz[:, :npoint].copy()
    sidx = np.asarray(sidx, np.int64)
    assert sidx.shape == (B, npoint) and sidx.min() >= 0 and sidx.max() < xyz.shape[1]
    return xyz[np.arange(B)[:, None], sidx]


def sample_query_centers(sets):
    """sets: [(xyz, sidx, npoint)] (one or two) -> centers (total + 1, 3) float32: set 0's, set 1's, then the origin row;
    and the per-set (B, npoint, 3) centres"""
    per = [sample_centres(*s) for s in sets]
    return np.concatenate([p.reshape(-1, 3) for p in per] + [np.zeros((1, 3), np.float32)]), per


# ---- o3d_gather_rows2 ------------------------------------------------------------------------------------------------------
def gather_rows2(a, b, idx, npoint):
    """a (B, N, Da), b (B, N, Db) | None, idx (B, ld_idx >= npoint): out[b, j, :] = src[b, idx[b, j], :] for j < npoint"""
    B = a.shape[0]
    ii = np.asarray(idx, np.int64)[:, :npoint]
    rows = np.arange(B)[:, None]
    return a[rows, ii], (None if b is None else b[rows, ii])


# ---- o3d_pack_rows[_ld] ----------------------------------------------------------------------------------------------------
def pack_rows(srcs, rows):
    """srcs: (B, C_i, N) arrays (any strides) -> X (rows, B*N): the sources stacked along the rows, column b*N + n; zero rows
    up to `rows`"""
    B, _, N = srcs[0].shape
    X = np.zeros((rows, B * N), np.float32)
    r = 0
    for s in srcs:
        C = s.shape[1]
        X[r:r + C] = np.asarray(s, np.float32).transpose(1, 0, 2).reshape(C, B * N)
        r += C
    assert r <= rows
    return X


# ---- o3d_prep_weights ------------------------------------------------------------------------------------------------------
def prep_weights(dst, src, ld, transpose):
    """src (rows, cols) into the prefilled flat `dst`: dst[r*ld + c] or, transposed, dst[c*ld + r]; nothing else is written"""
    rows, cols = src.shape
    out = dst.copy()
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    out[(c * ld + r) if transpose else (r * ld + c)] = src
    return out


# ---- cosine similarity map -------------------------------------------------------------------------------------------------
def norms(x, f):
    """x (B, f, K) -> Ref(n (B, K) = max(|x_k|, eps), raw = |x_k|, bound)"""
    raw = np.sqrt((f64(x) ** 2).sum(1))
    return Ref(n=np.maximum(raw, EPS), raw=raw, bound=((f + 8) / 2.0 + 1.0) * U * raw)


def cosine_sim(t, s, tn=None, sn=None):
    """t (B, f, M), s (B, f, N) -> Ref(sim (B, N, M) = <t_i, s_j> / (tn_i sn_j), tn, sn, sim_bound); tn / sn given: the
    stored norms (the bound of sim is over them), else max(|.|, eps) in fp64"""
    t, s = f64(t), f64(s)
    f = t.shape[1]
    nt, ns_ = norms(t, f), norms(s, f)
    tn = nt.n if tn is None else f64(tn)
    sn = ns_.n if sn is None else f64(sn)
    dot = np.einsum("bfi,bfj->bji", t, s)
    dabs = np.einsum("bfi,bfj->bji", np.abs(t), np.abs(s))
    den = sn[:, :, None] * tn[:, None, :]
    return Ref(sim=dot / den, tn=tn, sn=sn, tn_bound=nt.bound, sn_bound=ns_.bound, dot=dot, dot_abs=dabs,
               sim_bound=((f + 8) * dabs + 2 * np.abs(dot)) * U / den)


def cosine_sim_bwd(dsim, sim, tn, sn, t, s, keep_clamped=False):
    """the gradient of sum(dsim * sim) w.r.t. t and s, sim = <t_i, s_j> / (tn_i sn_j) with tn_i = max(|t_i|, eps): a norm at
    or below eps is a constant.  All six inputs are the entry's own inputs.  -> Ref(dt (B, f, M), ds (B, f, N), dt_bound,
    ds_bound, *_mag: the largest magnitude that enters each output's sum, for the exactness precondition).
    keep_clamped: the mistake of keeping the gradient through a clamped norm (for the sensitivity tests)"""
    dsim, sim, tn, sn, t, s = (f64(a) for a in (dsim, sim, tn, sn, t, s))
    B, N, M = dsim.shape
    prod = dsim * sim
    A, Aabs = prod.sum(1), np.abs(prod).sum(1)               # (B, M): over j
    Bq, Babs = prod.sum(2), np.abs(prod).sum(2)              # (B, N): over i
    live_t = (tn > EPS) | keep_clamped
    live_s = (sn > EPS) | keep_clamped
    ai = np.where(live_t, A / tn ** 2, 0.0)
    bj = np.where(live_s, Bq / sn ** 2, 0.0)
    ai_err = np.where(live_t, ((N + 8) * Aabs + 2 * np.abs(A)) / tn ** 2, 0.0)
    bj_err = np.where(live_s, ((M + 8) * Babs + 2 * np.abs(Bq)) / sn ** 2, 0.0)
    G = dsim / (sn[:, :, None] * tn[:, None, :])             # (B, N, M)
    Gs, Gs_abs = np.einsum("bji,bfj->bfi", G, s), np.einsum("bji,bfj->bfi", np.abs(G), np.abs(s))
    Gt, Gt_abs = np.einsum("bji,bfi->bfj", G, t), np.einsum("bji,bfi->bfj", np.abs(G), np.abs(t))
    ta, sb = t * ai[:, None, :], s * bj[:, None, :]
    return Ref(dt=Gs - ta, ds=Gt - sb,
               dt_bound=U * ((N + 11) * Gs_abs + np.abs(t) * ai_err[:, None, :] + 2 * np.abs(ta)),
               ds_bound=U * ((M + 11) * Gt_abs + np.abs(s) * bj_err[:, None, :] + 2 * np.abs(sb)),
               dt_mag=Gs_abs + np.abs(ta), ds_mag=Gt_abs + np.abs(sb), A_abs=Aabs, B_abs=Babs, ai=ai, bj=bj)


# ---- exact-leg inputs of the cosine map ------------------------------------------------------------------------------------
def pow2_columns(rng, B, f, K, zero_cols=()):
    """(B, f, K): every column holds exactly four non-zero entries +-2^k (one k per column, k in -2 .. 2): its norm is
    2^(k+1), every dot product of two such columns has at most four terms, all powers of two within 2^-4 .. 2^4"""
    x = np.zeros((B, f, K))
    for b in range(B):
        for k in range(K):
            if k in zero_cols:
                continue
            at = rng.choice(f, 4, replace=False)
            x[b, at, k] = rng.choice([-1.0, 1.0], 4) * 2.0 ** rng.randint(-2, 3)
    return x


def exact_bwd_inputs(rng, B, f, M, N, clamped_t=False):
    """inputs of the backward on grids that keep every sum exact: norms powers of two, dsim on 1/4, sim on 1/4, t and s on
    1/2.  clamped_t: every template norm is 2^-27 or 2^-28, below eps, so no gradient runs through it and G is 2^27 times
    larger; there dsim * sim is +p in template column 0 and -p in column 1, zero elsewhere: the sums over i (b_j, whose
    term s b_j would sit 2^30 below the others in ds) vanish while the sums over j (a_0 = -a_1, what the clamp must drop) do
    not"""
    g = lambda shape, step, lim: rng.randint(-int(lim / step), int(lim / step) + 1, size=shape) * step
    tn = 2.0 ** rng.randint(-28 if clamped_t else -1, -26 if clamped_t else 3, size=(B, M))
    sn = 2.0 ** rng.randint(-1, 3, size=(B, N))
    dsim, sim = g((B, N, M), 0.25, 2.0), g((B, N, M), 0.25, 1.0)
    if clamped_t:
        dsim[:, :, 0] = np.where(dsim[:, :, 0] == 0, 0.5, dsim[:, :, 0])
        sim[:, :, 0] = np.where(sim[:, :, 0] == 0, 0.75, sim[:, :, 0])
        dsim[:, :, 1], sim[:, :, 1], sim[:, :, 2:] = dsim[:, :, 0], -sim[:, :, 0], 0.0
    return Ref(dsim=dsim, sim=sim, tn=tn, sn=sn, t=g((B, f, M), 0.5, 1.0), s=g((B, f, N), 0.5, 1.0))


def assert_exact_bwd(i, r):
    """the terms of dt[c, i] are G[j, i] s[c, j] = (k/4) (k'/2) / (tn_i sn_j), all on the grid 2^-3 / (tn_i max_j sn_j) (the
    norms are powers of two), and, where the norm is live, t a_i = (k/2) (k'/16) / tn_i^2 on 2^-5 / tn_i^2; both grids are
    powers of two, so the finer one holds every term (the second only where a_i != 0).  Likewise ds.  The sum of magnitudes stays below 2^24 steps of it, and
    so do A_i and B_j on their grid 1/16."""
    def grid(own, other_max, coef):
        g = 2.0 ** -3 / (own * other_max)
        return np.where(coef != 0, np.minimum(g, 2.0 ** -5 / own ** 2), g)[:, None, :]
    gt = grid(i.tn, i.sn.max(1, keepdims=True), r.ai)
    gs = grid(i.sn, i.tn.max(1, keepdims=True), r.bj)
    worst = max(float((r.dt_mag / gt).max()), float((r.ds_mag / gs).max()))
    assert worst < 2.0 ** 24, worst
    assert float(r.A_abs.max()) * 16 < 2.0 ** 24 and float(r.B_abs.max()) * 16 < 2.0 ** 24
    return worst
