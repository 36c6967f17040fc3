"""Plain numpy fp64 reference of the inner-layer GEMM entry points of the compact (distinct-neighbour) layout --
o3d_mlp_conv_fwd_c, o3d_mlp_conv_dgrad_c (csrc/mlp_direct.hip), o3d_mlp_conv_wgrad2_c, o3d_mlp_conv_bwd_fused_c
(csrc/mlp_wgrad.hip) -- and of the statistics rows they write, the remainder-tile plan of csrc/mlp_common.hpp included.
Written from the text of include/o3dsot.h and the comments of the kernels; it imports nothing of the package under test.
Shared by tests/test_compact_gemm_oracle_cpu.py (which ties it to Conv2d / BatchNorm2d / ReLU under torch.autograd on the
slot-wise tensors) and tests/test_compact_gemm_kernels_gpu.py (which pins every launch class of every entry to it).

Conventions: those of tests/compact_oracle.py (Layout, *_abs, NaN = "nothing is written") and tests/gemm_oracle.py (Ref).
Columns: an entry works on the WRITTEN columns of a layout -- [start_s, start_s + live256_s) per segment -- and on no other.
Padding contract (include/o3dsot.h): on the padding columns [live, live256) cw = 0, the forward computes them like live ones,
and the backward entries assume dN == 0 there (with finite Y, X / Yprev); the oracle asserts that of its dN.
"""
from types import SimpleNamespace as Ref

import numpy as np

import compact_oracle as CO
import gemm_oracle as GO
from compact_oracle import Dyadic, Layout, _idx_from_counts, assert_exact  # noqa: F401  (re-exported for the tests)

# grid spacing of the terms of every exactly compared output, for the input steps of `Inputs` below
SPACING = {"cg.Y": 0.125, "cg.part0": 0.125, "cg.part1": 1.0 / 64, "cg.G": 0.125, "cg.gpart0": 0.125, "cg.gpart1": 1.0 / 32,
           "cg.dW": 1.0 / 16, "cg.fused_gx": 1.0 / 32, "cg.fused_bs": 1.0 / 64}
CO.SPACING.update(SPACING)

NATURAL_SLOTS = {64: 2048, 128: 1024, 256: 512}       # o3d_direct_tail_slots(output rows) on 256 compute units


# ---- the remainder-tile plan (csrc/mlp_common.hpp, restated from its description) ----------------------------------------
def tail_plan_why(T, S, cap):
    """T live 128-column tiles on S resident slots, at most `cap` workgroups for the segment -> (full, R, f, why): the last
    R = T mod S tiles are cut into f = 4 (4R <= S) or 2 (2R <= S) column blocks, the first `full` tiles stay whole.  No split
    (full = T, R = 0, f = 1) when S or T is not positive ("off"), T divides ("R0"), the remainder is more than half a round
    ("2R>S"), or the T + R*(f-1) workgroups do not fit the segment's grid ("cap")."""
    if S <= 0 or T <= 0:
        return T, 0, 1, "off"
    R = T % S
    if R == 0:
        return T, 0, 1, "R0"
    f = 4 if 4 * R <= S else 2 if 2 * R <= S else 1
    if f == 1:
        return T, 0, 1, "2R>S"
    if T + R * (f - 1) > cap:
        return T, 0, 1, "cap"
    return T - R, R, f, "f%d" % f


def tail_plan(T, S, cap):
    return tail_plan_why(T, S, cap)[:3]


def seg_caps(L, tile=128):
    """worst-case tiles of every segment, as the GEMM derives them from start1 and ldp"""
    return [L.start1 // tile, (L.ldp - L.start1) // tile] if L.nseg == 2 else [L.ldp // tile]


def stat_rows(L, tile, S=0):
    """the statistics rows of a forward / data-gradient launch with `tile` columns per row and S resident slots (tile 128
    only; 0 = no remainder split) -> (rows, nrows): rows = [(row, first column, one past the last, segment)] for every row
    that is written, nrows = regular + extra rows of the buffer (ldp / tile + nseg * S).  Every other row stays unwritten:
    dead tiles, unused extra rows, the other segment's slot block."""
    split = tile == 128 and S > 0
    regular = L.ldp // tile
    rows = []
    for s in range(L.nseg):
        t0, T = L.start[s] // tile, L.live256[s] // tile
        full, R, f = tail_plan(T, S, seg_caps(L)[s]) if split else (T, 0, 1)
        for t in range(full):
            rows.append((t0 + t, (t0 + t) * tile, (t0 + t + 1) * tile, s))
        w = tile // f
        for j in range(R):
            c0 = (t0 + full + j) * tile
            rows.append((t0 + full + j, c0, c0 + w, s))                                   # block 0: the tile's own row
            for blk in range(1, f):
                rows.append((regular + s * S + j * (f - 1) + blk - 1, c0 + blk * w, c0 + (blk + 1) * w, s))
    return rows, regular + (L.nseg * S if split else 0)


def plan_reasons(L, S):
    """why every segment of L gets its plan at S slots -> [(why, full)]"""
    plans = [tail_plan_why(L.live256[s] // 128, S, seg_caps(L)[s]) for s in range(L.nseg)]
    return [(p[3], p[0]) for p in plans]


class Dense:
    """meta = NULL, w = NULL, start1 = 0 of o3d_mlp_conv_bwd_fused_c: one segment, every column live, weight 1"""
    nseg, start1, start = 1, 0, [0]

    def __init__(self, ldp):
        self.ldp, self.live, self.live256 = ldp, [ldp], [ldp]
        self.written = np.arange(ldp)
        self.cw = np.ones(ldp)

    def seg_of_col(self, q):
        return np.zeros(np.shape(q), np.int64)

    def per_channel(self, v, C, seg):
        return np.asarray(v, np.float64).reshape(1, C)[seg].T


def padding(L):
    return np.concatenate([L.start[s] + np.arange(L.live[s], L.live256[s]) for s in range(L.nseg)]).astype(np.int64)


# ---- operands ------------------------------------------------------------------------------------------------------------
def act_c(L, X, in_scale, in_shift):
    """f = relu(X * in_scale[seg] + in_shift[seg]) on the written columns -> f, f_abs (Cin, len(L.written))"""
    q = L.written
    seg = L.seg_of_col(q)
    C = X.shape[0]
    sc, sh = L.per_channel(in_scale, C, seg), L.per_channel(in_shift, C, seg)
    x = np.asarray(X, np.float64)[:, q]
    n = x * sc + sh
    on = n > 0
    return np.where(on, n, 0.0), np.where(on, np.abs(x * sc) + np.abs(sh), 0.0)


def dy_c(L, dN, Y, A1, A2, A3):
    """dY = A1*dN + cw*(A2*Y + A3) on the written columns (segment 1: constants at +Cout) -> dY, dY_abs"""
    q = L.written
    pad = padding(L)
    assert not np.asarray(dN)[:, pad].any(), "padding contract: dN must be zero on the padding columns"
    assert np.isfinite(np.asarray(Y)[:, q]).all()
    seg = L.seg_of_col(q)
    C = dN.shape[0]
    a1, a2, a3 = (L.per_channel(a, C, seg) for a in (A1, A2, A3))
    w = L.cw[q][None, :]
    d, y = np.asarray(dN, np.float64)[:, q], np.asarray(Y, np.float64)[:, q]
    return a1 * d + w * (a2 * y + a3), np.abs(a1 * d) + w * (np.abs(a2 * y) + np.abs(a3))


def scatter(L, C, vals):
    out = np.full((C, L.ldp), np.nan)
    out[:, L.written] = vals
    return out


# ---- statistics rows ---------------------------------------------------------------------------------------------------
def stats_fwd_rows(L, Y, Y_abs, stat_c, rows, nrows):
    """part[row] = {sum cw*y, sum cw*(y - stat_c[seg])^2} over the row's columns -> part, part_abs (nrows, 2, C; NaN =
    unwritten), n (nrows,) = columns of the row"""
    C = Y.shape[0]
    part, pabs, n = np.full((nrows, 2, C), np.nan), np.full((nrows, 2, C), np.nan), np.zeros(nrows)
    sc = np.asarray(stat_c, np.float64).reshape(L.nseg, C) if stat_c is not None else np.zeros((L.nseg, C))
    for r, c0, c1, s in rows:
        w, y, ya, c = L.cw[c0:c1][None, :], Y[:, c0:c1], Y_abs[:, c0:c1], sc[s][:, None]
        part[r, 0], part[r, 1] = (w * y).sum(1), (w * (y - c) ** 2).sum(1)
        pabs[r, 0], pabs[r, 1] = (w * ya).sum(1), (w * (ya + np.abs(c)) ** 2).sum(1)
        n[r] = c1 - c0
    return part, pabs, n


def stats_bwd_rows(L, G, G_abs, Yprev, mean_p, rows, nrows):
    """part[row] = {sum g, sum g*(Yprev - mean_p[seg])} over the row's columns, no cw -> part, part_abs, n"""
    C = G.shape[0]
    part, pabs, n = np.full((nrows, 2, C), np.nan), np.full((nrows, 2, C), np.nan), np.zeros(nrows)
    mu = np.asarray(mean_p, np.float64).reshape(L.nseg, C)
    yp = np.asarray(Yprev, np.float64)
    for r, c0, c1, s in rows:
        g, ga, y, m = G[:, c0:c1], G_abs[:, c0:c1], yp[:, c0:c1], mu[s][:, None]
        part[r, 0], part[r, 1] = g.sum(1), (g * (y - m)).sum(1)
        pabs[r, 0], pabs[r, 1] = ga.sum(1), (ga * (np.abs(y) + np.abs(m))).sum(1)
        n[r] = c1 - c0
    return part, pabs, n


def seg_rows(L):
    """one pseudo-row per segment over its written columns: the totals a list of partial rows must add up to"""
    return [(s, L.start[s], L.start[s] + L.live256[s], s) for s in range(L.nseg)], L.nseg


# ---- the entries -----------------------------------------------------------------------------------------------------------
def fwd_c(L, X, W, in_scale, in_shift):
    """Y[:, q] = W . relu(X[:, q]*in_scale[seg] + in_shift[seg]) on every written column -> Ref(Y, Y_abs, n = Cin)"""
    W = np.asarray(W, np.float64)
    f, fa = act_c(L, X, in_scale, in_shift)
    return Ref(Y=scatter(L, W.shape[0], W @ f), Y_abs=scatter(L, W.shape[0], np.abs(W) @ fa), n=W.shape[1])


def dgrad_c(L, dN, Y, A1, A2, A3, Wt, Yprev, scale_p, shift_p):
    """dNprev = (Wt . dY) where fma(Yprev, scale_p[seg], shift_p[seg]) > 0, else 0 -> Ref(G, G_abs, mask, n = Cout)"""
    Wt = np.asarray(Wt, np.float64)
    Cin = Wt.shape[0]
    dY, dYa = dy_c(L, dN, Y, A1, A2, A3)
    q = L.written
    seg = L.seg_of_col(q)
    mask = np.asarray(Yprev, np.float64)[:, q] * L.per_channel(scale_p, Cin, seg) + L.per_channel(shift_p, Cin, seg) > 0
    G, Ga = np.where(mask, Wt @ dY, 0.0), np.where(mask, np.abs(Wt) @ dYa, 0.0)
    m = np.zeros((Cin, L.ldp), bool)
    m[:, q] = mask
    return Ref(G=scatter(L, Cin, G), G_abs=scatter(L, Cin, Ga), mask=m, n=Wt.shape[1])


def wgrad2_c(L, dN, Y, A1, A2, A3, X, in_scale, in_shift):
    """dW (Cout, Cin) = sum over the written columns of both segments of dY[:, q] f(X[:, q])^T, every segment with its own
    constants -> Ref(dW, dW_abs, n = written columns)"""
    dY, dYa = dy_c(L, dN, Y, A1, A2, A3)
    f, fa = act_c(L, X, in_scale, in_shift)
    return Ref(dW=dY @ f.T, dW_abs=dYa @ fa.T, n=len(L.written))


def fused_second_abs(L, G_abs, X, in_scale, in_shift, in_mean):
    """the yardstick of part_s[.][1] as o3d_mlp_conv_bwd_fused_c forms it (csrc/mlp_wgrad.hip: "the second from sum g*Xt"):
    sum g*(yprev - mean) = (sum g*xt - beta*sum g) / sc with xt = relu(sc*yprev + sh), beta = sh + sc*mean; a channel with
    sc == 0 is summed directly.  -> (gx_abs, bs_abs, total_abs) per segment, (nseg, Cin): sum|g|*(|sc*x| + |sh|),
    (|sh| + |sc*mean|) * sum|g|, and (gx_abs + bs_abs) / |sc| (sc == 0: sum|g|*(|x| + |mean|))"""
    C = G_abs.shape[0]
    gx, bs, tot = np.zeros((L.nseg, C)), np.zeros((L.nseg, C)), np.zeros((L.nseg, C))
    x = np.abs(np.asarray(X, np.float64))
    for s in range(L.nseg):
        sl = slice(L.start[s], L.start[s] + L.live256[s])
        sc, sh, mu = (np.asarray(v, np.float64).reshape(L.nseg, C)[s][:, None] for v in (in_scale, in_shift, in_mean))
        ga = G_abs[:, sl]
        gx[s] = (ga * (np.abs(sc) * x[:, sl] + np.abs(sh))).sum(1)
        bs[s] = ((np.abs(sh) + np.abs(sc * mu)) * ga).sum(1)
        direct = (ga * (x[:, sl] + np.abs(mu))).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            tot[s] = np.where(sc[:, 0] != 0, (gx[s] + bs[s]) / np.abs(sc[:, 0]), direct)
    return gx, bs, tot


# ---- BatchNorm constants of one or two segments from partial rows ---------------------------------------------------------
def bn_fwd_consts(L, part, counts, gamma, beta, eps, stat_c):
    """(nseg, C) mean, invstd, scale, shift from the written rows of `part` (NaN rows skipped), by segment"""
    out = []
    C = part.shape[2]
    for s in range(L.nseg):
        rows = [r for r in range(part.shape[0]) if not np.isnan(part[r, 0, 0]) and part_seg(L, r, part.shape[0]) == s]
        out.append(GO.bn_consts(part[rows], counts[s], gamma, beta, eps, np.asarray(stat_c).reshape(L.nseg, C)[s]))
    return [np.stack([o[k] for o in out]) for k in range(4)]


def part_seg(L, r, nrows, tile=128):
    """segment of statistics row r of a tile-128 buffer of nrows rows (regular rows by column, extra rows by slot block)"""
    regular = L.ldp // tile
    if r < regular:
        return int(L.seg_of_col(r * tile))
    S = (nrows - regular) // L.nseg
    return (r - regular) // S


# ---- inputs --------------------------------------------------------------------------------------------------------------
class Inputs:
    """operands of one layer (Cin -> Cout) over layout L, on the grids SPACING assumes (exact draw) or randn; NaN in every
    column no entry may read (beyond live256 of each segment); dN zero on the padding columns, as the contract asks.
    X doubles as Yprev, (in_scale, in_shift, in_mean) as (scale_p, shift_p, mean_p): one layer's backward."""

    def __init__(self, draw, L, Cin, Cout, nnz=8, dead_channel=False):
        d = draw
        self.L, self.Cin, self.Cout = L, Cin, Cout
        self.W = GO.sparse_rows(d, Cout, Cin, nnz)
        self.Wt = GO.sparse_rows(d, Cin, Cout, nnz)
        self.X, self.Y, self.dN = d.val((Cin, L.ldp), 0.5, 1.0), d.val((Cout, L.ldp), 0.5, 1.0), d.val((Cout, L.ldp), 0.5, 1.0)
        ns = L.nseg
        self.in_scale, self.in_shift = d.coef((ns * Cin,), zero=False), d.val((ns * Cin,), 0.25, 0.5)
        self.in_mean = d.val((ns * Cin,), 0.25, 0.5)
        if dead_channel:                                      # gamma == 0: relu(bn(x)) is the constant in_shift (> 0: unmasked)
            self.in_scale[3], self.in_shift[3] = 0.0, abs(self.in_shift[3]) + 0.25
        self.A1, self.A2, self.A3 = d.coef((ns * Cout,)), d.coef((ns * Cout,)), d.coef((ns * Cout,))
        self.stat_c = d.val((ns * Cout,), 0.125, 0.5)
        self.gamma_o, self.beta_o = d.coef((Cout,), zero=False), d.val((Cout,), 0.25, 0.5)      # BatchNorm of this layer
        self.gamma_i = d.coef((Cin,), zero=False)                                               # ... of the producer
        self.invstd_i = np.abs(d.coef((ns * Cin,), zero=False))
        self.dN[:, padding(L)] = 0.0
        dead = np.ones(L.ldp, bool)
        dead[L.written] = False
        for a in (self.X, self.Y, self.dN):
            a[:, dead] = np.nan


# ---- layouts -------------------------------------------------------------------------------------------------------------
_CACHE = {}


def layout(name):
    """the families of tests/compact_oracle.py that fit (paired, full, mixed) and one more, small and sparse:
    sparse   one segment, 24 worst-case tiles of 128, 700 live columns -> 6 live tiles: T + 3R == cap exactly, so the natural
             slot count cuts every tile in four, and one live column more per ball would refuse the split"""
    if name in _CACHE:
        return _CACHE[name]
    if name == "sparse":
        B, npoint, ns, N = 2, 96, 16, 64
        rng = np.random.RandomState(21)
        counts = np.full(B * npoint, 3)
        counts[:124] = 4                                      # 192 * 3 + 124 = 700 live columns
        L = Layout([(_idx_from_counts(rng, rng.permutation(counts), B, npoint, ns, N), 64)])
        assert (L.live, L.live256, L.ldp) == ([700], [768], 3072)
    else:
        L = CO.family_layout(name)
    assert L.ldp % 128 == 0 and L.start1 % 256 == 0
    _CACHE[name] = L
    return L


# ---- whole launches: output + statistics rows, and what the finalize entries make of them -----------------------------------
def ref_fwd(i, tile, S=0):
    """o3d_mlp_conv_fwd_c over Inputs i with `tile` columns per row and S slots -> Ref(Y, Y_abs, n, rows, nrows, part, ...)"""
    r = fwd_c(i.L, i.X, i.W, i.in_scale, i.in_shift)
    r.rows, r.nrows = stat_rows(i.L, tile, S)
    r.part, r.part_abs, r.part_n = stats_fwd_rows(i.L, r.Y, r.Y_abs, i.stat_c, r.rows, r.nrows)
    r.tot = stats_fwd_rows(i.L, r.Y, r.Y_abs, i.stat_c, *seg_rows(i.L))[0]
    return r


def ref_dgrad(i, tile, S=0):
    """o3d_mlp_conv_dgrad_c over Inputs i (Yprev = X, the producer's constants = in_*) -> Ref(G, G_abs, mask, n, rows, ...)"""
    r = dgrad_c(i.L, i.dN, i.Y, i.A1, i.A2, i.A3, i.Wt, i.X, i.in_scale, i.in_shift)
    r.rows, r.nrows = stat_rows(i.L, tile, S)
    r.part, r.part_abs, r.part_n = stats_bwd_rows(i.L, r.G, r.G_abs, i.X, i.in_mean, r.rows, r.nrows)
    r.tot, r.tot_abs, _ = stats_bwd_rows(i.L, r.G, r.G_abs, i.X, i.in_mean, *seg_rows(i.L))
    return r


def ref_wgrad(i):
    return wgrad2_c(i.L, i.dN, i.Y, i.A1, i.A2, i.A3, i.X, i.in_scale, i.in_shift)


def exact_fwd(r):
    assert_exact("cg.Y", r.Y_abs), assert_exact("cg.part0", r.part_abs[:, 0]), assert_exact("cg.part1", r.part_abs[:, 1])


def exact_dgrad(r):
    assert_exact("cg.G", r.G_abs), assert_exact("cg.gpart0", r.part_abs[:, 0]), assert_exact("cg.gpart1", r.part_abs[:, 1])


def exact_fused(i, r):
    """the fused entry forms its second statistic as (sum g*xt - beta*sum g) / sc: both products stay exact"""
    gx, bs, _ = fused_second_abs(i.L, r.G_abs, i.X, i.in_scale, i.in_shift, i.in_mean)
    assert_exact("cg.fused_gx", gx), assert_exact("cg.fused_bs", bs)
    assert_exact("cg.gpart0", r.tot_abs[:, 0]), assert_exact("cg.gpart1", r.tot_abs[:, 1])


def counts_of(L):
    """positions BatchNorm counts per segment: every slot, copies included (= the sum of cw over the segment)"""
    return [float(L.cw[L.start[s]:L.start[s] + L.live[s]].sum()) for s in range(L.nseg)]


def bn_fin_ref(tot, counts, gamma, beta, eps, stat_c, rm, rv, momentum):
    """o3d_bn_finalize from per-segment totals tot (nseg, 2, C) -> dict of (nseg, C) mean, invstd, scale, shift and the
    running statistics (C) after segment 0's update, then segment 1's"""
    nseg, _, C = tot.shape
    sc = np.asarray(stat_c, np.float64).reshape(nseg, C)
    out = {k: np.zeros((nseg, C)) for k in ("mean", "invstd", "scale", "shift")}
    rm, rv = np.array(rm, np.float64), np.array(rv, np.float64)
    for s in range(nseg):
        mean, invstd, scale, shift = GO.bn_consts(tot[s][None], counts[s], gamma, beta, eps, sc[s])
        out["mean"][s], out["invstd"][s], out["scale"][s], out["shift"][s] = mean, invstd, scale, shift
        var = 1.0 / invstd ** 2 - eps
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * counts[s] / (counts[s] - 1.0)
    out["running_mean"], out["running_var"] = rm, rv
    return out


def bn_bwd_fin_ref(tot, counts, gamma, mean, invstd):
    """o3d_bn_bwd_finalize from per-segment totals {sum g, sum g*(y - mean)} -> dgamma, dbeta (C; summed over the segments),
    A1, A2, A3 (nseg, C)"""
    nseg, _, C = tot.shape
    mean, invstd = np.asarray(mean, np.float64).reshape(nseg, C), np.asarray(invstd, np.float64).reshape(nseg, C)
    A = [GO.bn_bwd_coef(tot[s][None], counts[s], gamma, mean[s], invstd[s]) for s in range(nseg)]
    return dict(dgamma=sum(tot[s, 1] * invstd[s] for s in range(nseg)), dbeta=sum(tot[s, 0] for s in range(nseg)),
                A1=np.stack([a[0] for a in A]), A2=np.stack([a[1] for a in A]), A3=np.stack([a[2] for a in A]))


# ---- the cases of the GPU pins (shared with the CPU file, which proves the exactness condition of each) --------------------
# forward: Cout = M, Cin = K; data gradient: Cin = M, Cout = K.  (family, M, K, tile, launch class)
PLAIN_CASES = [("paired", 64, 48, 64, 2), ("full", 128, 16, 64, 2),
               ("paired", 128, 64, 64, 4), ("mixed", 64, 128, 64, 4), ("full", 256, 256, 64, 4), ("sparse", 128, 64, 64, 4),
               ("paired", 64, 64, 128, 3), ("mixed", 128, 64, 128, 3), ("full", 256, 128, 128, 3)]
# the remainder-split cases, tile 128: (family, slots, M, K); slots None = the natural slot count of M output rows
SPLIT_CASES = [("paired", 8, 64, 64), ("paired", 14, 128, 64), ("mixed", 15, 256, 64), ("mixed", 9, 64, 128),
               ("full", 4, 128, 64), ("full", 32, 64, 64), ("mixed", 128, 128, 64), ("sparse", None, 64, 64), ("sparse", None, 128, 128),
               ("sparse", None, 256, 64), ("paired", None, 128, 64)]
WGRAD_CASES = [("paired", 64, 64), ("mixed", 128, 64), ("full", 64, 128), ("sparse", 128, 128), ("paired", 256, 64)]   # Cout, Cin
# o3d_mlp_conv_bwd_fused_c (Cin = 64): (family or dense column count, Cout, dead channel)
FUSED_CASES = [("paired", 64, True), ("paired", 128, False), ("mixed", 64, False), ("sparse", 128, True), (1024, 64, False),
               (4160, 128, True)]


def case_seed(*key):
    return 9000 + sum((k + 1) * sum(map(ord, str(v))) for k, v in enumerate(key)) % 1000


def kind_dims(kind, M, K):
    """-> (Cin, Cout) of a forward / data-gradient case with M output rows and contraction K"""
    return (K, M) if kind == "fwd" else (M, K)


def cap_margin(T, S, cap):
    """workgroups the chosen split needs beyond the segment's grid: T + R*(f-1) - cap (None: no split was chosen)"""
    R = T % S if S > 0 and T > 0 else 0
    f = 4 if 4 * R <= S else 2 if 2 * R <= S else 1
    return T + R * (f - 1) - cap if R and f > 1 else None


def split_coverage(cases=None):
    """which branches of the plan the split cases reach together -> set of names.  cap_exact / cap_near: a split that fills
    its segment's grid exactly, and one refused for want of at most 4 workgroups -- a finalize whose cap is smaller, or larger,
    than the GEMM's then follows another plan than the launch did"""
    seen = set()
    for fam, S, M, _ in (cases or SPLIT_CASES):
        L = layout(fam)
        S = S if S is not None else NATURAL_SLOTS[M]
        why = plan_reasons(L, S)
        for s in range(L.nseg):
            m = cap_margin(L.live256[s] // 128, S, seg_caps(L)[s])
            if m is not None and 0 <= m <= 4:
                seen.add("cap_exact" if m == 0 else "cap_near")
        for w, full in why:
            seen.add({"f4": "f4_full0" if full == 0 else "f4_full>0"}.get(w, w))
        if L.nseg == 2 and why[0] != why[1]:
            seen.add("two_plans")
        seen.add("one_segment" if L.nseg == 1 else "two_segments")
    return seen


SPLIT_BRANCHES = {"R0", "f4_full0", "f4_full>0", "f2", "2R>S", "cap", "cap_exact", "cap_near", "two_plans", "one_segment",
                  "two_segments"}
