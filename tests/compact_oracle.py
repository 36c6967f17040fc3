"""Plain numpy fp64 reference of the compact (distinct-neighbour) layout and of the streaming kernels that work on it
(csrc/compact.hip), written from the formulas of include/o3dsot.h and the kernel comments.  It imports nothing of the
package under test.  Shared by tests/test_compact_oracle_cpu.py (which ties it to the slot-wise operator) and
tests/test_compact_kernels_gpu.py (which pins every export to it).

Conventions
  idx            (B, npoint, ns) per segment, padded as ball_query pads: a suffix of copies of the first hit
  columns        one per distinct entry of a ball, in (cloud, ball, slot) order; segment 1 starts at `start1`
  pooled values  handled here as (C, nballs) matrices (ball-major); `to_pooled` / `from_pooled` convert to and from the
                 device form: one (B, C, npoint_s) block per segment, segment 1's after segment 0's
  *_abs          the same sum over the absolute values of every product that enters a term: the yardstick of the exactness
                 condition (sum|terms| / spacing < 2^24) and of the rounding bound (n + 8) * 2^-24 * sum|terms|
"""
import numpy as np

FILL_I = -77777            # what the oracle puts where o3d_compact_build[2] writes nothing
TWO24 = float(1 << 24)


def ball_counts(idx):
    """distinct entries per ball = one past the last slot that differs from the first hit (1 when none does)"""
    ns = idx.shape[-1]
    last = np.where(idx != idx[..., :1], np.arange(ns), -1).max(-1)
    return np.maximum(last + 1, 1).reshape(-1).astype(np.int64)


class Layout:
    """segs: [(idx (B, npoint, ns), ld)] for one or two segments.  start1 / ldp / dummy_ball default to what the set
    abstraction modules use: start1 = worst case of segment 0 (all slots distinct), ldp = all slots, dummy = nballs."""

    def __init__(self, segs, start1=None, ldp=None, dummy_ball=None):
        self.nseg = len(segs)
        self.B, _, self.ns = segs[0][0].shape
        B, ns = self.B, self.ns
        self.npoint = [s[0].shape[1] for s in segs]
        self.ld = [s[1] for s in segs]
        self.nballs_s = [B * n for n in self.npoint]
        self.nballs = sum(self.nballs_s)
        self.ball_base = [0, self.nballs_s[0]][:self.nseg]
        self.pt_base = [0, B * self.ld[0]][:self.nseg]
        self.ldz = sum(B * l for l in self.ld)
        worst = [n * ns for n in self.nballs_s]
        self.start1 = (worst[0] if start1 is None else start1) if self.nseg == 2 else 0
        self.start = [0, self.start1][:self.nseg]
        self.ldp = sum(worst) if ldp is None else ldp
        self.dummy_ball = self.nballs if dummy_ball is None else dummy_ball
        self.gp = np.full(self.ldp, FILL_I, np.int64)
        self.cball = np.full(self.ldp, FILL_I, np.int64)
        self.cw = np.full(self.ldp, float(FILL_I))
        self.ball_cnt = np.zeros(self.nballs, np.int64)
        self.ball_off = np.zeros(self.nballs, np.int64)
        self.meta = np.zeros((self.nseg, 4), np.int64)
        self.live, self.live256 = [], []
        for s, (idx, ld) in enumerate(segs):
            n, np_s = self.nballs_s[s], self.npoint[s]
            cnt = ball_counts(idx)
            off = self.start[s] + np.concatenate([[0], np.cumsum(cnt)[:-1]])
            live = int(cnt.sum())
            live256 = (live + 255) // 256 * 256
            assert self.start[s] + live256 <= (self.start[s + 1] if s + 1 < self.nseg else self.ldp)
            sl = slice(self.ball_base[s], self.ball_base[s] + n)
            self.ball_cnt[sl], self.ball_off[sl] = cnt, off
            ball = np.repeat(np.arange(n), cnt)
            k = np.arange(live) - np.repeat(off - self.start[s], cnt)
            q = self.start[s] + np.arange(live)
            self.gp[q] = self.pt_base[s] + (ball // np_s) * ld + idx.reshape(n, ns)[ball, k]
            self.cball[q] = self.ball_base[s] + ball
            self.cw[q] = np.where(k == 0, 1 + ns - cnt[ball], 1)
            pad = np.arange(self.start[s] + live, self.start[s] + live256)
            self.gp[pad], self.cball[pad], self.cw[pad] = 0, self.dummy_ball, 0.0
            self.meta[s] = (live256, live, n, 0)
            self.live.append(live)
            self.live256.append(live256)
        # real columns in ball order, the columns the kernels may write (real + padding), the start of every ball in `real`
        self.real = np.concatenate([self.start[s] + np.arange(self.live[s]) for s in range(self.nseg)])
        self.written = np.concatenate([self.start[s] + np.arange(self.live256[s]) for s in range(self.nseg)])
        self.rstart = np.concatenate([[0], np.cumsum(self.ball_cnt)[:-1]])
        self.ball_seg = (np.arange(self.nballs) >= self.nballs_s[0]).astype(np.int64) if self.nseg == 2 else \
            np.zeros(self.nballs, np.int64)

    def seg_of_col(self, q):
        return ((self.start1 > 0) & (np.asarray(q) >= self.start1)).astype(np.int64)

    def unwritten(self):
        m = np.ones(self.ldp, bool)
        m[self.written] = False
        return m

    def per_channel(self, v, C, seg):
        """(nseg*C,) constants -> (C, len(seg)): every column / ball reads its segment's block"""
        return np.asarray(v, np.float64).reshape(self.nseg, C)[seg].T

    def to_pooled(self, M):
        out = []
        for s in range(self.nseg):
            blk = M[:, self.ball_base[s]:self.ball_base[s] + self.nballs_s[s]]
            out.append(blk.reshape(M.shape[0], self.B, self.npoint[s]).transpose(1, 0, 2).ravel())
        return np.concatenate(out)

    def from_pooled(self, flat, C):
        out, o = [], 0
        for s in range(self.nseg):
            n = self.nballs_s[s] * C
            out.append(np.asarray(flat[o:o + n]).reshape(self.B, C, self.npoint[s]).transpose(1, 0, 2).reshape(C, -1))
            o += n
        return np.concatenate(out, axis=1)


# ---- expand ------------------------------------------------------------------------------------------------------------
def expand(L, W0, centers, Z=None, X3=None):
    """Y0[c,q] = Z[c,gp[q]] - W0[c,0:3].centers[cball[q]]  (Z form; centers None: no centre term) or
    W0[c,0:3].(X3[:,gp[q]] - centers[cball[q]])  (X3 form), on every written column (padding included: gp 0, dummy ball).
    -> Y0, Y0_abs (C0, ldp), NaN where nothing is written."""
    C0 = W0.shape[0]
    q = L.written
    gp = L.gp[q]
    ctr = centers[L.cball[q]].T if centers is not None else np.zeros((3, len(q)))
    w = W0[:, :3]
    if X3 is not None:
        y = np.einsum("ck,kq->cq", w, X3[:3, gp] - ctr)
        ya = np.einsum("ck,kq->cq", np.abs(w), np.abs(X3[:3, gp]) + np.abs(ctr))
    else:
        y = Z[:, gp] - w @ ctr
        ya = np.abs(Z[:, gp]) + np.abs(w) @ np.abs(ctr)
    Y0, Ya = np.full((C0, L.ldp), np.nan), np.full((C0, L.ldp), np.nan)
    Y0[:, q], Ya[:, q] = y, ya
    return Y0, Ya


def expand_part(L, Y0, Y0_abs, stat_c):
    """part[chunk][0][c] = sum cw*Y0, part[chunk][1][c] = sum cw*(Y0 - stat_c[c])^2 per live 256-column chunk (segment 1
    reads stat_c + C0).  -> part, part_abs (ldp/256, 2, C0) with NaN in the dead rows, live (bool per row)."""
    C0, rows = Y0.shape[0], L.ldp // 256
    part, pabs = np.full((rows, 2, C0), np.nan), np.full((rows, 2, C0), np.nan)
    live = np.zeros(rows, bool)
    live[L.written[::256] // 256] = True
    for r in np.nonzero(live)[0]:
        sl = slice(r * 256, r * 256 + 256)
        seg = int(L.seg_of_col(r * 256))
        c = np.asarray(stat_c, np.float64).reshape(L.nseg, C0)[seg][:, None] if stat_c is not None else 0.0
        w = L.cw[sl][None, :]
        part[r, 0], part[r, 1] = (w * Y0[:, sl]).sum(1), (w * (Y0[:, sl] - c) ** 2).sum(1)
        pabs[r, 0], pabs[r, 1] = (w * Y0_abs[:, sl]).sum(1), (w * (Y0_abs[:, sl] + np.abs(c)) ** 2).sum(1)
    return part, pabs, live


# ---- pool ---------------------------------------------------------------------------------------------------------------
def pool_fwd(L, Y, scale, shift):
    """out = max(0, max_q fma(Y, scale, shift)) over the ball's columns, argq = the smallest column that attains the
    maximum, yarg = Y[c, argq]; segment 1 reads scale / shift at +C.  -> out, argq, yarg as (C, nballs)."""
    C = Y.shape[0]
    seg = L.seg_of_col(L.real)
    n = Y[:, L.real] * L.per_channel(scale, C, seg) + L.per_channel(shift, C, seg)
    m = np.maximum.reduceat(n, L.rstart, axis=1)
    pos = np.where(n == np.repeat(m, L.ball_cnt, axis=1), np.arange(len(L.real))[None, :], len(L.real))
    first = np.minimum.reduceat(pos, L.rstart, axis=1)
    argq = L.real[first]
    yarg = np.take_along_axis(Y, argq, axis=1)
    return np.maximum(m, 0.0), argq, yarg


def pool_bwd(L, dOut, out, argq, yarg, mean):
    """g = dOut where out > 0 (strictly) else 0; D[c, argq] = g, every other written column 0; per segment the totals
    sum g and sum g*(yarg - mean).  dOut None = zeros.  -> D (C, ldp; NaN where nothing is written), tot, tot_abs
    (nseg, 2, C), cnt (nseg,) = balls per segment (the number of terms)."""
    C = out.shape[0]
    g = np.where(out > 0, dOut, 0.0)
    D = np.full((C, L.ldp), np.nan)
    D[:, L.written] = 0.0
    D[np.arange(C)[:, None], argq] = g
    mu = L.per_channel(mean, C, L.ball_seg)
    tot, tabs = np.zeros((L.nseg, 2, C)), np.zeros((L.nseg, 2, C))
    for s in range(L.nseg):
        sl = slice(L.ball_base[s], L.ball_base[s] + L.nballs_s[s])
        tot[s, 0], tot[s, 1] = g[:, sl].sum(1), (g[:, sl] * (yarg[:, sl] - mu[:, sl])).sum(1)
        tabs[s, 0] = np.abs(g[:, sl]).sum(1)
        tabs[s, 1] = (np.abs(g[:, sl]) * (np.abs(yarg[:, sl]) + np.abs(mu[:, sl]))).sum(1)
    return D, tot, tabs, np.array(L.nballs_s)


# ---- layer-0 backward sums -----------------------------------------------------------------------------------------------
def layer0_dy(L, dN, Y0, A1, A2, A3):
    """dY = A1*dN + cw*(A2*Y0 + A3) on the real columns (segment 1: constants at +C0) -> dY, dY_abs (C0, len(L.real))"""
    C0 = dN.shape[0]
    seg = L.seg_of_col(L.real)
    a1, a2, a3 = (L.per_channel(a, C0, seg) for a in (A1, A2, A3))
    w = L.cw[L.real][None, :]
    d, y = dN[:, L.real], Y0[:, L.real]
    return a1 * d + w * (a2 * y + a3), np.abs(a1 * d) + w * (np.abs(a2 * y) + np.abs(a3))


def reduce_sums(L, dY):
    """S[c, point column] = sum of dY over the columns q with gp[q] = column; T[c, ball] = sum over the ball's columns"""
    S = np.zeros((dY.shape[0], L.ldz))
    np.add.at(S.T, L.gp[L.real], dY.T)
    return S, np.add.reduceat(dY, L.rstart, axis=1)


def dw0_xyz(L, dY, X, centers, absolute=False):
    """dW0[c,k] = sum_q dY[c,q] * (X[k,gp[q]] - centers[cball[q],k]) over both segments; absolute: dY is dY_abs and the
    relative coordinate is replaced by |X| + |centre|"""
    x, c = X[:3, L.gp[L.real]], centers[L.cball[L.real]].T
    return dY @ ((np.abs(x) + np.abs(c)) if absolute else (x - c)).T


# ---- centre terms, point packing -------------------------------------------------------------------------------------
def center_term(T, centers, dW, absolute=False):
    """dW (C0, ldw) with columns 0..2 -= T (C0, nballs) . centers (nballs, 3)"""
    out = np.abs(dW) if absolute else dW.copy()
    t = T @ centers[:T.shape[1]] if not absolute else np.abs(T) @ np.abs(centers[:T.shape[1]])
    out[:, :3] = out[:, :3] + t if absolute else out[:, :3] - t
    return out


def center_term_out(T, centers, dW, ncols, absolute=False):
    return center_term(T, centers, dW, absolute)[:, :ncols]


def center_grad(T, W0, scale, absolute=False):
    """out (3, nballs)[k, ball] = scale * sum_c W0[c, k] * T[c, ball]"""
    if absolute:
        return abs(scale) * (np.abs(W0[:, :3]).T @ np.abs(T))
    return scale * (W0[:, :3].T @ T)


def pack_points(xyz0, feats0, N0, ld0, xyz1, feats1, N1, ld1, B, nxyz, C, inv_radius, rows):
    """X0 (rows, B*(ld0+ld1)): rows [0,nxyz) = xyz^T * inv_radius, [nxyz, nxyz+C) = feats, the rest zero; cloud b of
    segment s in columns [base_s + b*ld_s, +N_s), zero up to ld_s"""
    segs = [(xyz0, feats0, N0, ld0)] + ([(xyz1, feats1, N1, ld1)] if N1 > 0 else [])
    X0 = np.zeros((rows, sum(B * s[3] for s in segs)))
    base = 0
    for xyz, feats, N, ld in segs:
        for b in range(B):
            c0 = base + b * ld
            if nxyz:
                X0[:nxyz, c0:c0 + N] = xyz[b].T * inv_radius
            if C:
                X0[nxyz:nxyz + C, c0:c0 + N] = feats[b]
        base += B * ld
    return X0


# ---- index families: hand-built, the smallest that reach a path ----------------------------------------------------------
def _rows(members, ns):
    row = np.full(ns, members[0], np.int64)
    row[:len(members)] = members
    return row


def _idx_from_counts(rng, counts, B, npoint, ns, N, hub=None):
    """balls of counts[b*npoint + j] distinct points below N; hub: a point every ball holds (first on even balls, last on
    odd ones)"""
    idx = np.zeros((B, npoint, ns), np.int64)
    pool = np.array([p for p in range(N) if p != hub])
    for b in range(B):
        for j in range(npoint):
            cnt = int(counts[b * npoint + j])
            if hub is None:
                mem = list(rng.choice(N, cnt, replace=False))
            else:
                rest = list(rng.choice(pool, cnt - 1, replace=False))
                mem = [hub] + rest if j % 2 == 0 else rest + [hub]
            idx[b, j] = _rows(mem, ns)
    return idx


_FAMILY_CACHE = {}
HUB = 7


def family(name):
    """-> dict(segs=[(idx, N, ld)], ns=, B=); deterministic"""
    if name in _FAMILY_CACHE:
        return _FAMILY_CACHE[name]
    rng = np.random.RandomState({"singles": 11, "full": 12, "mixed": 13, "paired": 14, "wide": 15}[name])
    if name == "singles":        # every ball one distinct point: 512 balls start in a 512-column chunk, 128 in a 128-column one
        B, npoint, ns, N, ld = 2, 320, 8, 320, 384
        idx = np.stack([np.repeat(rng.permutation(N)[:, None], ns, axis=1) for _ in range(B)])
        segs = [(idx, N, ld)]
    elif name == "full":         # every slot distinct: live = 1024 = ldp, no padding columns, cw = 1
        B, npoint, ns, N, ld = 2, 16, 32, 48, 64
        segs = [(_idx_from_counts(rng, np.full(B * npoint, ns), B, npoint, ns, N), N, ld)]
    elif name == "mixed":        # counts 1..32, twelve of each, in a seeded order; point HUB in every ball; N < ld
        B, npoint, ns, N, ld = 3, 128, 32, 100, 128
        counts = rng.permutation(np.tile(np.arange(1, ns + 1), B * npoint // ns))
        segs = [(_idx_from_counts(rng, counts, B, npoint, ns, N, hub=HUB), N, ld)]
    elif name == "paired":       # template (counts 1 or 2: fewer than 256 live columns) + search segment
        B, ns = 2, 16
        c0 = rng.randint(1, 3, B * 64)
        c1 = rng.randint(1, ns + 1, B * 128)
        segs = [(_idx_from_counts(rng, c0, B, 64, ns, 100), 100, 128), (_idx_from_counts(rng, c1, B, 128, ns, 200), 200, 256)]
    elif name == "wide":         # ns = 64, every count 1..64 once
        B, npoint, ns, N, ld = 1, 64, 64, 100, 128
        segs = [(_idx_from_counts(rng, rng.permutation(np.arange(1, 65)), B, npoint, ns, N), N, ld)]
    else:
        raise KeyError(name)
    _FAMILY_CACHE[name] = dict(segs=segs, ns=ns, B=B)
    return _FAMILY_CACHE[name]


_LAYOUT_CACHE = {}


def family_layout(name):
    if name not in _LAYOUT_CACHE:
        _LAYOUT_CACHE[name] = Layout([(idx, ld) for idx, _, ld in family(name)["segs"]])
    return _LAYOUT_CACHE[name]


def straddlers(L, m):
    """balls with a multiple of m strictly inside their column range -> [(ball, boundary column)]"""
    off, end = L.ball_off, L.ball_off + L.ball_cnt
    b = (end - 1) // m * m
    return [(int(i), int(b[i])) for i in np.nonzero((b > off) & (b < end))[0]]


# ---- inputs ------------------------------------------------------------------------------------------------------------
class Dyadic:
    """values on small dyadic grids: every product and partial sum of a correct kernel is then exact in fp32"""
    exact = True

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def val(self, shape, step, lim):
        k = int(round(lim / step))
        return self.rng.randint(-k, k + 1, size=shape) * float(step)

    def coef(self, shape, zero=True):
        return self.rng.choice(np.array([1.0, -1.0, 0.5, -0.5] + ([0.0] if zero else [])), size=shape)


# grid spacing of the terms of every exactly compared output (products of the input steps below)
SPACING = {"Y0": 0.25, "part0": 0.25, "part1": 1.0 / 16, "pool": 0.125, "bwd0": 0.25, "bwd1": 1.0 / 16, "S": 0.125, "T": 0.125,
           "dW0": 1.0 / 16, "center_term": 1.0 / 16, "center_grad": 1.0 / 16, "pack": 0.125}


def expand_inputs(L, C0, draw, ldw=5):
    ctr = draw.val((L.nballs + 1, 3), 0.5, 1.0)
    ctr[L.nballs] = 0.0                                   # the dummy ball of the padding columns: the origin
    return dict(Z=draw.val((C0, L.ldz), 0.5, 1.0), X3=draw.val((3, L.ldz), 0.5, 1.0), centers=ctr,
                W0=draw.coef((C0, ldw)), stat_c=draw.val((L.nseg * C0,), 0.25, 0.5))


def pool_inputs(L, C, draw):
    scale = draw.coef((L.nseg * C,), zero=False)
    if C > 5:
        scale[5] = 0.0                                    # a dead channel: every column ties
    return dict(Y=draw.val((C, L.ldp), 0.25, 2.0), scale=scale, shift=draw.val((L.nseg * C,), 0.25, 1.0),
                dOut=draw.val((C, L.nballs), 0.25, 2.0), mean=draw.val((L.nseg * C,), 0.25, 0.5))


def layer0_inputs(L, C0, draw):
    ctr = draw.val((L.nballs + 1, 3), 0.5, 1.0)
    ctr[L.nballs] = 0.0
    return dict(dN=draw.val((C0, L.ldp), 0.25, 2.0), Y0=draw.val((C0, L.ldp), 0.25, 2.0), A1=draw.coef((L.nseg * C0,)),
                A2=draw.coef((L.nseg * C0,)), A3=draw.coef((L.nseg * C0,)), X=draw.val((3, L.ldz), 0.5, 1.0), centers=ctr)


def center_inputs(nballs, C0, ldw, draw):
    return dict(T=draw.val((C0, nballs), 0.25, 2.0), centers=draw.val((nballs, 3), 0.25, 2.0), dW=draw.val((C0, ldw), 0.25, 2.0),
                W0=draw.coef((C0, ldw)))


def pack_inputs(two, draw, B=2, C=3):
    """N < ld in both segments; -> dict(N0, ld0, N1, ld1, xyz=[..], feats=[..]) (N1 = 0: one segment)"""
    N0, ld0, N1, ld1 = 100, 128, (37 if two else 0), (64 if two else 0)
    return dict(N0=N0, ld0=ld0, N1=N1, ld1=ld1, xyz=[draw.val((B, N, 3), 0.25, 2.0) for N in (N0, N1)],
                feats=[draw.val((B, C, N), 0.25, 2.0) for N in (N0, N1)])


def assert_exact(name, abs_sum):
    """the exactness condition of an output whose terms lie on the grid SPACING[name]: sum|terms| / spacing < 2^24"""
    worst = float(np.nanmax(abs_sum)) / SPACING[name]
    assert worst < TWO24, (name, worst, TWO24)
    return worst


def plant_pool(L, Y, scale, shift):
    """Overwrite Y (C >= 4 channels, in place) so that chosen balls meet the edges of the pool: -> [(what, channel, ball,
    argq or None, out)] the expected result of every plant.  Planted values are set through n = Y*scale + shift on the
    1/4 grid (scale of the planted channels is +-1 or +-1/2, so Y stays on the 1/4 grid, |Y| <= 8)."""
    C = Y.shape[0]
    sc = np.asarray(scale).reshape(L.nseg, C)
    sh = np.asarray(shift).reshape(L.nseg, C)
    plants = []

    def put(what, c, ball, n, want_rel, out):
        s = int(L.ball_seg[ball])
        assert sc[s, c] != 0.0
        off, cnt = int(L.ball_off[ball]), int(L.ball_cnt[ball])
        Y[c, off:off + cnt] = (np.asarray(n, np.float64) - sh[s, c]) / sc[s, c]
        plants.append((what, c, ball, None if want_rel is None else off + want_rel, out))

    used = set()
    for m in (128, 512):
        st = [(b, q) for b, q in straddlers(L, m) if b not in used]
        if st:
            ball, q = st[0]
            used.add(ball)
            off, cnt = int(L.ball_off[ball]), int(L.ball_cnt[ball])
            for c, rel in ((0, q - 1 - off), (1, q - off)):           # just before / just after the boundary
                n = np.full(cnt, -1.0)
                n[rel] = 1.5
                put("boundary%d%s" % (m, "-" if c == 0 else "+"), c, ball, n, rel, 1.5)
    big = [int(b) for b in np.nonzero(L.ball_cnt >= 3)[0] if int(b) not in used]
    pick = big[::max(1, len(big) // 7)][:7] if big else []
    if len(pick) == 7:
        cnts = [int(L.ball_cnt[b]) for b in pick]
        n = np.full(cnts[0], -0.5); n[0] = 1.0
        put("first", 0, pick[0], n, 0, 1.0)
        n = np.full(cnts[1], -0.5); n[-1] = 1.0
        put("last", 1, pick[1], n, cnts[1] - 1, 1.0)
        put("all_equal", 2, pick[2], np.full(cnts[2], 0.75), 0, 0.75)
        n = np.full(cnts[3], 0.25); n[1] = n[-1] = 1.25
        put("tie", 3, pick[3], n, 1, 1.25)
        n = np.full(cnts[4], 0.25); n[cnts[4] // 2] = n[cnts[4] // 2 + 1] = 1.25
        put("tie_adjacent", 0, pick[4], n, cnts[4] // 2, 1.25)
        put("all_negative", 1, pick[5], -0.25 - 0.25 * (np.arange(cnts[5]) % 3), None, 0.0)
        n = np.full(cnts[6], -0.5); n[cnts[6] - 1] = 0.0
        put("max_is_zero", 2, pick[6], n, cnts[6] - 1, 0.0)
    else:                       # balls of one column (singles): only the sign cases exist
        put("all_negative", 1, 3, [-0.25], None, 0.0)
        put("max_is_zero", 2, 5, [0.0], 0, 0.0)
    return plants
