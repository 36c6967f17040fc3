"""fp64 references, input builders and error bounds for tests/test_index_kernels_gpu.py -- TEST INFRASTRUCTURE.

The index operators proper (FPS, ball query, group / gather, 3-NN, kNN, the interpolation's fmaf chain) are compared for
EQUALITY with oracle.ops, the C restatement.  This file holds what that restatement does not:
  * the three scatter-adds in fp64 through np.add.at, with the number of terms n and sum |t_i| of every destination:
    |got - ref| <= gamma_n sum |t_i|, gamma_n = n u / (1 - n u), u = 2^-24 -- n - 1 additions (the first one, to the zero fill,
    is exact) plus the one rounding of the product g * w where there is one; the bound holds for every order of the atomics;
  * the interpolation forward without fma in fp64 and its bound 3 u sum |f_i w_i|;
  * BoxCloud: centre and corners in fp64 in the order of Box.corners (datasets/data_classes.py:226-250:
    x = l/2 [1,1,1,1,-1,-1,-1,-1], y = w/2 [1,-1,-1,1,1,-1,-1,1], z = h/2 [1,1,-1,-1,1,1,-1,-1], rotated, translated) and a bound
    propagated through csrc/boxcloud.hip operation by operation, one rounding per multiply, add and square root.  The kernel
    is built with contraction on; a contracted a * b + c rounds once where the separate operations round twice, so the bound
    derived WITHOUT contraction holds either way.  sqrtf is correctly rounded in this build: csrc/boxcloud.hip is compiled with
    the flags of csrc/xcorr.hip (no fast-math), for which DESIGN.md section 2 states it; the bound rests on that.  Underflow is
    ignored: every intermediate of the test's inputs is above 2^-100;
  * plain-numpy FPS / ball query / kNN with their tie rules as parameters, exact on dyadic inputs, which
    tests/test_index_oracle_cpu.py ties to oracle.ops and turns into the wrong variants the comparisons must reject;
  * the input builders of the GPU file (clouds, decoys, exact-leg values), so that the CPU file checks the very same inputs.
"""
import numpy as np

U = 2.0 ** -24
F32 = np.float32


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


# ==== clouds ========================================================================================================================
FPS_DECOY = 1.0e4            # the point behind a sampled cloud: farther than anything in it, so an over-read makes it the winner
FPS_SIZES = (1, 2, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)
FPS_KINDS = ("normal", "grid", "last")
FAR_SCALE = 2.0e5


def fps_cloud(kind, B, N, seed):
    """normal: randn.  grid: half-integers in [-4, 4] (ties in every round; points at the origin fall under the near-origin rule).
    last: a unit cube with point N - 1 moved 50 away from point 0 -- the unique farthest, held by the last slot in use.
    far: randn * 2e5 -- most pairwise d^2 above the 1e10f the running minimum starts from, rounds decided by the rank alone.
    fargrid: integers * 2^18, the same regime with every distance exact in fp32 and fp64."""
    rng = np.random.RandomState(seed)
    if kind == "normal":
        x = rng.randn(B, N, 3)
    elif kind == "grid":
        x = rng.randint(-8, 9, size=(B, N, 3)) * 0.5
    elif kind == "last":
        x = rng.rand(B, N, 3) + 1.0
        if N > 1:
            x[:, N - 1] = x[:, 0] + np.array([50.0, 0.0, 0.0])
    elif kind == "far":
        x = rng.randn(B, N, 3) * FAR_SCALE
    elif kind == "fargrid":
        x = rng.randint(-3, 4, size=(B, N, 3)) * 2.0 ** 18
    else:
        raise ValueError(kind)
    return x.astype(F32)


def lead_with(cloud, row, count=3):
    """cloud b >= 1 begins with `count` copies of `row` ((3,) or (B, 3): per preceding cloud): what an over-read of cloud b - 1
    would meet.  Only the last cloud has a device tail, so this is how the earlier ones get their decoys."""
    cloud = cloud.copy()
    row = np.asarray(row, F32)
    for b in range(1, cloud.shape[0]):
        c = min(count, cloud.shape[1])
        cloud[b, :c] = row if row.ndim == 1 else row[b - 1]
    return cloud


def far_fraction(cloud):
    """fraction of ordered pairs i != j of one cloud (N, 3) whose fp32 squared distance exceeds 1e10f"""
    x = cloud.astype(np.float64)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    n = len(x)
    return float(((d > 1e10).sum()) / (n * (n - 1)))


# ==== plain-numpy index operators with their tie rules open (exact on dyadic inputs) =====================================================
def opt_n_threads(n):
    p = 1
    while p * 2 <= n and p * 2 <= 512:
        p *= 2
    return p


def upstream_rank(N):
    """rank(k) = bitrev_L(k mod bs) * ceil(N / bs) + k div bs, bs = opt_n_threads(N): the lowest rank wins a tie"""
    bs = opt_n_threads(N)
    L = bs.bit_length() - 1
    k = np.arange(N)
    tid = k % bs
    rev = np.zeros(N, np.int64)
    for bit in range(L):
        rev |= ((tid >> bit) & 1) << (L - 1 - bit)
    return rev * ((N + bs - 1) // bs) + k // bs


def fps_numpy(xyz, npoint, rank=None, last_max=False):
    """FPS of (B, N, 3) in fp64 on fp32 inputs (exact when the inputs are dyadic and small): start at 0, points with
    |p|^2 <= 1e-3 never selected, the winner among equal maxima the lowest `rank` (default: upstream_rank), or the HIGHEST
    with last_max; nothing selectable -> 0"""
    xyz = np.asarray(xyz, F32).astype(np.float64)
    B, N, _ = xyz.shape
    rank = upstream_rank(N) if rank is None else np.asarray(rank)
    out = np.zeros((B, npoint), np.int32)
    for b in range(B):
        p = xyz[b]
        valid = (p * p).sum(-1) > 1e-3
        temp = np.full(N, float(F32(1e10)))
        old = 0
        for j in range(1, npoint):
            d = ((p - p[old]) ** 2).sum(-1)
            temp = np.where(valid, np.minimum(d, temp), temp)
            if not valid.any():
                old = 0
            else:
                top = valid & (temp == temp[valid].max())
                cand = np.flatnonzero(top)
                old = int(cand[np.argmax(rank[cand])] if last_max else cand[np.argmin(rank[cand])])
            out[b, j] = old
    return out


def ball_query_numpy(new_xyz, xyz, radius, nsample, pad_first=True, strict=True):
    """first nsample k (ascending) with d^2 < r^2, padded with the first hit, zeros if none; the two rules as switches"""
    c = np.asarray(new_xyz, F32).astype(np.float64)
    p = np.asarray(xyz, F32).astype(np.float64)
    r2 = float(F32(radius) * F32(radius))
    B, npoint, _ = c.shape
    out = np.zeros((B, npoint, nsample), np.int32)
    for b in range(B):
        for j in range(npoint):
            d = ((p[b] - c[b, j]) ** 2).sum(-1)
            hits = np.flatnonzero(d < r2 if strict else d <= r2)[:nsample]
            if len(hits):
                out[b, j, :] = hits[0] if pad_first else 0
                out[b, j, :len(hits)] = hits
    return out


def knn_numpy(query, ref, k, stable=True):
    """ascending squared distance; ties -> lowest index, or the highest with stable=False (what an unstable sort may give)"""
    q = np.asarray(query, F32).astype(np.float64)
    r = np.asarray(ref, F32).astype(np.float64)
    d = ((q[:, :, None, :] - r[:, None, :, :]) ** 2).sum(-1)                 # (B, Q, R)
    R = r.shape[1]
    if stable:
        order = np.argsort(d, axis=-1, kind="stable")
    else:
        order = (R - 1 - np.argsort(d[..., ::-1], axis=-1, kind="stable"))
    return order[..., :k].astype(np.int32)


# ==== the three scatter-adds ==================================================================================================================
class Scatter(object):
    """ref (fp64 sum), abs (sum |t_i|), cnt (terms per destination), bound = gamma_cnt * abs -- all (B, C, N)"""

    def __init__(self, ref, ab, cnt):
        self.ref, self.abs, self.cnt = ref, ab, cnt
        self.bound = gamma(cnt) * ab


def _scatter(terms, dest, N):
    """terms (B, C, T) fp64, dest (B, T) -> Scatter over (B, C, N)"""
    B, C, _ = terms.shape
    ref, ab, cnt = np.zeros((B, C, N)), np.zeros((B, C, N)), np.zeros((B, C, N))
    for b in range(B):
        np.add.at(ref[b], (slice(None), dest[b]), terms[b])
        np.add.at(ab[b], (slice(None), dest[b]), np.abs(terms[b]))
        np.add.at(cnt[b], (slice(None), dest[b]), 1.0)
    return Scatter(ref, ab, cnt)


def group_points_grad(grad_out, idx, N):
    """grad_out (B, C, npoint, nsample) [or (B, C, npoint): the gather], idx of the trailing shape -> Scatter (B, C, N)"""
    g = np.asarray(grad_out, F32).astype(np.float64)
    B, C = g.shape[:2]
    return _scatter(g.reshape(B, C, -1), np.asarray(idx).reshape(B, -1), N)


gather_points_grad = group_points_grad


def three_interpolate_grad(grad_out, idx, weight, m):
    """grad_out (B, c, n), idx / weight (B, n, 3) -> Scatter (B, c, m); the terms are the EXACT products g * w (fp64 holds the
    product of two fp32 exactly), their fp32 rounding is one of the n roundings gamma_n allows"""
    g = np.asarray(grad_out, F32).astype(np.float64)
    w = np.asarray(weight, F32).astype(np.float64)
    B, c, n = g.shape
    terms = (g[:, :, :, None] * w[:, None, :, :]).reshape(B, c, n * 3)
    return _scatter(terms, np.asarray(idx).reshape(B, n * 3), m)


def three_interpolate(feats, idx, weight):
    """-> (out fp64 (B, c, n) = sum of the three exact products, bound = 3 u sum |f_i w_i|)"""
    f = np.asarray(feats, F32).astype(np.float64)
    w = np.asarray(weight, F32).astype(np.float64)
    idx = np.asarray(idx)
    B, c, m = f.shape
    n = idx.shape[1]
    out, ab = np.zeros((B, c, n)), np.zeros((B, c, n))
    for b in range(B):
        for t in range(3):
            p = f[b][:, idx[b, :, t]] * w[b, :, t][None, :]
            out[b] = out[b] + p
            ab[b] = ab[b] + np.abs(p)
    return out, 3.0 * U * ab


def dyadic(rng, shape, den=64, top=4):
    """multiples of 1 / den with |v| <= top"""
    return (rng.randint(-top * den, top * den + 1, size=shape) / float(den)).astype(F32)


EXACT_TERMS = 4096           # at most this many terms per destination: 4096 * 4 * 256 = 2^22 < 2^24 units of the coarsest grid


def exact_scatter_idx(rng, B, Q, N, skip):
    """cloud 0: every one of the Q contributions lands on destination 2 (all others receive none); clouds >= 1: spread over
    every destination but `skip`, which receives none"""
    idx = np.zeros((B, Q), np.int32)
    idx[0] = 2
    pool = np.array([i for i in range(N) if i != skip])
    for b in range(1, B):
        idx[b] = pool[rng.randint(0, len(pool), size=Q)]
    return idx


def exact_interp_inputs(rng, B, c, n, m):
    """m >= 8.  cloud 0: neighbour 0 of every unknown is destination 2 (n terms), neighbours 1 / 2 spread over {0, 1, 3, 4} /
    {5, 6}, destination 7 and above receive nothing; clouds >= 1 spread over all but destination m - 1.  Weights 1/4, 1/2, 1."""
    g = dyadic(rng, (B, c, n))
    w = (2.0 ** rng.randint(-2, 1, size=(B, n, 3))).astype(F32)
    idx = np.zeros((B, n, 3), np.int32)
    idx[0, :, 0] = 2
    idx[0, :, 1] = np.array([0, 1, 3, 4])[rng.randint(0, 4, size=n)]
    idx[0, :, 2] = np.array([5, 6])[rng.randint(0, 2, size=n)]
    for b in range(1, B):
        idx[b] = rng.randint(0, m - 1, size=(n, 3))
    return g, idx, w


def assert_exact_scatter(s, unit):
    """the precondition of an exact case: at most EXACT_TERMS terms per destination and every possible partial sum a multiple
    of `unit` below 2^24 units -> representable in fp32 whatever the order"""
    assert s.cnt.max() <= EXACT_TERMS, s.cnt.max()
    assert np.array_equal(np.round(s.ref / unit), s.ref / unit) and np.array_equal(np.round(s.abs / unit), s.abs / unit)
    assert s.abs.max() / unit < 2.0 ** 24, s.abs.max() / unit
    return float(s.abs.max() / unit)


# ==== BoxCloud ================================================================================================================================
SX = np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float64)        # Box.corners: x = l / 2 * SX, y = w / 2 * SY, z = h / 2 * SZ
SY = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64)
SZ = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64)


def _d(x):
    """the operand as it is, in fp64 (the GPU file hands over the float32 arrays the kernel gets; the reference's fixture is fp64)"""
    return np.asarray(x).astype(np.float64)


def landmarks(center, wlh, rot, wlh_factor=1.0, swap_wl=False):
    """center (B, 3), wlh (B, 3) = width, length, height, rot (B, 3, 3) -> (B, 9, 3) fp64: centre, corners 0..7"""
    c = _d(center).reshape(-1, 3)
    s = _d(wlh).reshape(-1, 3) * float(F32(wlh_factor))
    R = _d(rot).reshape(-1, 3, 3)
    w, l, h = (s[:, 1], s[:, 0], s[:, 2]) if swap_wl else (s[:, 0], s[:, 1], s[:, 2])
    local = np.stack([l[:, None] / 2 * SX, w[:, None] / 2 * SY, h[:, None] / 2 * SZ], axis=1)      # (B, 3, 8)
    corners = np.einsum("bij,bjk->bik", R, local) + c[:, :, None]                                    # (B, 3, 8)
    return np.concatenate([c[:, None, :], corners.transpose(0, 2, 1)], axis=1)


def boxcloud(points, center, wlh, rot, wlh_factor=1.0, swap_wl=False):
    """points (B, N, 3) -> (B, N, 9) fp64 distances to [centre, corner 0..7]"""
    p = _d(points)
    lm = landmarks(center, wlh, rot, wlh_factor, swap_wl)
    d = p[:, :, None, :] - lm[:, None, :, :]
    return np.sqrt((d * d).sum(-1))


def boxcloud_bound(points, center, wlh, rot, wlh_factor=1.0):
    """|kernel - boxcloud()| <=, per element (B, N, 9).  Following csrc/boxcloud.hip with g_k = gamma(k):
      s' = fl(s * factor), halved and signed exactly: each local coordinate carries 1 rounding;
      corner coordinate  ((R0 x + R1 y) + R2 z) + c : a product term passes its own rounding, the multiply's and 3 adds -> g_5,
        the centre the last add only -> g_1:   eL = g_5 (|R0 x| + |R1 y| + |R2 z|) + g_1 |c|;   the centre landmark is exact;
      d' = fl(p - L'):                          eD = eL + u (|p - L| + eL);
      q' = (dx'^2 + dy'^2) + dz'^2, each square through its multiply and 2 adds -> g_3:
                                                eQ = sum_i [(2 |d_i| eD_i + eD_i^2)(1 + g_3) + g_3 d_i^2];
      |sqrt q' - sqrt q| <= min(eQ / sqrt q, sqrt eQ);  the square root rounds once: e = eS + u (sqrt q + eS)."""
    p = _d(points)
    c = _d(center).reshape(-1, 3)
    s = _d(wlh).reshape(-1, 3) * float(F32(wlh_factor))
    R = np.abs(_d(rot).reshape(-1, 3, 3))
    half = np.stack([s[:, 1], s[:, 0], s[:, 2]], axis=1) / 2                                     # |x|, |y|, |z| of every corner
    eL_corner = gamma(5) * np.einsum("bij,bj->bi", R, half) + gamma(1) * np.abs(c)               # (B, 3), the same for all 8
    eL = np.concatenate([np.zeros_like(eL_corner)[:, None, :], np.repeat(eL_corner[:, None, :], 8, axis=1)], axis=1)   # (B, 9, 3)
    lm = landmarks(center, wlh, rot, wlh_factor)
    d = np.abs(p[:, :, None, :] - lm[:, None, :, :])                                             # (B, N, 9, 3)
    eD = eL[:, None] + U * (d + eL[:, None])
    g3 = gamma(3)
    eQ = ((2 * d * eD + eD * eD) * (1 + g3) + g3 * d * d).sum(-1)
    q = (d * d).sum(-1)
    rq = np.sqrt(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        eS = np.where(q > 0, np.minimum(eQ / np.where(q > 0, rq, 1.0), np.sqrt(eQ)), np.sqrt(eQ))
    return eS + U * (rq + eS)


def boxcloud_f32(points, center, wlh, rot, wlh_factor=1.0):
    """the kernel's formula evaluated in float32, operation by operation, without contraction (numpy never contracts)"""
    p = np.asarray(points, F32)
    c = np.asarray(center, F32).reshape(-1, 3)
    s = np.asarray(wlh, F32).reshape(-1, 3) * F32(wlh_factor)
    R = np.asarray(rot, F32).reshape(-1, 3, 3)
    x = (F32(0.5) * s[:, 1])[:, None] * SX.astype(F32)
    y = (F32(0.5) * s[:, 0])[:, None] * SY.astype(F32)
    z = (F32(0.5) * s[:, 2])[:, None] * SZ.astype(F32)
    lm = np.zeros((len(c), 9, 3), F32)
    lm[:, 0] = c
    for i in range(3):
        lm[:, 1:, i] = ((R[:, i, 0:1] * x + R[:, i, 1:2] * y) + R[:, i, 2:3] * z) + c[:, i:i + 1]
    d = p[:, :, None, :] - lm[:, None, :, :]
    assert d.dtype == F32
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


QUADS = ((1, 2, 2, 3), (2, 3, 6, 7), (1, 4, 8, 9), (4, 4, 7, 9))        # x^2 + y^2 + z^2 = r^2
AXIS_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def signed_permutation(order, signs):
    R = np.zeros((3, 3), F32)
    for i in range(3):
        R[i, order[i]] = signs[i]
    return R


def exact_boxcloud_case(case):
    """One box per axis order (B = 6): a signed permutation matrix, centre and sizes dyadic, wlh_factor a power of two.  For
    every landmark k and every quadruple there are points  landmark_k + 2^e * (+-x, +-y, +-z)  (components permuted, signs and
    e varied), so that channel k of such a point is exactly 2^e r.  -> dict with the inputs, `want` (B, N) the exact distance
    and `chan` (N,) the channel that holds it.
    (A point whose difference to all nine landmarks at once is such a quadruple does not exist for integer half-sizes up to 12
    and offsets up to 28 -- an exhaustive search; so each point pins one landmark by equality, and its other eight channels are
    held to the rounded bound.)"""
    rng = np.random.RandomState(900 + case)
    factor = (1.0, 2.0, 0.5)[case % 3]
    B = 6
    rot = np.stack([signed_permutation(AXIS_ORDERS[(b + case) % 6], [(-1.0) ** ((b + case) >> i) for i in range(3)]) for b in range(B)])
    center = (rng.randint(-1024, 1025, size=(B, 3)) / 16.0).astype(F32)
    wlh = (rng.randint(1, 65, size=(B, 3)) / 8.0).astype(F32)
    lm = landmarks(center, wlh, rot, factor)                              # exact: dyadic throughout
    pts, chan, want = [], [], []
    perms = AXIS_ORDERS
    n = 0
    for k in range(9):
        for qi, (x, y, z, r) in enumerate(QUADS):
            for rep in range(2):
                perm = perms[(k + qi + rep * 3 + case) % 6]
                sg = np.array([(-1.0) ** ((n >> i) & 1) for i in range(3)])
                e = (n % 5) - 3                                           # 2^-3 .. 2^1
                v = np.array([x, y, z], np.float64)[list(perm)] * sg * 2.0 ** e
                pts.append(lm[:, k, :] + v[None, :])
                chan.append(k)
                want.append(r * 2.0 ** e)
                n += 1
    points = np.stack(pts, axis=1)                                        # (B, N, 3)
    assert np.array_equal(points.astype(F32).astype(np.float64), points)
    return dict(points=points.astype(F32), center=center, wlh=wlh, rot=rot, factor=factor, chan=np.array(chan),
                want=np.repeat(np.array(want)[None, :], B, axis=0))


def rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def rounded_boxcloud_case(B, N, seed):
    """general rotations, centres 400 .. 2000 m from the origin (box 0 near it), points within a few metres of the box"""
    rng = np.random.RandomState(seed)
    rot = np.stack([rotation(*rng.uniform(-np.pi, np.pi, 3)) for _ in range(B)]).astype(F32)
    dirs = rng.randn(B, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dist = np.array([1.0, 400.0, 2000.0, 1200.0])[np.arange(B) % 4]
    center = (dirs * dist[:, None]).astype(F32)
    wlh = rng.uniform(0.5, 5.0, size=(B, 3)).astype(F32)
    points = (center[:, None, :].astype(np.float64) + rng.randn(B, N, 3) * 2.0).astype(F32)
    if N > 1:
        points[:, 0] = center                                             # a point on the centre itself: channel 0 is 0
    return dict(points=points, center=center, wlh=wlh, rot=rot, factor=(1.25, 0.9, 1.5)[seed % 3])
