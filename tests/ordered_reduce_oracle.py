"""Plain numpy restatement of the ORDERED layer-0 list sums (o3d_group_reduce_gather_ordered, deterministic mode), written from
the order stated in include/o3dsot.h.  It imports compact_oracle (layouts, families) and nothing of the package under test.

  ordered_index(L)      the sorted index the entry must leave in `perm` / `poff`
  ordered_sums(L, dY)   S and T in float32 arithmetic, addition by addition in the stated order: what the kernel must give
                        BIT FOR BIT (tests/test_ordered_reduce_gpu.py), and what equals compact_oracle.reduce_sums exactly on
                        dyadic inputs (tests/test_ordered_reduce_oracle_cpu.py)

New index families (compact_oracle.py keeps its own): the smallest at which the fold can go wrong
  chunkcut    every cloud has more than RG_CH live columns and a point in every ball: its list is cut by the chunk boundary
  hubrun      one point in each of 640 balls of one chunk: its run spans many whole thread shares (shares of <= 8 entries)
  misaligned  two segments, segment 1's clouds longer than a chunk and its second cloud starting at a column that is no
              multiple of 4 (q0 != q0a): the chunk boundaries are not where a q0-based split would put them
"""
import numpy as np

import compact_oracle as O

RG_CH = 2048
THREADS = 256
NEW_FAMILIES = ["chunkcut", "hubrun", "misaligned"]
_FAM, _LAY = {}, {}


def family(name):
    if name not in NEW_FAMILIES:
        return O.family(name)
    if name in _FAM:
        return _FAM[name]
    rng = np.random.RandomState({"chunkcut": 21, "hubrun": 22, "misaligned": 23}[name])
    if name == "chunkcut":
        B, npoint, ns, N, ld = 2, 128, 32, 100, 128
        counts = rng.randint(20, ns + 1, B * npoint)
        segs = [(O._idx_from_counts(rng, counts, B, npoint, ns, N, hub=O.HUB), N, ld)]
    elif name == "hubrun":
        B, npoint, ns, N, ld = 2, 640, 4, 100, 128
        counts = rng.randint(2, 4, B * npoint)
        segs = [(O._idx_from_counts(rng, counts, B, npoint, ns, N, hub=O.HUB), N, ld)]
    else:
        B, ns = 2, 16
        c0 = rng.randint(1, 3, B * 64)
        c1 = rng.randint(9, ns + 1, B * 192)
        if c1[:192].sum() % 4 == 0:          # cloud 1 of segment 1 starts at start1 + this sum: keep it off the float4 grid
            c1[0] += 1 if c1[0] < ns else -1
        segs = [(O._idx_from_counts(rng, c0, B, 64, ns, 100), 100, 128),
                (O._idx_from_counts(rng, c1, B, 192, ns, 200, hub=O.HUB), 200, 256)]
    _FAM[name] = dict(segs=segs, ns=ns, B=B)
    return _FAM[name]


def family_layout(name):
    if name not in NEW_FAMILIES:
        return O.family_layout(name)
    if name not in _LAY:
        _LAY[name] = O.Layout([(idx, ld) for idx, _, ld in family(name)["segs"]])
    return _LAY[name]


def nchunk_of(L):
    return (max(L.npoint) * L.ns + 4 + RG_CH - 1) // RG_CH


def clouds(L):
    """-> [(cloud, pbase, bbase, npoint, ld, q0, q1, q0a)] in launch order (segment 1's clouds after segment 0's)"""
    out = []
    for s in range(L.nseg):
        for b in range(L.B):
            npoint, ld = L.npoint[s], L.ld[s]
            bbase = L.ball_base[s] + b * npoint
            q0 = int(L.ball_off[bbase])
            q1 = int(L.ball_off[bbase + npoint - 1] + L.ball_cnt[bbase + npoint - 1])
            out.append((s * L.B + b, L.pt_base[s] + b * ld, bbase, npoint, ld, q0, q1, q0 & ~3))
    return out


def cloud_chunks(L, cl):
    """chunks of one cloud, ascending -> [(k, lo, hi, points n, absolute columns q)]: the chunk's entries sorted by (point, column)"""
    _, pbase, _, _, _, q0, q1, q0a = cl
    out = []
    k, lo = 0, q0a
    while lo < q1:
        hi = min(lo + RG_CH, q1)
        q = np.arange(max(lo, q0), hi)
        n = L.gp[q] - pbase
        order = np.lexsort((q, n))
        out.append((k, lo, hi, n[order], q[order]))
        k, lo = k + 1, lo + RG_CH
    return out


def ordered_index(L):
    """-> perm (ldp; O.FILL_I where the entry writes nothing), poff (clouds, nchunk*max(ld) + 1; O.FILL_I beyond a cloud's own
    nchunk*ld + 1 entries)"""
    nchunk = nchunk_of(L)
    stride = nchunk * max(L.ld) + 1
    cls = clouds(L)
    perm = np.full(L.ldp, O.FILL_I, np.int64)
    poff = np.full((len(cls), stride), O.FILL_I, np.int64)
    for cl in cls:
        c, _, _, _, ld, q0, q1, q0a = cl
        cnt = np.zeros(nchunk * ld + 1, np.int64)
        pos = 0
        for k, lo, _, n, q in cloud_chunks(L, cl):
            perm[q0 + pos:q0 + pos + len(q)] = (n << 16) | (q - q0a - k * RG_CH)
            np.add.at(cnt, k * ld + n, 1)
            pos += len(q)
        assert pos == q1 - q0
        poff[c, :nchunk * ld + 1] = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return perm, poff


def ordered_sums(L, dY):
    """dY (C, len(L.real)) on the real columns, taken as float32 -> S (C, ldz), T (C, nballs) float32, every addition a float32
    addition in the order of include/o3dsot.h"""
    f32 = np.float32
    C = dY.shape[0]
    full = np.zeros((C, L.ldp), f32)
    full[:, L.real] = np.asarray(dY).astype(f32)
    S, T = np.zeros((C, L.ldz), f32), np.zeros((C, L.nballs), f32)
    for cl in clouds(L):
        _, pbase, bbase, npoint, _, _, _, _ = cl
        for _, lo, hi, n, q in cloud_chunks(L, cl):
            cnt = len(q)
            per = -(-cnt // THREADS)
            cols = full[:, q].T.copy()                 # (entries, C)
            a = 0
            while a < cnt:
                b = a
                while b < cnt and n[b] == n[a]:
                    b += 1
                total, p = None, a
                while p < b:                           # pieces: cut at the multiples of per
                    pe = min(b, (p // per + 1) * per)
                    piece = np.zeros(C, f32)
                    for e in range(p, pe):
                        piece = piece + cols[e]
                    total = piece if total is None else total + piece
                    p = pe
                S[:, pbase + n[a]] = S[:, pbase + n[a]] + total
                a = b
            for j in range(npoint):                    # the ball's columns inside the chunk, ascending
                b0 = int(L.ball_off[bbase + j])
                s0, s1 = max(b0, lo), min(b0 + int(L.ball_cnt[bbase + j]), hi)
                if s0 >= s1:
                    continue
                t = np.zeros(C, f32)
                for c in range(s0, s1):
                    t = t + full[:, c]
                T[:, bbase + j] = T[:, bbase + j] + t
    return S, T
