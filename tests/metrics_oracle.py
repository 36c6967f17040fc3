"""fp64 restatement of o3d_track_score (open3dsot_amd/csrc/metrics.hip) in the kernel's stated operation order: every
operation below is ONE IEEE fp64 operation on the fp32 inputs widened to double, in the order of the parentheses written at
the head of metrics.hip (Python floats: no fused multiply-add).  The CPU tests compare this against the reference's own
utils/metrics.py (tests/golden/ref_metrics.npz, a different algorithm for the intersection); the GPU tests use it where the
fixture does not reach.  Test infrastructure only -- the product has no CPU path."""
import math

import numpy as np

_SX = (1.0, 1.0, -1.0, -1.0)
_SY2 = (-1.0, 1.0, 1.0, -1.0)       # up = 2: corners [2,3,7,6] of Box.corners; up = 1 ([0,1,5,4]) has them negated


def up_index(up_axis):
    """the index of the non-zero component of up_axis; the reference supports (0,-1,0) and (0,0,1)"""
    u = [i for i, c in enumerate(up_axis) if c != 0]
    if u not in ([1], [2]):
        raise ValueError("up_axis %r" % (up_axis,))
    return u[0]


def footprint(box, up):
    b = [float(x) for x in np.asarray(box, np.float32).reshape(15)]
    v = 1 if up == 2 else 2
    hl, hw, hh = b[4] * 0.5, b[3] * 0.5, b[5] * 0.5
    flip = 1.0 if up == 2 else -1.0
    z = -flip * hh
    out = []
    for k in range(4):
        x, y = _SX[k] * hl, flip * _SY2[k] * hw
        out.append((b[0] + ((b[6] * x + b[7] * y) + b[8] * z), b[v] + ((b[6 + 3 * v] * x + b[7 + 3 * v] * y) + b[8 + 3 * v] * z)))
    return out


def signed_area2(p):
    s, m = 0.0, len(p)
    for j in range(m):
        xn, yn = p[(j + 1) % m]
        s = s + (p[j][0] * yn - p[j][1] * xn)
    return s


def clip(poly, P, Q):
    ex, ey = Q[0] - P[0], Q[1] - P[1]
    d = [ex * (y - P[1]) - ey * (x - P[0]) for x, y in poly]
    out, m = [], len(poly)
    for j in range(m):
        k = (j + 1) % m
        if d[j] >= 0.0:
            out.append(poly[j])
        if (d[j] >= 0.0) != (d[k] >= 0.0):
            t = d[j] / (d[j] - d[k])
            out.append((poly[j][0] + t * (poly[k][0] - poly[j][0]), poly[j][1] + t * (poly[k][1] - poly[j][1])))
    return out


def score_pair(a, b, dim=3, up=2):
    """-> (overlap, distance) as Python floats, before the kernel's one rounding to fp32"""
    A, B = footprint(a, up), footprint(b, up)
    sa, sb = signed_area2(A), signed_area2(B)
    if sb < 0.0:
        B = [B[0], B[3], B[2], B[1]]
    poly = A
    for e in range(4):
        poly = clip(poly, B[e], B[(e + 1) % 4]) if poly else poly
    inter = 0.5 * abs(signed_area2(poly)) if len(poly) >= 3 else 0.0
    fa, fb = [float(x) for x in np.asarray(a, np.float32).reshape(15)], [float(x) for x in np.asarray(b, np.float32).reshape(15)]
    dx, dy, dz = fa[0] - fb[0], fa[1] - fb[1], fa[2] - fb[2]
    if dim == 2:
        num, den = inter, (0.5 * abs(sa) + 0.5 * abs(sb)) - inter
        dist = abs(dz if up == 2 else dy)
    else:
        top, bottom = min(fa[up], fb[up]), max(fa[up] - fa[5], fb[up] - fb[5])
        num = inter * max(0.0, top - bottom)
        den = ((fa[3] * fa[4]) * fa[5] + (fb[3] * fb[4]) * fb[5]) - num
        dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
    finite = all(math.isfinite(x) for x in fa + fb)
    ov = num / den if finite and den > 0.0 else 0.0
    return (ov if math.isfinite(ov) else 0.0), dist


def score(a, b, dim=3, up=2):
    """a, b (..., 15) -> (overlaps, distances) float64 arrays of the leading shape"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    lead = a.shape[:-1]
    r = [score_pair(x, y, dim, up) for x, y in zip(a.reshape(-1, 15), b.reshape(-1, 15))]
    return (np.array([x[0] for x in r], np.float64).reshape(lead), np.array([x[1] for x in r], np.float64).reshape(lead))
