"""A small stand-in for shapely.geometry.Polygon for the metrics fixture generator (TEST ONLY): shapely is not installed where
the fixtures are made, and the reference's utils/metrics.py needs only this much of it -- Polygon(points) of a CONVEX polygon,
`.intersection(other)`, `.union(other)` and `.area`, in float64.  Only the first two coordinates of a point are read (the
reference hands bottom_corners' 3-D points over; shapely's area ignores z as well).

The intersection is found by VERTEX ENUMERATION, on purpose a different algorithm from the kernel's Sutherland-Hodgman clip
(open3dsot_amd/csrc/metrics.hip):
  * the vertices of each polygon that lie inside the other (signed distance to every edge line, scaled by the edge length,
    >= -1e-9),
  * the crossing points of every edge of one with every edge of the other (both line parameters within [-1e-12, 1 + 1e-12];
    parallel edges have none),
  * sorted by angle about their centroid; the shoelace area of that ring.
Without the two tolerances the enumeration loses coincident corners and shared edges (a corner exactly on an edge tests
-1e-17 "outside"); with them duplicates appear, which add zero area.  `union.area` is areaA + areaB - intersection.
What the fixture pins is therefore the reference's own metrics code over this stand-in, not shapely itself."""
import numpy as np

INSIDE_TOL = 1e-9
PARAM_TOL = 1e-12


def _shoelace(p):
    if len(p) < 3:
        return 0.0
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def _inside(ring, v):
    """ring counter-clockwise (n,2): v within INSIDE_TOL of the inside of every edge"""
    p, q = ring, np.roll(ring, -1, 0)
    e = q - p
    cross = e[:, 0] * (v[1] - p[:, 1]) - e[:, 1] * (v[0] - p[:, 0])
    return bool(np.all(cross >= -INSIDE_TOL * np.maximum(np.hypot(e[:, 0], e[:, 1]), 1e-300)))


class _Area:
    def __init__(self, area):
        self.area = float(area)


class Polygon:
    def __init__(self, points):
        p = np.array([[float(c[0]), float(c[1])] for c in points], np.float64)
        if len(p) > 1 and np.array_equal(p[0], p[-1]):
            p = p[:-1]
        signed = _shoelace(p)
        self.ring = p if signed >= 0 else p[::-1].copy()           # counter-clockwise
        self.area = abs(signed)

    def intersection(self, other):
        A, B = self.ring, other.ring
        if len(A) < 3 or len(B) < 3:
            return _Area(0.0)
        pts = [v for v in A if _inside(B, v)] + [v for v in B if _inside(A, v)]
        for i in range(len(A)):
            a0, r = A[i], A[(i + 1) % len(A)] - A[i]
            for j in range(len(B)):
                b0, s = B[j], B[(j + 1) % len(B)] - B[j]
                den = r[0] * s[1] - r[1] * s[0]
                if den == 0:
                    continue
                t = ((b0[0] - a0[0]) * s[1] - (b0[1] - a0[1]) * s[0]) / den
                u = ((b0[0] - a0[0]) * r[1] - (b0[1] - a0[1]) * r[0]) / den
                if -PARAM_TOL <= t <= 1 + PARAM_TOL and -PARAM_TOL <= u <= 1 + PARAM_TOL:
                    pts.append(a0 + t * r)
        if len(pts) < 3:
            return _Area(0.0)
        pts = np.array(pts)
        c = pts.mean(0)
        order = np.argsort(np.arctan2(pts[:, 1] - c[1], pts[:, 0] - c[0]), kind="stable")
        return _Area(abs(_shoelace(pts[order])))

    def union(self, other):
        return _Area(self.area + other.area - self.intersection(other).area)
