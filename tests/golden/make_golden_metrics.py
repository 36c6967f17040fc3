"""Generate tests/golden/ref_metrics.npz by running the REFERENCE'S OWN metrics code on seeded box pairs.

Run from the repo root, only where /root/reference exists:  python tests/golden/make_golden_metrics.py
Reference code executed (read-only, from /root/reference): utils/metrics.py (estimateOverlap, estimateAccuracy, fromBoxToPoly,
TorchSuccess, TorchPrecision) and datasets/data_classes.py (Box.corners / bottom_corners).  Stand-ins, because the packages
are absent here: shapely -> tests/golden/shapely_standin.py (convex polygons by vertex enumeration, a different algorithm from
the kernel's clip), torchmetrics -> tests/golden/torchmetrics_standin.py, pyquaternion -> tests/golden/quat_standin.py.  What
the fixture pins is therefore the reference's metrics code over these stand-ins, not shapely's own output.

The pair table (`a`, `b` (n,15) float32; PER_CLASS pairs of each class, `cls` (n,) the class index into CLASSES):
  tracking    small offsets and yaw differences, the same wlh                     unrelated   any wlh / yaw, offsets of metres
  equal_yaw   the same rotation (collinear edges)                                 same_centre the same centre and wlh, the rotation
  identical   b = a                                                                           times an EXACT 0 / 90 / 180 degree turn
  inside      b well inside a                                                     no_height   footprints overlap, heights do not
  height_rule the reference's height rule (centre down by h) differs from the true 3-D IoU by more than 1e-2 (asserted)
  tilted      a few degrees of pitch and roll on both boxes                       camera      camera-frame boxes (up = -y), turned
                                                                                              about y
`up` (n,) = the index of the non-zero component of the pair's up_axis: 2 = (0,0,1), 1 = (0,-1,0).  The last CAMERA_PER_CLASS
pairs of every class are drawn z-up like the others and then moved to the camera frame by the exact turn (x, y, z) -> (x, -z, y)
of centres and rotations; the `camera` class is drawn there.  (A z-up box has no footprint under up_axis (0,-1,0): the reference
divides by a zero union area.)  Every pair is scored for dim 2 and 3 under its own up_axis: `overlap.<dim>`, `distance.<dim>`
(n,) float64.  The boxes given to the reference carry the float32 matrix itself as their
orientation (`.rotation_matrix` returns it widened to double): the reference projects whatever matrix its Box holds, and the
kernel reads the same 9 numbers.  (A quaternion round trip would orthonormalise the float32 matrix, a change of ~6e-8.)

Conditions ASSERTED (a pair that violates one is redrawn, the number of redraws is printed), so that the fp32 rounding of a
result cannot move it across a threshold of the 21-point Success / Precision curves:
  * every overlap is exactly 0, exactly 1.0, or more than 1e-6 from every threshold of linspace(0, 1, 21);
  * every distance is exactly 0 or more than 1e-6 from every threshold of linspace(0, 2, 21).
EXEMPT from the first: pairs with the same footprint (identical, same_centre with a 0 / 180 degree turn), whose reference
overlap is 1 +- O(1e-16) rather than exactly 1.0 in places (and 1 + O(1e-7) for dim 3, where the footprint of a
float32 rotation matrix is not exactly w l while the volume is w l h).  They stay in the table; `in_success` (n,) marks the pairs the
Success / Precision subsets are drawn from (the non-exempt ones, and the exempt ones that are exactly 1.0 everywhere).

`sp.<dim>.<name>` (2,) float32 = TorchSuccess.compute(), TorchPrecision.compute() of the reference over the rows
`subset.<name>` for name in s1 (1 row), s65, s1000, and `two` = s65 and s1000 given in two update() calls.

`track.<case>.overlaps / .distances` (8,) float64 for each case of tests/tracking_oracle.py::CASES: the reference's scores
(IoU_space 3, up_axis (0,0,1)) of the result boxes stored in tests/golden/ref_tracking.npz against the ground truth of
synth.make_sequence(seq_seed); boxes through Quaternion(matrix=...) as in make_golden_tracking.py.  No tracking run is made.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_io  # noqa: E402
import quat_standin  # noqa: E402
import shapely_standin  # noqa: E402
import torchmetrics_standin  # noqa: E402
import tracking_oracle as TO  # noqa: E402
from open3dsot_amd import synth  # noqa: E402


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


stub("pyquaternion", Quaternion=quat_standin.Quaternion)
stub("shapely"); stub("shapely.geometry", Polygon=shapely_standin.Polygon)
stub("torchmetrics", Metric=torchmetrics_standin.Metric, utilities=torchmetrics_standin.utilities)
sys.modules["torchmetrics.utilities"] = torchmetrics_standin.utilities
sys.modules["torchmetrics.utilities.data"] = torchmetrics_standin.utilities.data
DC = load("datasets.data_classes", "datasets/data_classes.py")
M = load("utils.metrics", "utils/metrics.py")

CLASSES = ("tracking", "unrelated", "equal_yaw", "same_centre", "identical", "inside", "no_height", "height_rule", "tilted",
           "camera")
PER_CLASS, CAMERA_PER_CLASS = 200, 60
DIMS = (2, 3)
TO_CAMERA = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])       # (x, y, z) -> (x, -z, y): z-up becomes (0,-1,0)-up, exactly
UP_AXIS = {1: (0, -1, 0), 2: (0, 0, 1)}
THR_S = torch.linspace(0, 1, steps=21).double().numpy()
THR_P = torch.linspace(0, 2, steps=21).double().numpy()


class MatrixOrientation:
    """an orientation whose rotation_matrix is the given matrix itself"""

    def __init__(self, m):
        self.rotation_matrix = np.asarray(m, np.float64).reshape(3, 3).copy()


def box_of(b15, quaternion=False):
    b = np.asarray(b15, np.float64)
    o = quat_standin.Quaternion(matrix=b[6:15].reshape(3, 3)) if quaternion else MatrixOrientation(b[6:15])
    return DC.Box(b[0:3], b[3:6], o)


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]),
            "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


QUARTER = {0: np.eye(3), 1: np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), 2: np.array([[-1, 0, 0], [0, -1, 0], [0, 0, 1.0]])}


def vec(c, wlh, R):
    return np.concatenate([c, wlh, np.asarray(R).reshape(-1)]).astype(np.float32)


def draw(cls, rng):
    """-> (a, b, exempt): one pair of class `cls`, float32 15-vectors"""
    wlh = np.array([1.6, 3.9, 1.5]) * rng.uniform(0.8, 1.2, 3)
    c = np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-2, 0)])
    yaw = rng.uniform(-np.pi, np.pi)
    R = rot("z", yaw)
    exempt = False
    small = np.array([rng.normal(0, 0.3), rng.normal(0, 0.3), rng.normal(0, 0.1)])
    if cls == "tracking":
        b = vec(c + small, wlh, rot("z", yaw + rng.normal(0, 0.1)))
    elif cls == "unrelated":
        b = vec(c + rng.normal(0, 2.5, 3) * [1, 1, 0.3], np.array([1.6, 3.9, 1.5]) * rng.uniform(0.5, 1.5, 3),
                rot("z", rng.uniform(-np.pi, np.pi)))
    elif cls == "equal_yaw":
        b = vec(c + small, wlh, R)
    elif cls == "same_centre":
        k = int(rng.integers(0, 3))
        a = vec(c, wlh, R)
        b = a.copy()
        b[6:15] = (a[6:15].reshape(3, 3) @ QUARTER[k].astype(np.float32)).reshape(-1)      # exact: signs and places only
        return a, b, k != 1
    elif cls == "identical":
        a = vec(c, wlh, R)
        return a, a.copy(), True
    elif cls == "inside":
        b = vec(c + small * 0.2, wlh * rng.uniform(0.3, 0.6, 3), rot("z", yaw + rng.normal(0, 0.3)))
    elif cls == "no_height":
        dz = (wlh[2] + rng.uniform(0.1, 1.0)) * rng.choice([-1.0, 1.0])
        b = vec(c + [small[0], small[1], dz], wlh, rot("z", yaw + rng.normal(0, 0.1)))
    elif cls == "height_rule":
        hb = wlh[2] * rng.uniform(0.4, 0.7)
        dz = wlh[2] * rng.uniform(0.3, 0.5) * rng.choice([-1.0, 1.0])
        b = vec(c + [small[0], small[1], dz], [wlh[0], wlh[1], hb], rot("z", yaw + rng.normal(0, 0.1)))
    elif cls == "tilted":
        def tilt():
            return rot("y", np.deg2rad(rng.uniform(-5, 5))) @ rot("x", np.deg2rad(rng.uniform(-5, 5)))
        R = R @ tilt()
        b = vec(c + small, wlh, rot("z", yaw + rng.normal(0, 0.1)) @ tilt())
    elif cls == "camera":
        up = rot("x", np.pi / 2)                               # the box's height axis -> -y
        c = np.array([c[0], -c[2], abs(c[1]) + 5.0])
        R = rot("y", yaw) @ up
        b = vec(c + [small[0], small[2], small[1]], wlh, rot("y", yaw + rng.normal(0, 0.1)) @ up)
    else:
        raise KeyError(cls)
    return vec(c, wlh, R), b, exempt


def reference_scores(a, b, up):
    """the reference's estimateOverlap / estimateAccuracy of one pair for dim 2 and 3 -> {dim: (overlap, distance)}"""
    A, B = box_of(a), box_of(b)
    return {dim: (float(M.estimateOverlap(A, B, dim=dim, up_axis=UP_AXIS[up])),
                  float(M.estimateAccuracy(A, B, dim=dim, up_axis=UP_AXIS[up]))) for dim in DIMS}


def to_camera(b15):
    out = b15.copy()
    G = TO_CAMERA.astype(np.float32)
    out[0:3] = G @ b15[0:3]
    out[6:15] = (G @ b15[6:15].reshape(3, 3)).reshape(-1)
    return out


def clear_of(x, thr):
    return float(np.abs(x - thr).min()) > 1e-6


def overlap_ok(o):
    return o == 0.0 or o == 1.0 or clear_of(o, THR_S)


def distance_ok(d):
    return d == 0.0 or clear_of(d, THR_P)


def true_iou3(a, b, s):
    """the 3-D IoU with the height interval centred on the box (what the reference's rule is NOT), from the reference's own
    footprint intersection, recovered from its dim-2 overlap: inter = o2 (areaA + areaB) / (1 + o2) for yaw-only boxes"""
    o2 = s[2][0]
    inter = o2 * (a[3] * a[4] + b[3] * b[4]) / (1 + o2)
    top, bottom = min(a[2] + a[5] / 2, b[2] + b[5] / 2), max(a[2] - a[5] / 2, b[2] - b[5] / 2)
    iv = inter * max(0.0, top - bottom)
    return iv / (a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - iv)


def pair_table():
    rng = np.random.default_rng(20240607)
    A, B, cls, ups, ok_s, scores, redrawn = [], [], [], [], [], {dim: ([], []) for dim in DIMS}, 0
    for ci, name in enumerate(CLASSES):
        for i in range(PER_CLASS):
            while True:
                a, b, exempt = draw(name, rng)
                up = 1 if name == "camera" else 2
                s = reference_scores(a, b, up)
                good = True
                if name == "height_rule":
                    good = abs(s[3][0] - true_iou3(a.astype(np.float64), b.astype(np.float64), s)) > 1e-2
                if name == "no_height":
                    good = s[2][0] > 0 and s[3][0] == 0.0
                if up == 2 and i >= PER_CLASS - CAMERA_PER_CLASS:
                    a, b, up = to_camera(a), to_camera(b), 1
                    s = reference_scores(a, b, up)
                good = good and all(distance_ok(d) for _, d in s.values()) and (exempt or all(overlap_ok(o) for o, _ in s.values()))
                if good:
                    break
                redrawn += 1
            A.append(a); B.append(b); cls.append(ci); ups.append(up)
            ok_s.append(all(overlap_ok(o) for o, _ in s.values()))
            for dim in DIMS:
                scores[dim][0].append(s[dim][0]); scores[dim][1].append(s[dim][1])
    print("pair table: %d pairs (%d camera-frame), %d redrawn, %d outside the Success subsets" %
          (len(A), sum(u == 1 for u in ups), redrawn, len(A) - sum(ok_s)))
    out = {"a": np.stack(A), "b": np.stack(B), "cls": np.array(cls, np.int32), "up": np.array(ups, np.int32),
           "in_success": np.array(ok_s, bool)}
    for dim, (o, d) in scores.items():
        out["overlap.%d" % dim], out["distance.%d" % dim] = np.array(o, np.float64), np.array(d, np.float64)
    # the asserted conditions, on what is stored
    for dim in DIMS:
        o, d = out["overlap.%d" % dim], out["distance.%d" % dim]
        assert all(distance_ok(x) for x in d)
        assert all(overlap_ok(x) for x in o[out["in_success"]])
        assert np.all(np.isfinite(o)) and np.all((o >= 0) & (o <= 1.0 + 1e-6))
    return out


def curves(out):
    rng = np.random.default_rng(7)
    pool = np.flatnonzero(out["in_success"])
    subsets = {"s1": rng.choice(pool, 1, replace=False), "s65": rng.choice(pool, 65, replace=False),
               "s1000": rng.choice(pool, 1000, replace=False)}
    res = {"subset." + k: v.astype(np.int64) for k, v in subsets.items()}
    for dim in DIMS:
        o, d = out["overlap.%d" % dim], out["distance.%d" % dim]

        def run(parts):
            S, P = M.TorchSuccess(), M.TorchPrecision()
            for rows in parts:
                # as validation_step does: torch.tensor over the list that evaluate_one_sequence returns
                S(torch.tensor([np.float64(x) for x in o[rows]]))
                P(torch.tensor([np.float64(x) for x in d[rows]]))
            return np.array([float(S.compute()), float(P.compute())], np.float32)
        for k, rows in subsets.items():
            res["sp.%d.%s" % (dim, k)] = run([rows])
        res["sp.%d.two" % dim] = run([subsets["s65"], subsets["s1000"]])
    S, P = M.TorchSuccess(), M.TorchPrecision()
    assert S.compute() == 0 and P.compute() == 0                 # the empty metric
    return res


def tracking_scores():
    res = {}
    with fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_tracking.npz")) as z:
        for case in TO.CASES:
            _, cfg = TO.case_config(case)
            _, gt = synth.make_sequence(int(z[case + ".seq_seed"]), TO.SEQ_FRAMES, TO.SEQ_POINTS)
            o, d = [], []
            for t in range(TO.SEQ_FRAMES):
                A = box_of(gt[t], quaternion=True)
                B = A if t == 0 else box_of(z["%s.f%d.result_box" % (case, t)], quaternion=True)
                o.append(float(M.estimateOverlap(A, B, dim=cfg["IoU_space"], up_axis=cfg["up_axis"])))
                d.append(float(M.estimateAccuracy(A, B, dim=cfg["IoU_space"], up_axis=cfg["up_axis"])))
            res["track.%s.overlaps" % case], res["track.%s.distances" % case] = np.array(o), np.array(d)
            print("%s: overlaps %s" % (case, np.round(o, 4)))
    return res


def main():
    out = pair_table()
    out.update(curves(out))
    out.update(tracking_scores())
    written = fixture_io.save(os.path.join(ROOT, "tests", "golden", "ref_metrics.npz"), **out)
    print("wrote", [os.path.basename(p) for p in written], len(out), "arrays")


if __name__ == "__main__":
    main()
