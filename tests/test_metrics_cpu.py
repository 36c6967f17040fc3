"""Scoring tracked boxes, the parts that need no GPU: the entry point is exported, declared and validates its arguments before
any HIP call; the fp64 restatement of the kernel (tests/metrics_oracle.py, Sutherland-Hodgman) agrees with the reference's own
utils/metrics.py over a vertex-enumeration polygon stand-in (tests/golden/ref_metrics.npz) and with closed forms; the host
arithmetic of SuccessPrecision.compute reproduces the reference's TorchSuccess / TorchPrecision bit for bit."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fixture_io  # noqa: E402
import metrics_oracle as MO  # noqa: E402
from test_capi_symbols import declared_symbols, header_prototypes  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_metrics.npz"))


def box(c, wlh, yaw=0.0):
    cs, sn = math.cos(yaw), math.sin(yaw)
    return np.array(list(c) + list(wlh) + [cs, -sn, 0, sn, cs, 0, 0, 0, 1], np.float32)


def test_symbol_is_exported_declared_and_bound():
    from open3dsot_amd import build, capi, metrics  # noqa: F401  (metrics registers the signature)
    lib = ctypes.CDLL(build.build())
    assert "o3d_track_score" in declared_symbols() and hasattr(lib, "o3d_track_score")
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i"}
    assert [kind[a] for a in capi.SIGNATURES["o3d_track_score"]] == header_prototypes()["o3d_track_score"]
    assert ("metrics.hip", ["-ffp-contract=off"]) in [(s, list(f)) for s, f in build.SOURCES]


def test_bad_arguments_are_refused_before_touching_the_device():
    from open3dsot_amd import capi, metrics  # noqa: F401
    f = capi.load().o3d_track_score
    buf = (ctypes.c_float * 64)()
    cnt = (ctypes.c_int64 * 65)()
    p, c = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(cnt, ctypes.c_void_p)

    def call(a=p, b=p, valid=None, n=1, dim=3, up=2, ov=p, di=p, ts=None, ns=0, tp=None, npr=0, cs=None, cp=None, tot=None):
        return f(a, b, valid, n, dim, up, ov, di, ts, ns, tp, npr, cs, cp, tot, None)
    EINVAL = -1
    assert call(a=None) == EINVAL and call(b=None) == EINVAL                    # NULL boxes
    assert call(n=-1) == EINVAL
    assert [call(dim=d) for d in (0, 1, 4)] == [EINVAL] * 3
    assert [call(up=u) for u in (0, 3, -1)] == [EINVAL] * 3
    assert call(cs=c) == EINVAL and call(cp=c) == EINVAL                        # counters without thresholds
    assert call(cs=c, ts=p, ns=0) == EINVAL and call(cp=c, tp=p, npr=0) == EINVAL
    assert call(cs=c, ts=p, ns=65) == EINVAL and call(cp=c, tp=p, npr=65) == EINVAL   # more than 64 thresholds
    assert call(ts=p, ns=65) == EINVAL
    assert call(n=0) == 0                                                       # nothing to do: no launch
    assert call(n=0, cs=c, ts=p, ns=21, cp=c, tp=p, npr=21, tot=c) == 0
    assert call(n=0, dim=5) == EINVAL                                           # validation comes before the empty case


@pytest.mark.parametrize("dim", [2, 3])
def test_oracle_agrees_with_the_reference_over_a_different_algorithm(gold, dim):
    """both fp64: the clip of the restatement against the vertex enumeration under the reference's code, every pair"""
    a, b, up = gold["a"], gold["b"], gold["up"]
    assert a.shape == (2000, 15) and set(up.tolist()) == {1, 2} and len(set(gold["cls"].tolist())) == 10
    got = np.array([MO.score_pair(a[i], b[i], dim, int(up[i])) for i in range(len(a))])
    d_ov = np.abs(got[:, 0] - gold["overlap.%d" % dim]).max()
    d_di = np.abs(got[:, 1] - gold["distance.%d" % dim]).max()
    print("dim %d: max |oracle - reference| overlap %.2e, distance %.2e" % (dim, d_ov, d_di))
    assert d_ov <= 1e-12 and d_di <= 1e-12


def test_the_fixture_holds_what_it_promises(gold):
    o2, o3, cls = gold["overlap.2"], gold["overlap.3"], gold["cls"]
    names = ("tracking", "unrelated", "equal_yaw", "same_centre", "identical", "inside", "no_height", "height_rule", "tilted", "camera")
    sel = {n: cls == i for i, n in enumerate(names)}
    assert (o2[sel["unrelated"]] == 0).any() and (o2[sel["unrelated"]] > 0).any()           # disjoint ones included
    assert np.all(np.abs(o2[sel["identical"]] - 1) < 1e-6)
    assert np.all(o2[sel["no_height"]] > 0) and np.all(o3[sel["no_height"]] == 0)
    thr_s, thr_p = torch.linspace(0, 1, 21).double().numpy(), torch.linspace(0, 2, 21).double().numpy()
    ok = gold["in_success"]
    assert ok.sum() >= 1000 and not ok[sel["identical"]].all()
    for dim in (2, 3):
        o, d = gold["overlap.%d" % dim][ok], gold["distance.%d" % dim]
        clear = np.abs(o[:, None] - thr_s[None]).min(1) > 1e-6
        assert np.all(clear | (o == 0) | (o == 1))
        assert np.all((np.abs(d[:, None] - thr_p[None]).min(1) > 1e-6) | (d == 0))
    for k in ("s1", "s65", "s1000"):
        assert ok[gold["subset." + k]].all()
    # the height rule class: a kernel with the "corrected" (centred) height interval misses these by more than 1e-2
    a, b = gold["a"].astype(np.float64), gold["b"].astype(np.float64)
    rows = np.flatnonzero(sel["height_rule"] & (gold["up"] == 2))
    inter = o2[rows] * (a[rows, 3] * a[rows, 4] + b[rows, 3] * b[rows, 4]) / (1 + o2[rows])
    top = np.minimum(a[rows, 2] + a[rows, 5] / 2, b[rows, 2] + b[rows, 5] / 2)
    bot = np.maximum(a[rows, 2] - a[rows, 5] / 2, b[rows, 2] - b[rows, 5] / 2)
    iv = inter * np.maximum(0, top - bot)
    true = iv / (a[rows, 3:6].prod(1) + b[rows, 3:6].prod(1) - iv)
    assert len(rows) >= 100 and np.all(np.abs(true - o3[rows]) > 1e-2)


def test_closed_forms():
    a = box((1, 2, 0.5), (1.5, 4.0, 1.6), 0.3)
    for dim in (2, 3):
        ov, di = MO.score_pair(a, a, dim, 2)                                   # identical -> 1
        assert abs(ov - 1) <= 1e-6 and di == 0
        ov, di = MO.score_pair(a, box((11, 2, 0.5), (1.5, 4.0, 1.6), 0.3), dim, 2)      # disjoint -> 0
        assert ov == 0.0 and di == (10.0 if dim == 3 else 0.0)
    # two equal squares, the same centre, turned by 45 degrees: the octagon 2 (sqrt2 - 1) s^2
    s = 2.0
    ov, _ = MO.score_pair(box((0, 0, 0), (s, s, 1)), box((0, 0, 0), (s, s, 1), math.pi / 4), 2, 2)
    i8 = 2 * (math.sqrt(2) - 1)
    assert abs(ov - i8 / (2 - i8)) <= 1e-7                                     # the float32 cos / sin of 45 degrees
    # axis-aligned, shifted by half a length: inter l w / 2, union 3 l w / 2
    ov, di = MO.score_pair(box((0, 0, 0), (2, 4, 1)), box((2, 0, 0), (2, 4, 1)), 2, 2)
    assert abs(ov - 1 / 3) <= 1e-15 and di == 0.0                              # the dim-2 distance is the up component alone
    ov, di = MO.score_pair(box((0, 0, 0), (2, 4, 1)), box((2, 0, 0.25), (2, 4, 1)), 3, 2)
    assert abs(ov - (4 * 0.75) / (16 - 4 * 0.75)) <= 1e-15 and abs(di - math.hypot(2, 0.25)) <= 1e-15
    # the reference's height rule, not the centred interval: heights 1 and 2, centres 0.8 apart
    ov, _ = MO.score_pair(box((0, 0, 0.8), (2, 4, 2)), box((0, 0, 0), (2, 4, 1)), 3, 2)
    assert abs(ov - 8 / (16 + 8 - 8)) <= 1e-15                                 # rule: [-1.2, 0.8] and [-1, 0] share 1 (centred: 0.7)
    # degenerate input gives 0
    bad = box((0, 0, 0), (0, 0, 0))
    assert MO.score_pair(bad, bad, 2, 2)[0] == 0.0 and MO.score_pair(bad, bad, 3, 2)[0] == 0.0
    nan = a.copy()
    nan[7] = np.nan
    assert MO.score_pair(a, nan, 3, 2)[0] == 0.0


def test_success_precision_host_arithmetic_is_the_references_bit_for_bit(gold):
    """counts of the fixture's fp64 scores (the generator keeps them 1e-6 clear of every threshold) through curve_area equal
    the stored TorchSuccess / TorchPrecision compute() values bit for bit"""
    from open3dsot_amd import metrics
    xs, xp = torch.linspace(0, 1, steps=21), torch.linspace(0, 2, steps=21)
    for dim in (2, 3):
        o, d = gold["overlap.%d" % dim], gold["distance.%d" % dim]
        for name in ("s1", "s65", "s1000", "two"):
            rows = np.concatenate([gold["subset.s65"], gold["subset.s1000"]]) if name == "two" else gold["subset." + name]
            cs = [(o[rows] >= float(t)).sum() for t in xs]
            cp = [(d[rows] <= float(t)).sum() for t in xp]
            got = np.array([metrics.curve_area(cs, len(rows), xs, 1), metrics.curve_area(cp, len(rows), xp, 2)], np.float32)
            want = gold["sp.%d.%s" % (dim, name)]
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (dim, name, got, want)
    assert metrics.curve_area([0] * 21, 0, xs, 1) == 0.0                       # the empty metric


def test_cpu_tensors_are_refused():
    from open3dsot_amd import metrics
    with pytest.raises(RuntimeError, match="CPU not supported"):
        metrics.score_boxes(torch.zeros(4, 15), torch.zeros(4, 15))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        metrics.SuccessPrecision(device="cpu")
    with pytest.raises(ValueError):
        metrics.up_index((1, 0, 0))
    assert metrics.up_index((0, -1, 0)) == 1 and metrics.up_index([0, 0, 1]) == 2


def test_tracking_cases_are_scored(gold):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tracking_oracle as TO
    for case in TO.CASES:
        o, d = gold["track.%s.overlaps" % case], gold["track.%s.distances" % case]
        assert o.shape == d.shape == (TO.SEQ_FRAMES,) and abs(o[0] - 1) <= 1e-6 and d[0] == 0
