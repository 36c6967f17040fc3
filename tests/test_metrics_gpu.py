"""Scoring tracked boxes on the GPU: o3d_track_score against the reference's own utils/metrics.py (tests/golden/ref_metrics.npz)
and its fp64 restatement (tests/metrics_oracle.py), its counters against host counts of its own outputs, SuccessPrecision
against the reference's TorchSuccess / TorchPrecision bit for bit, and the evaluation loops of open3dsot_amd/tracking.py."""
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
import tracking_oracle as TO  # noqa: E402

pytestmark = pytest.mark.gpu
UP_AXIS = {1: (0, -1, 0), 2: (0, 0, 1)}
SIZES = (1, 63, 64, 65, 257, 1000)           # wave (64) and workgroup (256) edges


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_metrics.npz"))


@pytest.fixture(scope="module")
def track_gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_tracking.npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32).view(np.int32)


def device_scores(gold, dev, dim, rows=None, accumulate=None):
    """the table's rows (all of them when None) through o3d_track_score, one launch per up axis -> (overlaps, distances) numpy"""
    from open3dsot_amd import metrics
    rows = np.arange(len(gold["a"])) if rows is None else np.asarray(rows)
    a, b, up = gold["a"][rows], gold["b"][rows], gold["up"][rows]
    ov, di = np.full(len(rows), np.nan, np.float32), np.full(len(rows), np.nan, np.float32)
    for u in (1, 2):
        sel = np.flatnonzero(up == u)
        if len(sel):
            o, d = metrics.score_boxes(torch.from_numpy(a[sel]).to(dev), torch.from_numpy(b[sel]).to(dev), dim, UP_AXIS[u],
                                       accumulate=accumulate)
            ov[sel], di[sel] = o.cpu().numpy(), d.cpu().numpy()
    return ov, di


_FULL = {}


def full_run(gold, dev, dim):
    """the whole table once per dim, shared by the tests below and left unchanged"""
    if dim not in _FULL:
        _FULL[dim] = device_scores(gold, dev, dim)
    return _FULL[dim]


# ---- (a) the kernel against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_scores_equal_the_reference(gold, dev, dim):
    """every pair of the table, both up axes: |device - reference| <= 2e-7 on overlaps (the fp32 rounding of a value <= 1 is
    <= 6e-8), 2e-7 relative on distances"""
    ov, di = full_run(gold, dev, dim)
    ro, rd = gold["overlap.%d" % dim], gold["distance.%d" % dim]
    assert not np.isnan(ov).any() and not np.isnan(di).any()
    for u in (1, 2):
        s = gold["up"] == u
        print("dim %d up %d (%d pairs): max |overlap - reference| %.2e, max relative distance difference %.2e" %
              (dim, u, s.sum(), np.abs(ov[s] - ro[s]).max(), (np.abs(di[s] - rd[s]) / np.maximum(rd[s], 1e-30)).max()))
    assert np.abs(ov - ro).max() <= 2e-7
    assert np.all(np.abs(di - rd) <= 2e-7 * rd)
    # and the fp64 restatement rounded once: the same operation order, so at most the last bit apart
    want = np.array([MO.score_pair(gold["a"][i], gold["b"][i], dim, int(gold["up"][i])) for i in range(0, len(ov), 7)])
    assert np.abs(ov[::7] - want[:, 0]).max() <= 2e-7 and np.all(np.abs(di[::7] - want[:, 1]) <= 2e-7 * want[:, 1])


def test_degenerate_boxes_score_zero(gold, dev):
    from open3dsot_amd import metrics
    a, b = gold["a"][:4].copy(), gold["b"][:4].copy()
    a[0, 3:6] = 0
    b[0, 3:6] = 0                      # no extent at all: union 0
    b[1, 7] = np.nan
    a[2, 0] = np.inf
    a[3, 6:15] = 0                     # a zero matrix: no footprint
    for dim in (2, 3):
        ov, di = metrics.score_boxes(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), dim)
        assert ov.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
        assert torch.isfinite(di[[0, 1, 3]]).all()


# ---- (b) run sizes, the valid mask, the counters ---------------------------------------------------------------------------------
def host_counts(m, ov, di):
    xs, xp = m.xaxis[0].numpy(), m.xaxis[1].numpy()
    return ([int((ov >= t).sum()) for t in xs] + [int((di <= t).sum()) for t in xp] + [len(ov)])


@pytest.mark.parametrize("n", SIZES)
def test_run_sizes_valid_mask_and_counters(gold, dev, n):
    """rows [0:n] of the z-up pairs: the outputs bit-identical to the same rows of the full run; the counters equal a host count
    of the device's own outputs exactly -- also with every third row switched off (their outputs keep a sentinel) and with two
    launches adding to the same counters"""
    from open3dsot_amd import metrics
    dim = 3
    full_ov, full_di = full_run(gold, dev, dim)
    rows = np.flatnonzero(gold["up"] == 2)[:n]
    assert len(rows) == n
    a, b = torch.from_numpy(gold["a"][rows]).to(dev), torch.from_numpy(gold["b"][rows]).to(dev)
    m = metrics.SuccessPrecision(device=dev)
    ov, di = metrics.score_boxes(a, b, dim, accumulate=m)
    assert np.array_equal(bits(ov), bits(full_ov[rows])) and np.array_equal(bits(di), bits(full_di[rows]))
    ov_h, di_h = ov.cpu().numpy(), di.cpu().numpy()
    assert m.counts.cpu().tolist() == host_counts(m, ov_h, di_h)
    assert m.compute()["frames"] == n
    # a second launch into the same counters, with a mask
    valid = torch.ones(n, dtype=torch.int32, device=dev)
    valid[::3] = 0
    keep = valid.cpu().numpy() != 0
    out = (torch.full((n,), -7.0, device=dev), torch.full((n,), -9.0, device=dev))
    ov2, di2 = metrics.score_boxes(a, b, dim, valid=valid, out=out, accumulate=m)
    assert ov2 is out[0] and di2 is out[1]
    o2, d2 = ov2.cpu().numpy(), di2.cpu().numpy()
    assert np.all(o2[~keep] == -7.0) and np.all(d2[~keep] == -9.0)
    assert np.array_equal(bits(o2[keep]), bits(ov_h[keep])) and np.array_equal(bits(d2[keep]), bits(di_h[keep]))
    both = [x + y for x, y in zip(host_counts(m, ov_h, di_h), host_counts(m, ov_h[keep], di_h[keep]))]
    assert m.counts.cpu().tolist() == both
    # update() on device tensors counts like the launch
    m2 = metrics.SuccessPrecision(device=dev)
    m2.update(ov, di)
    m2.update(ov[keep], di[keep])
    assert m2.counts.cpu().tolist() == both
    m2.reset()
    assert m2.compute() == {"success": 0.0, "precision": 0.0, "frames": 0}


def test_outputs_and_counters_are_optional(gold, dev):
    """the C entry point with overlaps / distances NULL still counts; with the counters NULL it still writes"""
    from open3dsot_amd import capi, metrics
    n, dim = 257, 2
    rows = np.flatnonzero(gold["up"] == 1)[:n]
    a, b = torch.from_numpy(gold["a"][rows]).to(dev), torch.from_numpy(gold["b"][rows]).to(dev)
    m = metrics.SuccessPrecision(device=dev)
    ov, di = metrics.score_boxes(a, b, dim, UP_AXIS[1])
    k = m.n
    rc = capi.load().o3d_track_score(a.data_ptr(), b.data_ptr(), None, n, dim, 1, None, None, m.thresholds[0].data_ptr(), k,
                                     m.thresholds[1].data_ptr(), k, m.counts[:k].data_ptr(), m.counts[k:2 * k].data_ptr(),
                                     m.counts[2 * k:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    assert m.counts.cpu().tolist() == host_counts(m, ov.cpu().numpy(), di.cpu().numpy())


# ---- (c) Success / Precision against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_success_precision_equal_the_reference_bit_for_bit(gold, dev, dim):
    from open3dsot_amd import metrics
    for name in ("s1", "s65", "s1000", "two"):
        parts = [gold["subset.s65"], gold["subset.s1000"]] if name == "two" else [gold["subset." + name]]
        by_launch, by_update = metrics.SuccessPrecision(device=dev), metrics.SuccessPrecision(device=dev)
        for rows in parts:
            ov, di = device_scores(gold, dev, dim, rows, accumulate=by_launch)
            by_update.update(torch.from_numpy(ov).to(dev), torch.from_numpy(di).to(dev))
        want = gold["sp.%d.%s" % (dim, name)]
        for m in (by_launch, by_update):
            r = m.compute()
            got = np.array([r["success"], r["precision"]], np.float32)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (dim, name, got, want)
            assert r["frames"] == sum(len(p) for p in parts)


# ---- (d) evaluate_sequence on the tracking fixture's sequences ---------------------------------------------------------------------
_MODELS = {}


def make_model(case, dev, **over):
    from open3dsot_amd import trackers
    key = (case, tuple(sorted(over.items())))
    if key not in _MODELS:
        name, cfg = TO.case_config(case)
        cfg = dict(cfg, **over)
        model = trackers.get_model(name)(trackers.make_config(cfg))
        TO.init_weights(model)
        _MODELS[key] = (model.to(dev).eval(), cfg)
    return _MODELS[key]


def sequence_of(track_gold, case, dev):
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(int(track_gold[case + ".seq_seed"]), TO.SEQ_FRAMES, TO.SEQ_POINTS)
    return [torch.from_numpy(f).to(dev) for f in frames], gt


def score_bounds(gt, coord=2e-5, rot=1e-6, factor=1.0):
    """How far a score can move when the result box moves by at most `coord` per centre coordinate and `rot` per rotation
    entry -- the bounds the tracking tests put on the device loop against the reference (tests/test_tracking_gpu.py: 2e-5 m on
    coordinates, 1e-6 on the entries of a box's rotation) -- to first order, for a box of the case's own w, l, h:
      * a rotation entry off by `rot` moves a footprint corner by at most rot * sqrt(l^2 + w^2) / 2 (the corner's lever arm),
        so every footprint edge of the result box is displaced by at most e = coord + rot * sqrt(l^2 + w^2) / 2 and each end
        of the height interval by at most coord;
      * the intersection volume I is a footprint area times a height.  Moving one box's edges by e changes the footprint
        intersection by at most e times its perimeter, which is at most that of the box, 2 (w + l): relative to the box's own
        volume V = w l h that is e (2/w + 2/l); the height interval changes by at most 2 coord, relative to h: coord * 2/h.
        Together  dI / V <= e (2/w + 2/l) + coord * 2/h  (= coord (2/w + 2/l + 2/h) plus the yaw term);
      * overlap o = I / U with U = 2 V - I (both volumes are V: the tracker keeps wlh), so do = dI 2 V / U^2 =
        (dI / V) (1 + o)^2 / 2: `factor` = (1 + o)^2 / 2 is below 1 for o < 0.41 and at most 2.  The reference sequences
        (closed loop, untrained weights) end far from the target, o = 0 from frame 1 on, and at frame 0 both boxes are the
        ground truth itself (dI = 0): factor 1 covers them; a caller whose overlaps may be anything passes 2;
      * the distance is the norm of the centre difference: it moves by at most sqrt(3) coord.
    On top of both comes the fp32 rounding of the device's result, the 2e-7 (relative for the distance) of test (a)."""
    w, l, h = [float(x) for x in gt[0, 3:6]]
    e = coord + rot * np.hypot(l, w) / 2
    return factor * (e * (2 / w + 2 / l) + coord * 2 / h) + 2e-7, np.sqrt(3) * coord


@pytest.mark.parametrize("case", list(TO.CASES))
def test_evaluate_sequence_on_the_reference_sequences(gold, track_gold, dev, case):
    """evaluate_sequence (8 frames x 20 000 points): its scores equal the fp64 restatement on the tracker's own result boxes
    within 2e-7, and the reference's stored scores of the reference's own result boxes within score_bounds.
    Largest measured differences: see DESIGN.md section 12e."""
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(track_gold, case, dev)
    ious, dists, results = tracking.evaluate_sequence(model, frames, gt)
    assert ious.is_cuda and dists.is_cuda and results.is_cuda and tuple(results.shape) == (TO.SEQ_FRAMES, 15)
    ious, dists, results = ious.cpu().numpy(), dists.cpu().numpy(), results.cpu().numpy()
    assert np.array_equal(bits(results), bits(tracking.track_sequence(model, frames, gt[0])))      # the same loop
    want_o, want_d = MO.score(gt, results, cfg["IoU_space"], MO.up_index(cfg["up_axis"]))
    d_own_o, d_own_d = np.abs(ious - want_o).max(), (np.abs(dists - want_d) / np.maximum(want_d, 1e-30)).max()
    ref_o, ref_d = gold["track.%s.overlaps" % case], gold["track.%s.distances" % case]
    bound_o, bound_d = score_bounds(gt)
    d_ref_o, d_ref_d = np.abs(ious - ref_o), np.abs(dists - ref_d)
    print("%s: |device - oracle on its own boxes| overlap %.2e, distance (relative) %.2e" % (case, d_own_o, d_own_d))
    print("%s: |device - reference| overlap %s (bound %.2e)" % (case, " ".join("%.2e" % v for v in d_ref_o), bound_o))
    print("%s: |device - reference| distance %s (bound %.2e + 2e-7 d)" % (case, " ".join("%.2e" % v for v in d_ref_d), bound_d))
    assert d_own_o <= 2e-7 and d_own_d <= 2e-7
    assert abs(ious[0] - 1.0) <= 2e-7 and dists[0] == 0.0                       # frame 0: the first box against itself
    assert np.all(d_ref_o <= bound_o), (d_ref_o, bound_o)
    assert np.all(d_ref_d <= bound_d + 2e-7 * ref_d), (d_ref_d, bound_d)


@pytest.mark.parametrize("rule", ["previous_gt", "current_gt"])
def test_evaluate_sequence_hands_the_ground_truth_on(track_gold, dev, rule):
    """reference_BB previous_gt / current_gt: update() of frame t gets gt[t-1] / gt[t] (generate_search_area): the results are
    those of a SequenceTracker driven by hand, and the scores equal the restatement on the tracker's own boxes within 2e-7"""
    from open3dsot_amd import tracking
    model, cfg = make_model("bat_fap", dev, reference_BB=rule)
    frames, gt = sequence_of(track_gold, "bat_fap", dev)
    ious, dists, results = tracking.evaluate_sequence(model, frames, gt)
    trk = tracking.SequenceTracker(model)
    trk.init(frames[0], gt[0])
    for t in range(1, len(frames)):
        trk.update(frames[t], ref_box=gt[t - 1] if rule == "previous_gt" else gt[t])
    assert np.array_equal(bits(results), bits(trk.results()))
    want_o, want_d = MO.score(gt, results.cpu().numpy(), 3, 2)
    ious, dists = ious.cpu().numpy(), dists.cpu().numpy()
    print("%s: overlaps %s" % (rule, np.round(ious, 4)))
    assert np.abs(ious - want_o).max() <= 2e-7 and np.all(np.abs(dists - want_d) <= 2e-7 * want_d)
    # score() with a mask and a metric, by hand
    from open3dsot_amd import metrics
    m = metrics.SuccessPrecision(device=dev)
    valid = np.array([1, 1, 0, 1, 1, 0, 1, 1])
    o2, d2 = trk.score(gt, valid=valid, metrics=m)
    keep = valid != 0
    assert np.array_equal(bits(o2.cpu().numpy()[keep]), bits(ious[keep])) and np.all(o2.cpu().numpy()[~keep] == 0)
    assert m.counts.cpu().tolist() == host_counts(m, ious[keep], dists[keep])


# ---- (e) the test epoch ---------------------------------------------------------------------------------------------------------------
def test_evaluate_accumulates_over_tracklets_and_reads_back_once(track_gold, dev, monkeypatch):
    from open3dsot_amd import metrics, sampler, synth, tracking
    model, cfg = make_model("bat_fap", dev, reference_BB="previous_gt")
    fa, ga = sequence_of(track_gold, "bat_fap", dev)
    fb_np, gb = synth.make_sequence(77, 5, TO.SEQ_POINTS)
    fb = [torch.from_numpy(f).to(dev) for f in fb_np]
    reads = []
    real = metrics.SuccessPrecision._read
    monkeypatch.setattr(metrics.SuccessPrecision, "_read", lambda self: reads.append(1) or real(self))
    trackers_made = []
    real_for = tracking.tracker_for
    monkeypatch.setattr(tracking, "tracker_for", lambda *a, **k: trackers_made.append(real_for(*a, **k)) or trackers_made[-1])
    # by hand: one evaluate_sequence per tracklet, the scores fed to a metric through update()
    hand = metrics.SuccessPrecision(device=dev)
    per = {}
    for name, (f, g) in (("a", (fa, ga)), ("b", (fb, gb))):
        o, d, _ = tracking.evaluate_sequence(model, f, g)
        per[name] = (o, d)
    hand.update(*per["a"])
    hand.update(*per["b"])
    want_two = hand.compute()
    hand.reset()
    hand.update(*per["a"])
    hand.update(*per["a"])
    want_twice = hand.compute()
    reads.clear()
    trackers_made.clear()
    got_two = tracking.evaluate(model, sampler.DeviceTracklets([fa, fb], [ga, gb], device=dev))
    assert len(reads) == 1 and len(trackers_made) == 1                     # one read-back, one tracker (one graph) for the epoch
    assert trackers_made[0].graph is not None or trackers_made[0].graph_failed
    assert got_two == dict(want_two, tracklets=2) and got_two["frames"] == len(fa) + len(fb)
    reads.clear()
    got_twice = tracking.evaluate(model, [(fa, ga), (fa, ga)])             # any iterable of (frames, boxes)
    assert len(reads) == 1
    assert got_twice == dict(want_twice, tracklets=2) and got_twice["frames"] == 2 * len(fa)
    assert 0 < got_two["success"] < 100 and 0 < got_two["precision"] <= 100
    # a metric of the caller's is added to, not replaced
    mine = metrics.SuccessPrecision(device=dev)
    tracking.evaluate(model, [(fb, gb)], metrics=mine)
    tracking.evaluate(model, [(fa, ga)], metrics=mine)
    assert mine.compute() == want_two


# ---- (f) K targets --------------------------------------------------------------------------------------------------------------------
def test_evaluate_targets_equals_single_runs(dev):
    """K = 3 on synth.make_scene, target 1 without annotation from frame 4 on, reference_BB previous_gt (every frame starts from
    the ground truth, so the batched and the single loops see the same inputs and their boxes differ by the network's batch
    rounding alone: FEATURE_BOUND = 1e-4 m on the centre, tests/test_multi_tracking_gpu.py).  Bound on the scores: score_bounds
    with that coordinate bound and factor 2 (the overlaps here are anywhere in [0, 1])."""
    from open3dsot_amd import metrics, synth, tracking
    T, K, cut = 6, 3, 4
    model, cfg = make_model("bat_fap", dev, reference_BB="previous_gt")
    frames_np, gt = synth.make_scene(3, T, TO.SEQ_POINTS, K)
    frames = [torch.from_numpy(f).to(dev) for f in frames_np]
    valid = np.ones((T, K), np.int32)
    valid[cut:, 1] = 0
    m = metrics.SuccessPrecision(device=dev)
    ious, dists, results = tracking.evaluate_targets(model, frames, gt, valid=valid, metrics=m)
    assert tuple(ious.shape) == (T, K) and tuple(results.shape) == (T, K, 15)
    ious, dists, results = ious.cpu().numpy(), dists.cpu().numpy(), results.cpu().numpy()
    assert np.all(ious[cut:, 1] == 0) and np.all(dists[cut:, 1] == 0)                  # not scored: left as allocated
    assert np.array_equal(bits(results[cut:, 1]), bits(np.repeat(results[cut - 1:cut, 1], T - cut, 0)))     # retired: its box repeats
    keep = valid != 0
    assert m.counts.cpu().tolist() == host_counts(m, ious[keep], dists[keep]) and m.compute()["frames"] == T * K - (T - cut)
    want_o, want_d = MO.score(gt, results, 3, 2)
    assert np.abs(ious - want_o)[keep].max() <= 2e-7 and np.all((np.abs(dists - want_d) <= 2e-7 * want_d)[keep])
    worst_o = worst_d = 0.0
    for k in range(K):
        so, sd, _ = tracking.evaluate_sequence(model, frames, gt[:, k])
        so, sd = so.cpu().numpy(), sd.cpu().numpy()
        rows = keep[:, k]
        bound_o, bound_d = score_bounds(gt[:, k], coord=1e-4, factor=2.0)
        do, dd = np.abs(ious[rows, k] - so[rows]).max(), np.abs(dists[rows, k] - sd[rows]).max()
        worst_o, worst_d = max(worst_o, do), max(worst_d, dd)
        assert do <= bound_o and dd <= bound_d + 2e-7 * sd[rows].max(), (k, do, bound_o, dd, bound_d)
    print("evaluate_targets against single runs: largest overlap difference %.2e, distance %.2e" % (worst_o, worst_d))
    # all targets annotated: valid may be left out
    o_all, _, _ = tracking.evaluate_targets(model, frames, gt)
    assert np.array_equal(bits(o_all.cpu().numpy()[:, [0, 2]]), bits(ious[:, [0, 2]]))
