"""sampling="table" on the GPU (tracking.py; o3d_track_resample_tabled, o3d_track_motion_input_tabled and their lane forms): the
free-running loop on the reference's own index draw, read from a device table.

  the entry points   against the host-index entry points (o3d_track_resample, o3d_track_motion_input) handed
                     tracking.draw_indices of the same count, and the lane forms against the single forms: torch.equal
  the single loops   against the same class with sampling="reference" on the tracking fixtures, teacher-forced (inputs, boxes,
                     counts, recorded indices) and closed loop (results): torch.equal
  host stops         none after the first update() / outside a chunk boundary, uploads included
  lanes              every lane against a single sampling="reference" tracker on its tracklet; graph replay against eager;
                     evaluate(..., sampling="table", lanes=2) against the sequential reference epoch
  the table cache    shared by trackers of the same sizes, dropped by clear_draw_tables()

Every tracker here has capacities of 4096 (the fixture crops hold at most 2 518 points), so that a table is 8 or 17 MB."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import lane_oracle as LO  # noqa: E402
import motion_oracle as MO  # noqa: E402
import tracking_oracle as TO  # noqa: E402
import test_free_running_tracking_gpu as FR  # noqa: E402  (the fixture sequences, the models and the host_stops monkeypatch)
import test_lane_tracking_gpu as LT  # noqa: E402  (guard rows)

pytestmark = pytest.mark.gpu
gold, dev = FR.gold, FR.dev                        # the module-scoped fixtures of the free-running tests
up, tbits, guarded, untouched = FR.up, LT.tbits, LT.guarded, LT.untouched
SENT, ISENT = LT.SENT, LT.ISENT
MATCHING, MOTION = list(TO.CASES), list(MO.CASES)  # bat_fap, p2b, bat_first, bat_all; kitti, no_bc
CAP = 4096
# bank_capacity: the smallest power of two that holds every template of the fixture cases (2 x 1257 rows under
# firstandprevious at frame 1); test_bank_capacity_is_the_smallest_power_of_two_that_cuts_nothing pins that
MATCHING_KW = dict(search_capacity=CAP, model_capacity=CAP, bank_capacity=CAP)
MOTION_KW = dict(capacity=CAP)
TABLES = [(40, 8), (300, 257)]                     # S = 257 crosses one 256-thread workgroup


def kw_of(case):
    return MOTION_KW if case in MOTION else MATCHING_KW


_MOTION_MODELS = {}


def make_model(case, dev):
    """FR.make_model for every case of both fixtures (it knows one motion case)"""
    if case in MOTION and case != FR.MOTION:
        if case not in _MOTION_MODELS:
            from open3dsot_amd import m2track
            cfg = MO.case_config(case)
            _MOTION_MODELS[case] = (MO.init_weights(m2track.M2TRACK(**cfg)).to(dev).eval(), cfg)
        return _MOTION_MODELS[case]
    return FR.make_model(case, dev)


def drawn(n, S, dev):
    """tracking.draw_indices(n, S) -> (int32 device tensor | None for the zero-fill case, the (S,) array `used` must hold)"""
    from open3dsot_amd import tracking
    idx = tracking.draw_indices(n, S)
    if idx is None:
        return None, np.full((S,), -1, np.int32)
    return up(idx.astype(np.int32), dev), idx.astype(np.int32)


def counts_of(cap, S):
    return [0, 2, 3, S, cap, cap + 5]              # zero-filled twice, the smallest draw, the identity, full, min(count, cap)


# ---- the entry points against the host-index entry points ---------------------------------------------------------------------------
def tabled_alone(src, n, table, S, dev):
    """one o3d_track_resample_tabled job on its own -> (the job, dst, used, their guard rows)"""
    dst, dguard = guarded((S, 3), dev)
    used, uguard = guarded((S,), dev, ISENT, torch.int32)
    return (src, FR.count_of(n, dev), table, dst, used), dguard, uguard


def test_resample_tabled_equals_resample_on_the_reference_indices(dev):
    from open3dsot_amd import points_utils as PU, tracking
    rng = np.random.default_rng(7)
    alone = {}
    for cap, S in TABLES:
        table = tracking.draw_table(cap, S, dev)
        assert table.shape == (cap + 1, S) and table.dtype == torch.int32
        src = up(rng.normal(size=(cap, 3)).astype(np.float32), dev)
        for n in counts_of(cap, S):
            ne = min(n, cap)
            job, dguard, uguard = tabled_alone(src, n, table, S, dev)
            PU.resample_drawn([job])                                                  # n_jobs = 1
            idx, want_used = drawn(ne, S, dev)
            want = torch.full((S, 3), SENT, device=dev)
            PU.resample_jobs([(None if idx is None else src[:ne], idx, want)])
            assert torch.equal(tbits(job[3]), tbits(want)), (cap, S, n)
            assert np.array_equal(job[4].cpu().numpy(), want_used), (cap, S, n)
            assert untouched(dguard) and untouched(uguard, ISENT), (cap, S, n)
            if ne <= 2:
                assert not bool(job[3].any())
            alone[cap, n] = (job, job[3].clone(), job[4].clone())
        PU.resample_drawn([alone[cap, cap][0][:4] + (None,)])                          # used may be NULL
    # both jobs in one launch, each on its own table: every count of one against a count of the other, in both orders
    (ca, sa), (cb, sb) = TABLES
    for na, nb in zip(counts_of(ca, sa), reversed(counts_of(cb, sb))):
        for first, second in (((ca, na), (cb, nb)), ((cb, nb), (ca, na))):
            ja, jb = alone[first][0], alone[second][0]
            for j in (ja, jb):
                j[3].fill_(SENT)
                j[4].fill_(ISENT)
            PU.resample_drawn([ja, jb])
            for j, key in ((ja, first), (jb, second)):
                assert torch.equal(tbits(j[3]), tbits(alone[key][1])) and torch.equal(j[4], alone[key][2]), (first, second)


def test_a_table_entry_outside_the_cloud_leaves_its_row_zero(dev):
    """o3d_track_resample's rule for an index outside the source; `used` receives the entry as read"""
    from open3dsot_amd import points_utils as PU
    cap, S, n = 40, 8, 10
    table = torch.zeros((cap + 1, S), dtype=torch.int32, device=dev)
    table[n] = torch.tensor([0, 9, 10, -1, 40, 3, -5, 1 << 30], dtype=torch.int32, device=dev)
    src = up(np.random.default_rng(0).normal(size=(cap, 3)).astype(np.float32), dev)
    job, dguard, uguard = tabled_alone(src, n, table, S, dev)
    PU.resample_drawn([job])
    inside = [0, 1, 5]
    assert torch.equal(job[4], table[n]) and untouched(dguard) and untouched(uguard, ISENT)
    assert torch.equal(tbits(job[3][inside]), tbits(src[table[n][inside].long()]))
    assert not bool(job[3][[2, 3, 4, 6, 7]].any())


def test_a_launch_with_a_key_and_a_table_is_refused_before_anything_is_launched(dev):
    """key and table are two entry points of the C ABI: one launch takes one kind.  Both orders, single form and L = 2 lanes"""
    from open3dsot_amd import points_utils as PU, tracking
    cap, S, n, L = 8, 4, 5, 2
    table = tracking.draw_table(cap, S, dev)
    src = up(np.random.default_rng(3).normal(size=(L, cap, 3)).astype(np.float32), dev)
    for sources in ((1234, table), (table, 1234)):
        jobs = [tabled_alone(src[0], n, source, S, dev)[0] for source in sources]
        with pytest.raises(ValueError):
            PU.resample_drawn(jobs)
        dst = [torch.full((L, S, 3), SENT, device=dev) for _ in sources]
        used = [torch.full((L, S), ISENT, dtype=torch.int32, device=dev) for _ in sources]
        counts = up(np.full((L,), n, np.int32), dev)
        with pytest.raises(ValueError):
            PU.resample_drawn_lanes([(src, counts, 1, source, d, u) for source, d, u in zip(sources, dst, used)])
        torch.cuda.synchronize()
        for d, u in [(j[3], j[4]) for j in jobs] + list(zip(dst, used)):
            assert untouched(d) and untouched(u, ISENT)


@pytest.mark.parametrize("N", [1, 128, 129])
@pytest.mark.parametrize("with_bc", [True, False])
def test_motion_input_tabled_equals_motion_input_on_the_reference_indices(dev, N, with_bc):
    from open3dsot_amd import points_utils as PU, tracking
    cap = 300
    rng = np.random.default_rng([N, with_bc])
    table = tracking.draw_table(cap, N, dev)
    wlh = np.array([1.6, 3.9, 1.5], np.float32)
    half = np.array([wlh[1], wlh[0], wlh[2]]) * 1.25 / 2
    prev, cur = ((rng.uniform(-1.6, 1.6, (cap, 3)) * half).astype(np.float32) for _ in range(2))
    tp, tc, tw = up(prev, dev), up(cur, dev), up(wlh, dev)
    # a zero-filled previous half, the identity (N >= 3), a truncated current half, both halves zero-filled, the smallest draw
    for counts in ((2, 150), (N, N), (150, cap + 5), (1, 0), (3, cap)):
        ns = [min(c, cap) for c in counts]
        parts = [drawn(n, N, dev) for n in ns]
        zero = tuple(p[0] is None for p in parts)
        idx = None if all(zero) else torch.cat([torch.zeros((N,), dtype=torch.int32, device=dev) if p[0] is None else p[0] for p in parts])
        for first in (True, False):
            pts, pguard = guarded((2 * N, 5), dev)
            bc, bguard = guarded((2 * N, 9), dev)
            used, uguard = guarded((2 * N,), dev, ISENT, torch.int32)
            PU.motion_input_drawn(tp, tc, up(np.array(counts, np.int32), dev), table, tw, first, pts, bc if with_bc else False, used)
            want_pts, want_bc = PU.motion_input(None if zero[0] else tp[:ns[0]], None if zero[1] else tc[:ns[1]], idx, tw, first, zero=zero,
                                                out_points=torch.full((2 * N, 5), SENT, device=dev), out_bc=None if with_bc else False)
            assert torch.equal(tbits(pts), tbits(want_pts)), (N, counts, first)
            assert np.array_equal(used.cpu().numpy(), np.concatenate([p[1] for p in parts])), (N, counts, first)
            assert untouched(pguard) and untouched(bguard) and untouched(uguard, ISENT)
            if with_bc:
                assert torch.equal(tbits(bc), tbits(want_bc)), (N, counts, first)
            else:
                assert untouched(bc)                                                   # NULL: nothing written
    PU.motion_input_drawn(tp, tc, up(np.array([5, 7], np.int32), dev), table, tw, True, pts)      # used may be NULL


@pytest.mark.parametrize("L", [1, 3])
def test_resample_tabled_lanes_equals_the_single_entry_lane_by_lane(dev, L):
    from open3dsot_amd import points_utils as PU, tracking
    rng = np.random.default_rng(L)
    tables = [tracking.draw_table(cap, S, dev) for cap, S in TABLES]
    srcs = [up(rng.normal(size=(L, cap, 3)).astype(np.float32), dev) for cap, _ in TABLES]
    pools = [counts_of(cap, S) for cap, S in TABLES]
    for launch in range(6):
        counts = [np.array([pools[c][(launch + l + 2 * c) % 6] for l in range(L)], np.int32) for c in (0, 1)]
        # cloud 0 reads its counts at stride 2 from column 1 (the template count of a bank state), cloud 1 from column 0
        tab0, tab1 = np.full((L, 2), 12345, np.int32), np.full((L, 2), 54321, np.int32)
        tab0[:, 1], tab1[:, 0] = counts[0], counts[1]
        n0, n1 = up(tab0, dev), up(tab1, dev)
        for with_used in (True, False):
            dst, dguard, used, uguard = [], [], [], []
            for cap, S in TABLES:
                d, g = guarded((L, S, 3), dev)
                u, ug = guarded((L, S), dev, ISENT, torch.int32)
                dst.append(d), dguard.append(g), used.append(u), uguard.append(ug)
            PU.resample_drawn_lanes([(srcs[0], n0.view(-1)[1:], 2, tables[0], dst[0], used[0] if with_used else None),
                                     (srcs[1], n1, 2, tables[1], dst[1], used[1] if with_used else None)])
            for c, (cap, S) in enumerate(TABLES):
                assert untouched(dguard[c]) and untouched(uguard[c], ISENT)
                if not with_used:
                    assert untouched(used[c], ISENT)                                   # NULL: nothing written
                for l in range(L):
                    job, _, _ = tabled_alone(srcs[c][l], int(counts[c][l]), tables[c], S, dev)
                    PU.resample_drawn([job])
                    assert torch.equal(tbits(dst[c][l]), tbits(job[3])), (L, launch, c, l)
                    assert not with_used or torch.equal(used[c][l], job[4]), (L, launch, c, l)


@pytest.mark.parametrize("N", [1, 129])
@pytest.mark.parametrize("L", [1, 3])
def test_motion_input_tabled_lanes_equals_the_single_entry_lane_by_lane(dev, L, N):
    from open3dsot_amd import points_utils as PU, tracking
    rng = np.random.default_rng([L, N])
    cap = 300
    table = tracking.draw_table(cap, N, dev)
    pool = [(2, 150), (150, cap + 5), (N, N), (1, 0), (3, cap)]
    counts = np.array([pool[(l + N) % len(pool)] for l in range(L)], np.int32)
    wlh = rng.uniform(1.2, 4.0, (L, 3)).astype(np.float32)
    half = np.stack([wlh[:, 1], wlh[:, 0], wlh[:, 2]], 1)[:, None, :] * 1.25 / 2
    prev, cur = ((rng.uniform(-1.6, 1.6, (L, cap, 3)) * half).astype(np.float32) for _ in range(2))
    first = np.arange(L) % 2 == 0
    # one inactive lane: the motion input does not read `active` (an idle lane's rows feed a batch slot whose result
    # o3d_track_offset_box_lanes drops), so its rows are the single entry's as well
    lanes = LO.lane_table(L, first=first, active=np.arange(L) != 1)
    tp, tc, tw, tn, tl = up(prev, dev), up(cur, dev), up(wlh, dev), up(counts, dev), up(lanes, dev)
    for with_bc in (True, False):
        pts, pguard = guarded((L, 2 * N, 5), dev)
        bc, bguard = guarded((L, 2 * N, 9), dev)
        used, uguard = guarded((L, 2 * N), dev, ISENT, torch.int32)
        PU.motion_input_drawn_lanes(tp, tc, tn, table, tw, tl, pts, bc if with_bc else False, used)
        assert untouched(pguard) and untouched(bguard) and untouched(uguard, ISENT)
        if not with_bc:
            assert untouched(bc)
        for l in range(L):
            p1, b1 = torch.full((2 * N, 5), SENT, device=dev), torch.full((2 * N, 9), SENT, device=dev)
            u1 = torch.full((2 * N,), ISENT, dtype=torch.int32, device=dev)
            PU.motion_input_drawn(tp[l], tc[l], tn[l], table, tw[l], bool(first[l]), p1, b1 if with_bc else False, u1)
            assert torch.equal(tbits(pts[l]), tbits(p1)) and torch.equal(used[l], u1), (L, N, l)
            assert not with_bc or torch.equal(tbits(bc[l]), tbits(b1)), (L, N, l)
    PU.motion_input_drawn_lanes(tp, tc, tn, table, tw, tl, pts)                        # used may be NULL


# ---- the single loops against sampling="reference" -------------------------------------------------------------------------------
def used_of(trk):
    """the recorded indices of a tracker's last frame, [template | previous, search | current]"""
    return (trk.used_prev, trk.used_this) if hasattr(trk, "used_prev") else (trk.used_t, trk.used_s)


def reference_counts(entry, motion):
    """a line of the reference loop's `log` -> (the row of counts(), the two counts the draws were made for)"""
    if motion:
        return list(entry), list(entry)
    ns, nm, nt = entry
    return [ns, -1 if nm is None else nm], [nt, ns]


def sizes_of(trk, motion):
    return (int(trk.point_sample_size),) * 2 if motion else (int(trk.template_size), int(trk.search_size))


@pytest.mark.parametrize("case", MATCHING + MOTION)
def test_table_loop_equals_the_reference_loop_teacher_forced(gold, dev, case):
    """both loops set to the fixture's box before every frame: network inputs and result boxes torch.equal at every frame,
    counts() the reference loop's log, the recorded indices draw_indices of those counts"""
    from open3dsot_amd import tracking
    model, _ = make_model(case, dev)
    frames, gt = FR.sequence_of(gold, case, dev)
    motion = case in MOTION
    tab = tracking.tracker_for(model, sampling="table", record_indices=True, use_graph=False, **kw_of(case))
    ref = tracking.tracker_for(model, sampling="reference", use_graph=False)
    assert tab.free_running and tab.tabled and not ref.free_running
    for trk in (tab, ref):
        trk.init(frames[0], gt[0])
    want_counts = [[-1, -1]]
    for t in range(1, TO.SEQ_FRAMES):
        box = gold["%s.f%d.ref_box" % (case, t)]
        got = []
        for trk in (tab, ref):
            trk.set_box(box)
            got.append(trk.update(frames[t]))
        assert sorted(tab.inputs) == sorted(ref.inputs)
        for name in tab.inputs:
            assert torch.equal(tbits(tab.inputs[name]), tbits(ref.inputs[name])), (case, t, name)
        assert torch.equal(tbits(got[0]), tbits(got[1])), (case, t)
        row, ns = reference_counts(ref.log[-1], motion)
        want_counts.append(row)
        for used, n, S in zip(used_of(tab), ns, sizes_of(tab, motion)):
            assert np.array_equal(used.cpu().numpy(), drawn(n, S, dev)[1]), (case, t, n, S)
    assert tab.counts().tolist() == want_counts and tab.log == []
    assert tab.overflow() == (0, 0, 0), case
    assert np.array_equal(FR.bits(tab.results()), FR.bits(ref.results()))


@pytest.mark.parametrize("case", MATCHING + MOTION)
def test_table_loop_equals_the_reference_loop_closed_loop(gold, dev, case):
    """no set_box: the two loops feed the same inputs to the same batch-1 captured forward, so results() is equal in bits"""
    from open3dsot_amd import tracking
    model, _ = make_model(case, dev)
    frames, gt = FR.sequence_of(gold, case, dev)
    tab = tracking.tracker_for(model, sampling="table", **kw_of(case))
    ref = tracking.tracker_for(model, sampling="reference")
    for trk in (tab, ref):
        trk.init(frames[0], gt[0])
        for t in range(1, TO.SEQ_FRAMES):
            trk.update(frames[t])
    a, b = tab.results(), ref.results()
    differ = [t for t in range(TO.SEQ_FRAMES) if not np.array_equal(FR.bits(a[t]), FR.bits(b[t]))]
    print("table closed loop %s: frames whose box differs from the reference loop's: %s; graphs %s"
          % (case, differ, [tab.graph is not None, ref.graph is not None]))
    assert tab.overflow() == (0, 0, 0), case
    assert differ == [] and a.shape == (TO.SEQ_FRAMES, 15), (case, differ)
    assert np.abs(a[1:, :3] - a[:-1, :3]).max() > 1e-3                                  # the box does move
    # evaluate_sequence on the same tracker: the same loop once more, scored (track_sequence has no capacities to pass: its
    # tracker would build the default 134 MB tables, which no test does)
    ious, _, boxes = tracking.evaluate_sequence(model, frames, gt, tracker=tab, sampling="table")
    assert ious.shape == (TO.SEQ_FRAMES,) and np.array_equal(FR.bits(boxes.cpu().numpy()), FR.bits(b))


def test_bank_capacity_is_the_smallest_power_of_two_that_cuts_nothing(gold, dev):
    """4096 holds every template of the fixture cases closed loop (asserted case by case above, and here from the reference
    loop's own counts); 2048 does not: firstandprevious puts 2 x 1257 rows into the bank at frame 1"""
    from open3dsot_amd import tracking
    full = {}
    for case in MATCHING:
        model, _ = make_model(case, dev)
        frames, gt = FR.sequence_of(gold, case, dev)
        ref = tracking.tracker_for(model, sampling="reference", use_graph=False)
        ref.init(frames[0], gt[0])
        for t in range(1, TO.SEQ_FRAMES):
            ref.update(frames[t])
        counts = np.array([[-1, -1]] + [reference_counts(e, False)[0] for e in ref.log])
        assert tracking._matching_overflow(counts, CAP, CAP, CAP, ref.aggregation) == (0, 0, 0), case
        full[case] = tracking._matching_overflow(counts, CAP, CAP, CAP // 2, ref.aggregation)[2]
    assert max(full.values()) >= 1, full


# ---- host stops ------------------------------------------------------------------------------------------------------------------
def count_uploads(monkeypatch, log, stamp):
    """every host-to-device copy through Tensor.copy_ / .to / .cuda appends stamp() to `log` (undone by host_stops' exit)"""
    for owner, name in ((torch.Tensor, "copy_"), (torch.Tensor, "to"), (torch.Tensor, "cuda")):
        real = getattr(owner, name)

        def counted(self, *a, _real=real, _name=name, **k):
            out = _real(self, *a, **k)
            src, dst = (a[0], self) if _name == "copy_" else (self, out)
            if torch.is_tensor(src) and not src.is_cuda and dst.is_cuda:
                log.append(stamp())
            return out
        monkeypatch.setattr(owner, name, counted)


@pytest.mark.parametrize("case", ["bat_fap", FR.MOTION])
def test_no_host_stop_and_no_copy_after_the_first_update(gold, dev, case, monkeypatch):
    from open3dsot_amd import tracking
    model, _ = make_model(case, dev)
    frames, gt = FR.sequence_of(gold, case, dev)
    trk = tracking.tracker_for(model, sampling="table", use_graph=True, **kw_of(case))
    trk.init(frames[0], gt[0])
    trk.update(frames[1])                                  # the capture may synchronise
    uploads = []
    with FR.host_stops(monkeypatch) as stops:
        count_uploads(monkeypatch, uploads, lambda: trk.t)
        for t in range(2, TO.SEQ_FRAMES):
            trk.update(frames[t])
    assert stops.calls == [] and uploads == [] and trk.log == [], (stops.calls, uploads)
    assert trk.graph is not None and np.isfinite(trk.results()).all()


@pytest.mark.parametrize("case", ["bat_fap", FR.MOTION])
def test_no_host_stop_and_no_upload_in_a_lane_step_outside_a_chunk_boundary(gold, dev, case, monkeypatch):
    from open3dsot_amd import tracking
    trk = tracking.lane_tracker_for(make_model(case, dev)[0], 3, use_graph=True, plan_steps=4, sampling="table", **kw_of(case))
    steps = trk.begin(LT.tracklets_of(gold, case, dev))
    assert steps == 9 and trk.uploads == 1
    trk.step()                                             # the capture may synchronise
    uploads = []
    with FR.host_stops(monkeypatch) as stops:
        count_uploads(monkeypatch, uploads, lambda: trk.s)
        while trk.step():
            pass
    assert stops.calls == [], stops.calls
    assert uploads == [4, 8] and trk.uploads == 3                                       # one upload per chunk, in front of its first step
    assert np.isfinite(trk.boxes.cpu().numpy()).all() and trk.overflow() == (0, 0, 0)


# ---- lanes -----------------------------------------------------------------------------------------------------------------------
LENGTHS = [8, 3, 5]                                # three tracklets of different lengths: staggered restarts, an idle tail


def three_tracklets(gold, case, dev):
    frames, gt = FR.sequence_of(gold, case, dev)
    return [(frames[:n], gt[:n]) for n in LENGTHS]


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("case", ["bat_fap", "bat_all", FR.MOTION])
def test_table_lanes_equal_one_reference_tracker_per_tracklet_teacher_forced(gold, dev, case, L):
    """every lane against a single sampling="reference" tracker on the lane's tracklet, both set to the fixture's box before
    every frame: the network inputs bit for bit, the recorded indices draw_indices of the reference loop's counts"""
    from open3dsot_amd import tracking
    model, _ = make_model(case, dev)
    motion = case in MOTION
    tracklets = three_tracklets(gold, case, dev)
    trk = tracking.lane_tracker_for(model, L, record_indices=True, use_graph=False, sampling="table", **kw_of(case))
    assert isinstance(trk, tracking.MotionLaneTracker if motion else tracking.LaneTracker) and trk.tabled
    steps = trk.begin(tracklets)
    tracklet, frame = trk.schedule
    singles = [tracking.tracker_for(model, sampling="reference", use_graph=False) for _ in range(L)]
    seen = 0
    for s in range(steps):
        live = [(l, int(tracklet[s, l]), int(frame[s, l])) for l in range(L) if tracklet[s, l] >= 0]
        for l, j, t in live:
            if t == 1:
                singles[l].init(tracklets[j][0][0], tracklets[j][1][0])
            box = gold["%s.f%d.ref_box" % (case, t)]
            trk.set_box(l, box)
            singles[l].set_box(box)
        assert trk.step() == (s + 1 < steps)
        for l, j, t in live:
            one = singles[l]
            one.update(tracklets[j][0][t])
            for name in one.inputs:
                assert torch.equal(tbits(trk.inputs[name][l]), tbits(one.inputs[name][0])), (case, L, s, l, name)
            row, ns = reference_counts(one.log[-1], motion)
            sizes = sizes_of(one, motion)
            used = (trk.used[l, :sizes[0]], trk.used[l, sizes[0]:]) if motion else (trk.used_t[l], trk.used_s[l])
            for u, n, S in zip(used, ns, sizes):
                assert np.array_equal(u.cpu().numpy(), drawn(n, S, dev)[1]), (case, L, s, l, n, S)
            assert trk.counts(j)[t].tolist() == row, (case, L, s, l)
            seen += 1
    assert seen == sum(n - 1 for n in LENGTHS) and not trk.step()
    assert trk.overflow() == (0, 0, 0)


@pytest.mark.parametrize("case", ["bat_fap", FR.MOTION])
def test_table_lanes_graph_replay_equals_eager(gold, dev, case):
    from open3dsot_amd import tracking
    model, _ = make_model(case, dev)
    tracklets = three_tracklets(gold, case, dev)
    runs = {}
    for use_graph in (False, True):
        trk = tracking.lane_tracker_for(model, 2, use_graph=use_graph, sampling="table", **kw_of(case))
        runs[use_graph] = trk.run(tracklets).cpu().numpy()
        assert (trk.graph is not None) == use_graph and trk.overflow() == (0, 0, 0)
    assert runs[True].shape == (sum(LENGTHS), 15) and np.array_equal(FR.bits(runs[True]), FR.bits(runs[False]))
    assert np.abs(runs[False][1:8, :3] - runs[False][0:7, :3]).max() > 1e-3             # the box does move


@pytest.mark.parametrize("case", ["bat_fap", FR.MOTION])
def test_evaluate_on_lanes_with_the_table(gold, dev, case):
    """the lane epoch on the reference's indices against the sequential reference epoch: the same frames and tracklets; the
    two Success / Precision pairs are printed, not asserted equal (the forward at batch 2 is not the forward at batch 1 in
    bits, and a closed loop compounds the difference)"""
    from open3dsot_amd import tracking
    model, _ = make_model(case, dev)
    tracklets = three_tracklets(gold, case, dev)
    got = tracking.evaluate(model, tracklets, sampling="table", lanes=2, use_graph=False, **kw_of(case))
    want = tracking.evaluate(model, tracklets, sampling="reference", use_graph=False)
    print("evaluate %s: lanes=2 sampling=table success %.4f precision %.4f; sequential sampling=reference success %.4f precision %.4f"
          % (case, got["success"], got["precision"], want["success"], want["precision"]))
    assert got["frames"] == want["frames"] == sum(LENGTHS) and got["tracklets"] == want["tracklets"] == len(LENGTHS)
    for out in (got, want):
        assert np.isfinite(out["success"]) and np.isfinite(out["precision"])
    for sampling in ("reference", "nonsense"):
        with pytest.raises(ValueError, match="sampling"):
            tracking.evaluate(model, tracklets, sampling=sampling, lanes=2)


# ---- the table cache -------------------------------------------------------------------------------------------------------------
def test_trackers_of_the_same_sizes_share_one_table(gold, dev):
    from open3dsot_amd import tracking
    model, _ = make_model("bat_fap", dev)
    motion, _ = make_model(FR.MOTION, dev)
    tracking.clear_draw_tables()
    a = tracking.SequenceTracker(model, sampling="table", **MATCHING_KW)
    assert len(tracking._DRAW_TABLES) == 2                                              # (bank, template) and (search, search)
    b = tracking.LaneTracker(model, 2, sampling="table", **MATCHING_KW)
    assert a.table_t.data_ptr() == b.table_t.data_ptr() and a.table_s.data_ptr() == b.table_s.data_ptr()
    assert a.table_t.shape == (CAP + 1, int(a.template_size)) and a.table_s.shape == (CAP + 1, int(a.search_size))
    assert a.table_t.element_size() * a.table_t.numel() == 4 * (CAP + 1) * int(a.template_size)      # the docstring's formula
    m, n = tracking.MotionSequenceTracker(motion, sampling="table", **MOTION_KW), tracking.MotionLaneTracker(motion, 2, sampling="table", **MOTION_KW)
    assert m.table.data_ptr() == n.table.data_ptr()
    # search (4096, 1024) and the motion table (4096, 1024) are the same function of the same sizes: one table
    assert m.table.data_ptr() == a.table_s.data_ptr() and len(tracking._DRAW_TABLES) == 2
    assert tracking.draw_table(CAP, int(a.search_size), dev).data_ptr() == a.table_s.data_ptr()
    assert np.array_equal(a.table_t[:700].cpu().numpy(), tracking.draw_table_host(699, int(a.template_size)))
    device_mode = tracking.SequenceTracker(model, sampling="device", **MATCHING_KW)
    assert not hasattr(device_mode, "table_t") and len(tracking._DRAW_TABLES) == 2      # the other modes build none
    tracking.clear_draw_tables()
    assert tracking._DRAW_TABLES == {}
    c = tracking.SequenceTracker(model, sampling="table", **MATCHING_KW)
    assert c.table_t.data_ptr() != a.table_t.data_ptr() and torch.equal(c.table_t, a.table_t)      # built again; a keeps its own
