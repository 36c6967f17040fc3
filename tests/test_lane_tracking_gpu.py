"""The test epoch on L lanes on the GPU (tracking.LaneTracker / MotionLaneTracker): the lane kernels against their single
entry points and tests/lane_oracle.py bit for bit, the loop teacher-forced against one single tracker per tracklet, graph replay
against eager, the absence of any host stop or upload outside a chunk boundary, evaluate(..., lanes=3) and truncation."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import free_running_oracle as FO  # noqa: E402
import lane_oracle as LO  # noqa: E402
import test_free_running_tracking_gpu as FR  # noqa: E402  (the fixture sequences, the models and the host_stops monkeypatch)

pytestmark = pytest.mark.gpu
gold, dev = FR.gold, FR.dev                        # the module-scoped fixtures of the free-running tests
bits, up, MOTION = FR.bits, FR.up, FR.MOTION
LANES = [1, 3, 5]
FEATURE_BOUND = 1e-4                               # the project's bound on network outputs (tests/test_multi_tracking_gpu.py)
SENT, ISENT = -7.0, -9


def tbits(t):
    return t.contiguous().view(torch.int32)


def guarded(shape, dev, value=SENT, dtype=torch.float32):
    """-> (a sentinel-filled tensor of `shape`, its guard row behind it); both views of one allocation"""
    whole = torch.full((shape[0] + 1,) + tuple(shape[1:]), value, dtype=dtype, device=dev)
    return whole[:shape[0]], whole[shape[0]]


def untouched(guard, value=SENT):
    return bool((guard == value).all())


def tracklets_of(gold, case, dev):
    """the fixture sequence of a case cut to the lengths of lane_oracle.LENGTHS -> [(frames, gt boxes)]"""
    frames, gt = FR.sequence_of(gold, case, dev)
    return [(frames[:n], gt[:n]) for n in LO.LENGTHS]


# ---- the kernels, bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 128, 129, 512])
@pytest.mark.parametrize("L", LANES)
def test_resample_drawn_lanes_equals_the_single_entry_and_the_oracle(dev, L, S):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng([L, S])
    caps, sizes = (600, 520), (S, {1: 129, 128: 512, 129: 1, 512: 128}[S])             # two clouds of different capacity and size
    keys = FO.keys(2)
    srcs = [rng.normal(size=(L, cap, 3)).astype(np.float32) for cap in caps]
    tsrc = [up(s, dev) for s in srcs]
    for launch in range(-(-8 // L)):
        counts = []
        for c in (0, 1):
            pool = [0, 2, 3, sizes[c] - 1, sizes[c], sizes[c] + 1, caps[c], caps[c] + 1]
            counts.append(np.array([max(pool[(launch * L + l + 3 * c) % 8], 0) for l in range(L)], np.int32))
        # cloud 0 reads its counts at stride 2 from column 1 (the template count of a bank state), cloud 1 from column 0
        table = np.full((L, 2), 12345, np.int32)
        table[:, 1] = counts[0]
        table2 = np.full((L, 2), 54321, np.int32)
        table2[:, 0] = counts[1]
        n0, n1 = up(table, dev), up(table2, dev)
        for with_used in (True, False):
            dst, dguard, used, uguard = [], [], [], []
            for c in (0, 1):
                d, g = guarded((L, sizes[c], 3), dev)
                u, ug = guarded((L, sizes[c]), dev, ISENT, torch.int32)
                dst.append(d), dguard.append(g), used.append(u), uguard.append(ug)
            PU.resample_drawn_lanes([(tsrc[0], n0.view(-1)[1:], 2, keys[0], dst[0], used[0] if with_used else None),
                                     (tsrc[1], n1, 2, keys[1], dst[1], used[1] if with_used else None)])
            for c in (0, 1):
                want, want_used = LO.resample_drawn_lanes(srcs[c], counts[c], keys[c], sizes[c])
                assert np.array_equal(bits(dst[c].cpu().numpy()), bits(want)), (L, S, launch, c)
                assert untouched(dguard[c]) and untouched(uguard[c], ISENT)
                if with_used:
                    assert np.array_equal(used[c].cpu().numpy(), want_used), (L, S, launch, c)
                else:
                    assert untouched(used[c], ISENT)                                   # NULL: nothing written
                for l in range(L):                                                     # and the single entry on lane l's operands
                    one, one_used = torch.full((sizes[c], 3), SENT, device=dev), torch.full((sizes[c],), ISENT, dtype=torch.int32, device=dev)
                    PU.resample_drawn([(tsrc[c][l], FR.count_of(int(counts[c][l]), dev), keys[c], one, one_used)])
                    assert torch.equal(tbits(dst[c][l]), tbits(one)), (L, S, launch, c, l)
                    assert not with_used or torch.equal(used[c][l], one_used)


@pytest.mark.parametrize("rule", FO.RULES)
@pytest.mark.parametrize("L", LANES)
def test_bank_update_lanes_equals_the_single_entry_and_the_oracle(dev, L, rule):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(L)
    crop_cap, bank_cap = 1300, FR.SMALL_BANK                                            # `all` and firstandprevious fill this bank
    model_counts = FR.MODEL_COUNTS + [1305]                                             # the last crop is longer than its staging buffer
    bank, bguard = guarded((L, bank_cap, 3), dev)
    state = torch.zeros((2, L + 1, 2), dtype=torch.int32, device=dev)
    state[:, L] = ISENT                                                                 # the guard row of both slots
    one_bank = [torch.full((bank_cap, 3), SENT, device=dev) for _ in range(L)]
    one_state = torch.zeros((L, 2, 2), dtype=torch.int32, device=dev)
    want_bank, want_state = np.full((L, bank_cap, 3), SENT, np.float32), np.zeros((L, 2), np.int32)
    filled = False
    for s in range(1, 8):
        # lane l starts at step 1 + l % 3 (`first` mixed across the lanes); lane 1 sits out step 4, lane 2 has no crop at step 5
        t = np.array([s - l % 3 for l in range(L)])
        active = (t >= 1) & ~((np.arange(L) == 1) & (s == 4))
        first = t == 1
        has_crop = (first | (rule != "first")) & ~((np.arange(L) == 2) & (s == 5))
        lanes = LO.lane_table(L, active=active, first=first, has_crop=has_crop, t=np.maximum(t, 1))
        crop = rng.normal(size=(L, crop_cap, 3)).astype(np.float32)
        counts = np.array([model_counts[(s + 2 * l) % len(model_counts)] for l in range(L)], np.int32)
        counts[first] = model_counts[0]
        tcrop, tcounts = up(crop, dev), up(np.stack([np.full(L, 777, np.int32), counts], 1), dev)      # counts (L,2), column 1
        s_in, s_out = state[(s + 1) & 1], state[s & 1]
        before = bank.clone()
        PU.bank_update_lanes(tcrop, tcounts.view(-1)[1:], 2, bank, rule, up(lanes, dev), s_in[:L], s_out[:L])
        new_state = want_state.copy()
        LO.bank_update_lanes(want_state, crop, counts, rule, lanes, want_bank, new_state)
        want_state = new_state
        assert s_out[:L].cpu().numpy().tolist() == want_state.tolist(), (rule, s)
        assert np.array_equal(bits(bank.cpu().numpy()), bits(want_bank)), (rule, s)
        assert untouched(bguard) and untouched(state[:, L], ISENT)
        for l in range(L):
            on = bool(active[l] and has_crop[l])
            PU.bank_update(tcrop[l], tcounts[l, 1:], one_bank[l], rule, bool(first[l]), on, one_state[l, (s + 1) & 1], one_state[l, s & 1])
            assert torch.equal(one_state[l, s & 1], s_out[l]) and torch.equal(tbits(one_bank[l]), tbits(bank[l])), (rule, s, l)
            if not on:                                                                  # the state copied through, nothing else written
                assert torch.equal(s_out[l], s_in[l]) and torch.equal(tbits(bank[l]), tbits(before[l])), (rule, s, l)
        filled = filled or bool((want_state[:, 1] == bank_cap).any())
    assert filled == (rule in ("all", "firstandprevious"))


@pytest.mark.parametrize("N", [1, 128, 129])
@pytest.mark.parametrize("L", LANES)
def test_motion_input_drawn_lanes_equals_the_single_entry_and_the_oracle(dev, L, N):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng([L, N])
    cap = 2048
    pool = [(2, 1500), (1500, 1313), (N, N), (700, 3000), (1, 0)]                        # zero-filled, truncated, the identity
    counts = np.array([pool[(l + N) % len(pool)] for l in range(L)], np.int32)
    wlh = rng.uniform(1.2, 4.0, (L, 3)).astype(np.float32)
    half = np.stack([wlh[:, 1], wlh[:, 0], wlh[:, 2]], 1)[:, None, :] * 1.25 / 2
    prev, cur = ((rng.uniform(-1.6, 1.6, (L, cap, 3)) * half).astype(np.float32) for _ in range(2))
    first = np.arange(L) % 2 == 0 if L > 1 else np.array([False])                        # both values in one launch
    lanes = LO.lane_table(L, first=first)
    tp, tc, tw, tn, tl = up(prev, dev), up(cur, dev), up(wlh, dev), up(counts, dev), up(lanes, dev)
    keys = FO.keys(5)
    for with_bc in (True, False):
        pts, pguard = guarded((L, 2 * N, 5), dev)
        bc, bguard = guarded((L, 2 * N, 9), dev)
        used, uguard = guarded((L, 2 * N), dev, ISENT, torch.int32)
        PU.motion_input_drawn_lanes(tp, tc, tn, keys, tw, tl, pts, bc if with_bc else False, used)
        want_pts, _, want_used = LO.motion_input_drawn_lanes(prev, cur, counts, keys, N, wlh, lanes, with_bc=False)
        assert np.array_equal(used.cpu().numpy(), want_used) and np.array_equal(bits(pts.cpu().numpy()), bits(want_pts))
        assert untouched(pguard) and untouched(bguard) and untouched(uguard, ISENT)
        if not with_bc:
            assert untouched(bc)                                                       # NULL: nothing written
        for l in range(L):
            p1, b1, u1 = torch.full((2 * N, 5), SENT, device=dev), torch.full((2 * N, 9), SENT, device=dev), torch.full((2 * N,), ISENT, dtype=torch.int32, device=dev)
            PU.motion_input_drawn(tp[l], tc[l], tn[l], keys, tw[l], bool(first[l]), p1, b1 if with_bc else False, u1)
            assert torch.equal(tbits(pts[l]), tbits(p1)) and torch.equal(used[l], u1), (L, N, l)
            assert not with_bc or torch.equal(tbits(bc[l]), tbits(b1)), (L, N, l)
    PU.motion_input_drawn_lanes(tp, tc, tn, keys, tw, tl, pts)                          # used may be NULL


def random_boxes(rng, n):
    out = np.zeros((n, 15), np.float32)
    out[:, :3], out[:, 3:6] = rng.normal(size=(n, 3)) * 5, rng.uniform(1, 4, (n, 3))
    a = rng.uniform(-3, 3, n)
    out[:, 6], out[:, 7], out[:, 9], out[:, 10], out[:, 14] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1
    return out


@pytest.mark.parametrize("use_z", [True, False])
@pytest.mark.parametrize("degrees", [True, False])
@pytest.mark.parametrize("L", LANES)
def test_offset_box_lanes_equals_the_single_entry_and_the_oracle(dev, L, degrees, use_z):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng([L, degrees, use_z])
    R, seed = 12, 11
    cur, gt = random_boxes(rng, L), random_boxes(rng, R)
    yaw = np.concatenate([cur[:, 6:], rng.uniform(-1, 1, (L, 1)).astype(np.float32)], 1)
    scale = np.array([3, 3, 3, 30 if degrees else 0.5], np.float32)
    offset = rng.normal(size=(L, 4)).astype(np.float32) * scale
    offset[0, 0], offset[L - 1, 1] = cur[0, 3] + 1, 5                                   # beyond w and beyond min(l, 2): limit_box draws
    ll = np.arange(L)
    lanes = LO.lane_table(L, active=ll != 2, t=1 + 3 * ll, row=(2 * ll + 1) % R, ref_row=np.where(ll % 2 == 1, (ll + 5) % R, -1),
                          rebase=(ll % 3 == 1), has_crop=ll % 2 == 0)                   # a different t per lane; lane 2 inactive
    counts = rng.integers(0, 5000, (L, 2)).astype(np.int32)
    tcur, tgt, toff, tl, tcounts = up(cur, dev), up(gt, dev), up(offset, dev), up(lanes, dev), up(counts, dev)
    drew = 0
    for limit_box in (False, True):
        out, oguard = guarded((L, 15), dev)
        res, rguard = guarded((R, 15), dev)
        log, lguard = guarded((R, 2), dev, ISENT, torch.int32)
        st = up(yaw, dev)
        PU.offset_box_lanes(tcur, tgt, toff, st, tl, out, res, tcounts, log, degrees=degrees, use_z=use_z, limit_box=limit_box, seed=seed)
        w_out, w_res, w_log, w_st = np.full((L, 15), SENT, np.float32), np.full((R, 15), SENT, np.float32), np.full((R, 2), ISENT, np.int32), yaw.copy()
        LO.offset_box_lanes(cur, gt, offset, w_st, lanes, w_out, w_res, counts, w_log, degrees, use_z, limit_box, seed)
        g_out, g_res, g_st = out.cpu().numpy(), res.cpu().numpy(), st.cpu().numpy()
        # against the restatement: both round the same double once -- 2 ulp of a 32 m centre, 1e-6 on the rotation, as
        # tests/test_tracking_gpu.py bounds the single entry; the rows nothing writes and the integers are exact
        assert np.abs(g_out[:, :3] - w_out[:, :3]).max() <= 4e-6 and np.abs(g_out[:, 3:] - w_out[:, 3:]).max() <= 1e-6
        assert np.abs(g_res[:, :3] - w_res[:, :3]).max() <= 4e-6 and np.abs(g_res[:, 3:] - w_res[:, 3:]).max() <= 1e-6
        assert np.abs(g_st - w_st).max() <= 1e-6
        assert np.array_equal(g_res == SENT, w_res == SENT) and np.array_equal(log.cpu().numpy(), w_log)
        assert untouched(oguard) and untouched(rguard) and untouched(lguard, ISENT)
        for l in range(L):
            row = int(lanes[l, LO.COL["row"]])
            if not lanes[l, LO.COL["active"]]:                                         # every output, state and result row at the sentinel
                assert untouched(out[l]) and untouched(res[row]) and untouched(log[row], ISENT) and np.array_equal(bits(g_st[l]), bits(yaw[l]))
                continue
            ref_row, t = int(lanes[l, LO.COL["ref_row"]]), int(lanes[l, LO.COL["t"]])
            one, one_st = torch.full((15,), SENT, device=dev), up(yaw[l], dev)
            one_res, frame = torch.full((t + 1, 15), SENT, device=dev), torch.tensor([t], dtype=torch.int32, device=dev)
            PU.offset_box(tgt[ref_row] if ref_row >= 0 else tcur[l], toff[l], out=one, yaw_state=one_st, rebase=bool(lanes[l, LO.COL["rebase"]]),
                          degrees=degrees, use_z=use_z, limit_box=limit_box, seed=seed, results=one_res, frame=frame)
            assert torch.equal(tbits(out[l]), tbits(one)) and torch.equal(tbits(res[row]), tbits(one)), (L, l, limit_box)
            assert torch.equal(tbits(st[l]), tbits(one_st)) and torch.equal(tbits(one_res[t]), tbits(one))
            assert log[row].cpu().tolist() == [counts[l, 0], counts[l, 1] if lanes[l, LO.COL["has_crop"]] else -1]
            ref = gt[ref_row] if ref_row >= 0 else cur[l]
            drew += limit_box and bool(offset[l, 0] > ref[3] or offset[l, 1] > min(ref[4], 2))
    assert drew >= 1                                                                    # the draw did happen: (seed, t[l], component)


@pytest.mark.parametrize("L", LANES)
def test_lane_start_sets_what_init_sets(dev, L):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(L)
    R = 9
    gt = random_boxes(rng, R)
    ll = np.arange(L)
    lanes = LO.lane_table(L, active=ll != 1, first=ll != 3, t=np.where(ll != 3, 1, 2), row=np.minimum(2 * ll + 1, R - 1))
    cur, cguard = guarded((L, 15), dev)
    yaw, yguard = guarded((L, 10), dev)
    wlh, wguard = guarded((L, 3), dev)
    state, sguard = guarded((L, 2), dev, ISENT, torch.int32)
    PU.lane_start(up(gt, dev), up(lanes, dev), cur, yaw, wlh, state)
    w = [np.full((L, 15), SENT, np.float32), np.full((L, 10), SENT, np.float32), np.full((L, 3), SENT, np.float32), np.full((L, 2), ISENT, np.int32)]
    LO.lane_start(gt, lanes, *w)
    for got, want in zip((cur, yaw, wlh), w):
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert np.array_equal(state.cpu().numpy(), w[3])
    assert untouched(cguard) and untouched(yguard) and untouched(wguard) and untouched(sguard, ISENT)
    assert np.array_equal(bits(cur[0].cpu().numpy()), bits(gt[0])) and state[0].tolist() == [0, 0]      # lane 0 starts at row 1 - 1
    PU.lane_start(up(gt, dev), up(lanes, dev), cur, yaw, wlh)                           # state may be NULL


# ---- the loop, teacher-forced ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FR.CASES)
def test_lane_loop_equals_one_single_tracker_per_tracklet_teacher_forced(gold, dev, case):
    """every lane against a single free-running tracker on the lane's tracklet, both set to the reference's box before every
    frame: counts, indices, bank state and network inputs bit for bit, the chosen proposal equal, the centre within the
    feature bound, wlh in bits"""
    from open3dsot_amd import tracking
    model, cfg = FR.make_model(case, dev)
    tracklets = tracklets_of(gold, case, dev)
    L = 3
    trk = tracking.lane_tracker_for(model, L, record_indices=True, use_graph=False)
    assert isinstance(trk, tracking.MotionLaneTracker if case == MOTION else tracking.LaneTracker)
    steps = trk.begin(tracklets)
    tracklet, frame = trk.schedule
    assert steps == tracklet.shape[0] == 9 and tracklet.tolist() == LO.schedule(LO.LENGTHS, L)[0]
    singles = [tracking.tracker_for(model, sampling="device", record_indices=True, use_graph=False) for _ in range(L)]
    worst = 0.0
    for s in range(steps):
        live = [(l, int(tracklet[s, l]), int(frame[s, l])) for l in range(L) if tracklet[s, l] >= 0]
        for l, j, t in live:
            if t == 1:
                singles[l].init(tracklets[j][0][0], tracklets[j][1][0])
            ref = gold["%s.f%d.ref_box" % (case, t)]
            trk.set_box(l, ref)
            singles[l].set_box(ref)
        more = trk.step()
        assert more == (s + 1 < steps)
        for l, j, t in live:
            one = singles[l]
            restarts = s + 1 < steps and frame[s + 1, l] == 1
            box = one.update(tracklets[j][0][t])
            for name in one.inputs:
                assert torch.equal(tbits(trk.inputs[name][l]), tbits(one.inputs[name][0])), (case, s, l, name)
            if case == MOTION:
                assert torch.equal(trk.counts2[l], one.counts_dev) and torch.equal(trk.used[l], one.used), (case, s, l)
            else:
                n = 2 if (t == 1 or trk.aggregation != "first") else 1
                assert torch.equal(trk.counts2[l, :n], one.counts_dev[:n]), (case, s, l)
                assert torch.equal(trk.used_t[l], one.used_t) and torch.equal(trk.used_s[l], one.used_s), (case, s, l)
                # (a lane that starts its next tracklet at step s + 1 has been restarted already: bank emptied, box replaced)
                assert restarts or torch.equal(trk.bank_state[s & 1, l], one.bank_state[t & 1]), (case, s, l)
                assert int(trk.out[1][l].item()) == int(one.out[1].item()), (case, s, l)      # the chosen proposal
            got = trk.results(j)[t]
            assert restarts or torch.equal(tbits(got), tbits(trk.cur[l]))
            d = float((got[:3] - box[:3]).abs().max())
            worst = max(worst, d)
            assert d <= FEATURE_BOUND, (case, s, l, d)
            assert torch.equal(tbits(got[3:6]), tbits(box[3:6])), (case, s, l)
            assert trk.counts(j)[t].tolist() == one.counts()[t].tolist(), (case, s, l)
    print("lanes teacher-forced %s: worst centre difference to the single trackers %.2e m" % (case, worst))
    assert not trk.step()                                                               # done: nothing more is enqueued
    for j, (frames, gt) in enumerate(tracklets):                                        # row 0: the first box, the one-frame tracklet included
        assert trk.results(j).shape == (len(frames), 15) and np.array_equal(bits(trk.results(j)[0].cpu().numpy()), bits(gt[0]))
        assert np.all(trk.counts(j)[0] == -1) and trk.counts(j).shape == (len(frames), 2)
    assert trk.overflow() == (0, 0, 0)


# ---- closed loop: graph replay, evaluate, truncation -----------------------------------------------------------------------------
_RUNS = {}


def lane_run(gold, case, dev, L=3):
    """the eager closed-loop epoch of a case on L lanes, computed once -> (tracker, result pool on the host)"""
    from open3dsot_amd import tracking
    if (case, L) not in _RUNS:
        trk = tracking.lane_tracker_for(FR.make_model(case, dev)[0], L, use_graph=False)
        _RUNS[case, L] = (trk, trk.run(tracklets_of(gold, case, dev)).cpu().numpy())
    return _RUNS[case, L]


@pytest.mark.parametrize("case", ["bat_fap", MOTION])
def test_graph_replay_equals_eager(gold, dev, case):
    from open3dsot_amd import tracking
    _, eager = lane_run(gold, case, dev)
    trk = tracking.lane_tracker_for(FR.make_model(case, dev)[0], 3, use_graph=True)
    graph = trk.run(tracklets_of(gold, case, dev)).cpu().numpy()
    assert trk.graph is not None and eager.shape == (sum(LO.LENGTHS), 15)
    assert np.array_equal(bits(graph), bits(eager))
    assert np.abs(eager[1:8, :3] - eager[0:7, :3]).max() > 1e-3                          # the box does move


@pytest.mark.parametrize("case", ["bat_fap", MOTION])
def test_no_host_stop_and_no_upload_outside_a_chunk_boundary(gold, dev, case, monkeypatch):
    from open3dsot_amd import tracking
    trk = tracking.lane_tracker_for(FR.make_model(case, dev)[0], 3, use_graph=True, plan_steps=4)
    steps = trk.begin(tracklets_of(gold, case, dev))
    assert steps == 9 and trk.uploads == 1
    trk.step()                                                                          # the capture may synchronise
    uploads = []
    with FR.host_stops(monkeypatch) as stops:
        for owner, name in ((torch.Tensor, "copy_"), (torch.Tensor, "to"), (torch.Tensor, "cuda")):
            real = getattr(owner, name)

            def counted(self, *a, _real=real, _name=name, **k):
                out = _real(self, *a, **k)
                src, dst = (a[0], self) if _name == "copy_" else (self, out)
                if torch.is_tensor(src) and not src.is_cuda and dst.is_cuda:
                    uploads.append(trk.s)
                return out
            monkeypatch.setattr(owner, name, counted)
        while trk.step():
            pass
    assert stops.calls == [], stops.calls
    assert uploads == [4, 8] and trk.uploads == 3                                       # one upload per chunk, in front of its first step
    assert np.isfinite(trk.boxes.cpu().numpy()).all()
    assert np.array_equal(bits(trk.boxes.cpu().numpy()), bits(lane_run(gold, case, dev)[1]))      # chunks of 4 change nothing


@pytest.mark.parametrize("case", ["bat_fap", MOTION])
def test_evaluate_on_lanes(gold, dev, case):
    from open3dsot_amd import metrics as MT, tracking
    model, cfg = FR.make_model(case, dev)
    tracklets = tracklets_of(gold, case, dev)
    got = tracking.evaluate(model, tracklets, sampling="device", use_graph=False, lanes=3)
    # the sequential run: what evaluate(..., sampling="device") does, tracklet by tracklet on one tracker, its results kept
    one, m_seq, sequential = tracking.tracker_for(model, sampling="device", use_graph=False), MT.SuccessPrecision(device=dev), []
    for frames, gt in tracklets:
        tracking.evaluate_sequence(model, frames, gt, tracker=one, metrics=m_seq)
        sequential.append(one.results())
    seq = m_seq.compute()
    assert got["frames"] == seq["frames"] == sum(LO.LENGTHS) and got["tracklets"] == len(sequential) == len(LO.LENGTHS)
    trk, pool = lane_run(gold, case, dev)                                               # the same epoch: the kernels are deterministic
    m = MT.SuccessPrecision(device=dev)
    MT.score_boxes(trk.gt, trk.boxes, int(cfg.get("IoU_space", 3)), tuple(cfg.get("up_axis", (0, 0, 1))), accumulate=m)
    want = m.compute()
    assert (got["success"], got["precision"]) == (want["success"], want["precision"])
    assert np.isfinite(pool).all()
    Rm = pool[:, 6:].astype(np.float64).reshape(-1, 3, 3)
    assert np.abs(np.einsum("nji,njk->nik", Rm, Rm) - np.eye(3)).max() <= 1e-5
    for j, (frames, gt) in enumerate(tracklets):
        ref, mine = sequential[j], trk.results(j).cpu().numpy()
        assert np.array_equal(bits(mine[0]), bits(ref[0]))
        d = np.linalg.norm(mine[1:, :3].astype(np.float64) - ref[1:, :3], axis=1)
        print("lanes closed loop %s tracklet %d: centre distance to the sequential run, frames 1..%d [m]: %s"
              % (case, j, len(frames) - 1, " ".join("%.2e" % v for v in d)))
        if len(frames) > 1:                                                             # frame 1: the same box, identical inputs
            assert np.abs(mine[1, :3] - ref[1, :3]).max() <= FEATURE_BOUND, (case, j)
    again = tracking.lane_tracker_for(model, 2, use_graph=False)                         # the order moves tracklets between lanes, not their rows
    again.run(tracklets, order="longest_first")
    assert again.schedule[0][0].tolist() == [0, 5] and again.results(1).shape == (1, 15)
    rows = [0, 1, 8, 9, 10]                                                             # frames 0 and 1 of tracklets 0 and 2, the one-frame tracklet
    assert np.abs(again.boxes.cpu().numpy()[rows, :3] - pool[rows, :3]).max() <= FEATURE_BOUND


@pytest.mark.parametrize("rule,back", [("previous_gt", 1), ("current_gt", 0)])
def test_reference_bb_by_ground_truth_reads_the_pool(gold, dev, rule, back):
    """reference_BB previous_gt / current_gt: the search window and the offset start from a row of the ground-truth pool -- the
    search counts are the oracle's for those boxes, and every lane equals a single tracker handed the same boxes"""
    import tracking_oracle as TO
    from open3dsot_amd import tracking, trackers
    model, cfg = FR.make_model("bat_fap", dev)
    tracklets = tracklets_of(gold, "bat_fap", dev)
    old = model.config
    model.config = trackers.make_config(dict(cfg, reference_BB=rule))
    try:
        trk = tracking.LaneTracker(model, 3, use_graph=False)
        trk.run(tracklets)
        one = tracking.SequenceTracker(model, sampling="device", use_graph=False)
        for j, (frames, gt) in enumerate(tracklets):
            want = [TO.crop(frames[t].cpu().numpy(), gt[t - back], cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)[0]
                    for t in range(1, len(frames))]
            assert trk.counts(j)[1:, 0].tolist() == want, (rule, j)
            tracking.evaluate_sequence(model, frames, gt, tracker=one)
            ref, mine = one.results(), trk.results(j).cpu().numpy()
            assert np.array_equal(bits(mine[0]), bits(ref[0])) and np.isfinite(mine).all()
            assert np.abs(mine[:, :3] - ref[:, :3]).max() <= FEATURE_BOUND, (rule, j)    # every frame restarts from a ground-truth box
            assert np.array_equal(bits(mine[:, 3:6]), bits(ref[:, 3:6]))
    finally:
        model.config = old


def test_truncation_at_the_fixed_capacities(gold, dev):
    from open3dsot_amd import tracking
    tracklets = tracklets_of(gold, "bat_fap", dev)
    model, _ = FR.make_model("bat_fap", dev)
    trk = tracking.LaneTracker(model, 3, search_capacity=1000, model_capacity=1000, bank_capacity=1500, use_graph=False)
    trk.run(tracklets)
    over_s = over_m = full = 0
    for j, n in enumerate(LO.LENGTHS):
        counts = trk.counts(j)
        assert counts.shape == (n, 2)
        if n > 1:
            assert counts[1].tolist() == [1313, 1257]                                  # counted in full, written up to the capacity
        over_s += int((counts[1:, 0] > 1000).sum())
        over_m += int((counts[1:, 1] > 1000).sum())
        state, bank = (0, 0), np.zeros((1500, 3), np.float32)
        for t in range(1, n):                                                           # the bank's transitions, from the oracle
            nm = min(int(counts[t, 1]), 1000)
            need = 2 * nm if t == 1 else state[0] + nm
            full += need > 1500
            state = FO.bank_update(state, np.zeros((nm, 3), np.float32), "firstandprevious", t == 1, True, bank, 1500)
    assert trk.overflow() == (over_s, over_m, full) and over_s >= 5 and over_m >= 5 and full >= 5
    assert np.isfinite(trk.boxes.cpu().numpy()).all()
    motion = tracking.MotionLaneTracker(FR.make_model(MOTION, dev)[0], 3, capacity=1000, use_graph=False)
    motion.run(tracklets_of(gold, MOTION, dev))
    log = np.concatenate([motion.counts(j)[1:] for j in range(len(LO.LENGTHS))])
    assert motion.overflow() == (int((log[:, 0] > 1000).sum()), int((log[:, 1] > 1000).sum()), 0) and motion.overflow()[0] >= 1
