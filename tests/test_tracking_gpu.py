"""The device-resident tracking loop on the GPU: the three kernels of csrc/track.hip against their fp32 restatement
(tests/tracking_oracle.py; the crop bit for bit) and against the reference's own run (tests/golden/ref_tracking.npz),
teacher-forced frame by frame and in closed loop."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fixture_io  # noqa: E402
import tracking_oracle as TO  # noqa: E402

pytestmark = pytest.mark.gpu
K = TO.TEST_KEYS


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_tracking.npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def gpu_crop(jobs, dev):
    """jobs: (points np, box15 np, scale, offset, mode, capacity) -> [(count, out np (capacity,3) as written)]: one call"""
    from open3dsot_amd import points_utils as PU
    dj, keep = [], []
    for pts, box, scale, offset, mode, cap in jobs:
        p = torch.from_numpy(np.ascontiguousarray(pts, np.float32).reshape(-1, 3)).to(dev)
        b = torch.from_numpy(np.asarray(box, np.float32)).to(dev)
        out = torch.full((max(cap, 1), 3), -7.0, dtype=torch.float32, device=dev)        # a sentinel: rows not written stay -7
        cnt = torch.full((1,), -1, dtype=torch.int32, device=dev)
        dj.append((p, b, scale, offset, mode, out[:cap] if cap > 0 else out[:0], cnt))
        keep.append((out, cnt))
    PU.crop_jobs(dj)
    torch.cuda.synchronize()
    return [(int(c.item()), o.cpu().numpy()) for o, c in keep]


def near_points(n, seed=5):
    """n points of a 20 000-point frame in their original order: the (n + 1) // 2 nearest the target (so that small clouds
    have survivors) and the first n // 2 of the others (so that they have points to drop)"""
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(seed, 1, 20000)
    f = frames[0]
    order = np.argsort(np.linalg.norm(f - gt[0, :3], axis=1), kind="stable")
    return f[np.sort(np.concatenate([order[:(n + 1) // 2], np.sort(order[(n + 1) // 2:])[:n // 2]]))], gt[0]


@pytest.mark.parametrize("mode", [TO.SUBWINDOW, TO.MODEL])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 20000, 120000])
def test_crop_equals_the_oracle_bit_for_bit(dev, n, mode):
    from open3dsot_amd import synth
    if n == 120000:
        frames, gt = synth.make_sequence(9, 1, n)
        pts, box = frames[0], gt[0]
    else:
        pts, box = near_points(n)
    scale, offset = (K["search_bb_scale"], K["search_bb_offset"]) if mode == TO.SUBWINDOW else (K["model_bb_scale"], 0.3)
    want_n, want = TO.crop(pts, box, scale, offset, mode)
    (got_n, got), = gpu_crop([(pts, box, scale, offset, mode, max(n, 1))], dev)
    assert got_n == want_n
    if n >= 255:
        assert 0 < want_n < n                      # a real mask: some kept, some dropped
    assert np.array_equal(bits(got[:want_n]), bits(want))            # order and coordinates
    assert np.all(got[want_n:] == -7.0)                              # nothing written behind the survivors


def test_crop_edge_cases(dev):
    pts, box = near_points(20000)
    far = box.copy()
    far[:3] += 500.0
    (n0, out0), = gpu_crop([(pts, far, 1.25, 2.0, TO.SUBWINDOW, 64)], dev)
    assert n0 == 0 and np.all(out0 == -7.0)                                              # zero survivors
    keep, _ = TO.crop_mask(pts, box, 1.25, 2.0, TO.SUBWINDOW)
    inside = pts[keep]
    for mode in (TO.SUBWINDOW, TO.MODEL):
        (n1, out1), = gpu_crop([(inside, box, 1.25, 2.0, mode, inside.shape[0])], dev)
        assert n1 == inside.shape[0]                                                     # all survivors
        assert np.array_equal(bits(out1), bits(TO.crop(inside, box, 1.25, 2.0, mode)[1]))
    want_n, want = TO.crop(pts, box, 1.25, 2.0, TO.SUBWINDOW)
    cap = want_n // 3
    (n2, out2), = gpu_crop([(pts, box, 1.25, 2.0, TO.SUBWINDOW, cap)], dev)
    assert n2 == want_n and out2.shape[0] == cap and np.array_equal(bits(out2), bits(want[:cap]))   # counted, not written
    (n3, _), = gpu_crop([(pts, box, 1.25, 2.0, TO.SUBWINDOW, 0)], dev)
    assert n3 == want_n                                                                  # capacity 0: the count alone


def test_crop_jobs_in_one_call_equal_the_jobs_run_separately(dev):
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(11, 2, 20000)
    big, gbig = synth.make_sequence(12, 1, 120000)
    jobs = [(frames[1], gt[0], 1.25, 2.0, TO.SUBWINDOW, 4096), (frames[0], gt[0], 1.25, 0.0, TO.MODEL, 4096),
            (big[0], gbig[0], 1.25, 2.0, TO.SUBWINDOW, 8192), (frames[0][:0], gt[0], 1.25, 0.0, TO.MODEL, 16)]
    for group in (jobs[:2], jobs):
        together = gpu_crop(group, dev)
        for job, (n, out) in zip(group, together):
            (n1, out1), = gpu_crop([job], dev)
            assert n == n1 and np.array_equal(bits(out), bits(out1))
            wn, want = TO.crop(*job[:5])
            assert n == wn and np.array_equal(bits(out[:wn]), bits(want))


def test_resample_gathers_and_zero_fills(dev):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(700, 3)).astype(np.float32), rng.normal(size=(300, 3)).astype(np.float32)
    ia, ib = rng.integers(0, 700, 512).astype(np.int32), rng.integers(0, 300, 1024).astype(np.int32)
    ta, tb, tia, tib = (torch.from_numpy(x).to(dev) for x in (a, b, ia, ib))
    da, db = torch.full((512, 3), 9.0, device=dev), torch.full((1, 1024, 3), 9.0, device=dev)
    PU.resample_jobs([(ta, tia, da), (tb, tib, db)])
    assert np.array_equal(da.cpu().numpy(), TO.resample(a, ia, 512)) and np.array_equal(db[0].cpu().numpy(), TO.resample(b, ib, 1024))
    PU.resample_jobs([(None, None, da), (tb, tib, db)])
    assert np.all(da.cpu().numpy() == 0) and np.array_equal(db[0].cpu().numpy(), b[ib])
    PU.resample_jobs([(ta, tia, da)])
    assert np.array_equal(da.cpu().numpy(), a[ia])


# ---- o3d_track_offset_box ----------------------------------------------------------------------------------------------------
def gpu_offset(dev, ref, off, **kw):
    from open3dsot_amd import points_utils as PU
    out = PU.offset_box(torch.from_numpy(np.asarray(ref, np.float32)).to(dev), torch.from_numpy(np.asarray(off, np.float32)).to(dev), **kw)
    return out.cpu().numpy()


def test_offset_box_equals_the_reference_boxes(gold, dev):
    """centre <= 1e-5, rotation entries <= 1e-6 against the reference's getOffsetBB; degrees and use_z both ways"""
    worst_c = worst_r = 0.0
    for case in TO.CASES:
        _, cfg = TO.case_config(case)
        for t in range(1, TO.SEQ_FRAMES):
            k = "%s.f%d." % (case, t)
            ref, off, want = gold[k + "ref_box"], gold[k + "offset"].astype(np.float32), gold[k + "result_box"]
            rad = off.copy()
            rad[3] = np.float32(np.deg2rad(np.float64(off[3])))
            flat = want.copy()                      # use_z=False: the same box without the z component of the offset
            flat[:3] -= ref[6:15].reshape(3, 3)[:, 2] * np.float64(off[2])
            for o, degrees, use_z, w in ((off, True, True, want), (rad, False, True, want), (off, True, False, flat)):
                got = gpu_offset(dev, ref, o, degrees=degrees, use_z=use_z, limit_box=False)
                dc, dr = np.abs(got[:3] - w[:3]).max(), np.abs(got[6:] - w[6:]).max()
                worst_c, worst_r = max(worst_c, dc), max(worst_r, dr)
                # radians: theta itself is rounded to fp32 on the way in, |theta| < 0.5 rad -> 3e-8 more on the rotation
                assert dc <= 1e-5 and dr <= 1e-6, (case, t, degrees, use_z, dc, dr)
                assert np.array_equal(got[3:6], w[3:6].astype(np.float32))
                lim = gpu_offset(dev, ref, o, degrees=degrees, use_z=use_z, limit_box=True)
                if not (o[0] > ref[3] or o[1] > min(ref[4], 2) or (use_z and o[2] > ref[5])):
                    assert np.array_equal(bits(lim), bits(got)), (case, t)      # limit_box not triggering: identical
                want_o, _ = TO.offset_box(ref, o, degrees, use_z, False)
                # against the restatement: both round the same double once; 2 ulp of a 32 m centre, 1e-6 on the rotation
                assert np.abs(got[:3] - want_o[:3]).max() <= 4e-6 and np.abs(got[6:] - want_o[6:]).max() <= 1e-6
    print("offset box: largest centre deviation %.3e, rotation %.3e" % (worst_c, worst_r))


def test_offset_box_limit_box_draw(dev):
    from open3dsot_amd import points_utils as PU
    _, box = near_points(1)
    R = box[6:].reshape(3, 3).astype(np.float64)
    for comp, off in ((0, [box[3] + 1.0, 0.2, 0.1, 1.0]), (1, [0.2, 2.5, 0.1, 1.0])):
        def run(seed, frame):
            fr = torch.full((1,), frame, dtype=torch.int32, device=dev)
            res = torch.zeros((frame + 1, 15), device=dev)
            out = PU.offset_box(torch.from_numpy(box).to(dev), torch.tensor(off, dtype=torch.float32, device=dev), degrees=True,
                                use_z=True, limit_box=True, seed=seed, results=res, frame=fr, out=torch.zeros(15, device=dev))
            assert int(fr.item()) == frame + 1 and torch.equal(res[frame], out)
            return (R.T @ (out.cpu().numpy()[:3].astype(np.float64) - box[:3]))
        a, b, c, d = run(3, 5), run(3, 5), run(3, 6), run(4, 5)
        assert np.array_equal(a, b)                                         # reproducible for a fixed (seed, frame)
        assert -1.0 - 1e-5 <= a[comp] < 1.0 and abs(a[comp] - float(TO.limit_draw(3, 5, comp))) <= 1e-5
        assert abs(a[1 - comp] - off[1 - comp]) <= 1e-5 and abs(a[2] - off[2]) <= 1e-5      # the others untouched
        assert a[comp] != c[comp] and a[comp] != d[comp]
    # z: set to 0, literally `offset[2] > h` without abs
    out = gpu_offset(dev, box, [0.1, 0.1, box[5] + 0.5, 0.0], degrees=True, use_z=True, limit_box=True)
    assert abs((R.T @ (out[:3].astype(np.float64) - box[:3]))[2]) <= 1e-5
    out = gpu_offset(dev, box, [0.1, 0.1, -box[5] - 0.5, 0.0], degrees=True, use_z=True, limit_box=True)
    assert abs((R.T @ (out[:3].astype(np.float64) - box[:3]))[2] + box[5] + 0.5) <= 1e-5
    draws = np.array([float(TO.limit_draw(0, f, c)) for f in range(2000) for c in (0, 1)])
    assert draws.min() >= -1 and draws.max() < 1 and abs(draws.mean()) < 0.05 and abs(draws.std() - 3 ** -0.5) < 0.03


def test_offset_box_500_chained_updates_stay_orthonormal(dev):
    from open3dsot_amd import points_utils as PU
    _, box = near_points(1)
    cur = torch.from_numpy(box).to(dev)
    state = torch.cat([cur[6:15], torch.zeros(1, device=dev)]).contiguous()
    res = torch.zeros((501, 15), device=dev)
    fr = torch.ones((1,), dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    offs = torch.from_numpy(np.concatenate([rng.uniform(-0.5, 0.5, (500, 3)), rng.uniform(-9, 9, (500, 1))], 1).astype(np.float32)).to(dev)
    for i in range(500):
        PU.offset_box(cur, offs[i], out=cur, yaw_state=state, degrees=True, use_z=True, limit_box=False, results=res, frame=fr)
    assert int(fr.item()) == 501
    Rs = res[1:, 6:].cpu().numpy().astype(np.float64).reshape(500, 3, 3)
    dev_max = np.abs(np.einsum("nji,njk->nik", Rs, Rs) - np.eye(3)).max()
    assert dev_max <= 1e-5, dev_max
    # the accumulated yaw against the fp64 sum: each of the 500 fp32 additions rounds by at most half an ulp of the running
    # yaw, so the bound comes from the largest |yaw| the chain passes through (known from the inputs, in fp64)
    run = np.cumsum(np.deg2rad(offs[:, 3].cpu().numpy().astype(np.float64)))
    yaw = run[-1]
    bound = 500 * float(np.spacing(np.float32(np.abs(run).max()))) / 2 + 1e-6
    want = box[6:].reshape(3, 3).astype(np.float64) @ np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    got = np.abs(Rs[-1] - want).max()
    print("500 chained updates: |R^T R - I| %.2e, |R - R0 Rz(sum)| %.2e (bound %.2e)" % (dev_max, got, bound))
    assert got <= bound, (got, bound)


# ---- the loop against the reference's run ------------------------------------------------------------------------------------
def make_model(case, dev):
    from open3dsot_amd import trackers
    name, cfg = TO.case_config(case)
    model = trackers.get_model(name)(trackers.make_config(cfg))
    TO.init_weights(model)
    return model.to(dev).eval(), cfg


def sequence_of(gold, case, dev):
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(int(gold[case + ".seq_seed"]), TO.SEQ_FRAMES, TO.SEQ_POINTS)
    return [torch.from_numpy(f).to(dev) for f in frames], gt


FEATURE_BOUND = 1e-4          # the project's bound on network outputs against the reference (relative to the largest entry)


@pytest.mark.parametrize("case", list(TO.CASES))
def test_teacher_forced_frames_equal_the_reference(gold, dev, case):
    """every frame t starts from the reference's box t-1: counts equal, regularised clouds <= 2e-5, BoxCloud <= 1e-4, the
    chosen proposal equal, its offset within the feature bound, the result centre within 1e-4 + 2e-5"""
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    trk = tracking.SequenceTracker(model)
    trk.init(frames[0], gt[0])
    worst = {}
    for t in range(1, TO.SEQ_FRAMES):
        k = "%s.f%d." % (case, t)
        trk.set_box(gold[k + "ref_box"])
        box = trk.update(frames[t])
        ns, nm, nt = trk.log[-1]
        assert [ns, nt] == gold[k + "counts"].tolist(), (case, t)
        d = {"template": np.abs(trk.inputs["template_points"][0].cpu().numpy() - gold[k + "template_points"]).max(),
             "search": np.abs(trk.inputs["search_points"][0].cpu().numpy() - gold[k + "search_points"]).max()}
        assert d["template"] <= 2e-5 and d["search"] <= 2e-5, (case, t, d)
        if trk.with_boxcloud:
            d["boxcloud"] = np.abs(trk.inputs["points2cc_dist_t"][0].cpu().numpy() - gold[k + "points2cc_dist_t"]).max()
            assert d["boxcloud"] <= 1e-4, (case, t, d)
        best, idx = trk.out
        props = gold[k + "proposals"]
        assert int(idx.item()) == int(props[:, 4].argmax()), (case, t)
        d["offset"] = np.abs(best[0].cpu().numpy() - gold[k + "offset"]).max() / max(1.0, np.abs(gold[k + "offset"]).max())
        d["centre"] = np.abs(box.cpu().numpy()[:3] - gold[k + "result_box"][:3]).max()
        print("%s frame %d:" % (case, t), {kk: "%.2e" % v for kk, v in d.items()})
        assert d["offset"] <= FEATURE_BOUND, (case, t, d)
        assert d["centre"] <= 1e-4 + 2e-5, (case, t, d)
        for kk, v in d.items():
            worst[kk] = max(worst.get(kk, 0.0), float(v))
    print("%s teacher-forced worst:" % case, {kk: "%.2e" % v for kk, v in worst.items()})


def by_hand(model, cfg, frames, box0, dev):
    """the loop written with the public pieces, frame by frame (firstandprevious / first / all)"""
    from open3dsot_amd import points_utils as PU, tracking
    agg = tracking._aggregation(cfg["shape_aggregation"])
    boxes = [PU.pack_box(box0, dev)]
    state = torch.cat([boxes[0][6:15], torch.zeros(1, device=dev)]).contiguous()
    for t in range(1, len(frames)):
        search = PU.generate_subwindow(frames[t], boxes[-1], cfg["search_bb_scale"], cfg["search_bb_offset"])
        if agg == "first":
            tpl, canon = PU.cropAndCenterPC(frames[0], boxes[0], offset=cfg["model_bb_offset"], scale=cfg["model_bb_scale"])
        elif agg == "firstandprevious":
            tpl, canon = PU.getModel([frames[0], frames[t - 1]], [boxes[0], boxes[t - 1]], offset=cfg["model_bb_offset"], scale=cfg["model_bb_scale"])
        else:
            tpl, canon = PU.getModel(frames[:t], boxes[:t], offset=cfg["model_bb_offset"], scale=cfg["model_bb_scale"])
        tp, _ = PU.regularize_pc(tpl, cfg["template_size"], seed=1)
        sp, _ = PU.regularize_pc(search, cfg["search_size"], seed=1)
        data = {"template_points": tp[None].contiguous(), "search_points": sp[None].contiguous()}
        if hasattr(model, "mlp_bc"):
            data["points2cc_dist_t"] = PU.get_point_to_box_distance(tp, *canon)[None]
        with torch.no_grad():
            best, _ = model.evaluate_one_sample(data)
        c, s, r = PU.getOffsetBB(PU.unpack_box(boxes[-1]), best[0], degrees=cfg["degrees"], use_z=cfg["use_z"],
                                 limit_box=cfg["limit_box"], frame=t, yaw_state=state)
        boxes.append(torch.cat([c, s, r.reshape(-1)]))
    return torch.stack(boxes).cpu().numpy()


@pytest.mark.parametrize("case", ["bat_fap", "p2b", "bat_all"])
def test_track_sequence_equals_the_public_pieces_chained_by_hand(gold, dev, case):
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    eager = tracking.track_sequence(model, frames, gt[0], use_graph=False)
    hand = by_hand(model, cfg, frames, gt[0], dev)
    assert eager.shape == (TO.SEQ_FRAMES, 15) and np.array_equal(bits(eager), bits(hand))          # bit for bit
    graph = tracking.track_sequence(model, frames, gt[0], use_graph=True)
    assert np.array_equal(bits(graph), bits(eager))                                                 # replay == eager


def test_a_second_tracker_on_the_same_model_does_not_disturb_the_first(gold, dev):
    from open3dsot_amd import synth, tracking
    model, cfg = make_model("bat_fap", dev)
    fa, ga = sequence_of(gold, "bat_fap", dev)
    fb_np, gb = synth.make_sequence(77, TO.SEQ_FRAMES, TO.SEQ_POINTS)
    fb = [torch.from_numpy(f).to(dev) for f in fb_np]
    solo_a, solo_b = tracking.track_sequence(model, fa, ga[0]), tracking.track_sequence(model, fb, gb[0])
    ta, tb = tracking.SequenceTracker(model), tracking.SequenceTracker(model)
    ta.init(fa[0], ga[0])
    tb.init(fb[0], gb[0])
    for t in range(1, TO.SEQ_FRAMES):
        ta.update(fa[t])
        tb.update(fb[t])
    assert np.array_equal(bits(ta.results()), bits(solo_a)) and np.array_equal(bits(tb.results()), bits(solo_b))
    assert not np.array_equal(solo_a, solo_b)


def test_reference_bb_from_the_caller(gold, dev):
    """reference_BB previous_gt / current_gt through ref_box: the search window and the offset start from the given box"""
    from open3dsot_amd import tracking, trackers
    model, cfg = make_model("bat_fap", dev)
    model.config = trackers.make_config(dict(cfg, reference_BB="previous_gt"))
    frames, gt = sequence_of(gold, "bat_fap", dev)
    trk = tracking.SequenceTracker(model)
    trk.init(frames[0], gt[0])
    with pytest.raises(ValueError, match="ref_box"):
        trk.update(frames[1])
    for t in range(1, 4):
        box = trk.update(frames[t], ref_box=gt[t - 1]).cpu().numpy()
        want, _ = TO.offset_box(gt[t - 1], trk.out[0][0].cpu().numpy(), cfg["degrees"], cfg["use_z"], cfg["limit_box"])
        assert np.abs(box[:3] - want[:3]).max() <= 4e-6 and np.abs(box[3:] - want[3:]).max() <= 1e-6
        assert trk.log[-1][0] == TO.crop(frames[t].cpu().numpy(), gt[t - 1], cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)[0]
    assert trk.results().shape == (4, 15)


@pytest.mark.parametrize("case", list(TO.CASES))
def test_closed_loop_follows_the_reference_trajectory(gold, dev, case):
    """No teacher: frame 1 under the teacher-forced bound; from frame 2 on the deviation compounds through the network and is
    MEASURED (printed; recorded in profiles/tracking_frontend.txt and DESIGN.md), while what the generator's margins make
    discrete -- the crop counts and the chosen proposal -- must equal the reference's at every frame."""
    from open3dsot_amd import tracking
    model, cfg = make_model(case, dev)
    frames, gt = sequence_of(gold, case, dev)
    trk = tracking.SequenceTracker(model)
    trk.init(frames[0], gt[0])
    dev_c, dev_r = [], []
    for t in range(1, TO.SEQ_FRAMES):
        k = "%s.f%d." % (case, t)
        box = trk.update(frames[t]).cpu().numpy()
        want = gold[k + "result_box"]
        dev_c.append(float(np.abs(box[:3] - want[:3]).max()))
        dev_r.append(float(np.abs(box[6:] - want[6:]).max()))
    print("closed loop %s: centre deviation per frame 1..7 [m]: %s" % (case, " ".join("%.2e" % v for v in dev_c)))
    print("closed loop %s: rotation deviation per frame 1..7: %s" % (case, " ".join("%.2e" % v for v in dev_r)))
    assert dev_c[0] <= 1e-4 + 2e-5, dev_c
    trk2 = tracking.SequenceTracker(model)
    trk2.init(frames[0], gt[0])
    for t in range(1, TO.SEQ_FRAMES):
        k = "%s.f%d." % (case, t)
        trk2.update(frames[t])
        ns, nm, nt = trk2.log[-1]
        assert [ns, nt] == gold[k + "counts"].tolist(), (case, t, dev_c)
        assert int(trk2.out[1].item()) == int(gold[k + "proposals"][:, 4].argmax()), (case, t, dev_c)
