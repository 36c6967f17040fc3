"""The multi-target tracking loop on the GPU: the three o3d_track_*_multi kernels bit for bit against the single-target entry
points, and tracking.MultiTargetTracker against the reference's own runs (tests/golden/ref_multi_tracking.npz: three targets
in shared frames) and against K SequenceTrackers."""
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
KEYS = TO.TEST_KEYS
FEATURE_BOUND = 1e-4          # the project's bound on network outputs (tests/test_tracking_gpu.py)
# the fixture's case and the other aggregation modes / P2B, pinned through the single tracker
MODES = {"bat_fap": ("BAT", {}), "bat_first": ("BAT", {"shape_aggregation": "first"}),
         "bat_previous": ("BAT", {"shape_aggregation": "previous"}), "bat_all": ("BAT", {"shape_aggregation": "all"}),
         "p2b": ("P2B", {})}


@pytest.fixture(scope="module")
def gold():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_multi_tracking.npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scene(gold, dev):
    """the fixture's scene: (frames on the device, gt (T,K,15))"""
    from open3dsot_amd import synth
    frames, gt = synth.make_scene(int(gold["scene_seed"]), int(gold["n_frames"]), int(gold["n_points"]), int(gold["n_targets"]))
    return [torch.from_numpy(f).to(dev) for f in frames], gt


_MODELS = {}


def make_model(mode, dev):
    from open3dsot_amd import trackers
    if mode not in _MODELS:
        name, over = MODES[mode]
        cfg = dict(trackers.BAT_CAR if name == "BAT" else trackers.P2B_CAR)
        cfg.update(KEYS)
        cfg.update(over)
        model = trackers.get_model(name)(trackers.make_config(cfg))
        TO.init_weights(model)
        _MODELS[mode] = (model.to(dev).eval(), cfg)
    return _MODELS[mode]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def tbits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def near_points(n, seed=5):
    """tests/test_tracking_gpu.py::near_points: n points of a 20 000-point frame in their original order, half of them the
    nearest to the target (around its crop planes), half of them from the rest"""
    from open3dsot_amd import synth
    frames, gt = synth.make_sequence(seed, 1, 20000)
    f = frames[0]
    order = np.argsort(np.linalg.norm(f - gt[0, :3], axis=1), kind="stable")
    return f[np.sort(np.concatenate([order[:(n + 1) // 2], np.sort(order[(n + 1) // 2:])[:n // 2]]))], gt[0]


# ---- o3d_track_crop_multi ------------------------------------------------------------------------------------------------------
def turned(box, dx, deg):
    """the box moved by dx along x and turned by deg about z"""
    b = np.array(box, np.float64)
    a = np.deg2rad(deg)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    b[0] += dx
    b[6:] = (rz @ b[6:].reshape(3, 3)).reshape(-1)
    return b.astype(np.float32)


def target_set(pts, box, K):
    """K targets (box, scale, offset, mode, capacity) with the modes mixed.  From K = 3 on: target 1 keeps nothing and
    target 2 repeats target 0; from K = 5 on: target 3's survivors exceed its capacity."""
    n = max(pts.shape[0], 1)
    out = []
    for k in range(K):
        mode = TO.MODEL if k % 2 else TO.SUBWINDOW
        scale, offset = (KEYS["search_bb_scale"], KEYS["search_bb_offset"]) if mode == TO.SUBWINDOW else (KEYS["model_bb_scale"], 0.3)
        out.append([turned(box, 0.11 * k, 3.0 * k), scale, offset, mode, n])
    if K >= 3:
        far = box.copy()
        far[:3] += 500.0
        out[1][0] = far
        out[2] = list(out[0])
    if K >= 5:
        want = TO.crop(pts, *out[3][:4])[0]
        out[3][4] = want // 3
    return [tuple(t) for t in out]


def device_targets(targets, dev):
    """-> [(box, scale, offset, mode, out view (capacity,3), count, whole out buffer)] with sentinel fills"""
    res = []
    for box, scale, offset, mode, cap in targets:
        whole = torch.full((max(cap, 1) + 2, 3), -7.0, dtype=torch.float32, device=dev)     # rows not written stay -7
        cnt = torch.full((1,), -1, dtype=torch.int32, device=dev)
        res.append((torch.from_numpy(np.asarray(box, np.float32)).to(dev), scale, offset, mode, whole[:cap], cnt, whole))
    return res


def crop_single(pts_dev, targets, dev):
    """every target as its own o3d_track_crop call -> [(count, whole out buffer as written)]"""
    from open3dsot_amd import points_utils as PU
    dt = device_targets(targets, dev)
    for b, scale, offset, mode, out, cnt, _ in dt:
        PU.crop_jobs([(pts_dev, b, scale, offset, mode, out, cnt)])
    torch.cuda.synchronize()
    return [(int(d[5].item()), d[6].cpu().numpy()) for d in dt]


def crop_multi(groups, dev):
    """groups: [(points on the device, targets)] in ONE o3d_track_crop_multi call -> per group [(count, whole out buffer)]"""
    from open3dsot_amd import points_utils as PU
    dts = [device_targets(targets, dev) for _, targets in groups]
    tabs = [PU.crop_target_table([d[:6] for d in dt], dev) for dt in dts]
    PU.crop_multi([(p, tab) for (p, _), tab in zip(groups, tabs)])
    torch.cuda.synchronize()
    return [[(int(d[5].item()), d[6].cpu().numpy()) for d in dt] for dt in dts]


def assert_same_crops(got, want, what):
    assert len(got) == len(want)
    for k, ((gn, gout), (wn, wout)) in enumerate(zip(got, want)):
        assert gn == wn, (what, k, gn, wn)
        assert np.array_equal(bits(gout), bits(wout)), (what, k)


@pytest.mark.parametrize("K", [1, 3, 5, 33])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1031])
def test_crop_multi_equals_k_single_crops_bit_for_bit(dev, n, K):
    from open3dsot_amd import points_utils as PU
    assert K != 33 or K == PU.CROP_MULTI_CHUNK + 1            # one more target than the kernel stages in LDS at a time
    pts, box = near_points(n)
    targets = target_set(pts, box, K)
    p = torch.from_numpy(pts).to(dev)
    want = crop_single(p, targets, dev)
    (got,) = crop_multi([(p, targets)], dev)
    assert_same_crops(got, want, (n, K))
    counts = [c for c, _ in got]
    if n >= 255:
        assert 0 < counts[0] < n                            # a real mask: some kept, some dropped
    if K >= 3:
        assert counts[1] == 0 and np.all(got[1][1] == -7.0)                                  # keeps nothing
        assert counts[2] == counts[0] and np.array_equal(bits(got[2][1]), bits(got[0][1]))   # the same box twice
    if K >= 5:
        cap = targets[3][4]
        assert counts[3] > cap or counts[3] == 0            # counted, not written: the rows past the capacity keep the fill
        assert np.all(got[3][1][cap:] == -7.0)
        if n >= 255:
            assert counts[3] > cap > 0
    for (c, out), t in zip(got, targets):
        assert np.all(out[min(c, t[4]):] == -7.0)           # nothing written behind the survivors


def test_crop_multi_equals_the_oracle(dev):
    pts, box = near_points(1031)
    targets = target_set(pts, box, 5)
    (got,) = crop_multi([(torch.from_numpy(pts).to(dev), targets)], dev)
    for k, ((c, out), (b, scale, offset, mode, cap)) in enumerate(zip(got, targets)):
        wn, want = TO.crop(pts, b, scale, offset, mode, capacity=cap)
        assert c == wn and np.array_equal(bits(out[:min(wn, cap)]), bits(want)), k


def test_crop_multi_two_groups_in_one_call_equal_two_calls(dev):
    pa, box_a = near_points(1031)
    pb, box_b = near_points(257, seed=6)
    ta, tb = target_set(pa, box_a, 5), target_set(pb, box_b, 3)
    da, db = torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev)
    together = crop_multi([(da, ta), (db, tb)], dev)
    (alone_a,), (alone_b,) = crop_multi([(da, ta)], dev), crop_multi([(db, tb)], dev)
    assert_same_crops(together[0], alone_a, "group 0")
    assert_same_crops(together[1], alone_b, "group 1")
    assert_same_crops(together[1], crop_single(db, tb, dev), "group 1 against single crops")
    # an empty cloud in a group: its targets' counts are written as 0
    empty = crop_multi([(da, ta), (db[:0], tb)], dev)
    assert_same_crops(empty[0], alone_a, "group 0 beside an empty group")
    assert [c for c, _ in empty[1]] == [0, 0, 0] and all(np.all(o == -7.0) for _, o in empty[1])


# ---- o3d_track_resample_multi ---------------------------------------------------------------------------------------------------
def test_resample_multi_equals_resample_jobs_bit_for_bit(dev):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(700, 3)).astype(np.float32), rng.normal(size=(3, 3)).astype(np.float32)
    ia = rng.integers(0, 700, 512).astype(np.int32)
    ib = rng.integers(0, 3, 1031).astype(np.int32)
    ic = ia.copy()
    ic[[0, 17, 511]] = [-1, 700, 2 ** 31 - 1]                      # outside the source: zero rows
    ta, tb, tia, tib, tic = (torch.from_numpy(x).to(dev) for x in (a, b, ia, ib, ic))

    def outputs():      # rows of batched static inputs, as the tracker's are
        return torch.full((3, 512, 3), 9.0, device=dev), torch.full((2, 1031, 3), 9.0, device=dev)
    m512, m1031 = outputs()
    s512, s1031 = outputs()

    def jobs(d512, d1031):
        return [(ta, tia, d512[0]), (None, None, d512[1]), (ta, tic, d512[2]), (tb, tib, d1031[0]), (None, None, d1031[1])]
    PU.resample_multi(PU.resample_job_table(jobs(m512, m1031), dev))
    for job in jobs(s512, s1031):
        PU.resample_jobs([job])
    torch.cuda.synchronize()
    assert torch.equal(tbits(m512), tbits(s512)) and torch.equal(tbits(m1031), tbits(s1031))
    got = m512.cpu().numpy()
    assert np.array_equal(got[0], a[ia]) and np.all(got[1] == 0)
    assert np.all(got[2][[0, 17, 511]] == 0) and np.array_equal(got[2][1:17], a[ia[1:17]])
    assert np.array_equal(m1031[0].cpu().numpy(), b[ib]) and np.all(m1031[1].cpu().numpy() == 0)
    # the first n_jobs records only
    m512b, m1031b = outputs()
    PU.resample_multi(PU.resample_job_table(jobs(m512b, m1031b), dev), 2)
    assert torch.equal(tbits(m512b[:2]), tbits(s512[:2])) and bool((m512b[2] == 9.0).all()) and bool((m1031b == 9.0).all())


# ---- o3d_track_offset_box_multi -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degrees", [True, False])
@pytest.mark.parametrize("use_z", [True, False])
def test_offset_box_multi_equals_four_single_chains_bit_for_bit(dev, degrees, use_z):
    """20 chained updates of 4 targets: limit_box with seeds seed + k (offsets beyond w / min(l, 2) / h among them), a per-target
    rebase at two steps, target 3 retired from step 10 on (and handed another ref at step 13: it goes to out unchanged)"""
    from open3dsot_amd import points_utils as PU
    K, steps, seed = 4, 20, 11
    _, box = near_points(1)
    rng = np.random.default_rng(3)
    boxes0 = np.stack([turned(box, 1.5 * k, 20.0 * k) for k in range(K)])
    offs = np.concatenate([rng.uniform(-0.5, 0.5, (steps, K, 3)), rng.uniform(-9, 9, (steps, K, 1))], 2).astype(np.float32)
    offs[rng.uniform(size=(steps, K)) < 0.3, 0] = 2.5          # > w: replaced by the draw
    offs[rng.uniform(size=(steps, K)) < 0.3, 1] = 2.25         # > min(l, 2)
    offs[rng.uniform(size=(steps, K)) < 0.3, 2] = 1.9          # > h: set to 0 when use_z
    if not degrees:
        offs[..., 3] = np.deg2rad(offs[..., 3])
    rebase_at = {7: [0, 1, 0, 0], 13: [1, 0, 0, 1]}
    retire_from = 10

    cur = torch.from_numpy(boxes0).to(dev)
    state = torch.cat([cur[:, 6:15], torch.zeros((K, 1), device=dev)], 1).contiguous()
    res = torch.zeros((steps + 1, K, 15), device=dev)
    fr = torch.ones((1,), dtype=torch.int32, device=dev)
    active = torch.ones((K,), dtype=torch.int32, device=dev)
    s_cur = [torch.from_numpy(boxes0[k]).to(dev) for k in range(K)]
    s_state = [state[k].clone() for k in range(K)]
    s_res = [torch.zeros((steps + 1, 15), device=dev) for _ in range(K)]
    s_fr = [torch.ones((1,), dtype=torch.int32, device=dev) for _ in range(K)]
    kw = dict(degrees=degrees, use_z=use_z, limit_box=True)
    for i in range(steps):
        if i == retire_from:
            active[3] = 0
        rb = rebase_at.get(i)
        ref = cur.clone()
        if rb is not None:
            for k in range(K):
                if rb[k]:
                    ref[k] = torch.from_numpy(turned(boxes0[k], 0.3 * i, 7.0 * i)).to(dev)
        off = torch.from_numpy(offs[i]).to(dev)
        PU.offset_box_multi(ref, off, yaw_state=state, out=cur, results=res, frame=fr,
                            rebase=torch.tensor(rb, dtype=torch.int32, device=dev) if rb is not None else None,
                            active=active, seed=seed, **kw)
        for k in range(K):
            if k == 3 and i >= retire_from:                 # a retired target: its ref unchanged to out and to its row
                s_cur[k].copy_(ref[k])
                s_res[k][i + 1].copy_(ref[k])
                continue
            PU.offset_box(ref[k].contiguous(), off[k].contiguous(), out=s_cur[k], yaw_state=s_state[k], rebase=bool(rb and rb[k]),
                          seed=seed + k, results=s_res[k], frame=s_fr[k], **kw)
        for k in range(K):
            assert torch.equal(tbits(cur[k]), tbits(s_cur[k])), (i, k)
            assert torch.equal(tbits(state[k]), tbits(s_state[k])), (i, k)
    assert int(fr.item()) == steps + 1
    for k in range(K):
        assert torch.equal(tbits(res[:, k]), tbits(s_res[k])), k
    # the retired target repeats its box (ref is its own last box) until step 13 hands it another ref, then repeats that one;
    # its yaw state stays where it was at retirement (compared with s_state[3], which no launch touches after step 9)
    r3 = res[:, 3].cpu().numpy()
    assert all(np.array_equal(r3[i], r3[retire_from]) for i in range(retire_from, 14)) and not np.array_equal(r3[1], r3[retire_from])
    assert all(np.array_equal(bits(r3[i]), bits(turned(boxes0[3], 0.3 * 13, 7.0 * 13))) for i in range(14, steps + 1))
    assert not np.array_equal(res[steps, 0].cpu().numpy(), res[retire_from, 0].cpu().numpy())
    # the draws differ between the targets: seed + k
    assert len({float(TO.limit_draw(seed + k, 1, 0)) for k in range(K)}) == K
    # without a results buffer: out alone
    out = PU.offset_box_multi(cur, torch.from_numpy(offs[0]).to(dev), seed=seed, **kw)
    for k in range(K):
        assert torch.equal(tbits(out[k]), tbits(PU.offset_box(cur[k].contiguous(), torch.from_numpy(offs[0, k]).to(dev), seed=seed + k, **kw)))


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def test_teacher_forced_frames_equal_the_reference(gold, dev, scene):
    """every target starts every frame from the reference's box: the bounds of
    tests/test_tracking_gpu.py::test_teacher_forced_frames_equal_the_reference for every target and frame"""
    from open3dsot_amd import tracking
    model, cfg = make_model("bat_fap", dev)
    frames, gt = scene
    K, T = gt.shape[1], gt.shape[0]
    trk = tracking.MultiTargetTracker(model, K)
    assert trk.init(frames[0], gt[0]).shape == (K, 15)
    worst = {}
    for t in range(1, T):
        for k in range(K):
            trk.set_box(k, gold["t%d.f%d.ref_box" % (k, t)])
        boxes = trk.update(frames[t])
        assert boxes.shape == (K, 15)
        ns, nm, nt = trk.log[-1]
        best, idx = trk.out
        for k in range(K):
            key = "t%d.f%d." % (k, t)
            assert [int(ns[k]), int(nt[k])] == gold[key + "counts"].tolist(), (k, t)
            d = {"template": np.abs(trk.inputs["template_points"][k].cpu().numpy() - gold[key + "template_points"]).max(),
                 "search": np.abs(trk.inputs["search_points"][k].cpu().numpy() - gold[key + "search_points"]).max(),
                 "boxcloud": np.abs(trk.inputs["points2cc_dist_t"][k].cpu().numpy() - gold[key + "points2cc_dist_t"]).max()}
            assert d["template"] <= 2e-5 and d["search"] <= 2e-5, (k, t, d)
            assert d["boxcloud"] <= 1e-4, (k, t, d)
            assert int(idx[k].item()) == int(gold[key + "proposals"][:, 4].argmax()), (k, t)
            d["offset"] = np.abs(best[k].cpu().numpy() - gold[key + "offset"]).max() / max(1.0, np.abs(gold[key + "offset"]).max())
            d["centre"] = np.abs(boxes[k].cpu().numpy()[:3] - gold[key + "result_box"][:3]).max()
            print("target %d frame %d:" % (k, t), {kk: "%.2e" % v for kk, v in d.items()})
            assert d["centre"] <= 1e-4 + 2e-5, (k, t, d)
            for kk, v in d.items():
                worst[kk] = max(worst.get(kk, 0.0), float(v))
    print("multi-target teacher-forced worst:", {kk: "%.2e" % v for kk, v in worst.items()})
    assert trk.results().shape == (T, K, 15)


@pytest.mark.parametrize("mode", list(MODES))
def test_batched_equals_k_single_trackers_teacher_forced(gold, dev, scene, mode):
    """on the fixture's scene, every target of the batched loop against its own SequenceTracker, both started from the same
    boxes at every frame: the network's inputs bit for bit, the chosen proposal equal, the centre within the feature bound"""
    from open3dsot_amd import tracking
    model, cfg = make_model(mode, dev)
    frames, gt = scene
    K, T = gt.shape[1], gt.shape[0]
    multi = tracking.MultiTargetTracker(model, K)
    multi.init(frames[0], gt[0])
    singles = [tracking.SequenceTracker(model) for _ in range(K)]
    for k, s in enumerate(singles):
        s.init(frames[0], gt[0, k])
    worst = 0.0
    for t in range(1, T):
        for k in range(K):
            teacher = gold["t%d.f%d.ref_box" % (k, t)]
            multi.set_box(k, teacher)
            singles[k].set_box(teacher)
        boxes = multi.update(frames[t])
        ns, nm, nt = multi.log[-1]
        for k, s in enumerate(singles):
            sbox = s.update(frames[t])
            sns, snm, snt = s.log[-1]
            assert (int(ns[k]), None if nm is None else int(nm[k]), int(nt[k])) == (sns, snm, snt), (mode, k, t)
            for name in s.inputs:
                assert torch.equal(tbits(multi.inputs[name][k]), tbits(s.inputs[name][0])), (mode, k, t, name)
            assert int(multi.out[1][k].item()) == int(s.out[1].item()), (mode, k, t)
            d = float((boxes[k, :3] - sbox[:3]).abs().max())
            worst = max(worst, d)
            assert d <= FEATURE_BOUND, (mode, k, t, d)
            assert torch.equal(tbits(boxes[k, 3:6]), tbits(sbox[3:6]))
    print("%s: largest |batched - single| centre %.3e" % (mode, worst))
    assert multi.with_boxcloud == (mode != "p2b")


def test_closed_loop_follows_the_reference_trajectories(gold, dev, scene):
    """No teacher: every target's frame 1 under the teacher-forced bound; later frames compound through the network and are
    printed, as tests/test_tracking_gpu.py::test_closed_loop_follows_the_reference_trajectory does"""
    from open3dsot_amd import tracking
    model, cfg = make_model("bat_fap", dev)
    frames, gt = scene
    K, T = gt.shape[1], gt.shape[0]
    res = tracking.track_targets(model, frames, gt[0])
    assert res.shape == (T, K, 15) and np.array_equal(bits(res[0]), bits(gt[0]))
    for k in range(K):
        dc = [float(np.abs(res[t, k, :3] - gold["t%d.f%d.result_box" % (k, t)][:3]).max()) for t in range(1, T)]
        dr = [float(np.abs(res[t, k, 6:] - gold["t%d.f%d.result_box" % (k, t)][6:]).max()) for t in range(1, T)]
        print("closed loop target %d: centre deviation per frame 1..%d [m]: %s" % (k, T - 1, " ".join("%.2e" % v for v in dc)))
        print("closed loop target %d: rotation deviation per frame 1..%d: %s" % (k, T - 1, " ".join("%.2e" % v for v in dr)))
        assert dc[0] <= 1e-4 + 2e-5, (k, dc)


def test_one_target_reproduces_the_single_tracker(gold, dev, scene):
    """K = 1 with reference_BB previous_gt: the single tracker's inputs bit for bit, the boxes within the bounds of
    tests/test_tracking_gpu.py::test_reference_bb_from_the_caller"""
    from open3dsot_amd import tracking, trackers
    name, over = MODES["bat_fap"]
    cfg = dict(trackers.BAT_CAR)
    cfg.update(KEYS)
    cfg["reference_BB"] = "previous_gt"
    model = TO.init_weights(trackers.get_model(name)(trackers.make_config(cfg))).to(dev).eval()
    frames, gt = scene
    gt1 = gt[:, 1]
    multi, single = tracking.MultiTargetTracker(model, 1), tracking.SequenceTracker(model)
    multi.init(frames[0], [gt1[0]])
    single.init(frames[0], gt1[0])
    with pytest.raises(ValueError, match="ref_boxes"):
        multi.update(frames[1])
    for t in range(1, 4):
        box = multi.update(frames[t], ref_boxes=gt1[t - 1][None]).cpu().numpy()
        single.update(frames[t], ref_box=gt1[t - 1])
        assert box.shape == (1, 15)
        for key in single.inputs:
            assert torch.equal(tbits(multi.inputs[key]), tbits(single.inputs[key])), (t, key)
        want, _ = TO.offset_box(gt1[t - 1], multi.out[0][0].cpu().numpy(), cfg["degrees"], cfg["use_z"], cfg["limit_box"])
        assert np.abs(box[0, :3] - want[:3]).max() <= 4e-6 and np.abs(box[0, 3:] - want[3:]).max() <= 1e-6
        assert int(multi.log[-1][0][0]) == TO.crop(frames[t].cpu().numpy(), gt1[t - 1], cfg["search_bb_scale"], cfg["search_bb_offset"], TO.SUBWINDOW)[0]
        assert (int(multi.log[-1][0][0]), int(multi.log[-1][2][0])) == (single.log[-1][0], single.log[-1][2])
    assert multi.results().shape == (4, 1, 15)


@pytest.mark.parametrize("mode", ["bat_fap", "p2b", "bat_all"])
def test_graph_replay_equals_the_eager_loop(dev, scene, mode):
    from open3dsot_amd import tracking
    model, cfg = make_model(mode, dev)
    frames, gt = scene
    eager = tracking.track_targets(model, frames, gt[0], use_graph=False)
    graph = tracking.track_targets(model, frames, gt[0], use_graph=True)
    assert eager.shape == (gt.shape[0], gt.shape[1], 15) and np.array_equal(bits(graph), bits(eager))
    assert not np.array_equal(eager[1], eager[0])


def test_small_capacities_grow_and_change_nothing(dev, scene):
    from open3dsot_amd import tracking
    model, cfg = make_model("bat_all", dev)
    frames, gt = scene
    K, T = gt.shape[1], gt.shape[0]
    runs = []
    for kw in ({}, dict(search_capacity=64, model_capacity=64)):
        trk = tracking.MultiTargetTracker(model, K, **kw)
        trk.init(frames[0], gt[0])
        for t in range(1, T):
            trk.update(frames[t])
        runs.append(trk)
    big, small = runs
    assert np.array_equal(bits(small.results()), bits(big.results()))
    for a, b in zip(small.log, big.log):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the log shows the re-crop: counts beyond the 64 rows the buffers started with, and more crop calls than frames
    assert max(int(e[0].max()) for e in small.log) > 64 and max(int(e[1].max()) for e in small.log) > 64
    assert small.crop_calls > T - 1 and big.crop_calls == T - 1
    assert small.search_buf.shape[1] > 64 and small.model_capacity > 64


def test_a_second_multi_tracker_on_the_same_model_does_not_disturb_the_first(gold, dev, scene):
    from open3dsot_amd import synth, tracking
    model, cfg = make_model("bat_fap", dev)
    fa, ga = scene
    K, T = ga.shape[1], ga.shape[0]
    fb_np, gb = synth.make_scene(77, T, 20000, K)
    fb = [torch.from_numpy(f).to(dev) for f in fb_np]
    solo_a, solo_b = tracking.track_targets(model, fa, ga[0]), tracking.track_targets(model, fb, gb[0])
    ta, tb = tracking.MultiTargetTracker(model, K), tracking.MultiTargetTracker(model, K)
    ta.init(fa[0], ga[0])
    tb.init(fb[0], gb[0])
    for t in range(1, T):
        ta.update(fa[t])
        tb.update(fb[t])
    assert np.array_equal(bits(ta.results()), bits(solo_a)) and np.array_equal(bits(tb.results()), bits(solo_b))
    assert not np.array_equal(solo_a, solo_b)


def test_retire_repeats_the_box_and_leaves_the_others_alone(dev, scene):
    from open3dsot_amd import tracking
    model, cfg = make_model("bat_fap", dev)
    frames, gt = scene
    K, T = gt.shape[1], gt.shape[0]
    full = tracking.track_targets(model, frames, gt[0])
    trk = tracking.MultiTargetTracker(model, K)
    trk.init(frames[0], gt[0])
    for t in range(1, T):
        if t == 3:
            trk.retire(1)
        trk.update(frames[t])
    res = trk.results()
    assert np.array_equal(bits(res[:3]), bits(full[:3]))
    assert all(np.array_equal(bits(res[t, 1]), bits(res[2, 1])) for t in range(3, T))
    assert not np.array_equal(res[3, 0], res[2, 0])
    # the other targets' inputs do not depend on target 1's box: their frame-3 boxes move within the batch's rounding
    assert np.abs(res[3, [0, 2], :3] - full[3, [0, 2], :3]).max() <= FEATURE_BOUND


def test_a_retired_target_ignores_the_callers_reference_boxes(dev, scene):
    """reference_BB previous_gt: the caller hands a box for every target at every frame; a retired target's rows still
    repeat its last box, and the other targets follow as they do when nothing is retired"""
    from open3dsot_amd import tracking, trackers
    cfg = dict(trackers.BAT_CAR)
    cfg.update(KEYS)
    cfg["reference_BB"] = "previous_gt"
    model = TO.init_weights(trackers.get_model("BAT")(trackers.make_config(cfg))).to(dev).eval()
    frames, gt = scene
    K = gt.shape[1]
    full, trk = tracking.MultiTargetTracker(model, K), tracking.MultiTargetTracker(model, K)
    full.init(frames[0], gt[0])
    trk.init(frames[0], gt[0])
    for t in range(1, 4):
        if t == 2:
            trk.retire(1)
            yaw_state = trk.yaw_state[1].clone()
        full.update(frames[t], ref_boxes=gt[t - 1])
        mine = torch.from_numpy(gt[t - 1]).to(dev)
        trk.update(frames[t], ref_boxes=mine)
        assert np.array_equal(bits(mine.cpu().numpy()), bits(gt[t - 1]))       # the caller's tensor is read only
    res, want = trk.results(), full.results()
    assert np.array_equal(bits(res[:2]), bits(want[:2]))
    assert np.array_equal(bits(res[2, 1]), bits(res[1, 1])) and np.array_equal(bits(res[3, 1]), bits(res[1, 1]))
    assert not np.array_equal(want[2, 1], want[1, 1])
    assert np.abs(res[2:, [0, 2], :3] - want[2:, [0, 2], :3]).max() <= FEATURE_BOUND
    assert torch.equal(tbits(trk.yaw_state[1]), tbits(yaw_state))
