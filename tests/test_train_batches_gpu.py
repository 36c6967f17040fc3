"""Training batches built on the device (csrc/train_batch.hip, open3dsot_amd/sampler.py) on the GPU: the grouped crop
against o3d_track_crop_multi bit for bit, the selection, the labels and the sample kernel against tests/sampler_oracle.py,
the builder teacher-forced with the reference's own draws against the reference's outputs
(tests/golden/ref_train_batches.npz), the builder with device draws, and training steps on its output."""
import os

import numpy as np
import pytest
import torch

import fixture_io
import sampler_oracle as SO
import tracking_oracle as TO
from test_train_batches_cpu import CASES, SELECT_PATTERNS, case_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_train_batches.npz"))


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def random_box(rng, spread=1.0):
    return np.concatenate([rng.uniform(-spread, spread, 3), rng.uniform(1.5, 4.0, 3), rot_z(rng.uniform(-3, 3)).reshape(-1)]).astype(np.float32)


# ---- (a) o3d_track_crop_groups against o3d_track_crop_multi, group by group, bit for bit ------------------------------------------------
def target_set(rng, n, k_targets, dev):
    """k targets for a cloud of n points: device boxes, sentinel-filled outs of capacity + 1 rows (the guard row), counts"""
    from open3dsot_amd import points_utils as PU
    boxes = torch.from_numpy(np.stack([random_box(rng) for _ in range(k_targets)])).to(dev)
    caps = [5 if k % 3 == 1 else max(n, 1) for k in range(k_targets)]          # every third target: a capacity below its count
    outs = [torch.full((c + 1, 3), SENTINEL, dtype=torch.float32, device=dev) for c in caps]
    counts = torch.full((k_targets,), -5, dtype=torch.int32, device=dev)
    tab = np.zeros(k_targets, PU.CROP_TARGET)
    for k in range(k_targets):
        mode = PU.CROP_MODEL if k % 2 else PU.CROP_SUBWINDOW
        tab[k] = (boxes[k].data_ptr(), 1.25, 0.0 if mode == PU.CROP_MODEL else 0.5, mode, outs[k].data_ptr(), caps[k],
                  counts.data_ptr() + 4 * k)
    return torch.from_numpy(tab.view(np.uint8)).to(dev), boxes, outs, counts, caps


@pytest.mark.parametrize("G", [1, 3, 7])
def test_crop_groups_equals_crop_multi(dev, G):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(100 + G)
    sizes, per_group = [0, 1, 255, 256, 257, 1000], [1, 4, 33]
    ns = [sizes[(g + G) % 6] for g in range(G)] if G < 6 else sizes + [1000]
    clouds = [torch.from_numpy(rng.uniform(-3, 3, (n, 3)).astype(np.float32)).to(dev) for n in ns]
    sets = [[target_set(np.random.default_rng(1000 * G + g), ns[g], per_group[g % 3], dev) for g in range(G)] for _ in range(2)]
    plan, dev_plan, need = PU.crop_groups_table([(clouds[g], sets[0][g][0]) for g in range(G)], dev)
    scratch = torch.full((need + 1,), 12345, dtype=torch.int32, device=dev)
    PU.crop_groups(plan, dev_plan, scratch[:need])
    for g in range(G):                                   # the yardstick: the two-group entry on this group alone
        PU.crop_multi([(clouds[g], sets[1][g][0])])
    torch.cuda.synchronize()
    assert int(scratch[need]) == 12345
    truncated = 0
    for g in range(G):
        (_, _, outs_a, counts_a, caps), (_, _, outs_b, counts_b, _) = sets[0][g], sets[1][g]
        assert torch.equal(counts_a, counts_b), g
        assert int(counts_a.min()) >= 0
        for k, (a, b) in enumerate(zip(outs_a, outs_b)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (g, k)
            assert bool((a[caps[k]] == SENTINEL).all())                        # the guard row behind the buffer
            truncated += int(counts_a[k]) > caps[k]
    if G == 7:
        assert truncated >= 3 and int(sum(int(s[3].sum()) for s in sets[0])) > 2000


# ---- (b) o3d_train_select -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SELECT_PATTERNS) + ["overflow", "wide"])
def test_select(dev, name):
    from open3dsot_amd import points_utils as PU
    if name == "overflow":
        counts, B, caps = np.array([(30, 40, 50), (5, 5, 5), (10, 100, 25)], np.int32), 3, (32, 32, 32)
    elif name == "wide":                                 # every wave of the workgroup takes part
        rng = np.random.default_rng(5)
        counts, B, caps = rng.integers(0, 60, (1024, 3)).astype(np.int32), 700, (40, 40, 40)
    else:
        counts, B, caps = np.array(SELECT_PATTERNS[name][0], np.int32), SELECT_PATTERNS[name][1], (1 << 20,) * 3
    sel = torch.full((B,), -9, dtype=torch.int32, device=dev)
    nv, over = torch.full((1,), -9, dtype=torch.int32, device=dev), torch.full((1,), -9, dtype=torch.int32, device=dev)
    PU.train_select(torch.from_numpy(counts).to(dev), B, caps, sel, nv, over)
    want = SO.select(counts, B, caps)
    assert np.array_equal(sel.cpu().numpy(), want[0]) and int(nv) == want[1] and int(over) == want[2]
    if name in SELECT_PATTERNS:
        assert want[0].tolist() == SELECT_PATTERNS[name][2]


# ---- (d) o3d_train_labels -----------------------------------------------------------------------------------------------------------------
def test_labels(dev):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(3)
    J = 300                                              # more than one workgroup
    gt = np.stack([random_box(rng, 30.0) for _ in range(J)])
    sb = gt.copy()
    sb[:, :3] += rng.normal(0, 1, (J, 3)).astype(np.float32)
    for j in range(J):
        sb[j, 6:] = (gt[j, 6:].reshape(3, 3).astype(np.float64) @ rot_z(np.deg2rad(rng.normal(0, 3)))).reshape(-1)
    tb = np.stack([random_box(rng) for _ in range(J)])
    off = rng.normal(0, 2, (J, 4)).astype(np.float32)
    outs = [torch.full((J, w), SENTINEL, dtype=torch.float32, device=dev) for w in (15, 4, 3, 15)]
    PU.train_labels(*[torch.from_numpy(x).to(dev) for x in (gt, sb, tb, off)], *outs)
    got = [o.cpu().numpy() for o in outs]
    for j in range(J):
        want = SO.labels(gt[j], sb[j], tb[j], off[j])
        for g, w in zip(got, want):
            # double inside, rounded once: one fp32 rounding of the exact value on either side
            assert np.all(np.abs(g[j] - w) <= np.spacing(np.abs(w).astype(np.float32))), j
        assert got[1][j][3] == -off[j][3] and np.array_equal(got[2][j], gt[j][3:6]) and np.array_equal(got[3][j][3:6], tb[j][3:6])


# ---- (c) o3d_train_sample against the oracle, exact ---------------------------------------------------------------------------------------
CLOUD_SIZES = [3, 20, 21, 511, 512, 513, 1025, 5000]
CAPS = (2048, 4096, 5000)


@pytest.fixture(scope="module")
def pools(dev):
    """J = 13 candidates: 8 with template and search clouds of CLOUD_SIZES rows, then an empty first part, an empty second
    part, a truncated search crop (count 6 000 > capacity 5 000), a cloud of 2 rows, and one that no row selects"""
    rng = np.random.default_rng(11)
    counts = [(n // 3, n - n // 3, n) for n in CLOUD_SIZES] + [(0, 700, 100), (700, 0, 100), (100, 100, 6000), (1, 1, 2), (50, 50, 50)]
    counts = np.array(counts, np.int32)
    J = counts.shape[0]
    host = tuple(rng.uniform(-3, 3, (J, c, 3)).astype(np.float32) for c in CAPS)
    boxes = np.stack([random_box(rng) for _ in range(J)])
    sel = np.array(list(range(J - 1)) + [-1], np.int32)
    return dict(J=J, counts=counts, host=host, boxes=boxes, sel=sel, dev=tuple(torch.from_numpy(p).to(dev) for p in host),
                counts_d=torch.from_numpy(counts).to(dev), boxes_d=torch.from_numpy(boxes).to(dev), sel_d=torch.from_numpy(sel).to(dev))


def run_sample(dev, pools, S, idx=None, seed=0, counter=0):
    from open3dsot_amd import points_utils as PU
    J = B = pools["J"]
    out = {"template_points": (B, S, 3), "search_points": (B, S, 3), "seg_label": (B, S), "box_label": (B, 4), "bbox_size": (B, 3)}
    out = {k: torch.full(v, SENTINEL, dtype=torch.float32, device=dev) for k, v in out.items()}
    used = [torch.full((B, S), -9, dtype=torch.int32, device=dev) for _ in range(2)]
    lab, size = torch.arange(4 * J, dtype=torch.float32, device=dev), torch.arange(3 * J, dtype=torch.float32, device=dev) + 0.5
    bc = torch.full((2, 15 * B), SENTINEL, dtype=torch.float32, device=dev)
    model = torch.arange(15 * J, dtype=torch.float32, device=dev) * 0.25
    idx_d = [torch.from_numpy(x).to(dev) for x in idx] if idx is not None else [None, None]
    a = PU._TrainSampleArgs(
        pools["sel_d"].data_ptr(), pools["counts_d"].data_ptr(), *[p.data_ptr() for p in pools["dev"]], *CAPS, J, B, S, S,
        idx_d[0].data_ptr() if idx is not None else None, idx_d[1].data_ptr() if idx is not None else None, seed, counter,
        pools["boxes_d"].data_ptr(), model.data_ptr(), lab.data_ptr(), size.data_ptr(), out["template_points"].data_ptr(),
        out["search_points"].data_ptr(), out["seg_label"].data_ptr(), out["box_label"].data_ptr(), out["bbox_size"].data_ptr(),
        bc.data_ptr(), used[0].data_ptr(), used[1].data_ptr())
    PU.train_sample(a, dev)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update(used_t=used[0].cpu().numpy(), used_s=used[1].cpu().numpy(), bc=bc.cpu().numpy(), model=model.cpu().numpy().reshape(J, 15))
    return got


def check_sample(got, pools, S, idx=None, seed=0, counter=0):
    want = SO.sample(pools["sel"], pools["counts"], pools["host"], CAPS, S, S, pools["boxes"], None if idx is None else idx[0],
                     None if idx is None else idx[1], seed, counter)
    for k, w in want.items():
        assert np.array_equal(got[k].view(np.int32), w.view(np.int32)), k
    J = B = pools["J"]
    live = pools["sel"] >= 0
    # the label rows the batch takes: candidate sel[r]'s, zeros for sel[r] < 0
    lab, size = np.arange(4 * J, dtype=np.float32).reshape(J, 4), np.arange(3 * J, dtype=np.float32).reshape(J, 3) + 0.5
    assert np.array_equal(got["box_label"][live], lab[pools["sel"][live]]) and not got["box_label"][~live].any()
    assert np.array_equal(got["bbox_size"][live], size[pools["sel"][live]]) and not got["bbox_size"][~live].any()
    for which, src in enumerate((got["model"], pools["boxes"])):
        b = got["bc"][which]
        rows = np.concatenate([b[:3 * B].reshape(B, 3), b[3 * B:6 * B].reshape(B, 3), b[6 * B:].reshape(B, 9)], 1)
        assert np.array_equal(rows[live], src[pools["sel"][live]]) and not rows[~live].any()
    return want


@pytest.mark.parametrize("S", [1, 64, 512])
def test_sample_device_draw(dev, pools, S):
    got = run_sample(dev, pools, S, seed=17, counter=3)
    want = check_sample(got, pools, S, seed=17, counter=3)
    for r, n in enumerate(CLOUD_SIZES):                  # the three routes, on the device's own output
        u = got["used_s"][r]
        assert u.min() >= 0 and u.max() < n
        if S < n:
            assert np.unique(u).size == S
        if S == n:
            assert np.array_equal(u, np.arange(n))
    assert (want["used_s"][10] < 5000).all() and want["used_s"][10].max() >= 0          # the truncated crop: drawn below its capacity
    assert not got["template_points"][11].any() and not got["search_points"][11].any()  # 2 rows: zeros
    assert not got["template_points"][12].any() and (got["used_t"][12] == -1).all()     # sel = -1
    if S == 512:
        assert (got["used_t"][8] >= 0).all() and (got["used_t"][9] >= 0).all()          # an empty part of the concatenation
        other = run_sample(dev, pools, S, seed=17, counter=4)
        assert not np.array_equal(other["used_s"][7], got["used_s"][7])                 # the batch counter is part of the key


def test_sample_given_indices(dev, pools):
    S = 64
    rng = np.random.default_rng(23)
    n_t = np.minimum(pools["counts"][:, 0], CAPS[0]) + np.minimum(pools["counts"][:, 1], CAPS[1])
    n_s = np.minimum(pools["counts"][:, 2], CAPS[2])
    idx = [np.stack([rng.integers(0, max(n, 1), S) for n in ns]).astype(np.int32) for ns in (n_t, n_s)]
    for i, ns in zip(idx, (n_t, n_s)):
        i[:, 5] = ns                                     # an index equal to n: a zero row
        i[:, 6] = -1
    got = run_sample(dev, pools, S, idx)
    want = check_sample(got, pools, S, idx)
    assert (want["used_t"][:8, 5] == -1).all() and not got["search_points"][:8, 5].any() and not got["seg_label"][:, 5].any()
    assert 0 < want["seg_label"].sum() < want["seg_label"].size


# ---- the builder --------------------------------------------------------------------------------------------------------------------------
def fixture_builder(ref, case, dev, **kw):
    """a builder and its J = 9 samples: the 8 samples of the fixture's case with the 500 m candidate at place 2"""
    from open3dsot_amd import sampler
    cfg, frames, gt, samples = case_inputs(ref, case)
    trk = sampler.DeviceTracklets(frames, gt, device=dev)[0]
    far_gt = gt.copy()
    far_gt[:, 0] += float(ref["far.shift"])
    far = sampler.DeviceTracklet(trk.frames, far_gt)
    keys = ["%s.s%d." % (case, s) for s in range(len(samples))]
    cand = [(trk,) + s for s in samples]
    cand.insert(2, (far,) + tuple(int(v) for v in ref["far.sample"]))
    keys.insert(2, None)
    builder = sampler.SiameseBatchBuilder(cfg, 8, candidates=9, capacity=4096, **kw)
    return builder, cand, keys, cfg


@pytest.mark.parametrize("case", list(CASES))
def test_builder_teacher_forced_matches_the_reference(ref, dev, case):
    builder, cand, keys, cfg = fixture_builder(ref, case, dev, record_indices=True)
    M, N = cfg["template_size"], cfg["search_size"]
    draws = {"offset_t": np.zeros((9, 3)), "offset_s": np.zeros((9, 3)), "idx_t": np.zeros((9, M), np.int32), "idx_s": np.zeros((9, N), np.int32)}
    for j, k in enumerate(keys):
        if k is not None:
            for name in draws:
                draws[name][j] = ref[k + name]
    batch = builder.build(cand, draws)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in batch.items()}
    assert builder.sel.cpu().tolist() == [0, 1, 3, 4, 5, 6, 7, 8]              # the 500 m candidate is skipped
    assert int(got["n_valid"][0]) == 8 and int(got["overflow"][0]) == 0
    counts = builder.counts.cpu().numpy()
    assert counts[2].tolist() == [0, 0, 0] and bool(ref["far.raises"])
    assert ("points2cc_dist_t" in got) == CASES[case]
    for r, j in enumerate(builder.sel.cpu().tolist()):
        assert np.array_equal(counts[j], ref[keys[j] + "counts"]), keys[j]
        SO.check_against_reference({k: v[r] for k, v in got.items() if v.ndim > 1}, ref, keys[j], CASES[case])
        assert np.array_equal(builder.used_t.cpu().numpy()[r], ref[keys[j] + "idx_t"])


def test_builder_device_draws(ref, dev):
    """B = 4 from J = 6 with the indices drawn on the device: reproducible, every output row a row of its crop, seg_label
    the crop test of the row, the indices those of the oracle's restatement of the draw"""
    from open3dsot_amd import sampler
    cfg, frames, gt, samples = case_inputs(ref, "bat")
    trk = sampler.DeviceTracklets(frames, gt, device=dev)[0]
    cand = [(trk,) + s for s in samples[:6]]
    runs = []
    for _ in range(2):
        b = sampler.SiameseBatchBuilder(cfg, 4, candidates=6, capacity=(1024, 4096, 4096), seed=5, record_indices=True)
        first = {k: v.clone() for k, v in b.build(cand).items()}
        second = b.build(cand)
        torch.cuda.synchronize()
        runs.append((b, first, {k: v.cpu().numpy() for k, v in second.items()}))
    (b, first, got), (_, first2, got2) = runs
    for k in got:
        assert np.array_equal(got[k], got2[k]) and torch.equal(first[k], first2[k]), k       # same seed and counter: identical
    assert not torch.equal(first["search_points"], torch.from_numpy(got["search_points"]).to(dev))   # the counter moved on
    sel, counts = b.sel.cpu().numpy(), b.counts.cpu().numpy()
    assert sel.tolist() == [0, 1, 2, 3] and int(got["n_valid"][0]) == 6
    assert int(got["overflow"][0]) == int((counts[sel] > np.array(b.caps)).sum()) > 0             # the first-frame crop is truncated
    crops = [c.cpu().numpy() for c in b.crops]
    search_box = b._search_box.cpu().numpy()
    want = SO.sample(sel, counts, crops, b.caps, b.M, b.N, search_box, seed=5, counter=1)
    assert np.array_equal(b.used_t.cpu().numpy(), want["used_t"]) and np.array_equal(b.used_s.cpu().numpy(), want["used_s"])
    for k in ("template_points", "search_points", "seg_label"):
        assert np.array_equal(got[k], want[k]), k                                             # rows of the crops; crop_test of the row
    assert (want["used_t"] >= 0).all() and 0 < got["seg_label"].mean() < 1
    for r in range(4):
        keep, _ = TO.crop_mask(got["search_points"][r], search_box[sel[r]], 1.0, 0.0, TO.SUBWINDOW)
        assert np.array_equal(got["seg_label"][r], keep.astype(np.float32))
        assert np.abs(got["points2cc_dist_s"][r] - SO.boxcloud(got["search_points"][r], search_box[sel[r]])).max() <= 1e-4


def test_builder_writes_into_given_tensors_and_sampler_iterates(ref, dev):
    from open3dsot_amd import dist as D, sampler
    cfg, frames, gt, _ = case_inputs(ref, "sparse")
    tracklets = sampler.DeviceTracklets([frames, frames[:5]], [gt, gt[:5]], device=dev)
    builder = sampler.SiameseBatchBuilder(cfg, 2, candidates=4, capacity=2048, seed=1)
    it = sampler.DeviceBatchSampler(tracklets, builder, random_sample=False)
    assert len(it) == (8 + 5) * 4 // 4
    s = [it.sample(i) for i in (0, 5, 4 * 8 + 2, 4 * 12 + 3)]
    assert [(x[0] is tracklets[0], x[1:]) for x in s] == [(True, (0, 0, 0, 0)), (True, (0, 0, 1, 1)), (False, (0, 0, 0, 2)), (False, (0, 3, 4, 3))]
    batches = list(it)
    assert len(batches) == 13 and all(int(b["n_valid"]) == 4 for b in batches)
    flat = D.FlatBatch({k: torch.zeros_like(v) for k, v in batches[0].items()})
    builder2 = sampler.SiameseBatchBuilder(cfg, 2, candidates=4, capacity=2048, seed=1)
    out = builder2.build([it.sample(i) for i in range(4)], out=flat)
    assert all(out[k] is flat[k] for k in flat)
    for k in flat:
        assert torch.equal(flat[k], batches[0][k]), k
    rnd = sampler.DeviceBatchSampler(tracklets, sampler.SiameseBatchBuilder(cfg, 2, candidates=4, capacity=2048), random_sample=True,
                                     seed=3, sample_per_epoch=2)
    assert len(list(rnd)) == 2


@pytest.mark.parametrize("graph", [False, True])
def test_training_steps_on_builder_output(ref, dev, graph):
    """three DataParallelStep steps of BAT at batch 2 on builder output, eager and captured: finite losses"""
    from open3dsot_amd import dist as D, sampler, trackers
    cfg, frames, gt, samples = case_inputs(ref, "bat")
    trk = sampler.DeviceTracklets(frames, gt, device=dev)[0]
    builder = sampler.SiameseBatchBuilder(cfg, 2, candidates=3, capacity=4096, seed=2)
    batches = [builder.build([(trk,) + s for s in samples[i:i + 3]]) for i in range(3)]
    torch.manual_seed(4)
    model = trackers.BAT().to(dev).train()
    step = D.DataParallelStep(model, optimizer=torch.optim.SGD(model.parameters(), lr=1e-3), world=1, graph=graph, graph_warmup=1,
                              require_graph=graph)
    losses = [float(step.step(batches[i], next_batch=batches[i + 1] if i < 2 else None)) for i in range(3)]
    assert (step.graph is not None) == graph, step.graph_error
    assert all(np.isfinite(l) and l > 0 for l in losses), losses
