"""M2-Track training batches built on the device (csrc/train_batch.hip, open3dsot_amd/sampler.py::MotionBatchBuilder) on the
GPU: the augmented grouped crop against o3d_track_crop_groups (records off) and against tests/motion_sampler_oracle.py
(records on) bit for bit, the per-candidate kernels against the fp64 oracle, the selection, the sample kernel, the builder
teacher-forced with the reference's own draws against the reference's outputs (tests/golden/ref_motion_batches.npz), the
builder with device draws, and training steps on its output."""
import os

import numpy as np
import pytest
import torch

import fixture_io
import motion_sampler_oracle as MSO
import sampler_oracle as SO
import tracking_oracle as TO
from test_motion_batches_cpu import CASES, SELECT_PATTERNS, case_draws, case_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.0
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_motion_batches.npz"))


def random_box(rng, spread=1.0, yaw=None):
    yaw = rng.uniform(-3, 3) if yaw is None else yaw
    return np.concatenate([rng.uniform(-spread, spread, 3), rng.uniform(1.5, 4.0, 3), MSO.rz(yaw).reshape(-1)]).astype(f32)


def up(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def aug_table(recs, dev):
    """records (None | dict) -> the CROP_AUG table on the device (uint8)"""
    from open3dsot_amd import points_utils as PU
    tab = np.zeros(len(recs), PU.CROP_AUG)
    for k, r in enumerate(recs):
        if r is not None:
            tab[k] = (r["enabled"], r["box"], r["A"], r["c"])
    return up(tab.view(np.uint8), dev)


def target_table(boxes_d, specs, counts_d, dev):
    """specs: per target (scale, offset, mode, capacity) -> (the CROP_TARGET table on the device, sentinel-filled outs with one
    guard row each)"""
    from open3dsot_amd import points_utils as PU
    outs = [torch.full((max(cap, 0) + 1, 3), SENTINEL, dtype=torch.float32, device=dev) for _, _, _, cap in specs]
    tab = np.zeros(len(specs), PU.CROP_TARGET)
    for k, (scale, offset, mode, cap) in enumerate(specs):
        tab[k] = (boxes_d[k].data_ptr(), scale, offset, mode, outs[k].data_ptr() if cap > 0 else 0, cap, counts_d.data_ptr() + 4 * k)
    return up(tab.view(np.uint8), dev), outs


def specs_for(n, K):
    """both modes, every third target with a capacity below its count"""
    from open3dsot_amd import points_utils as PU
    return [(1.25, 0.0, PU.CROP_MODEL, 5 if k % 3 == 1 else max(n, 1)) if k % 2 else (1.25, 0.5, PU.CROP_SUBWINDOW, 5 if k % 3 == 1 else max(n, 1))
            for k in range(K)]


# ---- (1) o3d_track_crop_groups_aug without an enabled record: o3d_track_crop_groups bit for bit -------------------------------------------
@pytest.mark.parametrize("K", [1, 33])
@pytest.mark.parametrize("records", ["no_array", "null_entries", "disabled"])
def test_crop_groups_aug_off_equals_crop_groups(dev, K, records):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(200 + K)
    ns = [0, 1, 255, 256, 257, 1000]
    G = len(ns)
    clouds = [up(rng.uniform(-3, 3, (n, 3)).astype(f32), dev) for n in ns]
    sides = []
    for _ in range(2):                                     # [0]: the augmented entry, [1]: the yardstick
        side = []
        for g, n in enumerate(ns):
            boxes = up(np.stack([random_box(np.random.default_rng(1000 * K + 10 * g + k)) for k in range(K)]), dev)
            counts = torch.full((K,), -5, dtype=torch.int32, device=dev)
            tab, outs = target_table(boxes, specs_for(n, K), counts, dev)
            side.append((tab, outs, counts, boxes))
        sides.append(side)
    plan, dev_plan, need = PU.crop_groups_table([(clouds[g], sides[0][g][0]) for g in range(G)], dev)
    scratch = torch.full((need + 1,), 12345, dtype=torch.int32, device=dev)
    keep = []
    if records == "no_array":
        ptrs = None
    elif records == "null_entries":
        ptrs = torch.zeros(G, dtype=torch.int64, device=dev)
    else:                                                  # enabled = 0 beside a matrix that would move every point
        junk = {"enabled": 0, "box": random_box(rng), "A": rng.normal(size=9).astype(f32), "c": rng.normal(size=3).astype(f32)}
        keep = [aug_table([junk] * K, dev) for _ in range(G)]
        ptrs = up(np.array([t.data_ptr() for t in keep], np.int64), dev)
    PU.crop_groups_aug(plan, dev_plan, ptrs, scratch[:need])
    plan_b, dev_plan_b, need_b = PU.crop_groups_table([(clouds[g], sides[1][g][0]) for g in range(G)], dev)
    scratch_b = torch.empty(need_b, dtype=torch.int32, device=dev)
    PU.crop_groups(plan_b, dev_plan_b, scratch_b)
    torch.cuda.synchronize()
    assert int(scratch[need]) == 12345 and need == need_b
    truncated = 0
    for g, n in enumerate(ns):
        (_, outs_a, counts_a, _), (_, outs_b, counts_b, _) = sides[0][g], sides[1][g]
        assert torch.equal(counts_a, counts_b) and int(counts_a.min()) >= 0, g
        for k, (a, b) in enumerate(zip(outs_a, outs_b)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (g, k)
            assert bool((a[-1] == SENTINEL).all())                              # the guard row behind the buffer
            truncated += int(counts_a[k]) > a.shape[0] - 1
    if K == 33:
        assert truncated >= 3


# ---- (2) o3d_track_crop_groups_aug with enabled records against the oracle, bit for bit ----------------------------------------------------
def crop_margin64(p, box, scale, offset, mode):
    """fp64, per point: min over the crop's inequalities of (bound - |coordinate|)"""
    b = np.asarray(box, np.float64)
    d = p - b[:3]
    w, l, h = b[3:6]
    R = b[6:].reshape(3, 3)
    m = (np.array([l, w, h]) * scale / 2 + offset - np.abs(d @ R)).min(1)
    if mode == TO.MODEL:
        m = np.minimum(m, ((np.abs(R) @ (np.array([l, w, h]) * 4 * scale / 2) + 2 * offset) - np.abs(d)).min(1))
    return m


def clear_cloud(rng, n, targets):
    """n points of U(-4, 4)^3 that lie at least 1e-3 m (fp64) from the augmentation mask of every enabled record and, moved
    or not, from the crop boundary of every target"""
    cand = rng.uniform(-4, 4, (4 * n + 64, 3)).astype(f32)
    ok = np.ones(cand.shape[0], bool)
    for box, (scale, offset, mode, _), rec in targets:
        p = cand.astype(np.float64)
        if rec is not None and rec["enabled"]:
            gb = rec["box"].astype(np.float64)
            m = crop_margin64(p, gb, 1.25, 0.0, TO.SUBWINDOW)
            ok &= np.abs(m) >= 1e-3
            moved = (p - gb[:3]) @ rec["A"].astype(np.float64).reshape(3, 3).T + rec["c"].astype(np.float64)
            p = np.where((m > 0)[:, None], moved, p)
        ok &= np.abs(crop_margin64(p, box, scale, offset, mode)) >= 1e-3
    out = cand[ok][:n]
    assert out.shape[0] == n
    return out


def test_crop_groups_aug_on_equals_the_oracle(dev):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(31)
    K = 33                                                 # the records cross an LDS chunk of 32
    groups = []
    for g, n in enumerate((1, 257, 1000, 300)):
        targets = []
        for k in range(K):
            gt = random_box(rng, 1.0)
            draw = np.array([*rng.uniform(-0.3, 0.3, 3), rng.uniform(-10, 10), k % 2, (k // 2) % 2], f32)
            new_box, rec = MSO.augment(gt, draw)
            box = random_box(rng, 1.0) if k % 5 == 4 else new_box          # mostly: the crop follows the moved box
            spec = specs_for(n, K)[k]
            if g == 3:
                rec = None                                  # the group with a NULL table
            elif k % 4 == 3:
                rec = dict(rec, enabled=0)
            if g == 1 and k == 7:                           # a disabled count-only target of capacity 0 between enabled ones
                box, spec, rec = gt, (1.0, 0.0, PU.CROP_SUBWINDOW, 0), dict(rec, enabled=0)
            targets.append((box, spec, rec))
        groups.append((clear_cloud(rng, n, targets), targets))
    tables, keep = [], []
    for pts, targets in groups:
        boxes = up(np.stack([t[0] for t in targets]), dev)
        counts = torch.full((K,), -5, dtype=torch.int32, device=dev)
        tab, outs = target_table(boxes, [t[1] for t in targets], counts, dev)
        recs = aug_table([t[2] for t in targets], dev) if targets[0][2] is not None or targets[1][2] is not None else None
        tables.append((up(pts, dev), tab, outs, counts, recs))
        keep.append(boxes)
    plan, dev_plan, need = PU.crop_groups_table([(t[0], t[1]) for t in tables], dev)
    scratch = torch.full((need + 1,), 12345, dtype=torch.int32, device=dev)
    ptrs = up(np.array([t[4].data_ptr() if t[4] is not None else 0 for t in tables], np.int64), dev)
    assert int((ptrs == 0).sum()) == 1
    PU.crop_groups_aug(plan, dev_plan, ptrs, scratch[:need])
    torch.cuda.synchronize()
    assert int(scratch[need]) == 12345
    moved_rows = 0
    for (pts, targets), (_, _, outs, counts, _) in zip(groups, tables):
        counts = counts.cpu().numpy()
        for k, (box, (scale, offset, mode, cap), rec) in enumerate(targets):
            want_n, want = MSO.crop_aug(pts, box, scale, offset, mode, rec, max(cap, 0))
            assert counts[k] == want_n, k
            got = outs[k].cpu().numpy()
            assert np.array_equal(got[:want.shape[0]].view(np.int32), want.view(np.int32)), k
            assert (got[want.shape[0]:] == SENTINEL).all()
            if rec is not None and rec["enabled"]:
                plain = TO.crop(pts, box, scale, offset, mode, max(cap, 0))
                moved_rows += plain[0] != want_n or not np.array_equal(plain[1], want)
    assert moved_rows >= 10                                 # the records did move points into and out of the crops


# ---- (3) o3d_train_augment / o3d_train_motion_labels against the fp64 oracle ------------------------------------------------------------
def within_one_ulp(got, want64):
    """|got - float32(want64)| <= one float32 ulp of it; 1e-15 on top: a sum of products of O(1) terms that cancels to zero
    is only known to the roundoff of the fp64 products on either side"""
    w = np.asarray(want64, np.float64).astype(f32)
    return np.all(np.abs(np.asarray(got, np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64) + 1e-15)


def label_inputs(rng, J, kind):
    """-> (gt (2J,15), draw (2J,6), offset (J,4)): `kind` = random | zero (zero draws) | flip (flip_x on the current frame
    only: the relative yaw lies near +-pi, kept 1e-3 away by the +-2 degree rotations)"""
    prev = np.stack([random_box(rng, 30.0) for _ in range(J)])
    this = prev.copy()
    this[:, :3] += rng.normal(0, 0.5, (J, 3)).astype(f32)
    for j in range(J):
        this[j, 6:] = (prev[j, 6:].reshape(3, 3).astype(np.float64) @ MSO.rz(np.deg2rad(rng.uniform(-3, 3)))).reshape(-1)
    gt = np.concatenate([prev, this]).astype(f32)
    draw = np.zeros((2 * J, 6), f32)
    off = np.zeros((J, 4), f32)
    if kind == "random":
        draw[:, :3], draw[:, 3] = rng.uniform(-0.3, 0.3, (2 * J, 3)), rng.uniform(-10, 10, 2 * J)
        draw[:, 4:] = rng.integers(0, 2, (2 * J, 2))
        draw[J:, 4] = draw[:J, 4]                          # the same flip_x on both frames: the relative yaw stays small
        off[:, :2], off[:, 3] = rng.uniform(-0.3, 0.3, (J, 2)), rng.uniform(-0.09, 0.09, J)
    elif kind == "flip":
        draw[:, 3] = rng.uniform(-1, 1, 2 * J)
        draw[J:, 4] = 1
        this[:, 6:] = prev[:, 6:]
        gt = np.concatenate([prev, this]).astype(f32)
        draw[J:, 3] += np.where(rng.uniform(size=J) < 0.5, 3.0, -3.0)   # |relative yaw| = pi - (1..5 degrees)
    return gt, draw, off


@pytest.mark.parametrize("J,kind,degrees", [(1, "random", False), (1024, "random", False), (300, "random", True), (64, "zero", False),
                                            (300, "flip", False), (300, "flip", True)])
def test_augment_and_labels_against_the_fp64_oracle(dev, J, kind, degrees):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(40 + J)
    gt, draw, off = label_inputs(rng, J, kind)
    out_box = torch.full((2 * J, 15), SENTINEL, dtype=torch.float32, device=dev)
    recs = torch.zeros(2 * J * PU.CROP_AUG.itemsize + 16, dtype=torch.uint8, device=dev)
    recs[-16:] = 0x5a                                      # the guard behind the records
    PU.train_augment(up(gt, dev), up(draw, dev), out_box, recs)
    ref_box = PU.offset_box_multi(out_box[:J].contiguous(), up(off, dev), degrees=degrees, use_z=False, limit_box=False)
    outs = [torch.full((J, w), SENTINEL, dtype=torch.float32, device=dev) for w in (15, 15, 15, 4, 4, 4)]
    state, size = torch.full((J,), -9, dtype=torch.int32, device=dev), torch.full((J, 3), SENTINEL, dtype=torch.float32, device=dev)
    PU.train_motion_labels(out_box[:J].contiguous(), out_box[J:].contiguous(), ref_box, degrees, 0.15, *outs, state, size)
    torch.cuda.synchronize()
    assert bool((recs[-16:] == 0x5a).all())
    got_box, got_ref = out_box.cpu().numpy(), ref_box.cpu().numpy()
    tab = recs[:-16].cpu().numpy().view(PU.CROP_AUG)
    for k in range(2 * J):
        c, R2, A = MSO.augment64(gt[k], draw[k])
        assert within_one_ulp(got_box[k][:3], c) and within_one_ulp(got_box[k][6:], R2) and within_one_ulp(tab[k]["A"], A), k
        assert np.array_equal(got_box[k][3:6], gt[k][3:6]) and tab[k]["enabled"] == 1
        assert np.array_equal(tab[k]["box"], gt[k]) and np.array_equal(tab[k]["c"], got_box[k][:3])
        if kind == "zero":
            assert np.array_equal(got_box[k], gt[k])
    names = ("this_box", "prev_box", "canon_box", "box_label", "box_label_prev", "motion_label")
    got = {n: o.cpu().numpy() for n, o in zip(names, outs)}
    state, size = state.cpu().numpy(), size.cpu().numpy()
    tol = MSO.THETA_TOL[degrees]
    near_pi = 0
    for j in range(J):
        want = MSO.motion_labels64(got_box[j], got_box[J + j], got_ref[j], degrees, 0.15)
        for n in ("this_box", "prev_box", "canon_box"):
            assert within_one_ulp(got[n][j], want[n]), (j, n)
        for n in ("box_label", "box_label_prev", "motion_label"):
            assert within_one_ulp(got[n][j][:3], want[n][:3]), (j, n)
            assert abs(float(got[n][j][3]) - want[n][3]) <= tol, (j, n, got[n][j][3], want[n][3])
        theta = abs(want["motion_label"][3]) * (np.pi / 180 if degrees else 1.0)
        assert theta < np.pi - 1e-3
        near_pi += theta > 3.0
        assert np.array_equal(size[j], got_box[J + j][3:6])
        if abs(want["motion_distance"] - 0.15) > 1e-5:     # nearer than that, the comparison may hang on the last rounding
            assert state[j] == want["motion_state_label"], j
    assert (near_pi == J) == (kind == "flip")
    if J >= 300:
        assert 0 < state.sum() < J or kind != "random"


def test_augment_slots_follow_the_table_order(dev):
    """slot_src: record k lands in the slot that names it, a negative entry gives a disabled all-zero record"""
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(5)
    gt, draw, _ = label_inputs(rng, 3, "random")
    src = np.array([4, -1, 0, 5, -1, 1, 3, 2, -1], np.int32)
    out_box = torch.full((6, 15), SENTINEL, dtype=torch.float32, device=dev)
    recs = torch.full((9 * PU.CROP_AUG.itemsize,), 0x5a, dtype=torch.uint8, device=dev)
    PU.train_augment(up(gt, dev), up(draw, dev), out_box, recs, up(src, dev))
    straight = torch.zeros(6 * PU.CROP_AUG.itemsize, dtype=torch.uint8, device=dev)
    PU.train_augment(up(gt, dev), up(draw, dev), torch.empty_like(out_box), straight)
    tab, want = recs.cpu().numpy().view(PU.CROP_AUG), straight.cpu().numpy().view(PU.CROP_AUG)
    for i, k in enumerate(src):
        assert tab[i].tobytes() == (want[k].tobytes() if k >= 0 else bytes(PU.CROP_AUG.itemsize)), i
    assert not bool((out_box == SENTINEL).any())


def test_inside_box_is_the_oracles(dev):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(8)
    box = random_box(rng)
    pts = rng.uniform(-3, 3, (1000, 3)).astype(f32)
    half = np.array([box[4], box[3], box[5]], f32) * f32(1.25) * f32(0.5)
    pts[:8] = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [0, 0, 0]], f32) * half)
    ident = np.concatenate([np.zeros(3), box[3:6], np.eye(3).reshape(-1)]).astype(f32)
    for b in (box, ident):
        got = PU.inside_box(up(pts, dev), up(b, dev), 1.25).cpu().numpy()
        assert np.array_equal(got.astype(bool), MSO.inside_box(pts, b, 1.25)[0]) and 0 < got.sum() < 1000
    assert got[:8].all()                                   # on a face, an edge, a corner of the axis-aligned box: inside (inclusive)


# ---- (4) o3d_train_select_motion ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SELECT_PATTERNS) + ["thresholds", "overflow", "wide"])
def test_select_motion(dev, name):
    from open3dsot_amd import points_utils as PU
    if name == "thresholds":
        counts, B, caps = np.array([(10, 99, 99), (11, 99, 20), (11, 0, 21), (10, 0, 21), (11, 99, 21)], np.int32), 4, (1 << 20,) * 2
    elif name == "overflow":
        counts, B, caps = np.array([(30, 40, 50), (5, 50, 50), (11, 100, 25)], np.int32), 3, (32, 32)
    elif name == "wide":                                 # J = 1024: every wave of the workgroup takes part
        rng = np.random.default_rng(5)
        counts, B, caps = rng.integers(0, 60, (1024, 3)).astype(np.int32), 700, (40, 40)
    else:
        counts, B, caps = np.array(SELECT_PATTERNS[name][0], np.int32), SELECT_PATTERNS[name][1], (1 << 20,) * 2
    sel = torch.full((B,), -9, dtype=torch.int32, device=dev)
    nv, over = torch.full((1,), -9, dtype=torch.int32, device=dev), torch.full((1,), -9, dtype=torch.int32, device=dev)
    PU.train_select_motion(up(counts, dev), B, caps, sel, nv, over)
    want = MSO.select(counts, B, caps)
    assert np.array_equal(sel.cpu().numpy(), want[0]) and int(nv) == want[1] and int(over) == want[2]
    if name in SELECT_PATTERNS:
        assert want[0].tolist() == SELECT_PATTERNS[name][2]
    if name == "thresholds":
        assert want[0].tolist() == [2, 4, 2, 4]
    if name == "overflow":
        assert want[2] == 5


# ---- (5) o3d_train_motion_sample against the oracle, exact -------------------------------------------------------------------------------
HALF_SIZES = [3, 20, 21, 511, 512, 513, 1025, 5000]
CAPS = (4096, 5000)


@pytest.fixture(scope="module")
def pools(dev):
    """J = 13 candidates: 8 whose halves have HALF_SIZES rows (the previous half reversed), then an empty previous half, a
    current half of 2 rows, a truncated current crop (count 6 000 > capacity 5 000), a candidate 0 again, and one that no row
    selects"""
    rng = np.random.default_rng(12)
    counts = [(50, HALF_SIZES[7 - i], n) for i, n in enumerate(HALF_SIZES)] + [(50, 0, 100), (50, 100, 2), (50, 100, 6000), (50, 70, 70), (50, 50, 50)]
    counts = np.array(counts, np.int32)
    J = counts.shape[0]
    host = tuple(rng.uniform(-3, 3, (J, c, 3)).astype(f32) for c in CAPS)
    boxes = [np.stack([random_box(rng) for _ in range(J)]) for _ in range(2)]
    canon = np.stack([np.concatenate([np.zeros(3), rng.uniform(1.5, 4.0, 3), np.eye(3).reshape(-1)]).astype(f32) for _ in range(J)])
    cid = np.array([j % 4 for j in range(J)], np.int32)
    cid[11] = 0
    sel = np.array(list(range(J - 1)) + [-1], np.int32)
    return dict(J=J, counts=counts, host=host, prev_box=boxes[0], this_box=boxes[1], canon=canon, cid=cid, sel=sel,
                dev={k: up(v, dev) for k, v in dict(counts=counts, p0=host[0], p1=host[1], prev_box=boxes[0], this_box=boxes[1],
                                                    canon=canon, cid=cid, sel=sel).items()})


def run_motion_sample(dev, pools, N, idx=None, seed=0, counter=0, with_bc=True):
    from open3dsot_amd import points_utils as PU
    J = B = pools["J"]
    d = pools["dev"]
    out = {"points": (B, 2 * N, 5), "candidate_bc": (B, 2 * N, 9), "box_label": (B, 4), "box_label_prev": (B, 4), "motion_label": (B, 4),
           "bbox_size": (B, 3), "bc_boxes": (2, 15 * B), "xyz": (2, B, N, 3)}
    out = {k: torch.full(v, SENTINEL, dtype=torch.float32, device=dev) for k, v in out.items()}
    seg, state = torch.full((B, 2 * N), -9, dtype=torch.int64, device=dev), torch.full((B,), -9, dtype=torch.int64, device=dev)
    used = [torch.full((B, N), -9, dtype=torch.int32, device=dev) for _ in range(2)]
    labs = [torch.arange(4 * J, dtype=torch.float32, device=dev) + 1000 * i for i in range(3)]
    cstate = (torch.arange(J, dtype=torch.int32, device=dev) % 2).contiguous()
    size = torch.arange(3 * J, dtype=torch.float32, device=dev) + 0.5
    idx_d = [up(x, dev) for x in idx] if idx is not None else [None, None]
    a = PU._TrainMotionSampleArgs(
        d["sel"].data_ptr(), d["counts"].data_ptr(), d["p0"].data_ptr(), d["p1"].data_ptr(), CAPS[0], CAPS[1], J, B, N,
        idx_d[0].data_ptr() if idx is not None else None, idx_d[1].data_ptr() if idx is not None else None, d["cid"].data_ptr(), seed, counter,
        d["prev_box"].data_ptr(), d["this_box"].data_ptr(), d["canon"].data_ptr(), labs[0].data_ptr(), labs[1].data_ptr(), labs[2].data_ptr(),
        cstate.data_ptr(), size.data_ptr(), out["points"].data_ptr(), out["candidate_bc"].data_ptr() if with_bc else None, seg.data_ptr(),
        out["box_label"].data_ptr(), out["box_label_prev"].data_ptr(), out["motion_label"].data_ptr(), state.data_ptr(),
        out["bbox_size"].data_ptr(), out["bc_boxes"].data_ptr() if with_bc else None, out["xyz"].data_ptr() if with_bc else None,
        used[0].data_ptr(), used[1].data_ptr())
    PU.train_motion_sample(a, dev)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update(seg_label=seg.cpu().numpy(), motion_state_label=state.cpu().numpy(), used_prev=used[0].cpu().numpy(), used_this=used[1].cpu().numpy())
    return got


def check_motion_sample(got, pools, N, idx=None, seed=0, counter=0, with_bc=True):
    want = MSO.sample(pools["sel"], pools["counts"], pools["host"], CAPS, N, pools["prev_box"], pools["this_box"], pools["canon"], pools["cid"],
                      None if idx is None else idx[0], None if idx is None else idx[1], seed, counter, with_bc)
    for k in ("seg_label", "used_prev", "used_this"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["points"].view(np.int32), want["points"].view(np.int32))      # xyz gathered, channels 3 and 4: bit for bit
    J = B = pools["J"]
    sel, live = pools["sel"], pools["sel"] >= 0
    if with_bc:
        assert np.abs(got["candidate_bc"] - want["candidate_bc"]).max() <= 2e-6             # sqrtf against numpy's: an ulp or two below 16 m
        assert not got["candidate_bc"][:, N:].any()
        for half in range(2):
            assert np.array_equal(got["xyz"][half], got["points"][:, half * N:(half + 1) * N, :3])
        for which, src in enumerate((pools["prev_box"], pools["this_box"])):
            b = got["bc_boxes"][which]
            rows = np.concatenate([b[:3 * B].reshape(B, 3), b[3 * B:6 * B].reshape(B, 3), b[6 * B:].reshape(B, 9)], 1)
            assert np.array_equal(rows[live], src[sel[live]]) and not rows[~live].any()
    else:
        assert (got["candidate_bc"] == SENTINEL).all() and (got["bc_boxes"] == SENTINEL).all() and (got["xyz"] == SENTINEL).all()
    for i, name in enumerate(("box_label", "box_label_prev", "motion_label")):
        lab = np.arange(4 * J, dtype=f32).reshape(J, 4) + 1000 * i
        assert np.array_equal(got[name][live], lab[sel[live]]) and not got[name][~live].any()
    size = np.arange(3 * J, dtype=f32).reshape(J, 3) + 0.5
    assert np.array_equal(got["bbox_size"][live], size[sel[live]]) and not got["bbox_size"][~live].any()
    assert np.array_equal(got["motion_state_label"][live], sel[live] % 2) and not got["motion_state_label"][~live].any()
    # candidate 0: prior 1 / 0, the others 0.8 / 0.2; time stamps 0 / 0.1; the current half's prior 0.5
    for r in np.flatnonzero(live):
        prior = set(np.unique(got["points"][r, :N, 4]).tolist())
        assert prior <= ({1.0, 0.0} if pools["cid"][sel[r]] == 0 else {float(f32(0.8)), float(f32(0.2))}), r
        assert (got["points"][r, :N, 3] == 0).all() and (got["points"][r, N:, 3] == f32(0.1)).all() and (got["points"][r, N:, 4] == 0.5).all()
    assert not got["points"][~live].any() and not got["seg_label"][~live].any() and (got["used_prev"][~live] == -1).all()
    return want


@pytest.mark.parametrize("N", [1, 64, 512])
def test_motion_sample_device_draw(dev, pools, N):
    got = run_motion_sample(dev, pools, N, seed=17, counter=3)
    want = check_motion_sample(got, pools, N, seed=17, counter=3)
    for r, n in enumerate(HALF_SIZES):                   # the three routes, on the device's own output
        for u, m in ((got["used_this"][r], n), (got["used_prev"][r], HALF_SIZES[7 - r])):
            assert u.min() >= 0 and u.max() < m
            if N < m:
                assert np.unique(u).size == N
            if N == m:
                assert np.array_equal(u, np.arange(m))
    assert (got["used_prev"][8] == -1).all() and not got["points"][8, :N, :3].any() and (got["used_this"][8] >= 0).all()      # n = 0
    assert (got["used_this"][9] == -1).all() and not got["points"][9, N:, :3].any() and (got["used_prev"][9] >= 0).all()      # n = 2
    assert (want["used_this"][10] < 5000).all() and want["used_this"][10].max() >= 0      # the truncated crop: drawn below its capacity
    if N == 512:
        assert 0 < got["seg_label"].sum() < got["seg_label"].size
        other = run_motion_sample(dev, pools, N, seed=17, counter=4)
        assert not np.array_equal(other["used_this"][7], got["used_this"][7])            # the batch counter is part of the key
        assert not np.array_equal(got["used_prev"][11], got["used_this"][11])            # and so is the cloud (both halves 70 rows)


def test_motion_sample_given_indices_and_no_boxcloud(dev, pools):
    N = 64
    rng = np.random.default_rng(23)
    ns = [np.minimum(pools["counts"][:, 1 + h], CAPS[h]) for h in range(2)]
    idx = [np.stack([rng.integers(0, max(n, 1), N) for n in m]).astype(np.int32) for m in ns]
    for i, m in zip(idx, ns):
        i[:, 5] = m                                      # an index equal to n: a zero row
        i[:, 6] = -1
    got = run_motion_sample(dev, pools, N, idx)
    want = check_motion_sample(got, pools, N, idx)
    assert (want["used_prev"][:8, 5] == -1).all() and not got["points"][:8, 5, :3].any() and not got["points"][:8, N + 6, :3].any()
    check_motion_sample(run_motion_sample(dev, pools, N, idx, with_bc=False), pools, N, idx, with_bc=False)


# ---- (6) the builder, teacher-forced with the reference's draws ---------------------------------------------------------------------------
def fixture_builder(ref, case, dev, **kw):
    """a builder and its samples: the samples of the fixture's case with the 500 m candidate at place 2 (J = one more than the
    case holds, B = what it holds)"""
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
    builder = sampler.MotionBatchBuilder(cfg, len(samples), candidates=len(samples) + 1, capacity=4096, **kw)
    return builder, cand, keys, cfg


@pytest.mark.parametrize("case", list(CASES))
def test_builder_teacher_forced_matches_the_reference(ref, dev, case):
    from open3dsot_amd import synth
    builder, cand, keys, cfg = fixture_builder(ref, case, dev, record_indices=True)
    batch = builder.build(cand, case_draws(ref, cfg, keys))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in batch.items()}
    B = len(keys) - 1
    sel = builder.sel.cpu().tolist()
    assert sel == [j for j in range(B + 1) if j != 2]                          # the 500 m candidate is skipped
    assert int(got["n_valid"][0]) == B and int(got["overflow"][0]) == 0
    counts = builder.counts.cpu().numpy()
    assert counts[2].tolist() == [0, 0, 0] and bool(ref["far.raises"])
    assert ("candidate_bc" in got) == ("prev_bc" in got) == ("this_bc" in got) == cfg["box_aware"]
    like = synth.to_torch(synth.make_motion_batch(0, B, cfg["point_sample_size"]))
    for k, v in like.items():
        if k in batch:
            assert batch[k].dtype == v.dtype and tuple(batch[k].shape) == tuple(v.shape), k
        else:
            assert k in ("candidate_bc", "prev_bc", "this_bc") and not cfg["box_aware"]
    assert set(batch) - set(like) == {"bbox_size", "n_valid", "overflow"}
    for r, j in enumerate(sel):
        k = keys[j]
        assert np.array_equal(counts[j][1:], ref[k + "counts"]), k
        assert abs(int(counts[j][0]) - int(ref[k + "inbox_count"])) <= int(ref[k + "inbox_slack"]), k
        MSO.check_against_reference({name: v[r] for name, v in got.items() if v.shape[0] == B}, ref, k, cfg)
        assert np.array_equal(builder.used_prev.cpu().numpy()[r], ref[k + "idx_prev"])
        assert np.array_equal(builder.used_this.cpu().numpy()[r], ref[k + "idx_this"])


# ---- (7) the builder with device draws ---------------------------------------------------------------------------------------------------
def test_builder_device_draws(ref, dev):
    """B = 4 from J = 6 with augmentation and indices drawn: reproducible, the counter moves the draw, the indices are those of
    the oracle's restatement of the draw, every row is a row of its crop and carries the labels of the row"""
    from open3dsot_amd import sampler
    cfg, frames, gt, samples = case_inputs(ref, "aug")
    trk = sampler.DeviceTracklets(frames, gt, device=dev)[0]
    cand = [(trk,) + s for s in samples[:6]]
    runs = []
    for _ in range(2):
        b = sampler.MotionBatchBuilder(cfg, 4, candidates=6, capacity=(1024, 4096), seed=5, record_indices=True)
        first = {k: v.clone() for k, v in b.build(cand).items()}
        second = b.build(cand)
        torch.cuda.synchronize()
        runs.append((b, first, {k: v.cpu().numpy() for k, v in second.items()}))
    (b, first, got), (_, first2, got2) = runs
    for k in got:
        assert np.array_equal(got[k], got2[k]) and torch.equal(first[k], first2[k]), k       # same seed and counter: identical
    assert not torch.equal(first["points"], torch.from_numpy(got["points"]).to(dev))          # the counter moved on
    sel, counts = b.sel.cpu().numpy(), b.counts.cpu().numpy()
    N = b.N
    assert sel.tolist() == [0, 1, 2, 3] and int(got["n_valid"][0]) == 6
    assert int(got["overflow"][0]) == int((counts[sel][:, 1:] > np.array(b.caps)).sum()) > 0   # the previous crop is truncated
    crops = [c.cpu().numpy() for c in b.crops]
    boxes = [x.cpu().numpy() for x in (b._prev_box, b._this_box, b._canon_box)]
    want = MSO.sample(sel, counts, crops, b.caps, N, *boxes, [s[3] for s in cand], seed=5, counter=1)
    assert np.array_equal(b.used_prev.cpu().numpy(), want["used_prev"]) and np.array_equal(b.used_this.cpu().numpy(), want["used_this"])
    assert np.array_equal(got["points"].view(np.int32), want["points"].view(np.int32))        # rows of the crops, and their channels
    assert np.array_equal(got["seg_label"], want["seg_label"]) and 0 < got["seg_label"].mean() < 1
    assert (want["used_prev"] >= 0).all() and (want["used_prev"] < 1024).all()
    for r in range(4):
        j = sel[r]
        assert np.abs(got["prev_bc"][r] - SO.boxcloud(got["points"][r, :N, :3], boxes[0][j])).max() <= 1e-4
        assert np.abs(got["this_bc"][r] - SO.boxcloud(got["points"][r, N:, :3], boxes[1][j])).max() <= 1e-4
    # the host draws are the Generator's: another seed, another augmentation
    other = sampler.MotionBatchBuilder(cfg, 4, candidates=6, capacity=(1024, 4096), seed=6)
    assert not torch.equal(other.build(cand)["box_label"], first["box_label"])


# ---- (8) out= and the sampler -------------------------------------------------------------------------------------------------------------
def test_builder_writes_into_given_tensors_and_sampler_iterates(ref, dev):
    from open3dsot_amd import dist as D, sampler
    cfg, frames, gt, _ = case_inputs(ref, "sparse")
    tracklets = sampler.DeviceTracklets([frames, frames[:5]], [gt, gt[:5]], device=dev)
    builder = sampler.MotionBatchBuilder(cfg, 2, candidates=4, capacity=2048, seed=1)
    it = sampler.DeviceBatchSampler(tracklets, builder)
    assert len(it) == (8 + 5) * 4 // 4
    s = [it.sample(i) for i in (0, 5, 4 * 8 + 2, 4 * 12 + 3)]
    assert [(x[0] is tracklets[0], x[1:]) for x in s] == [(True, (0, 0, 0)), (True, (0, 1, 1)), (False, (0, 0, 2)), (False, (3, 4, 3))]
    batches = list(it)
    assert len(batches) == 13 and all(int(b["n_valid"]) == 4 for b in batches)
    flat = D.FlatBatch({k: torch.zeros_like(v) for k, v in batches[0].items()})
    builder2 = sampler.MotionBatchBuilder(cfg, 2, candidates=4, capacity=2048, seed=1)
    out = builder2.build([it.sample(i) for i in range(4)], out=flat)
    assert all(out[k] is flat[k] for k in flat)
    for k in flat:
        assert torch.equal(flat[k], batches[0][k]), k
    with pytest.raises(ValueError, match="random_sample"):
        sampler.DeviceBatchSampler(tracklets, builder, random_sample=True)


# ---- (9) training -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_training_steps_on_builder_output(ref, dev, graph):
    """three DataParallelStep steps of M2TRACK at batch 2, N = 256 on builder output, eager and captured: finite losses"""
    from open3dsot_amd import dist as D, m2track, sampler
    cfg, frames, gt, samples = case_inputs(ref, "aug")
    cfg = dict(cfg, point_sample_size=256)
    trk = sampler.DeviceTracklets(frames, gt, device=dev)[0]
    builder = sampler.MotionBatchBuilder(cfg, 2, candidates=3, capacity=4096, seed=2)
    batches = [builder.build([(trk,) + s for s in samples[i:i + 3]]) for i in range(3)]
    torch.manual_seed(4)
    model = m2track.M2TRACK().to(dev).train()
    step = D.DataParallelStep(model, optimizer=torch.optim.SGD(model.parameters(), lr=1e-3), world=1, graph=graph, graph_warmup=1,
                              require_graph=graph)
    losses = [float(step.step(batches[i], next_batch=batches[i + 1] if i < 2 else None)) for i in range(3)]
    assert (step.graph is not None) == graph, step.graph_error
    assert all(np.isfinite(l) and l > 0 for l in losses), losses
