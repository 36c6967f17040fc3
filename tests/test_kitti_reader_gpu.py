"""The KITTI reader on the GPU (csrc/preload.hip, open3dsot_amd/datasets.py): the three launches against the numpy restatement
of the device rule (tests/kitti_oracle.py) bit for bit, the reader against the reference's own kittiDataset
(tests/golden/ref_kitti.npz) bit for bit, the cache, and the reader's output through DeviceBatchSampler and
tracking.evaluate_sequence."""
import os

import numpy as np
import pytest
import torch

import fixture_io
import kitti_oracle as KO
import kitti_tree
import tracking_oracle as TO
from test_kitti_reader_cpu import cases, ref_clouds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.0
INF = np.inf


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_kitti.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return kitti_tree.build(str(tmp_path_factory.mktemp("kitti") / "tree"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- (a) the kernels against the oracle -----------------------------------------------------------------------------------------------
FRAME_N = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
FRAME_BOXES = [1, 1, 0, 1, 32, 33, 65, 2, 4]             # 0, 1, 32, 33 and 65 boxes: below, at and beyond the LDS chunk of 32
CAMERA = np.array([[0.02, -0.999, 0.01, -0.004], [0.01, 0.03, -0.9995, -0.076], [0.9997, 0.02, 0.01, -0.27]], np.float64)


def kernel_case(T):
    """-> raw (rows,4) with NaN intensities, per frame its raw rows and its (k,6) float32 bounds"""
    rng = np.random.default_rng(11)
    raws, bounds = [], []
    for n, k in zip(FRAME_N, FRAME_BOXES):
        raw = rng.uniform(-10, 10, size=(n, 4)).astype(np.float32)
        raw[::3, 3] = np.nan                                # the intensity is never looked at
        b = np.concatenate([rng.uniform(-12, 0, size=(k, 3)), rng.uniform(0, 12, size=(k, 3))], 1).astype(np.float32)
        raws.append(raw)
        bounds.append(b)
    p = KO.transform(raws[-1], T)                           # the 1 000-point frame: the four special boxes
    bounds[-1][0] = [100, 100, 100, 101, 101, 101]          # keeps nothing
    bounds[-1][1] = [-INF] * 3 + [INF] * 3                  # keeps everything
    bounds[-1][2] = [p[5, 0], -INF, p[9, 2], INF, INF, INF]           # lo equal to a coordinate of points 5 (x) and 9 (z)
    bounds[-1][3] = [-INF, -INF, -INF, p[7, 0], p[8, 1], INF]         # hi equal to a coordinate of points 7 (x) and 8 (y)
    bounds[-2][1] = [-INF] * 3 + [INF] * 3                  # 257 points, all kept: survivors in two workgroups
    return raws, bounds


@pytest.mark.parametrize("mode", ["velodyne", "camera"])
def test_kernels_equal_the_oracle_bit_for_bit(dev, mode):
    from open3dsot_amd import points_utils as PU
    T = CAMERA if mode == "camera" else None
    raws, bounds = kernel_case(T)
    want = [KO.crop(raw, b, T) for raw, bs in zip(raws, bounds) for b in bs]
    B = len(want)
    # the strict compares: the points whose coordinate equals a bound are out, on both sides, and they would be in otherwise
    p = KO.transform(raws[-1], T)
    lo_box, hi_box = want[B - 2], want[B - 1]
    for i, box in ((5, lo_box), (9, lo_box), (7, hi_box), (8, hi_box)):
        assert not (bits(box) == bits(p[i])).all(1).any()
    assert 0 < lo_box.shape[0] < 1000 and 0 < hi_box.shape[0] < 1000
    assert want[B - 4].shape[0] == 0 and want[B - 3].shape[0] == 1000 and want[0].shape[0] == 0
    frames = np.zeros((len(FRAME_N), PU.PRELOAD_COLS), np.int32)
    frames[:, 0] = np.concatenate([[0], np.cumsum(FRAME_N)[:-1]])
    frames[:, 1], frames[:, 3] = FRAME_N, FRAME_BOXES
    need, wgs, nb = PU.preload_plan(frames, sum(FRAME_N))
    assert nb == B and (list(frames[:, 2]), list(frames[:, 4]), list(frames[:, 5]), need, wgs, nb) == KO.plan(FRAME_N, FRAME_BOXES)
    raw = torch.from_numpy(np.concatenate(raws)).to(dev)
    dev_frames = torch.from_numpy(frames).to(dev)
    dev_bounds = torch.from_numpy(np.concatenate(bounds)).to(dev)
    scratch = torch.full((need + 8,), -1, dtype=torch.int32, device=dev)
    counts = torch.full((B + 4,), -5, dtype=torch.int32, device=dev)
    PU.preload_count(raw, frames, dev_frames, dev_bounds, T, scratch[:need], counts[:B])
    got_counts = counts.cpu().numpy()
    assert list(got_counts[:B]) == [w.shape[0] for w in want] and (got_counts[B:] == -5).all()
    assert (scratch[need:].cpu().numpy() == -1).all()
    # every box's slice three rows after the one before: the rows between, before and after stay untouched
    first = np.cumsum([3] + [w.shape[0] + 3 for w in want[:-1]]).astype(np.int64)
    rows = int(first[-1]) + want[-1].shape[0]
    assert want[-1].shape[0] > 0
    out_row = torch.from_numpy(first).to(dev)
    for short in (0, 1):                                    # the pool as planned, then one row short of the need
        pool = torch.full((rows + 8, 3), SENTINEL, dtype=torch.float32, device=dev)
        PU.preload_scatter(raw, frames, dev_frames, dev_bounds, T, scratch[:need], out_row, pool, pool_rows=rows - short)
        got = pool.cpu().numpy()
        expect = np.full((rows + 8, 3), SENTINEL, np.float32)
        for f, w in zip(first, want):
            expect[f:f + w.shape[0]] = w
        if short:
            expect[rows - 1] = SENTINEL                     # the last survivor of the last box: not written
        assert np.array_equal(bits(got), bits(expect)), (mode, short)


def test_empty_calls_launch_nothing_and_succeed(dev):
    from open3dsot_amd import points_utils as PU
    z32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)      # noqa: E731
    zf = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)      # noqa: E731
    for n in ([], [0, 7]):                                  # no frame; frames without a box
        frames = np.zeros((len(n), PU.PRELOAD_COLS), np.int32)
        frames[:, 1] = n
        frames[:, 0] = np.concatenate([[0], np.cumsum(n)[:-1]]) if n else []
        assert PU.preload_plan(frames, sum(n)) == (0, 0, 0)
        pool = torch.full((4, 3), SENTINEL, device=dev)
        PU.preload_count(zf(sum(n), 4), frames, z32(frames.size), zf(0, 6), None, z32(0), z32(0))
        PU.preload_scatter(zf(sum(n), 4), frames, z32(frames.size), zf(0, 6), None, z32(0), torch.zeros(0, dtype=torch.int64, device=dev), pool)
        assert (pool.cpu().numpy() == SENTINEL).all()


# ---- (b) the reader against the reference ---------------------------------------------------------------------------------------------
def check_against_ref(trk, ref, name):
    want = ref_clouds(ref, name)
    assert [len(t) for t in trk] == list(ref[name + ".lengths"])
    assert trk.get_num_tracklets() == len(want) and trk.get_num_frames_total() == sum(len(w) for w in want)
    boxes = np.concatenate([t.boxes for t in trk])
    assert boxes.dtype == np.float32 and np.array_equal(boxes, ref[name + ".boxes"].astype(np.float32))
    assert np.array_equal(np.concatenate([m[2] for m in trk.meta]), ref[name + ".frames"])
    assert [m[0] for m in trk.meta] == [str(s) for s in ref[name + ".scenes"]]
    assert [m[1] for m in trk.meta] == list(ref[name + ".track_ids"])
    lo, hi = trk.pool.data_ptr(), trk.pool.data_ptr() + trk.pool.numel() * 4
    store = trk.pool.untyped_storage().data_ptr()
    for k, (t, w) in enumerate(zip(trk, want)):
        assert trk.get_num_frames_tracklet(k) == len(w)
        for f, (g, c) in enumerate(zip(t.frames, w)):
            assert g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == c.shape, (name, k, f)
            assert np.array_equal(bits(g.cpu().numpy()), bits(c)), (name, k, f)
            assert g.untyped_storage().data_ptr() == store                    # a view of the pool: nothing was copied
            if g.numel():
                assert lo <= g.data_ptr() and g.data_ptr() + g.numel() * 4 <= hi


def test_reader_equals_the_reference_bit_for_bit(dev, ref, tree):
    from open3dsot_amd import datasets as D
    for name, mode, offset, category, split in cases(ref):
        for chunk in (1, 64):
            trk = D.KittiTracklets(tree, split, category, coordinate_mode=mode, preload_offset=offset, device=dev, chunk_frames=chunk)
            check_against_ref(trk, ref, name)
    fr = trk.get_frames(0, [0, 1])
    assert len(fr) == 2 and fr[1]["pc"] is trk[0].frames[1] and fr[1]["3d_bbox"].shape == (15,)
    with pytest.raises(ValueError):
        D.KittiTracklets(tree, "traintiny", device=dev, chunk_frames=0)


def test_cache_round_trip(dev, ref, tree, tmp_path):
    from open3dsot_amd import datasets as D
    name = "camera.10.Other.traintiny"
    a = D.KittiTracklets(tree, "traintiny", "Other", coordinate_mode="camera", preload_offset=10, device=dev)
    file = str(tmp_path / "cache.dat")
    a.save(file)
    assert os.path.exists(file)                              # the name as given
    with np.load(file) as z:
        assert sorted(z.files) == ["boxes", "frames", "info", "lengths", "pool", "rows", "scene_list", "scenes", "track_ids"]
    b = D.KittiTracklets.load(file, device=dev)
    check_against_ref(b, ref, name)
    assert (b.split, b.category_name, b.coordinate_mode, b.preload_offset) == ("traintiny", "Other", "camera", 10)
    assert np.array_equal(bits(a.pool.cpu().numpy()), bits(b.pool.cpu().numpy()))
    for x, y in zip(a.boxes64, b.boxes64):
        assert np.array_equal(x, y)
    assert b.scene_list == ["0000"]


# ---- (c) plumbing ---------------------------------------------------------------------------------------------------------------------
def test_the_batch_sampler_takes_the_reader(dev, ref, tree):
    """DeviceBatchSampler over the reader's tracklets yields the batch that the fixture's clouds, uploaded by hand, yield"""
    from open3dsot_amd import datasets as D, sampler as S
    name = "velodyne.10.Car.traintiny"
    trk = D.KittiTracklets(tree, "traintiny", "Car", preload_offset=10, device=dev)
    clouds = ref_clouds(ref, name)
    ends = np.cumsum(ref[name + ".lengths"])
    boxes = np.split(ref[name + ".boxes"].astype(np.float32), ends[:-1])
    by_hand = S.DeviceTracklets([[torch.from_numpy(c.copy()) for c in w] for w in clouds], boxes, device=dev)
    batches = []
    for tracklets in (trk, by_hand):
        it = iter(S.DeviceBatchSampler(tracklets, S.SiameseBatchBuilder({}, 4, seed=3), seed=3))
        batches.append({k: v.clone() if torch.is_tensor(v) else v for k, v in next(it).items()})
    a, b = batches
    assert set(a) == set(b) and len(a) >= 5 and int(a["n_valid"]) >= 1
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].shape == b[k].shape and torch.equal(a[k].cpu().view(torch.uint8), b[k].cpu().view(torch.uint8)), k
        else:
            assert a[k] == b[k], k


def test_evaluate_sequence_takes_a_tracklet_of_the_reader(dev, tree):
    """the tracklet with the one-point frame (the missing file) and a (0,3) frame (the empty file): finite boxes come back"""
    from open3dsot_amd import datasets as D, tracking, trackers
    trk = D.KittiTracklets(tree, "traintiny", "Car", preload_offset=10, device=dev)
    t = trk[0]                                               # track 0: every frame of scene 0000
    assert [f.shape[0] for f in t.frames][3:5] == [1, 0]
    cfg = dict(trackers.BAT_CAR)
    cfg.update(TO.TEST_KEYS)
    model = TO.init_weights(trackers.get_model("BAT")(trackers.make_config(cfg))).to(dev).eval()
    ious, distances, results = tracking.evaluate_sequence(model, t.frames, t.boxes)
    assert tuple(results.shape) == (len(t), 15) and torch.isfinite(results).all()
    assert torch.isfinite(ious).all() and torch.isfinite(distances).all()
