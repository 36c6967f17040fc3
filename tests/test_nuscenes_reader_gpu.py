"""The NuScenes reader on the GPU (csrc/preload.hip, open3dsot_amd/datasets.py): the steps launches against the numpy
restatement of the device rule (tests/nuscenes_oracle.py) bit for bit, the reader against the reference's own NuScenesDataset
(tests/golden/ref_nuscenes.npz) bit for bit, the cache, and the reader's output through DeviceBatchSampler with a
SiameseBatchBuilder and a MotionBatchBuilder and through tracking.evaluate_sequence.  Every comparison is exact."""
import os
import shutil

import numpy as np
import pytest
import torch

import fixture_io
import nuscenes_oracle as NO
import nuscenes_tree
import tracking_oracle as TO
from nuscenes_oracle import cases, ref_clouds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = nuscenes_tree.VERSION
SPLITS = nuscenes_tree.SPLITS
INF = np.inf
NAN_BITS = 0x7FC00000                                       # what the spare pool rows hold


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref():
    return fixture_io.load(os.path.join(ROOT, "tests", "golden", "ref_nuscenes.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return nuscenes_tree.build(str(tmp_path_factory.mktemp("nuscenes") / "tree"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def reader(tree, split, category="Car", **kw):
    from open3dsot_amd import datasets as D
    return D.NuScenesTracklets(tree, split, category, version=V, scenes=SPLITS, **kw)


# ---- (a) the kernels against the oracle -----------------------------------------------------------------------------------------------
# frames of 0, 1, 63, 64, 65 (around a wave), 255, 256, 257 (around a workgroup) and 513 points (three workgroups) with 0, 1 or
# CHUNK + 1 boxes per record (CHUNK = O3D_CROP_MULTI_CHUNK, the boxes staged in LDS at a time), then a frame of 65 points with
# O3D_PRELOAD_MAX_BOXES + 1 boxes, which is two records over the same raw rows with the same steps
FRAME_N = [0, 1, 63, 64, 65, 255, 256, 257, 513, 65]
ODD = 7                                                     # the frame of 257 points holds a NaN and two infinite coordinates


def some_steps(i, n_steps):
    """a chain of rigid steps, another for every record i: a calibrated sensor (metres), then ego poses (hundreds of metres)"""
    out = []
    for s in range(n_steps):
        rot, tr = nuscenes_tree.calibrated(i % 4, "LIDAR_TOP") if s == 0 else nuscenes_tree.ego(i % 4, i, s)
        out.append(np.hstack([nuscenes_tree.matrix(rot), np.array(tr, np.float64).reshape(3, 1)]).reshape(12))
    return np.array(out)


def kernel_case(row_floats, n_steps, translate32):
    """-> raw (rows,row_floats), records [(first raw row, n, boxes)], steps (F,n_steps,12), bounds (B,6) float32"""
    from open3dsot_amd import points_utils as PU
    chunk, most = PU.CROP_MULTI_CHUNK + 1, PU.PRELOAD_MAX_BOXES
    rng = np.random.default_rng(100 * row_floats + 10 * n_steps + translate32)
    raws = [rng.uniform(-40, 40, size=(n, row_floats)).astype(np.float32) for n in FRAME_N]
    raws[ODD][100, 0], raws[ODD][101, 1], raws[ODD][102, 2] = np.nan, np.inf, -np.inf
    for r in raws:
        r[::3, 3:] = np.nan                                 # whatever lies behind z is never looked at
    first = np.concatenate([[0], np.cumsum(FRAME_N)[:-1]])
    boxes = [1, chunk, 0, 1, chunk, 1, 0, chunk, 2, most, 1]
    frame_of = list(range(len(FRAME_N))) + [len(FRAME_N) - 1]
    records = [(int(first[f]), FRAME_N[f], k) for f, k in zip(frame_of, boxes)]
    steps = np.stack([some_steps(i, n_steps) for i in range(len(records))])
    steps[-1] = steps[-2]
    bounds = []
    for (row0, n, k), S in zip(records, steps):
        c = NO.chain(np.zeros((1, 3), np.float32), S, translate32)[0].astype(np.float64)     # where the sensor is: the points lie within 70 m
        bounds.append(np.concatenate([c - rng.uniform(0, 45, size=(k, 3)), c + rng.uniform(0, 45, size=(k, 3))], 1).astype(np.float32))
    bounds[1][1] = [-INF] * 3 + [INF] * 3                   # the frame of one point keeps it
    p = NO.chain(raws[ODD], steps[ODD], translate32)
    bounds[ODD][0] = [-INF] * 3 + [INF] * 3                 # keeps every point but the three odd ones: survivors in two workgroups
    fin = np.sort(p[np.isfinite(p).all(1)], 0)              # per axis, the finite coordinates in order
    bounds[ODD][1] = [fin[40, 0], -INF, fin[40, 2], INF, INF, INF]     # lo equal to a coordinate of a point in x, of one in z
    bounds[ODD][chunk - 1] = [-INF, -INF, -INF, fin[200, 0], fin[200, 1], INF]     # beyond the chunk: hi equal to coordinates
    bounds[5][0] = [0, 0, 0, 1, 1, 1]                       # hundreds of metres away: keeps nothing
    bounds[8][1] = [-INF] * 3 + [INF] * 3                   # 513 points, all kept: three workgroups
    q = NO.chain(raws[9], steps[9], translate32)
    bounds[9][3] = [-INF, -INF, -INF, np.sort(q[:, 0])[32], INF, INF]       # keeps 32 of the 65 points
    bounds[10][0] = bounds[9][3]                            # the same rows, steps and bounds as a box of the record before
    bounds[9][most - 1] = [-INF] * 3 + [INF] * 3            # the last box of a full record
    return np.concatenate(raws), records, steps, np.concatenate(bounds)


def device_tables(dev, records):
    from open3dsot_amd import points_utils as PU
    frames = np.zeros((len(records), PU.PRELOAD_COLS), np.int32)
    frames[:, 0], frames[:, 1], frames[:, 3] = [r[0] for r in records], [r[1] for r in records], [r[2] for r in records]
    need, wgs, B = PU.preload_plan(frames, sum(FRAME_N))
    return frames, torch.from_numpy(frames).to(dev), need, B


def nan_pool(rows, dev):
    return torch.full((rows, 3), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def run_kernels(dev, raw, records, steps_h, bounds_h, translate32, want):
    """count, then scatter with every box's slice two spare rows behind the one before and eight guard rows at the end ->
    asserts counts and the whole pool, spare rows included"""
    from open3dsot_amd import points_utils as PU
    B = len(want)
    frames, dev_frames, need, nb = device_tables(dev, records)
    assert nb == B
    dev_bounds = torch.from_numpy(bounds_h).to(dev)
    dev_steps = torch.from_numpy(steps_h).to(dev)
    scratch = torch.full((need + 8,), -1, dtype=torch.int32, device=dev)
    counts = torch.full((B + 4,), -5, dtype=torch.int32, device=dev)
    PU.preload_count(raw, frames, dev_frames, dev_bounds, None, scratch[:need], counts[:B], steps=dev_steps, translate32=translate32)
    got_counts = counts.cpu().numpy()
    assert list(got_counts[:B]) == [w.shape[0] for w in want] and (got_counts[B:] == -5).all()
    assert (scratch[need:].cpu().numpy() == -1).all()
    first = np.cumsum([2] + [w.shape[0] + 2 for w in want[:-1]]).astype(np.int64)
    rows = int(first[-1]) + want[-1].shape[0]
    pool = nan_pool(rows + 8, dev)
    PU.preload_scatter(raw, frames, dev_frames, dev_bounds, None, scratch[:need], torch.from_numpy(first).to(dev), pool, pool_rows=rows,
                       steps=dev_steps, translate32=translate32)
    expect = np.full((rows + 8, 3), NAN_BITS, np.int32)
    for f, w in zip(first, want):
        expect[f:f + w.shape[0]] = bits(w)
    assert np.array_equal(pool.cpu().numpy().view(np.int32), expect)


@pytest.mark.parametrize("translate32", [0, 1])
@pytest.mark.parametrize("n_steps", [1, 2, 3])
@pytest.mark.parametrize("row_floats", [3, 4, 5])
def test_steps_kernels_equal_the_oracle_bit_for_bit(dev, row_floats, n_steps, translate32):
    from open3dsot_amd import points_utils as PU
    chunk, most = PU.CROP_MULTI_CHUNK + 1, PU.PRELOAD_MAX_BOXES
    raw_h, records, steps_h, bounds_h = kernel_case(row_floats, n_steps, translate32)
    want = NO.crop_steps(raw_h, row_floats, records, bounds_h, steps_h, translate32)
    B = len(want)
    assert B == 5 + 3 * chunk + most + 1 and [r[2] for r in records[-2:]] == [most, 1] and records[-1][:2] == records[-2][:2]
    b_odd = 1 + chunk + 0 + 1 + chunk + 1 + 0               # the first box of the frame with the odd points
    p = NO.chain(raw_h[sum(FRAME_N[:ODD]):sum(FRAME_N[:ODD + 1]), :3], steps_h[ODD], translate32)
    assert not np.isfinite(p[100:103]).all(1).any() and np.isfinite(np.delete(p, [100, 101, 102], 0)).all()
    assert want[b_odd].shape[0] == 257 - 3                  # the +-inf box: everything but the NaN and the infinite points
    for b, cols in ((b_odd + 1, (0, 2)), (b_odd + chunk - 1, (3, 4))):
        for col in cols:                                    # strict compares: a point with a coordinate equal to a bound is out
            on = np.flatnonzero(bits(p[:, col % 3]) == bits(bounds_h[b, col]))
            assert len(on) >= 1 and not any((bits(want[b]) == bits(p[i])).all(1).any() for i in on)
    assert 0 < want[b_odd + 1].shape[0] < 254 and 0 < want[b_odd + chunk - 1].shape[0] < 254
    b_big = B - most - 1                                    # the first box of the frame with most + 1 boxes
    assert want[0].shape[0] == 0 and want[2].shape[0] == 1 and want[2 + 2 * chunk].shape[0] == 0 and want[B - 2].shape[0] == 65
    assert 0 < want[b_big - 2].shape[0] < 513 and want[b_big - 1].shape[0] == 513
    assert want[B - 1].shape[0] > 0 and np.array_equal(bits(want[b_big + 3]), bits(want[B - 1]))      # two records, one frame, one chain
    assert sum(w.shape[0] for w in want[:b_big]) > 1000
    if n_steps > 1:                                         # the other mode gives other bits: the wrong mode cannot pass
        other = NO.crop_steps(raw_h, row_floats, records[:-2], bounds_h[:b_big], steps_h[:-2], 1 - translate32)
        assert any(a.shape != b.shape or not np.array_equal(bits(a), bits(b)) for a, b in zip(other, want))
    run_kernels(dev, torch.from_numpy(raw_h).to(dev), records, steps_h, bounds_h, translate32, want)


def test_rows_of_five_floats_need_four_byte_alignment_only(dev):
    """a raw table that starts one float into a device buffer (4-byte aligned, not 16): row_floats 5 (and 3) is served and
    equals the oracle; row_floats 4 at such an address is refused"""
    from open3dsot_amd import capi, points_utils as PU
    for row_floats in (5, 3):
        raw_h, records, steps_h, bounds_h = kernel_case(row_floats, 2, 0)
        want = NO.crop_steps(raw_h, row_floats, records, bounds_h, steps_h, 0)
        buf = torch.full((raw_h.size + 8,), -777.0, dtype=torch.float32, device=dev)
        raw = buf[1:1 + raw_h.size].view(-1, row_floats)
        raw.copy_(torch.from_numpy(raw_h))
        assert raw.data_ptr() % 16 == 4 and raw.is_contiguous()
        run_kernels(dev, raw, records, steps_h, bounds_h, 0, want)
        assert (buf[:1].cpu().numpy() == -777.0).all() and (buf[1 + raw_h.size:].cpu().numpy() == -777.0).all()
    f4 = np.zeros((1, PU.PRELOAD_COLS), np.int32)
    f4[0, 1], f4[0, 3] = 8, 1
    need4, _, _ = PU.preload_plan(f4, 8)
    z = torch.zeros((64,), dtype=torch.float64, device=dev)
    rc = capi.load().o3d_preload_steps_count(raw.data_ptr(), 8, 4, f4.ctypes.data, z.data_ptr(), 1, z.data_ptr(), 1, z.data_ptr(), 2, 0,
                                             z.data_ptr(), need4, z.data_ptr(), None)
    assert rc == capi.CONSTANTS["O3D_EINVAL"]


def test_one_step_equals_the_posed_launches_where_one_rounding_is_exact(dev):
    """a chain of ONE step whose translation is zero rounds once, like the posed rule: on rows of three floats both launches
    give the same scratch, counts and pool"""
    from open3dsot_amd import points_utils as PU
    raw_h, records, steps_h, _ = kernel_case(3, 1, 0)
    raw_h = np.nan_to_num(raw_h, nan=0.5, posinf=1.5, neginf=-1.5)
    steps_h = steps_h.copy()
    steps_h.reshape(-1, 3, 4)[:, :, 3] = 0.0
    rng = np.random.default_rng(5)
    frames, dev_frames, need, B = device_tables(dev, records)
    bounds_h = np.concatenate([-rng.uniform(0, 45, size=(B, 3)), rng.uniform(0, 45, size=(B, 3))], 1).astype(np.float32)
    raw, dev_bounds = torch.from_numpy(raw_h).to(dev), torch.from_numpy(bounds_h).to(dev)
    dev_steps = torch.from_numpy(steps_h).to(dev)
    out = []
    for kw in (dict(poses=dev_steps.view(-1, 12)), dict(steps=dev_steps, translate32=0), dict(steps=dev_steps, translate32=1)):
        scratch = torch.full((need,), -1, dtype=torch.int32, device=dev)
        counts = torch.full((B,), -5, dtype=torch.int32, device=dev)
        PU.preload_count(raw, frames, dev_frames, dev_bounds, None, scratch, counts, **kw)
        n = counts.cpu().numpy().astype(np.int64)
        out_row = torch.from_numpy(np.concatenate([[0], np.cumsum(n)[:-1]])).to(dev)
        pool = nan_pool(int(n.sum()) + 2, dev)
        PU.preload_scatter(raw, frames, dev_frames, dev_bounds, None, scratch, out_row, pool, pool_rows=int(n.sum()), **kw)
        out.append((n, scratch.cpu().numpy(), pool.cpu().numpy()))
    (n0, s0, p0), (n1, s1, p1), (n2, s2, p2) = out
    assert n0.sum() > 1000 and np.array_equal(n0, n1) and np.array_equal(s0, s1) and p0.tobytes() == p1.tobytes()
    assert np.array_equal(n0, n2) and np.array_equal(s0, s2) and p0.tobytes() == p2.tobytes()       # r + 0 is r in either mode


def test_empty_steps_calls_launch_nothing_and_succeed(dev):
    from open3dsot_amd import points_utils as PU
    z32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)      # noqa: E731
    zf = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)      # noqa: E731
    for n in ([], [0, 7]):                                  # no frame; frames without a box
        frames = np.zeros((len(n), PU.PRELOAD_COLS), np.int32)
        frames[:, 1] = n
        frames[:, 0] = np.concatenate([[0], np.cumsum(n)[:-1]]) if n else []
        assert PU.preload_plan(frames, sum(n)) == (0, 0, 0)
        pool = nan_pool(4, dev)
        steps = torch.zeros((len(n), 2, 12), dtype=torch.float64, device=dev)
        PU.preload_count(zf(sum(n), 5), frames, z32(frames.size), zf(0, 6), None, z32(0), z32(0), steps=steps, translate32=1)
        PU.preload_scatter(zf(sum(n), 5), frames, z32(frames.size), zf(0, 6), None, z32(0), torch.zeros(0, dtype=torch.int64, device=dev),
                           pool, steps=steps, translate32=1)
        assert (pool.cpu().numpy().view(np.int32) == NAN_BITS).all()


# ---- (b) the reader against the reference ---------------------------------------------------------------------------------------------
def check_against(trk, want, ref, name):
    assert [len(t) for t in trk] == list(ref[name + ".lengths"])
    assert trk.get_num_tracklets() == len(want) and trk.get_num_frames_total() == sum(len(w) for w in want)
    boxes = np.concatenate([t.boxes for t in trk] + [np.zeros((0, 15), np.float32)])
    assert boxes.dtype == np.float32 and np.array_equal(boxes, ref[name + ".boxes"].astype(np.float32))
    assert np.concatenate(list(trk.boxes64) + [np.zeros((0, 15))]).tobytes() == ref[name + ".boxes"].tobytes()
    assert [m[0] for m in trk.meta] == [str(k) for k in ref[name + ".keys"]]
    assert [f for m in trk.meta for f in m[1]] == [str(f) for f in ref[name + ".files"]]
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
    assert len(cases(ref)) == 14
    for name, category, offset, split, key_only, min_points in cases(ref):
        for chunk in (1, 64):
            trk = reader(tree, split, category.capitalize(), preload_offset=offset, key_frame_only=key_only, min_points=min_points,
                         device=dev, chunk_frames=chunk)
            check_against(trk, ref_clouds(ref, name), ref, name)
            if offset <= 0:                                  # no crop: a sweep is written once, its tracklets share it
                assert trk.pool.shape[0] == sum({f: c.shape[0] for t, w in zip(trk.meta, ref_clouds(ref, name))
                                                 for f, c in zip(t[1], w)}.values())
    trk = reader(tree, "train", device=dev, preload_offset=10)
    assert (trk.split, trk.category_name, trk.version, trk.translate, trk.key_frame_only, trk.min_points) == ("train", "Car", V, "float64", False, False)
    assert trk[0].frames[1].data_ptr() != trk[1].frames[0].data_ptr()       # cropped: a slice per tracklet frame
    shared = D.NuScenesTracklets(tree, "train", version=V, scenes=os.path.join(tree, "splits.json"), device=dev)
    assert shared.preload_offset == -1 and shared[0].frames[1].data_ptr() == shared[1].frames[0].data_ptr()       # the reference's defaults
    fr = trk.get_frames(0, [0, 1])
    assert len(fr) == 2 and fr[1]["pc"] is trk[0].frames[1] and fr[1]["3d_bbox"].shape == (15,)
    assert fr[1]["meta"] == (nuscenes_tree.token("instance", "scene-0001", "car_a"), nuscenes_tree.sweeps()[1])
    with pytest.raises(ValueError):
        reader(tree, "train", device=dev, chunk_frames=0)
    with pytest.raises(ValueError):
        reader(tree, "train", device=dev, translate="float16")


def test_scenes_none_without_the_devkit(dev, tree, monkeypatch):
    import sys
    from open3dsot_amd import datasets as D
    for name in ("nuscenes", "nuscenes.utils", "nuscenes.utils.splits"):
        monkeypatch.setitem(sys.modules, name, None)
    with pytest.raises(ValueError, match="scenes="):
        D.NuScenesTracklets(tree, "train", version=V, device=dev)


def test_the_float32_mode_reaches_the_kernel(dev, ref, tree):
    """translate="float32" gives the oracle's float32 mode bit for bit, which is not the fixture"""
    from open3dsot_amd import datasets as D
    for name, offset in (("car.10.train.k0.m0", 10), ("car.-1.train.k0.m0", -1)):
        annos, files, steps = D.nuscenes_annotations(tree, "train", "Car", V, scenes=SPLITS)
        want = NO.reader(annos, files, steps, offset, lambda f: NO.read_sweep(os.path.join(tree, f)), 1)
        trk = reader(tree, "train", preload_offset=offset, translate="float32", device=dev)
        check_against(trk, want, ref, name)
        fix = ref_clouds(ref, name)
        assert any(a.shape != b.shape or not np.array_equal(bits(a), bits(b)) for w, x in zip(want, fix) for a, b in zip(w, x))


def test_every_sweep_file_is_opened_once(dev, tree, monkeypatch):
    """several tracklets share sweeps: each distinct file is read once, whatever the chunking and the crop"""
    from open3dsot_amd import datasets as D
    real = D._read_rows
    for offset, chunk in ((10, 1), (10, 4), (-1, 64)):
        opened = []
        monkeypatch.setattr(D, "_read_rows", lambda host, path, n: (opened.append(path), real(host, path, n))[1])
        trk = reader(tree, "train", preload_offset=offset, device=dev, chunk_frames=chunk)
        files = [os.path.join(tree, f) for m in trk.meta for f in m[1]]
        assert len(files) == 36 and len(opened) == 9 and sorted(opened) == sorted(set(files))


def test_odd_sweep_files(dev, ref, tree, tmp_path):
    """an empty sweep gives (0,3) frames; a length that is no multiple of 20 bytes raises ValueError naming the file; a missing
    sweep raises FileNotFoundError"""
    odd = str(tmp_path / "odd")
    shutil.copytree(tree, odd)
    victim = os.path.join(odd, nuscenes_tree.sweeps()[1])
    open(victim, "wb").close()
    name = "car.10.train.k0.m0"
    for offset in (10, -1):
        trk = reader(odd, "train", preload_offset=offset, device=dev)
        sizes = [[f.shape[0] for f in t.frames] for t in trk]
        assert sizes[0][1] == 0 and sizes[1][0] == 0 and tuple(trk[0].frames[1].shape) == (0, 3) and sizes[0][0] > 0
    want = ref_clouds(ref, name)
    trk = reader(odd, "train", preload_offset=10, device=dev)
    assert np.array_equal(bits(trk[0].frames[2].cpu().numpy()), bits(want[0][2]))       # the sweeps around it are as before
    with open(victim, "wb") as f:
        f.write(b"\0" * 50)
    with pytest.raises(ValueError, match=os.path.basename(victim)):
        reader(odd, "train", device=dev)
    os.remove(victim)
    with pytest.raises(FileNotFoundError):
        reader(odd, "train", device=dev)


def test_cache_round_trip(dev, ref, tree, tmp_path):
    from open3dsot_amd import datasets as D
    name = "pedestrian.10.train.k0.m0"
    a = reader(tree, "train", "Pedestrian", preload_offset=10, min_points=0, device=dev)
    file = str(tmp_path / "cache.dat")
    a.save(file)
    assert os.path.exists(file)                              # the name as given
    with np.load(file) as z:
        assert sorted(z.files) == ["boxes", "files", "info", "keys", "lengths", "pool", "rows"]
    b = D.NuScenesTracklets.load(file, device=dev)
    check_against(b, ref_clouds(ref, name), ref, name)
    assert (b.split, b.category_name, b.version, b.translate) == ("train", "Pedestrian", V, "float64")
    assert (b.preload_offset, b.key_frame_only, b.min_points) == (10, False, 0) and type(b.preload_offset) is int
    assert np.array_equal(bits(a.pool.cpu().numpy()), bits(b.pool.cpu().numpy()))
    for x, y in zip(a.boxes64, b.boxes64):
        assert np.array_equal(x, y)
    assert b.meta == a.meta
    c = reader(tree, "val", translate="float32", device=dev)
    c.save(file)
    d = D.NuScenesTracklets.load(file, device=dev)
    assert (d.translate, d.preload_offset, d.min_points) == ("float32", -1, False) and d.meta == c.meta
    assert np.array_equal(bits(c.pool.cpu().numpy()), bits(d.pool.cpu().numpy()))


# ---- (c) plumbing ---------------------------------------------------------------------------------------------------------------------
def by_hand(ref, name, dev):
    from open3dsot_amd import sampler as S
    clouds = ref_clouds(ref, name)
    ends = np.cumsum(ref[name + ".lengths"])
    boxes = np.split(ref[name + ".boxes"].astype(np.float32), ends[:-1])
    return S.DeviceTracklets([[torch.from_numpy(c.copy()) for c in w] for w in clouds], boxes, device=dev)


@pytest.mark.parametrize("kind", ["SiameseBatchBuilder", "MotionBatchBuilder"])
def test_the_batch_builders_take_the_reader(dev, ref, tree, kind):
    """DeviceBatchSampler with either builder over the reader's tracklets yields the batch that the fixture's clouds, uploaded
    by hand, yield"""
    from open3dsot_amd import sampler as S
    name = "bus.10.train.k0.m0"
    trk = reader(tree, "train", "Bus", preload_offset=10, device=dev)
    batches = []
    for tracklets in (trk[:1], by_hand(ref, name, dev)[:1]):           # one tracklet: the bus of scene-0001, five frames
        it = iter(S.DeviceBatchSampler(tracklets, getattr(S, kind)({}, 4, seed=3), seed=3))
        batches.append({k: v.clone() if torch.is_tensor(v) else v for k, v in next(it).items()})
    a, b = batches
    assert set(a) == set(b) and len(a) >= 5 and int(a["n_valid"]) >= 1
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].shape == b[k].shape and torch.equal(a[k].cpu().view(torch.uint8), b[k].cpu().view(torch.uint8)), k
        else:
            assert a[k] == b[k], k


def test_evaluate_sequence_takes_a_tracklet_of_the_reader(dev, tree):
    """a tracklet in global coordinates of hundreds of metres: finite boxes come back"""
    from open3dsot_amd import tracking, trackers
    trk = reader(tree, "train", "Car", preload_offset=10, device=dev)
    t = trk[0]
    assert len(t) == 5 and min(f.shape[0] for f in t.frames) > 20
    cfg = dict(trackers.BAT_CAR)
    cfg.update(TO.TEST_KEYS)
    model = TO.init_weights(trackers.get_model("BAT")(trackers.make_config(cfg))).to(dev).eval()
    ious, distances, results = tracking.evaluate_sequence(model, t.frames, t.boxes)
    assert tuple(results.shape) == (len(t), 15) and torch.isfinite(results).all()
    assert torch.isfinite(ious).all() and torch.isfinite(distances).all()
