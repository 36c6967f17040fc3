"""The planned training epoch, the part that needs no GPU: the epoch's order and frame choice (sampler.epoch_order /
epoch_frames), the chunk planner (sampler.plan_chunk) against the C planner of the grouped crop, the host side of
o3d_train_draw (declared, exported, validated before any launch) and the statistics of its numpy restatement
(tests/epoch_plan_oracle.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import epoch_plan_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (1) the order ---------------------------------------------------------------------------------------------------------------------
def test_epoch_order_is_a_permutation_cut_to_whole_batches():
    from open3dsot_amd import sampler
    a = sampler.epoch_order(103, 5, True, 7, 0)
    assert a.shape == (20, 5) and a.dtype == np.int64
    assert np.unique(a).size == 100 and a.min() >= 0 and a.max() < 103
    assert np.array_equal(a.reshape(-1), np.random.default_rng([7, 0]).permutation(103)[:100])
    assert np.array_equal(a, sampler.epoch_order(103, 5, True, 7, 0))
    assert not np.array_equal(a, sampler.epoch_order(103, 5, True, 7, 1))
    assert not np.array_equal(a, sampler.epoch_order(103, 5, True, 8, 0))
    assert np.array_equal(sampler.epoch_order(103, 5, False, 7, 3), np.arange(100).reshape(20, 5))
    assert sampler.epoch_order(4, 5, True, 0, 0).shape == (0, 5)


@pytest.mark.parametrize("shuffle", [False, True])
def test_ranks_take_disjoint_shares_of_one_order(shuffle):
    from open3dsot_amd import sampler
    whole = sampler.epoch_order(103, 5, shuffle, 3, 2)
    shares = [sampler.epoch_order(103, 5, shuffle, 3, 2, rank=r, world=3) for r in range(3)]
    assert all(s.shape == (6, 5) for s in shares)                              # 20 batches: 18 in whole rounds, 2 dropped
    for r, s in enumerate(shares):
        assert np.array_equal(s, whole[r:18:3])
    together = np.concatenate(shares).reshape(-1)
    assert np.unique(together).size == together.size == 90
    assert set(together.tolist()) == set(whole[:18].reshape(-1).tolist())
    with pytest.raises(ValueError):
        sampler.epoch_order(103, 5, shuffle, 3, 2, rank=3, world=3)


class FakeTracklet:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class FakeBuilder:
    def __init__(self, motion, J=5, num_candidates=4):
        self.motion, self.J, self.num_candidates = motion, J, num_candidates


@pytest.mark.parametrize("motion", [False, True])
def test_unshuffled_order_and_frames_are_todays_samples(motion):
    """lengths (1, 2, 7): a one-frame tracklet and max(this - 1, 0) at every tracklet's first annotation"""
    from open3dsot_amd import sampler
    tracklets = [FakeTracklet(n) for n in (1, 2, 7)]
    it = sampler.DeviceBatchSampler(tracklets, FakeBuilder(motion))
    assert it.length == 40 and len(it) == 8
    order = sampler.epoch_order(it.length, 5, False, 0, 0)
    assert np.array_equal(order.reshape(-1), np.arange(40))                    # what __next__ feeds sample() today
    trk, frames, cand = sampler.epoch_frames(order, it.starts, it.num_candidates, motion)
    assert frames.shape == (8, 5, 2 if motion else 3)
    for b in range(8):
        for j in range(5):
            want = it.sample(int(order[b, j]))
            assert want[0] is tracklets[trk[b, j]]
            assert tuple(want[1:]) == tuple(frames[b, j].tolist()) + (int(cand[b, j]),)
    assert (frames[..., -2] == np.maximum(frames[..., -1] - 1, 0)).all() and frames[..., -1].max() == 6


def test_random_draw_gives_two_distinct_frames():
    from open3dsot_amd import sampler
    lengths = np.array([1, 2, 7])
    t, a, b = sampler.random_draw(lengths, 4000, 5, 0)
    assert set(t.tolist()) == {0, 1, 2} and (a < lengths[t]).all() and (b < lengths[t]).all() and a.min() >= 0 and b.min() >= 0
    assert ((a != b) | (lengths[t] == 1)).all() and not a[t == 0].any() and not b[t == 0].any()
    seven = t == 2
    assert set(zip(a[seven].tolist(), b[seven].tolist())) == {(x, y) for x in range(7) for y in range(7) if x != y}
    again = sampler.random_draw(lengths, 4000, 5, 0)
    assert all(np.array_equal(x, y) for x, y in zip((t, a, b), again))
    assert not np.array_equal(sampler.random_draw(lengths, 4000, 5, 1)[1], a)
    trk, frames, cand = sampler.epoch_frames(np.array([[0, 5], [3999, 6]]), np.array([0, 1, 3, 10]), 4, False, (t, a, b))
    assert np.array_equal(trk, t[[[0, 5], [3999, 6]]]) and not frames[..., 0].any()
    assert np.array_equal(frames[..., 1], a[[[0, 5], [3999, 6]]]) and np.array_equal(cand, [[0, 1], [3, 2]])


def test_sampler_arguments():
    from open3dsot_amd import sampler
    tracklets = [FakeTracklet(n) for n in (1, 2, 7)]
    with pytest.raises(ValueError, match="plan_batches"):
        sampler.DeviceBatchSampler(tracklets, FakeBuilder(False), shuffle=True)
    with pytest.raises(ValueError):
        sampler.DeviceBatchSampler(tracklets, FakeBuilder(False), plan_batches=0)
    it = sampler.DeviceBatchSampler(tracklets, FakeBuilder(False), shuffle=True, plan_batches=3, world=2)
    assert len(it) == 4
    with pytest.raises(RuntimeError):
        sampler.DeviceBatchSampler(tracklets, FakeBuilder(False)).begin(0)


# ---- (2) the planner -------------------------------------------------------------------------------------------------------------------
J, P = 5, 3
LENGTHS = (1, 3, 4)
FN = np.array([1, 256, 257, 1000, 0, 255, 300, 513], np.int64)                 # the frame sizes of the 8 pool rows
FPTR = 0x7f0000000000 + 0x100000 * np.arange(8, dtype=np.int64)
BASE, AUG_BASE = 0x7e0000000000, 0x7d0000000000


def fixed_records(PU):
    rec = np.zeros((3, J), PU.CROP_TARGET)
    for c in range(3):
        rec["box"][c] = 0x1000 * (c + 1) + 60 * np.arange(J)
        rec["capacity"][c] = 100 * (c + 1) + np.arange(J)                      # tells the records apart
    return rec


def planned_epoch(motion, aug=False):
    """the tables of every chunk of a shuffled epoch over LENGTHS with 5 candidate ids: 40 samples, 8 batches of 5, chunks of
    3, 3 and 2 batches"""
    from open3dsot_amd import points_utils as PU, sampler
    starts = np.concatenate([[0], np.cumsum(LENGTHS)])
    order = sampler.epoch_order(int(starts[-1]) * 5, J, True, 11, 0)
    trk, frames, cand = sampler.epoch_frames(order, starts, 5, motion)
    rows = starts[:-1][trk][..., None] + frames
    cols = (0, 0, 1) if motion else (0, 1, 2)
    rec = fixed_records(PU)
    chunks = []
    for s in range(0, order.shape[0], P):
        ch = sampler.ChunkTables(P, J, rows.shape[-1], aug, base=BASE)
        sampler.plan_chunk(ch, FPTR, FN, rows[s:s + P], cand[s:s + P], rec, cols, AUG_BASE if aug else None)
        chunks.append((ch, rows[s:s + P], cand[s:s + P]))
    return chunks, rec, cols


@pytest.mark.parametrize("motion,aug", [(False, False), (True, False), (True, True)])
def test_chunk_planner(motion, aug):
    from open3dsot_amd import points_utils as PU
    chunks, rec, cols = planned_epoch(motion, aug)
    assert [c[1].shape[0] for c in chunks] == [3, 3, 2]
    shared = 0
    for ch, rows, cand in chunks:
        S = rows.shape[0]
        assert np.array_equal(ch.rows[:S], rows) and np.array_equal(ch.cand[:S], cand)
        assert ch.rows.dtype == np.int32 and ch.rows.shape == (P, J, 2 if motion else 3) and ch.cand.shape == (P, J)
        for k in range(S):
            G = int(ch.groups[k])
            plan = ch.plan[k, :G]
            # the C planner fills a copy: the same plan, grids and scratch need
            mine = plan.copy()
            for name in ("wg_start", "row_start", "sbase"):
                mine[name] = -1
            need, wgs, scan = PU.crop_groups_plan(mine)
            assert np.array_equal(mine, plan) and need == ch.need[k] and wgs == ch.grid[k] and scan == 3 * J
            assert need == np.maximum(1, -(-FN[rows[k][:, list(cols)]] // 256)).sum()
            # every distinct frame is one group, with the frame's address and size
            frames = set(rows[k][:, list(cols)].reshape(-1).tolist())
            assert G == len(frames) and sorted(plan["points"].tolist()) == sorted(FPTR[list(frames)].tolist())
            assert plan["n_targets"].sum() == 3 * J
            shared += int((plan["n_targets"] > 1).sum())
            # every crop (c, j) exactly once, under the group of its own frame
            seen = set()
            t0 = ch.dev("targets", k)
            assert t0 == BASE + ch._layout["targets"][0] + k * 3 * J * PU.CROP_TARGET.itemsize
            for g in range(G):
                frame = int(np.flatnonzero(FPTR == plan["points"][g])[0])
                assert plan["n"][g] == FN[frame]
                first = (int(plan["targets"][g]) - t0) // PU.CROP_TARGET.itemsize
                assert first == plan["row_start"][g]
                for pos in range(first, first + int(plan["n_targets"][g])):
                    t = ch.targets[k, pos]
                    c, j = int(t["capacity"]) // 100 - 1, int(t["capacity"]) % 100
                    assert t == rec[c, j] and rows[k][j, cols[c]] == frame and (c, j) not in seen
                    seen.add((c, j))
                    if aug:                                    # the record slot: none for the in-box count, else row (c - 1) J + j of refs / aug
                        assert ch.slots[k, pos] == (-1 if c == 0 else (c - 1) * J + j)
                if aug:
                    assert ch.augptr[k, g] == AUG_BASE + PU.CROP_AUG.itemsize * first
            assert len(seen) == 3 * J
    assert shared > 0
    assert hasattr(chunks[0][0], "slots") == aug


def test_chunk_tables_layout():
    from open3dsot_amd import points_utils as PU, sampler
    ch = sampler.ChunkTables(4, 7, 2, True, base=4096)
    ends = 0
    for name in ("rows", "cand", "slots", "augptr", "targets", "plan"):
        off, nbytes = ch._layout[name]
        assert off % 64 == 0 and off >= ends and ch.dev(name, 0) == 4096 + off and ch.dev(name, 3) == 4096 + off + 3 * nbytes // 4
        ends = off + nbytes
    assert ch.host.size >= ends and ch.plan.shape == (4, 21) and ch.plan.dtype == PU.CROP_PLAN
    ch.plan["n"][3, 20] = 77                                   # the views write the one buffer
    assert ch.host[ch._layout["plan"][0]:].view(PU.CROP_PLAN)[4 * 21 - 1]["n"] == 77


# ---- (3) the entry ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_draw_and_the_library_exports_it():
    from open3dsot_amd import build, capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "o3dsot.h")).read(), flags=re.S)
    assert "o3d_train_draw" in set(re.findall(r"\b(o3d_[a-z0-9_]+)\s*\(", hdr))
    assert hasattr(ctypes.CDLL(build.build()), "o3d_train_draw")
    # pointers, ints and the stream: the two uint32 travel in the bits of an int
    p, i = ctypes.c_void_p, ctypes.c_int
    assert capi.SIGNATURES["o3d_train_draw"] == [p, i, p, p, i, i, i, i, i, i, p, p, p, p, p]
    assert (capi.CONSTANTS["O3D_TRAIN_DRAW_SIAMESE"], capi.CONSTANTS["O3D_TRAIN_DRAW_MOTION"],
            capi.CONSTANTS["O3D_TRAIN_DRAW_MOTION_AUG"]) == (EO.SIAMESE, EO.MOTION, EO.MOTION_AUG)


def test_draw_validates_before_any_launch():
    """host buffers stand in for device pointers: nothing dereferences them, every call returns before a HIP call"""
    from open3dsot_amd import capi
    lib = capi.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    good = dict(gt=p, R=7, rows=p, cand=p, J=5, seed=1, counter=2, degrees=1, num_candidates=4, mode=EO.SIAMESE, refs=p, first=p,
                offs=p, aug=None)
    bad = [dict(gt=None), dict(rows=None), dict(cand=None), dict(refs=None), dict(offs=None), dict(first=None), dict(J=0),
           dict(J=capi.CONSTANTS["O3D_TRAIN_MAX_CANDIDATES"] + 1), dict(R=0), dict(num_candidates=0), dict(mode=3), dict(mode=-1),
           dict(mode=EO.MOTION_AUG, aug=None), dict(mode=EO.MOTION, offs=None)]
    for over in bad:
        assert lib.o3d_train_draw(*dict(good, **over).values(), None) == capi.CONSTANTS["O3D_EINVAL"], over


# ---- (4) the draw's restatement ------------------------------------------------------------------------------------------------------------
N_DRAWS = 100000


def within(values, mean, var, fourth):
    """mean and variance of n samples within 5 standard errors of the exact values (fourth = the central fourth moment)"""
    n = values.size
    ok_mean = abs(values.mean() - mean) <= 5 * np.sqrt(var / n)
    ok_var = abs(((values - mean) ** 2).mean() - var) <= 5 * np.sqrt((fourth - var ** 2) / n)
    return ok_mean and ok_var


def test_key_is_the_index_draws():
    from open3dsot_amd import points_utils as PU
    for seed, counter, j, tag in ((0, 0, 0, 2), (17, 3, 59, 3), (0xFFFFFFFF, 0xFFFFFFFE, 1023, 5), (5, 1 << 20, 7, 4)):
        assert int(EO.key(seed, counter, j, tag)) == PU.draw_key(seed, counter, j, tag)
        assert int(EO.mix32(seed)) == PU._mix32(seed)
    assert {EO.TAG_JITTER, EO.TAG_SEARCH, EO.TAG_AUG_PREV, EO.TAG_AUG_THIS}.isdisjoint({0, 1})      # the index draw's clouds


def test_draw_statistics():
    """10^5 draws: 100 builds of 1 000 candidates.  The bounds follow from n alone."""
    j = np.arange(1000)
    cand = np.ones(1000, int)
    jit = np.concatenate([EO.jitter(9, c, j, cand, True) for c in range(100)]).astype(np.float64)
    srch = np.concatenate([EO.search_offset(9, c, j, cand, False, 4) for c in range(100)]).astype(np.float64)
    aug = np.concatenate([EO.augmentation(9, c, j, EO.TAG_AUG_PREV) for c in range(100)]).astype(np.float64)
    assert jit.shape == (N_DRAWS, 4) and not jit[:, 2].any() and not srch[:, 2].any()
    for col, half in ((jit[:, 0], 0.3), (jit[:, 1], 0.3), (jit[:, 3], 1.5), (aug[:, 0], 0.3), (aug[:, 1], 0.3), (aug[:, 2], 0.3), (aug[:, 3], 10.0)):
        assert np.abs(col).max() <= half + 1e-6 and np.abs(col).max() > 0.999 * half
        assert within(col, 0.0, half ** 2 / 3, half ** 4 / 5)                  # U(-a, a): variance a^2 / 3, fourth moment a^4 / 5
    ang = np.deg2rad(5)
    for col, var in ((srch[:, 0], 1.0), (srch[:, 1], 1.0), (srch[:, 3], ang)):
        assert within(col, 0.0, var, 3 * var ** 2) and np.abs(col).max() > 3.5 * np.sqrt(var)
    for col in (aug[:, 4], aug[:, 5]):                         # a fair bit: 5 standard errors of 1/2
        assert set(np.unique(col)) == {0.0, 1.0} and abs(col.mean() - 0.5) <= 5 * 0.5 / np.sqrt(N_DRAWS)
    # components and tags are streams of their own
    assert abs(np.corrcoef(jit[:, 0], jit[:, 1])[0, 1]) <= 5 / np.sqrt(N_DRAWS)
    assert abs(np.corrcoef(srch[:, 0], srch[:, 1])[0, 1]) <= 5 / np.sqrt(N_DRAWS)
    other = np.concatenate([EO.augmentation(9, c, j, EO.TAG_AUG_THIS) for c in range(100)]).astype(np.float64)
    assert abs(np.corrcoef(aug[:, 0], other[:, 0])[0, 1]) <= 5 / np.sqrt(N_DRAWS) and (aug[:, 4] != other[:, 4]).mean() > 0.49
    assert abs(np.corrcoef(aug[:, 0], jit[:, 0])[0, 1]) <= 5 / np.sqrt(N_DRAWS)
    keys = np.stack([EO.key(9, 0, j, t) for t in (0, 1, 2, 3, 4, 5)])
    assert np.unique(keys).size == keys.size
    assert not np.array_equal(EO.jitter(9, 0, j, cand, True), EO.jitter(9, 1, j, cand, True))           # the counter
    assert not np.array_equal(EO.jitter(9, 0, j, cand, True), EO.jitter(10, 0, j, cand, True))          # the seed


def test_candidate_zero_rows():
    j = np.arange(8)
    cand = j % 4
    zero = cand == 0
    for degrees in (False, True):
        jit = EO.jitter(3, 5, j, cand, degrees)
        assert not jit[zero].any() and jit[~zero][:, [0, 1, 3]].all()
        many, one = EO.search_offset(3, 5, j, cand, degrees, 4), EO.search_offset(3, 5, j, cand, degrees, 1)
        assert not many[zero].any() and one[zero][:, [0, 1, 3]].all() and np.array_equal(many[~zero], one[~zero])
    assert EO.augmentation(3, 5, j, EO.TAG_AUG_PREV)[:, :4].all()              # the augmentation is drawn for every candidate
    gt = np.arange(7 * 15, dtype=np.float32).reshape(7, 15) + 1
    rows = np.array([[0, 6, 3], [7, 3, -1], [6, 6, 0]])
    got = EO.draw(gt, rows, [1, 2, 0], 0, 0, True, 4, EO.SIAMESE)
    assert np.array_equal(got["first"], [gt[0], np.zeros(15), gt[6]])
    assert np.array_equal(got["refs"], [gt[6], gt[3], gt[6], gt[3], np.zeros(15), gt[0]])
    assert got["offs"].shape == (6, 4) and not got["offs"][2].any() and not got["offs"][5].any()
    mot = EO.draw(gt, rows[:, :2], [1, 2, 0], 0, 0, False, 4, EO.MOTION_AUG)
    assert np.array_equal(mot["refs"], [gt[0], np.zeros(15), gt[6], gt[6], gt[3], gt[6]]) and mot["offs"].shape == (3, 4) and mot["aug"].shape == (6, 6)
    assert "aug" not in EO.draw(gt, rows[:, :2], [1, 2, 0], 0, 0, False, 4, EO.MOTION)
