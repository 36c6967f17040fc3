"""The planned training epoch on the GPU: o3d_train_draw against its numpy restatement (tests/epoch_plan_oracle.py), the planned
build against the per-batch build teacher-forced with the planned route's own draws (bit for bit), chunk invariance, two
epochs, and a training step on a planned batch."""
import numpy as np
import pytest
import torch

import epoch_plan_oracle as EO

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def up(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---- (5) o3d_train_draw per call -------------------------------------------------------------------------------------------------------
R, SPARE = 7, 3


def within_one_ulp(got, want):
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("degrees,num_candidates", [(True, 4), (False, 1)])
@pytest.mark.parametrize("mode", [EO.SIAMESE, EO.MOTION, EO.MOTION_AUG])
@pytest.mark.parametrize("J", [1, 5, 257])
def test_train_draw_against_the_oracle(dev, J, mode, degrees, num_candidates):
    from open3dsot_amd import points_utils as PU
    rng = np.random.default_rng(1000 * J + 10 * mode + num_candidates)
    cols = 3 if mode == EO.SIAMESE else 2
    gt = rng.uniform(-30, 30, (R, 15)).astype(f32)
    rows = rng.integers(0, R, (J, cols)).astype(np.int32)
    cand = (np.arange(J) % 4).astype(np.int32)                # ids 0 and others, whatever num_candidates says
    rows[0] = [0, R - 1, R][:cols] if cols == 3 else [0, R]   # the first row, the last, one past the pool
    if J >= 5:
        rows[1], rows[2], rows[3] = 3, [R - 1, -1, 0][:cols], [0, R - 1, 5][:cols]          # a repeated row, one before the pool
        cand[4] = 0
    seed, counter = 0x9ABCDEF1, 0xFFFFFFF0 + J                 # both use the high bit
    shapes = {"refs": (2 * J, 15), "first": (J, 15), "offs": (2 * J if mode == EO.SIAMESE else J, 4), "aug": (2 * J, 6)}
    used = {"refs", "offs"} | ({"first"} if mode == EO.SIAMESE else set()) | ({"aug"} if mode == EO.MOTION_AUG else set())
    out = {k: torch.full((shapes[k][0] + SPARE, shapes[k][1]), float("nan"), dtype=torch.float32, device=dev) for k in used}
    PU.train_draw(up(gt, dev), up(rows, dev), up(cand, dev), J, seed, counter, degrees, num_candidates, mode, out["refs"],
                  out.get("first"), out["offs"], out.get("aug"))
    torch.cuda.synchronize()
    want = EO.draw(gt, rows, cand, seed, counter, degrees, num_candidates, mode)
    assert set(want) == used
    for k in used:
        got = out[k].cpu().numpy()
        n = shapes[k][0]
        assert np.isnan(got[n:]).all(), k                      # the spare rows behind the output
        assert not np.isnan(got[:n]).any(), k
        got = got[:n]
        if k in ("refs", "first"):
            assert np.array_equal(got.view(np.int32), want[k].view(np.int32)), k             # gathered boxes: exact
            continue
        zero = ~want[k].any(1)
        assert not got[zero].any(), k                          # the zero rows: exact
        if k == "offs":
            assert not got[:, 2].any() and within_one_ulp(got, want[k])
            assert zero[:J].tolist() == (cand == 0).tolist()
            if mode == EO.SIAMESE:
                assert zero[J:].tolist() == ((cand == 0) & (num_candidates > 1)).tolist()
        else:
            assert np.array_equal(got[:, 4:], want[k][:, 4:]) and within_one_ulp(got[:, :4], want[k][:, :4])      # flips: exact
            assert not zero.any()
    assert ((rows < 0) | (rows >= R)).any()                    # whose boxes the oracle gives as zeros: compared above


# ---- the epochs of tests 6 - 9: three tracklets of 4, 4 and 1 frames of 3 000 points -----------------------------------------------------------
B, J = 4, 5
KINDS = {"bat": dict(template_size=64, search_size=128), "p2b": dict(template_size=64, search_size=128, box_aware=False),
         "motion_aug": dict(point_sample_size=128), "motion_plain": dict(point_sample_size=128, use_augmentation=False)}


@pytest.fixture(scope="module")
def tracklets(dev):
    from open3dsot_amd import sampler, synth
    seqs = [synth.make_sequence(900 + i, n, 3000) for i, n in enumerate((4, 4, 1))]
    return sampler.DeviceTracklets([s[0] for s in seqs], [s[1] for s in seqs], device=dev)


def make_builder(kind, seed=3, **kw):
    from open3dsot_amd import sampler
    if kind.startswith("motion"):
        return sampler.MotionBatchBuilder(dict(sampler.MOTION_DATA_KEYS, **KINDS[kind]), B, candidates=J, capacity=1024, seed=seed, **kw)
    return sampler.SiameseBatchBuilder(dict(sampler.DATA_KEYS, **KINDS[kind]), B, candidates=J, capacity=1024, seed=seed, **kw)


def snapshot(builder, batch):
    """a build's outputs and the builder's intermediate results, cloned (the next build overwrites them)"""
    got = {k: v.clone() for k, v in batch.items()}
    got.update(sel=builder.sel.clone(), counts=builder.counts.clone())
    return got


def refuse(*a, **k):
    raise AssertionError("the planned route made a per-batch upload or a numpy Generator while a batch was built")


class Refuse:
    def __getattr__(self, name):
        refuse()


_EPOCHS = {}


def planned_epochs(tracklets, kind, P, epochs=1):
    """the batches of `epochs` shuffled planned epochs (computed once per (kind, P) and shared): per epoch a list of
    (snapshot, the draws read back, the samples as build() takes them), and the uploads of every epoch.  While __next__ runs,
    the per-batch upload and every numpy Generator are replaced by refusals."""
    from open3dsot_amd import sampler
    if (kind, P, epochs) in _EPOCHS:
        return _EPOCHS[kind, P, epochs]
    builder = make_builder(kind)
    it = sampler.DeviceBatchSampler(tracklets, builder, seed=21, shuffle=True, plan_batches=P)
    assert len(it) == 36 // J
    result, uploads = [], []
    for _ in range(epochs):
        iter(it)                                               # begins the next epoch: epoch 0 first
        assert it.batches == len(it) == 7
        keep = builder._upload, builder.rng, sampler.np.random.default_rng
        builder._upload, builder.rng, sampler.np.random.default_rng = refuse, Refuse(), refuse
        try:
            batches = []
            for s in range(it.batches):
                got = snapshot(builder, next(it))
                draws = {k: (v.clone() if v is not None else None) for k, v in builder.draws().items()}
                batches.append((got, draws, s))
            with pytest.raises(StopIteration):
                next(it)
        finally:
            builder._upload, builder.rng, sampler.np.random.default_rng = keep
        torch.cuda.synchronize()
        result.append([(got, draws, it.samples(s)) for got, draws, s in batches])
        uploads.append(it.uploads)
    _EPOCHS[kind, P, epochs] = (result, uploads)
    return result, uploads


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- (6) planned build == teacher-forced per-batch build ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_planned_build_equals_the_teacher_forced_build(tracklets, kind):
    (epoch,), _ = planned_epochs(tracklets, kind, 3)
    teacher = make_builder(kind)                                # the same seed; its counter runs with the planned builder's
    motion = kind.startswith("motion")
    valid = 0
    for got, draws, samples in epoch:
        offs = draws["offs"].cpu().numpy()
        if motion:
            forced = {"offset": offs[:, [0, 1, 3]]}
            if draws["aug"] is not None:
                forced.update(aug_prev=draws["aug"][:J].cpu().numpy(), aug_this=draws["aug"][J:].cpu().numpy())
        else:
            forced = {"offset_t": offs[:J][:, [0, 1, 3]], "offset_s": offs[J:][:, [0, 1, 3]]}
        same(got, snapshot(teacher, teacher.build(samples, draws=forced)))
        assert int(got["n_valid"]) >= B and int(got["overflow"]) == 0 and got["sel"].min() >= 0
        valid += int(got["n_valid"])
        keys = ("points",) if motion else ("template_points", "search_points")
        assert all(bool(got[k].any()) for k in keys)
        assert (kind == "motion_aug") == (draws["aug"] is not None)
        assert ("points2cc_dist_t" in got) == (kind == "bat") and ("prev_bc" in got) == motion
    assert valid == 7 * J                                      # 3 000-point frames: every candidate is valid
    # shuffled: in order, the 5 candidates of a batch come from at most 2 annotations
    assert max(len({(id(s[0]), s[-2]) for s in samples}) for _, _, samples in epoch) >= 3


# ---- (7) chunk invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bat", "motion_aug"])
def test_batches_do_not_depend_on_the_chunking(tracklets, kind):
    (base,), uploads = planned_epochs(tracklets, kind, 3)
    assert uploads == [3]
    for P, want in ((1, 7), (8, 1)):
        (other,), uploads = planned_epochs(tracklets, kind, P)
        assert uploads == [want] and len(other) == len(base) == 7
        for (a, da, sa), (b, db, sb) in zip(base, other):
            same(a, b)
            assert [s[1:] for s in sa] == [s[1:] for s in sb] and all(x[0] is y[0] for x, y in zip(sa, sb))
            assert all(torch.equal(da[k], db[k]) for k in da if da[k] is not None)


# ---- (8) two epochs ------------------------------------------------------------------------------------------------------------------------
def test_two_epochs_differ_and_reproduce(tracklets):
    (e0, e1), uploads = planned_epochs(tracklets, "p2b", 3, epochs=2)
    assert uploads == [3, 3]
    assert [[s[1:] for s in x[2]] for x in e0] != [[s[1:] for s in x[2]] for x in e1]       # another order
    assert not any(torch.equal(a[0]["search_points"], b[0]["search_points"]) for a, b in zip(e0, e1))
    (first,), _ = planned_epochs(tracklets, "p2b", 3)          # another sampler and builder of the same seeds: epoch 0 again
    for a, b in zip(e0, first):
        same(a[0], b[0])
    _EPOCHS.pop(("p2b", 3, 2))
    (f0, f1), _ = planned_epochs(tracklets, "p2b", 3, epochs=2)   # and both epochs, from a third
    for a, b in zip(e0 + e1, f0 + f1):
        same(a[0], b[0])


def test_random_sample_plans_an_epoch(tracklets):
    from open3dsot_amd import sampler
    it = sampler.DeviceBatchSampler(tracklets, make_builder("p2b"), random_sample=True, seed=4, sample_per_epoch=5, plan_batches=2)
    batches = list(it)
    assert len(batches) == len(it) == 4 and it.uploads == 2 and all(int(b["n_valid"]) >= B for b in batches)
    frames = np.concatenate([it._frames[s] for s in range(4)])
    lengths = np.array([len(tracklets[t]) for t in it._trk.reshape(-1)])
    assert not frames[:, 0].any() and ((frames[:, 1] != frames[:, 2]) | (lengths == 1)).all()


# ---- (9) one training step per model family ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("family", ["BAT", "M2TRACK"])
def test_training_step_on_a_planned_batch(tracklets, dev, family, graph):
    """three DataParallelStep steps (the third one replays the captured graph) at batch 2 on planned batches: finite losses"""
    from open3dsot_amd import dist as D, m2track, sampler, trackers
    if family == "BAT":
        builder = sampler.SiameseBatchBuilder(sampler.DATA_KEYS, 2, candidates=2, capacity=4096, seed=2)
    else:
        builder = sampler.MotionBatchBuilder(dict(sampler.MOTION_DATA_KEYS, point_sample_size=256), 2, candidates=2, capacity=4096, seed=2)
    it = iter(sampler.DeviceBatchSampler(tracklets, builder, seed=1, shuffle=True, plan_batches=2))
    batches = [{k: v.clone() for k, v in next(it).items()} for _ in range(3)]
    assert all(int(b["n_valid"]) == 2 for b in batches)          # J = B: every candidate is valid
    torch.manual_seed(4)
    model = (trackers.BAT() if family == "BAT" else m2track.M2TRACK()).to(dev).train()
    step = D.DataParallelStep(model, world=1, graph=graph, graph_warmup=1, require_graph=graph)      # the model's own optimizer
    losses = [float(step.step(batches[i], next_batch=batches[i + 1] if i < 2 else None)) for i in range(3)]
    assert (step.graph is not None) == graph, step.graph_error
    assert all(np.isfinite(l) and l > 0 for l in losses), losses
