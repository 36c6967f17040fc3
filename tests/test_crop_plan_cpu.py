"""The one host planner of the grouped-crop tables (open3dsot_amd/crop_plan.py) without a GPU: (a) the tables of the planned
batches, of the per-batch route and of the lane epoch are, in every word that is read, those of the three planners it
replaced (sha256 constants); (b) the lane tables against the C planner and the schedule; (c) plan_groups on its own."""
import hashlib

import numpy as np
import pytest

import test_epoch_plan_cpu as EP

# ---- the inputs ------------------------------------------------------------------------------------------------------------------------
LANE_LENGTHS, L, PLAN_STEPS = (3, 1, 2, 4, 2), 2, 3        # 4 steps = chunks of 3 and 1: a one-frame tracklet, restarts, an idle tail
LANE_FN = np.array([1, 256, 257, 1000, 0, 255, 300, 513, 2, 512, 40, 768], np.int64)       # the frame sizes of the 12 pool rows
LANE_FPTR = 0x7f0000000000 + 0x100000 * np.arange(12, dtype=np.int64)
ADDR = dict(cur=0x7c0000000000, gt=0x7b0000000000, counts=0x7a0000000000)
LANE_BASE = 0x790000000000
OUT, CAPS = (0x780000000000, 0x770000000000), (1000, 300)
LANE_CASES = [("matching", agg, ref) for agg in ("firstandprevious", "first") for ref in ("previous_result", "previous_gt", "current_gt")]
LANE_CASES.append(("motion", None, "previous_result"))


class Cloud:
    """a frame of the pool as the planners see it: an address and a size"""

    def __init__(self, ptr, n):
        self.ptr, self.shape = int(ptr), (int(n), 3)

    def data_ptr(self):
        return self.ptr


def lane_clouds(kind):
    """LaneTracker._clouds / MotionLaneTracker._clouds with fixed addresses: (frames back, by the reference box, scale, offset,
    mode, out, capacity, gated by has_crop)"""
    from open3dsot_amd import points_utils as PU
    if kind == "motion":
        return tuple((1 - h, True, 1.25, 2.0, PU.CROP_SUBWINDOW, OUT[h], CAPS[0], False) for h in (0, 1))
    return ((0, True, 1.25, 2.0, PU.CROP_SUBWINDOW, OUT[0], CAPS[0], False), (1, False, 1.25, 0.0, PU.CROP_MODEL, OUT[1], CAPS[1], True))


def lane_rule(ref):
    """reference_BB -> (by_gt, back)"""
    return ref != "previous_result", 1 if ref == "previous_gt" else 0


def lane_frames():
    return [[Cloud(p, n) for p, n in zip(LANE_FPTR[a:b], LANE_FN[a:b])]
            for a, b in zip(np.cumsum((0,) + LANE_LENGTHS[:-1]), np.cumsum(LANE_LENGTHS))]


def lane_chunks(kind, agg, ref):
    """-> per chunk (tables, tracklet (S,L), frame (S,L), groups, need, starts) of plan_lane_steps over the schedule"""
    from open3dsot_amd import crop_plan, points_utils as PU, tracking
    pool = crop_plan.FramePool(lane_frames())
    assert np.array_equal(pool.fptr, LANE_FPTR) and np.array_equal(pool.fn, LANE_FN)
    assert pool.row0.tolist() == [0, 3, 4, 6, 10, 12]
    js, ts = tracking.lane_schedule(LANE_LENGTHS, L)
    assert js.tolist() == [[0, 2], [0, 3], [4, 3], [-1, 3]] and ts.tolist() == [[1, 1], [2, 1], [1, 2], [0, 3]]
    by_gt, back = lane_rule(ref)
    out = []
    for s in range(0, js.shape[0], PLAN_STEPS):
        tab = crop_plan.Tables(PLAN_STEPS, {"lanes": (np.int32, (L, PU.LANE_COLS)), "plan": (PU.CROP_PLAN, (2 * L,)),
                                            "targets": (PU.CROP_TARGET, (2 * L,))}, LANE_BASE)
        got = tracking.plan_lane_steps(tab, js[s:s + PLAN_STEPS], ts[s:s + PLAN_STEPS], pool.row0, pool, lane_clouds(kind), ADDR,
                                       by_gt, back, agg != "first")
        out.append((tab, js[s:s + PLAN_STEPS], ts[s:s + PLAN_STEPS]) + tuple(got))
    return out


# ---- (a) the digests -------------------------------------------------------------------------------------------------------------------
def sha(*parts):
    """the digest of arrays; a record array field by field: the padding between its fields is nobody's to read"""
    h = hashlib.sha256()
    for a in parts:
        for col in ([a[name] for name in a.dtype.names] if a.dtype.names else [a]):
            h.update(np.ascontiguousarray(col).tobytes())
    return h.hexdigest()


def read_parts(plan, targets, groups, targets_dev):
    """what the device reads of the crop tables of S steps: per step the first groups[k] rows of plan (S,n) and the records of
    targets (S,n) they point at; the `targets` column counts from the step's own table at targets_dev + k n records, so that
    the digest does not depend on where the buffer puts its sections"""
    parts = []
    for k in range(len(groups)):
        rows = plan[k, :int(groups[k])].copy()
        rows["targets"] -= np.uint64(targets_dev + targets.dtype.itemsize * targets.shape[1] * k)
        parts += [rows, targets[k, :int(rows["n_targets"].sum())]]
    return parts


def chunk_digest(ch, S, aug):
    """of a sampler.ChunkTables that holds S batches"""
    parts = [ch.rows[:S], ch.cand[:S]] + read_parts(ch.plan, ch.targets, ch.groups[:S], ch.dev("targets"))
    if aug:
        parts += [ch.slots[:S]] + [ch.augptr[k, :int(ch.groups[k])] for k in range(S)]
    return sha(*parts, *(np.asarray(v[:S], np.int64) for v in (ch.groups, ch.need, ch.grid)))


def lane_digest(lanes, plan, targets, targets_dev, groups, starts, need):
    """of S steps of a lane chunk: the lane table, the crop tables, groups, starts and the chunk's largest scratch need"""
    return sha(lanes, *read_parts(plan, targets, groups, targets_dev), np.asarray(groups, np.int64), np.asarray(starts, np.int64),
               np.asarray([need], np.int64))


def batch_digest(plan, targets, targets_dev, need, slots=None, augptr=None):
    """of one batch of the per-batch route"""
    parts = read_parts(plan[None], targets[None], [len(plan)], targets_dev) + [np.asarray([need], np.int64)]
    return sha(*parts, *([slots, augptr[:len(plan)]] if slots is not None else []))


# How the constants were made: on the commit before crop_plan.py existed, with the helpers above,
#   PLANNED:   chunk_digest of every chunk of EP.planned_epoch(motion, aug) (sampler.plan_chunk as it was),
#   LANES:     lane_digest per chunk of _Lanes._plan_chunk called unbound on a stub object (the schedule, FramePool's arrays and
#              _lane_state's host views as attributes; cur, gt, counts_dev and the clouds' buffers objects with the constant
#              data_ptr() of ADDR / OUT; the table's device copy at LANE_BASE; scratch an empty CPU tensor, whose length after the
#              call is the chunk's need),
#   PER_BATCH: batch_digest of _DeviceBatchBuilder._crop_tables for batch s of the same epoch (the `wanted` list and, with aug,
#              the slots / augptr loop of MotionBatchBuilder.build as they were) on StandIn below.
PLANNED = {
    (False, False): [
        "0561eaccc90cde3ded69e49a8a55b9f6601356712c05c86b1abcbf706846362f",
        "377931fa2234dffc30e69ac4bec6ffd12bbb294fa447e15bc5ec1a8cac6d90ec",
        "07dea246d4a89f4af064240a76c82627dfd96743994fb19155b82123a0870035",
    ],
    (True, False): [
        "e86c8be9bebe4d63a92a065ad8dd94325954a007d42034c605f8222d20375e2f",
        "ecc9edb56d7a628379af32330bbf9aa6802cc8cf23906861878f46bd0df8d74e",
        "df79ca857139bf0d97ec8592aab00cd41d2c5ead451347f1f86c4e60fc3529ef",
    ],
    (True, True): [
        "6855fc49ca3e2ffd3691d2934be246df62d2bd170af687d11861bed35caed89f",
        "2950480a2f4e34908607182275c491b7f5b7d856269bffac678fb544c17f2575",
        "b649d9b81a52d08c4a44256d3e6cffa5aac8a3541aeb06f258ffb88acedfc342",
    ],
}
LANES = {
    ('matching', 'firstandprevious', 'previous_result'): [
        "0d67a29e12fd1a8150781c2dd3ea709b7ba77ad89fcb1662391a75933052adf9",
        "843591cfc5fb8f781e415a7ef2e4dee8d0a2bbe71f646197bf1c4a9c3b595ce5",
    ],
    ('matching', 'firstandprevious', 'previous_gt'): [
        "362fe7014d28aae9ce8db530413038e0fa1731d7265dd2202590478f17ca67ab",
        "3fc3ea539b2e11f98111ad61045c82f6de765a61ac79c841faa94e7809c29f76",
    ],
    ('matching', 'firstandprevious', 'current_gt'): [
        "5fe7aec53da37f06b3ac41222e6c0bbfb277d4f74b35236c57af8f4fe30713b6",
        "c6910b84f3f536208d9e550753f20a729ad6b34c5284454c0713e37c368a2a09",
    ],
    ('matching', 'first', 'previous_result'): [
        "51505269e6b08c492cf61e0aca320b4e11cc154b09f6b0b7ab94c00607b5b805",
        "fa577cb1878eebe5eac06a12d905fdebaaa2dbb25d0fd579a23faebd01323d95",
    ],
    ('matching', 'first', 'previous_gt'): [
        "a7170295e5c43bacf45fcf58df0f46f30925b8dc98c0da03b4f91018fa877e08",
        "0ed96464b1add0ac5845f151157f5fc7ceecda75f2f07c493fdd619b4f20f6b0",
    ],
    ('matching', 'first', 'current_gt'): [
        "b3b28bb226ff0c4ae71c993f2f343b02087e7f0999f9491d88fc976514c0f33d",
        "90aebf9ba0923b187ff84c102ca36fc3857d763aebb9a4b1f37f3c611a786090",
    ],
    ('motion', None, 'previous_result'): [
        "66870fc659806ce100e83bf671096df5276b27eecfc36d326a0bba0990a64469",
        "a41b3666f7c2f231854bdebc6204fda15dd8710401bc46b465fd5f837430e8c5",
    ],
}
PER_BATCH = {
    (False, False): [
        "3a383c5697656bec2614c108043175fd3f3a399043cda0b7111d4e97f03ec6e9",
        "29142521d5c4cd67cd374e826e74333a6655b3d2c57c94c144d0513e9187d84c",
        "3949f02abcf6db0051bfd48d2c58020d77af5ba068a29d1dc926970121419b16",
        "62118cf9ff0e76a66fdd1a8826d000a7f727a399ca88ef46d89957ad0bfd116a",
        "7036552b310587072d254be41c76f06b3cbbbf953ef7c10eae718ce4ccda5b60",
        "9fdd27dc5f597cf0345c24fb452d9f99fc539be91d4cf09fd4007b63711d3ab6",
        "e2ebb8bb0ca0010bd02476de5433344c7e08fc862c2dff3a0953da1475037af3",
        "3575ddca076554954defafe4200e5dccfbfed42bf44669786a932267b46c96df",
    ],
    (True, False): [
        "3a383c5697656bec2614c108043175fd3f3a399043cda0b7111d4e97f03ec6e9",
        "7a66682803c83adbc880c0ea522ecb7eb32ac6f625de2b9171d93f05b108ab6e",
        "a9f6c52d32839ed777aa50691768a9cd150ad1608da0479ca3c9f07bb74d3a94",
        "ea091529944c93a07a5dc6c3ebad2349223238d9e7df6a3d12312f83a10d4dde",
        "e74007e06bf4c2072e5dc446ba73fa34b13022abce153ce355ffe494c86ef421",
        "f4c8c16d20696786bbb09b3802e7c2a42e5192ba3f4b67b76d4de7afe758586a",
        "562960c64c4d1d0cf69348ba0a8fdc3a0bc0242fe0644c14d9b5dc7a6517a0c0",
        "8135b70f939d0631df3138f70f19ea811a6672cffa3406797566941403a02cc9",
    ],
    (True, True): [
        "4c5916721b4a42c3f13412e31b71748e9f0246705c7d89566c6b5d52c44c38fa",
        "4c4a2f3a473d72cd250a37b7cf4a901da813da3beff159d6bf6e19e682785676",
        "f2277e79efd2bf563290e3933f924bd93a7228a5bde425dd66f523ada526d754",
        "5dc3c41589e02291c5a7387700fbb296e2e2074bbbdf37a23637419251f3401c",
        "5dd42e37ff91feebc51a6384ac5e58699e480e4f61fbb7557d6b823faad21fd6",
        "2b5ced1eb2309dd1464a410cfe1a72b3e5da70f6d4cb88e640d30d1d3ee1f03a",
        "3db52818e5e5b3a0f0a04bc3a32910824df695139511d90a172603f21b2aaab9",
        "3f8f06e61e5c80a6a347002dcceec09457964c0f90c07af714830524ad5c2447",
    ],
}


@pytest.mark.parametrize("motion,aug", [(False, False), (True, False), (True, True)])
def test_planned_chunks_are_the_parents(motion, aug):
    chunks, _, _ = EP.planned_epoch(motion, aug)
    assert [chunk_digest(ch, rows.shape[0], aug) for ch, rows, _ in chunks] == PLANNED[motion, aug]


@pytest.mark.parametrize("case", LANE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_lane_chunks_are_the_parents(case):
    got = []
    for tab, js, ts, groups, need, starts in lane_chunks(*case):
        S = js.shape[0]
        got.append(lane_digest(tab.view("lanes")[:S], tab.view("plan"), tab.view("targets"), tab.dev("targets"), groups, starts,
                               need.max()))
    assert got == LANES[case]


def stand_in(motion, aug):
    """a batch builder whose pinned views and uploaded buffer are host memory at a fixed address: what _crop_tables needs"""
    import torch
    from open3dsot_amd import crop_plan, points_utils as PU, sampler

    class StandIn(sampler.MotionBatchBuilder if motion else sampler.SiameseBatchBuilder):
        def __init__(self):
            self.J, self.augment, self.device = EP.J, aug, torch.device("cpu")
            self._rec = EP.fixed_records(PU)
            self._layout = {"_end": 0}
            for name, nbytes in (("slots", 3 * EP.J * 4), ("augptr", 3 * EP.J * 8), ("targets", 3 * EP.J * PU.CROP_TARGET.itemsize),
                                 ("plan", 3 * EP.J * PU.CROP_PLAN.itemsize)):
                crop_plan._section(self._layout, name, nbytes)
            self._host = np.zeros(self._layout["_end"], np.uint8)
            self._scratch = torch.zeros(1 << 12, dtype=torch.int32)
            self._aug = Cloud(EP.AUG_BASE, 0)

        def _view(self, slot, name, dtype, shape):
            off, nbytes = self._layout[name]
            return self._host[off:off + nbytes].view(dtype).reshape(shape)

        def _dev(self, name):
            return EP.BASE + self._layout[name][0]

        def reserve_scratch(self, need):
            self.need = need
    return StandIn()


def epoch_samples(motion):
    """the batches of planned_epoch's epoch as the tuples build() takes: DeviceBatchSampler.samples on the planned arrays"""
    from open3dsot_amd import sampler
    starts = np.concatenate([[0], np.cumsum(EP.LENGTHS)])
    tracklets = [EP.FakeTracklet(n) for n in EP.LENGTHS]
    for t, a in zip(tracklets, starts):
        t.frames = [Cloud(p, n) for p, n in zip(EP.FPTR[a:a + len(t)], EP.FN[a:a + len(t)])]
    it = sampler.DeviceBatchSampler(tracklets, EP.FakeBuilder(motion, EP.J, 5), shuffle=True, plan_batches=EP.P)
    order = sampler.epoch_order(it.length, EP.J, True, 11, 0)
    it._trk, it._frames, it._cand = sampler.epoch_frames(order, starts, 5, motion)
    return [it.samples(s) for s in range(order.shape[0])]


@pytest.mark.parametrize("motion,aug", [(False, False), (True, False), (True, True)])
def test_per_batch_tables_are_the_parents(motion, aug):
    from open3dsot_amd import points_utils as PU
    b, got = stand_in(motion, aug), []
    for samples in epoch_samples(motion):
        plan, order = b._crop_tables(0, samples)
        extra = {}
        if aug:
            b._aug_tables(0, plan, order)
            extra = dict(slots=b._view(0, "slots", np.int32, (3 * EP.J,)), augptr=b._view(0, "augptr", np.uint64, (3 * EP.J,)))
        got.append(batch_digest(plan, b._view(0, "targets", PU.CROP_TARGET, (3 * EP.J,)), b._dev("targets"), b.need, **extra))
    assert got == PER_BATCH[motion, aug]


# ---- (b) the lane planner against the C planner and the schedule -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", LANE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_lane_tables_against_the_c_planner_and_the_schedule(case):
    from open3dsot_amd import points_utils as PU
    kind, agg, ref = case
    by_gt, back = lane_rule(ref)
    clouds = lane_clouds(kind)
    row0 = np.concatenate([[0], np.cumsum(LANE_LENGTHS)])
    idle = restarts = 0
    for c, (tab, js, ts, groups, need, starts) in enumerate(lane_chunks(*case)):
        S = js.shape[0]
        assert S == (3, 1)[c] and groups.shape == need.shape == starts.shape == (S,)
        lanes, targets = tab.view("lanes"), tab.view("targets")
        for k in range(S):
            G = int(groups[k])
            plan = tab.view("plan")[k, :G]
            mine = plan.copy()
            for name in ("wg_start", "row_start", "sbase"):
                mine[name] = -1
            c_need, c_grid, scan = PU.crop_groups_plan(mine) if G else (0, 0, 0)
            assert np.array_equal(mine, plan) and need[k] == c_need and (plan["n_targets"] == 1).all()
            seen = {}
            t0 = tab.dev("targets", k)
            assert t0 == LANE_BASE + tab._layout["targets"][0] + k * 2 * L * PU.CROP_TARGET.itemsize
            for g in range(G):
                pos = (int(plan["targets"][g]) - t0) // PU.CROP_TARGET.itemsize
                assert pos == g == plan["row_start"][g]
                t = targets[k, pos]
                l, cl = divmod(int(t["count"]) - ADDR["counts"], 8)
                cl //= 4
                assert int(t["count"]) == ADDR["counts"] + 8 * l + 4 * cl and 0 <= l < L and cl in (0, 1) and (l, cl) not in seen
                seen[l, cl] = g
                shift, by_ref, scale, offset, mode, out, cap, gated = clouds[cl]
                j, f = int(js[k, l]), int(ts[k, l])
                row = int(row0[j]) + f
                assert j >= 0 and plan["points"][g] == LANE_FPTR[row - shift] and plan["n"][g] == LANE_FN[row - shift]
                want_box = ADDR["gt"] + 60 * (row - back) if by_ref and by_gt else ADDR["cur"] + 60 * l
                assert int(t["box"]) == want_box
                assert (t["scale"], t["offset"], t["mode"], int(t["out"]), t["capacity"]) == (np.float32(scale), np.float32(offset),
                                                                                               mode, out + 12 * cap * l, cap)
            # every active (lane, cloud) exactly once (a gated cloud only where the step has a crop), an idle lane nowhere
            want = set()
            for l in range(L):
                on, first = js[k, l] >= 0, js[k, l] >= 0 and ts[k, l] == 1
                has_crop = on and (first or agg != "first")
                row = int(row0[js[k, l]]) + int(ts[k, l]) if on else -1
                want |= {(l, cl) for cl in (0, 1) if on and (has_crop or not clouds[cl][7])}
                assert lanes[k, l].tolist() == [on, first, has_crop, ts[k, l], row, row - back if on and by_gt else -1, on and by_gt]
                idle += not on
                restarts += bool(first and k > 0)
            assert set(seen) == want and sorted(seen, key=seen.get) == sorted(seen, key=lambda lc: lc[1] * L + lc[0])
            assert starts[k] == bool(lanes[k, :, PU.LANE["first"]].any())
    assert idle == 1 and restarts == 2


# ---- (c) plan_groups on its own ----------------------------------------------------------------------------------------------------------
def run_plan_groups(key, frame, fn, valid=None):
    from open3dsot_amd import crop_plan, points_utils as PU
    key = np.asarray(key, np.int64)
    S, n = key.shape
    rec = np.zeros(n, PU.CROP_TARGET)
    rec["capacity"] = np.arange(n)
    targets, plan = np.zeros((S, n), PU.CROP_TARGET), np.zeros((S, n), PU.CROP_PLAN)
    fn = np.asarray(fn, np.int64)
    groups, need, grid, order = crop_plan.plan_groups(key, frame, rec, 4096 * (1 + np.arange(fn.size)), fn, targets, plan, 1 << 20,
                                                      valid)
    assert np.array_equal(targets["capacity"], order)
    return groups, need, grid, order, plan


def test_plan_groups_distinct_keys_give_groups_of_one():
    groups, need, grid, order, plan = run_plan_groups([[3, 1, 2, 0]], [[0, 1, 2, 3]], [1, 256, 257, 1000])
    assert groups.tolist() == [4] and order.tolist() == [[3, 1, 2, 0]] and (plan["n_targets"][0] == 1).all()
    assert plan["n"][0].tolist() == [1000, 256, 257, 1] and plan["points"][0].tolist() == [4096 * 4, 4096 * 2, 4096 * 3, 4096]
    assert plan["wg_start"][0].tolist() == [0, 4, 5, 7] and plan["sbase"][0].tolist() == [0, 4, 5, 7] and need.tolist() == grid.tolist() == [8]
    assert plan["row_start"][0].tolist() == [0, 1, 2, 3] and plan["targets"][0].tolist() == [(1 << 20) + 48 * i for i in range(4)]


def test_plan_groups_equal_keys_give_one_group():
    groups, need, grid, order, plan = run_plan_groups([[5, 5, 5], [7, 7, 7]], [[1, 1, 1], [0, 0, 0]], [513, 257])
    assert groups.tolist() == [1, 1] and order.tolist() == [[0, 1, 2]] * 2 and plan["n_targets"][:, 0].tolist() == [3, 3]
    assert plan["n"][:, 0].tolist() == [257, 513] and need.tolist() == [6, 9] and grid.tolist() == [2, 3]
    assert plan["targets"][:, 0].tolist() == [1 << 20, (1 << 20) + 3 * 48] and not plan["wg_start"][:, 0].any()


def test_plan_groups_drops_invalid_records_and_an_empty_step():
    valid = np.array([[False, True, False, True], [False] * 4, [True] * 4])
    groups, need, grid, order, plan = run_plan_groups([[0, 1, 2, 3]] * 3, [[0, 0, 1, 1]] * 3, [300, 0], valid)
    assert groups.tolist() == [2, 0, 4] and need.tolist() == grid.tolist() == [3, 0, 6]
    assert order[0].tolist() == [1, 3, 0, 2] and order[2].tolist() == [0, 1, 2, 3]             # the valid ones first, in their order
    assert plan["n"][0, :2].tolist() == [300, 0] and plan["wg_start"][0, :2].tolist() == [0, 2]
    assert plan["wg_start"][2].tolist() == [0, 2, 4, 5] and not plan[1].view(np.uint8).any()  # the empty step writes no row


def test_plan_groups_an_empty_cloud_takes_one_workgroup():
    groups, need, grid, order, plan = run_plan_groups([[0, 0, 1]], [[0, 0, 1]], [0, 0])
    assert groups.tolist() == [2] and plan["n"][0, :2].tolist() == [0, 0] and plan["n_targets"][0, :2].tolist() == [2, 1]
    assert plan["wg_start"][0, :2].tolist() == [0, 1] and plan["sbase"][0, :2].tolist() == [0, 2] and need.tolist() == [3] and grid.tolist() == [2]


def test_frame_pool_worst_scratch():
    from open3dsot_amd import crop_plan
    pool = crop_plan.FramePool(lane_frames())
    assert pool.wgs.tolist() == [1, 1, 2, 4, 1, 1, 2, 3, 1, 2, 1, 3]
    assert pool.worst_scratch(np.array([[0, 1, -1], [3, 3, 7], [-1, -1, -1]])) == 11 and pool.worst_scratch(np.zeros((0, 4))) == 0
