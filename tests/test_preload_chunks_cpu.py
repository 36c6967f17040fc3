"""The one cut rule of the dataset readers (open3dsot_amd/datasets.py: preload_chunks) and the shared / per-user boxes of a
frame (frame_boxes), on the host: hand-written items, limits small enough to bind, the expected cuts written out."""
import numpy as np

from open3dsot_amd import datasets as D


def item(name, n=1, k=1, group=None):
    return D.PreloadItem(name, n, np.zeros((k, 6), np.float32), [[(0, 0)]] * k, group)


def cuts(items, chunk_frames=64, **limits):
    return [[it.source for it in chunk] for chunk in D.preload_chunks(items, chunk_frames, **limits)]


def test_the_limits_default_to_the_library_s():
    import inspect
    from open3dsot_amd import points_utils as PU
    p = inspect.signature(D.preload_chunks).parameters
    assert (p["max_rows"].default, p["max_records"].default, p["max_boxes"].default) == \
        (PU.PRELOAD_MAX_ROWS, PU.PRELOAD_MAX_FRAMES, PU.PRELOAD_MAX_BOXES)


def test_chunk_frames():
    assert cuts([item(i) for i in range(7)], 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert cuts([item(i) for i in range(6)], 3) == [[0, 1, 2], [3, 4, 5]]
    assert cuts([item(i) for i in range(3)], 1) == [[0], [1], [2]]


def test_raw_rows():
    """the oversize item is alone and is not refused here: preload_plan refuses it"""
    items = [item("a", 4), item("b", 4), item("c", 4), item("d", 11), item("e", 1)]
    assert cuts(items, max_rows=10) == [["a", "b"], ["c"], ["d"], ["e"]]
    assert cuts([item("a", 5), item("b", 5), item("c", 1)], max_rows=10) == [["a", "b"], ["c"]]      # exactly the limit fits


def test_records():
    """k boxes are max(1, ceil(k / max_boxes)) records; no box is one record all the same"""
    assert cuts([item("a", k=1), item("b", k=5), item("c", k=1)], max_boxes=2, max_records=3) == [["a"], ["b"], ["c"]]
    assert cuts([item("a", k=1), item("b", k=4), item("c", k=1)], max_boxes=2, max_records=3) == [["a", "b"], ["c"]]
    assert cuts([item("a", k=0), item("b", k=0), item("c", k=0)], max_boxes=2, max_records=2) == [["a", "b"], ["c"]]
    assert cuts([item("a", k=0), item("b", k=2), item("c", k=3)], max_boxes=2, max_records=2) == [["a", "b"], ["c"]]


def test_groups():
    items = [item("a", group="0019"), item("b", group="0019"), item("c", group="0020"), item("d", group="0020"), item("e", group="0019")]
    assert cuts(items) == [["a", "b"], ["c", "d"], ["e"]]
    assert cuts([item(i) for i in range(5)]) == [[0, 1, 2, 3, 4]]          # no key: never cut at a group change
    assert cuts(items, 1) == [["a"], ["b"], ["c"], ["d"], ["e"]]


def test_two_limits_at_one_item_cut_once():
    items = [item("a", 6, 2, "x"), item("b", 6, 2, "y"), item("c", 1, 1, "y")]     # b: another group, too many rows and records
    assert cuts(items, 2, max_rows=10, max_records=3, max_boxes=1) == [["a"], ["b", "c"]]
    items = [item("a", 6, 2), item("b", 6, 2), item("c", 6, 2)]                    # full by chunk_frames where the rows bind too
    assert cuts(items, 1, max_rows=10) == [["a"], ["b"], ["c"]]


def test_empty_input():
    assert cuts([]) == [] and cuts(iter(())) == []


def test_items_are_pulled_lazily_and_once():
    """when a chunk arrives, at most one item beyond those received has been pulled; nothing is pulled twice"""
    for chunk_frames, limits in ((3, {}), (64, dict(max_rows=10)), (2, dict(max_rows=7)), (64, dict(max_records=2))):
        pulled = []

        def source():
            for i, n in enumerate([4, 4, 4, 11, 1, 3, 3, 3]):
                pulled.append(i)
                yield item(i, n)
        received = 0
        for chunk in D.preload_chunks(source(), chunk_frames, **limits):
            received += len(chunk)
            assert len(pulled) <= received + 1, (chunk_frames, limits)
        assert pulled == list(range(8)) and received == 8
    pulled = []
    chunks = D.preload_chunks((pulled.append(i) or item(i) for i in range(5)), 2)
    assert pulled == [] and [it.source for it in next(chunks)] == [0, 1] and pulled == [0, 1]      # full: nothing held back


def test_frame_boxes_shared_or_one_box_per_user():
    rng = np.random.default_rng(5)
    annos = [{"boxes": np.concatenate([rng.uniform(-20, 20, (3, 3)), rng.uniform(1, 4, (3, 3)), np.tile(np.eye(3).reshape(1, 9), (3, 1))], 1)}
             for _ in range(3)]
    users = [(2, 0), (0, 1), (1, 2)]
    for offset in (0, -1, -0.5):
        bounds, who = D.frame_boxes(annos, users, offset)
        assert bounds.dtype == np.float32 and bounds.shape == (1, 6)
        assert np.array_equal(bounds, [[-np.inf] * 3 + [np.inf] * 3]) and who == [users]
    for offset in (2, 0.25):
        bounds, who = D.frame_boxes(annos, users, offset)
        want = D.preload_bounds(np.stack([annos[2]["boxes"][0], annos[0]["boxes"][1], annos[1]["boxes"][2]]), offset)
        assert bounds.dtype == np.float32 and bounds.shape == (3, 6) and np.array_equal(bounds, want) and np.isfinite(bounds).all()
        assert who == [[(2, 0)], [(0, 1)], [(1, 2)]]
