"""The host-side helpers that the trackers of open3dsot_amd/tracking.py share, where no GPU is needed: the reference_BB rule,
the parsing of a set of boxes, the score settings and the one frame loop of the convenience functions."""
import types

import numpy as np
import pytest
import torch


def test_reference_rule_on_the_three_spellings_and_a_bad_one():
    from open3dsot_amd import tracking
    assert tracking._reference_rule("previous_result") == (False, 0)
    assert tracking._reference_rule("previous_gt") == (True, 1)
    assert tracking._reference_rule("current_gt") == (True, 0)
    assert tracking._reference_rule("Previous_GT") == (True, 1)            # the reference matches on the upper-cased name
    with pytest.raises(ValueError, match="reference_BB 'next_gt'"):
        tracking._reference_rule("next_gt")


def test_boxes15_takes_a_tensor_an_array_a_list_and_an_empty_list():
    from open3dsot_amd import tracking
    rng = np.random.default_rng(0)
    want = rng.standard_normal((3, 15)).astype(np.float32)
    as_list = [(b[0:3], b[3:6], b[6:15].reshape(3, 3)) for b in want]
    for given in (torch.from_numpy(want), want, want.astype(np.float64), want.reshape(-1), as_list, list(want)):
        got = tracking._boxes15(given, "cpu")
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (3, 15)
        assert np.array_equal(got.numpy(), want)
    empty = tracking._boxes15([], "cpu")
    assert empty.dtype == torch.float32 and tuple(empty.shape) == (0, 15)
    kept = tracking._boxes15(torch.from_numpy(want).double(), "meta", keep=True)      # keep: a tensor stays where it is
    assert kept.device.type == "cpu" and kept.dtype == torch.float32 and np.array_equal(kept.numpy(), want)
    assert tracking._boxes15(want, "cpu", keep=True).device.type == "cpu"


def test_score_space_defaults_and_host():
    from open3dsot_amd import tracking
    assert tracking._score_space(types.SimpleNamespace()) == (3, (0, 0, 1))
    assert tracking._score_space(types.SimpleNamespace(IoU_space=2, up_axis=[0, -1, 0])) == (2, (0, -1, 0))
    a = np.arange(3)
    assert tracking._host(a) is a and np.array_equal(tracking._host(torch.arange(3)), a)


class Stub:
    """a tracker that records its calls"""

    def __init__(self, reference_BB=None):
        self.calls = []
        if reference_BB is not None:
            self.reference_BB = reference_BB

    def init(self, frame, box):
        self.calls.append(("init", frame, box))

    def update(self, frame, *ref):
        self.calls.append(("update", frame) + ref)

    def retire(self, k):
        self.calls.append(("retire", k))


FRAMES, GT = ["f0", "f1", "f2", "f3"], ["g0", "g1", "g2", "g3"]


def test_drive_hands_refs_to_update_frame_by_frame():
    from open3dsot_amd import tracking
    trk = Stub()
    tracking._drive(trk, FRAMES, "box0")
    assert trk.calls == [("init", "f0", "box0"), ("update", "f1"), ("update", "f2"), ("update", "f3")]
    trk = Stub("previous_gt")                                              # refs as given: the rule is not asked
    tracking._drive(trk, FRAMES, "box0", GT)
    assert trk.calls == [("init", "f0", "box0"), ("update", "f1", "g1"), ("update", "f2", "g2"), ("update", "f3", "g3")]


@pytest.mark.parametrize("rule,want", [("previous_result", [(), (), ()]), ("previous_gt", [("g0",), ("g1",), ("g2",)]),
                                       ("current_gt", [("g1",), ("g2",), ("g3",)]), (None, [(), (), ()])])
def test_drive_follows_the_reference_rule_of_the_tracker(rule, want):
    from open3dsot_amd import tracking
    trk = Stub(rule)                                                       # None: a motion tracker, which has no reference_BB
    tracking._drive(trk, FRAMES, GT[0], GT, by_rule=True)
    assert trk.calls == [("init", "f0", "g0")] + [("update", f) + w for f, w in zip(FRAMES[1:], want)]


def test_drive_retires_a_target_in_front_of_its_first_invalid_frame_and_never_again():
    from open3dsot_amd import tracking
    live = np.array([[1, 1, 1], [1, 0, 1], [1, 0, 1], [0, 0, 1]], bool)     # target 1 ends at frame 1, target 0 at frame 3
    trk = Stub("current_gt")
    tracking._drive(trk, FRAMES, GT[0], GT, retire=live, by_rule=True)
    assert trk.calls == [("init", "f0", "g0"), ("retire", 1), ("update", "f1", "g1"), ("update", "f2", "g2"), ("retire", 0),
                         ("update", "f3", "g3")]
    assert all(type(c[1]) is int for c in trk.calls if c[0] == "retire")
