"""What every tracker of open3dsot_amd/tracking.py launches, call by call (tools/tracker_trace.py on its fourteen configurations):
the ordered C entries, the host stops and the upload counters of every init / update / step / event equal
tests/golden/tracker_launches.json, recorded before the frame bodies were folded into one feed per model family and one frame per
loop shape.  A change of the frame order shows here as a diff of entry lists."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tracker_trace as TT  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def traced():
    """one run of all configurations, shared by the tests"""
    return TT.launches(TT.run(ROOT))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "tracker_launches.json")) as fh:
        return json.load(fh)


def frames_of(calls):
    return [c for c in calls if c["call"].split()[0] in ("update", "step")]


def test_all_fourteen_configurations_ran(traced, recorded):
    assert len(TT.CONFIGS) == 14 and sorted(traced) == sorted(TT.CONFIGS) == sorted(recorded)


@pytest.mark.parametrize("name", sorted(TT.CONFIGS))
def test_entries_host_stops_and_counters_equal_the_recorded_ones(traced, recorded, name):
    got, want = traced[name], recorded[name]
    assert [c["call"] for c in got] == [c["call"] for c in want]
    for g, w in zip(got, want):
        assert g["entries"] == w["entries"], (name, g["call"])
        assert g == w, (name, g["call"])                   # the host stops and every counter the class has


def test_a_scene_frame_without_an_event_uploads_nothing_and_never_stops_the_host(traced):
    scenes = [name for name, (_, loop, _) in TT.CONFIGS.items() if loop == "scene"]
    assert len(scenes) == 4
    for name in scenes:
        frames = frames_of(traced[name])
        assert [f["call"] for f in frames] == ["update %d" % t for t in range(1, TT.SCENE_FRAMES)]
        # the lane table changes at frame 1 (every slot's first frame), 2 (no slot's), 3 (the enrolled slot's) and 4 (no slot's)
        assert [f["lane_uploads"] for f in frames] == [1, 2, 3, 4, 4], name
        assert [f["crop_calls"] for f in frames] == [1, 2, 3, 4, 5], name
        assert frames[-1]["host_stops"] == 0, name
        assert all(f["host_stops"] == 0 for f in frames[1:]), name         # update 1 captures the graph, which synchronises


def test_a_managed_frame_uploads_no_lane_table(traced):
    for name, (_, loop, _) in TT.CONFIGS.items():
        if loop == "managed":
            calls = traced[name]
            assert all(c["lane_uploads"] == 0 for c in calls), name
            assert all(c["host_stops"] == 0 for c in frames_of(calls)[1:]), name
            assert [c["entries"][-1] for c in frames_of(calls)] == ["scene_manage"] * (TT.FRAMES - 1), name      # after the box update


def test_every_free_running_frame_has_one_crop_entry_and_one_box_update(traced):
    for name, (_, loop, sampling) in TT.CONFIGS.items():
        if sampling == "reference":
            continue
        frames = frames_of(traced[name])
        assert frames, name
        for f in frames:
            assert sum(e in TT.CROPS for e in f["entries"]) == 1, (name, f["call"])
            assert sum(e in TT.BOX_UPDATES for e in f["entries"]) == 1, (name, f["call"])
