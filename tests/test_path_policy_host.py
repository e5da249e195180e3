"""The kernel-path planner (airwave_amd/csrc/host/path_policy.hpp) on the CPU: compiled with plain g++ (tests/emu/emu_path_policy.cpp) and
replayed against tests/golden/path_policy_parent.json — the decisions the library made on the MI355X before the policy moved into the
planner, recorded by tools/policy_table.py through info().  Every row, every field; the file's header carries the device's compute-unit
and persistent-workgroup counts."""
import json
import os
import sys

import pytest

from policy_points import LONG_HRIR_PATHS, LONG_HRIR_STREAMS, WINDOW_POLICY

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_path_policy as pp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "path_policy_parent.json")))


def test_creation_rows(recorded):
    head = recorded["header"]
    assert head["create_columns"] == ["channels", "taps", "streams", "knob_set", "path", "fft", "hop", "partitions", "history", "overlap_add_rows_policy"]
    wrong = []
    for C, taps, S, ks, *want in recorded["create"]:
        p = pp.Plan(C, taps, S, head["knob_sets"][ks])
        got = [p.path, p.fft, p.hop, p.partitions, p.hist_len, p.ola_h]
        if got != want:
            wrong.append(((C, taps, S, head["knob_sets"][ks]), got, want))
    assert len(recorded["create"]) > 2000 and not wrong, (len(wrong), wrong[:20])


def test_call_rows(recorded):
    """One spatializer per run of rows with the same key: reserve() builds the tables of the plan for its length, from then on calls of
    up to that length choose among those; info()'s overlap-add rows are those of the last call that ran a fused tile."""
    head = recorded["header"]
    assert head["call_columns"] == ["channels", "taps", "streams", "knob_set", "reserved", "frames", "long_window_rows", "long_window_rows_rest", "overlap_add_rows"]
    cus, wgs, bit = head["cus"], head["persistent_wgs"], {R: 1 << i for i, R in enumerate(pp.lw_rows())}
    wrong, key, n = [], None, 0
    for C, taps, S, ks, reserved, frames, *want in recorded["calls"]:
        if key != (C, taps, S, ks, reserved) or frames <= last_frames:          # (call lengths ascend within one spatializer)
            key = (C, taps, S, ks, reserved)
            p = pp.Plan(C, taps, S, head["knob_sets"][ks])
            have, reserved_frames, last_ola = 0, 0, 0
            if reserved:
                for R in p.lw_choose(head["reserve"], cus, for_reserve=True):
                    have |= bit.get(R, 0)
                reserved_frames = head["reserve"]
        last_frames = frames
        lw = p.lw_choose(frames, cus, reserved_frames, have)
        for R in lw:
            have |= bit.get(R, 0)                                               # a call builds the tables it lacks
        if not lw[0] and p.path == 0:
            last_ola = p.ola_h if p.use_ola_tile(frames, wgs) else 0
        got = [lw[0], lw[1], last_ola]
        n += 1
        if got != want:
            wrong.append(((C, taps, S, head["knob_sets"][ks], reserved, frames), got, want))
    assert n > 1000 and not wrong, (len(wrong), wrong[:20])


@pytest.mark.parametrize("channels,taps,streams,fft", WINDOW_POLICY)
def test_window_policy_points(channels, taps, streams, fft):
    p = pp.Plan(channels, taps, streams)
    assert (p.path, p.fft) == (0, fft)


@pytest.mark.parametrize("taps,channels,path,fft", LONG_HRIR_PATHS)
def test_long_hrir_path_points(taps, channels, path, fft):
    p = pp.Plan(channels, taps, LONG_HRIR_STREAMS)
    assert (p.path, p.fft) == (path, fft)


def test_overlap_add_tile_stops_at_its_byte_offsets():
    """The tile addresses a stream with 32-bit byte offsets: one frame past them the call runs the overlap-save tile (too long a
    stream to record on a device: the rule alone, every block count satisfied)."""
    p = pp.Plan(16, 4320, 1)
    assert p.ola_h == 7
    limit = pp.lib().pp_ola_max_bytes() // (16 * 4)
    assert p.use_ola_tile(limit, 8) and not p.use_ola_tile(limit + 1, 8)
