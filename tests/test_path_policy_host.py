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


HOP_ALIGNS = [0, 1, 2, 3, 48, 64, 100, 4096, -64, 7, 333]
HOP_TAPS = [1, 2, 3, 64, 65, 300, 1023, 1024, 2049, 3969, 4097, 4320, 4321, 4609, 5121, 5122, 6000, 6145, 6146, 8640, 8641, 12288, 12289, 20000]


def align_hop(hop_align, hop):
    """path_policy.hpp restated: values below 2 switch the rounding off, and a hop of at most 16 hop_align frames is left alone."""
    return hop - hop % hop_align if hop_align > 1 and hop > 16 * hop_align else hop


@pytest.mark.parametrize("window", [8192, 16384])
@pytest.mark.parametrize("hop_align", HOP_ALIGNS)
def test_every_hop_alignment_gives_a_plan_the_kernels_can_run(window, hop_align):
    """AW_HOP_ALIGN goes through atoi unchecked: whatever it holds, a fused plan has 0 < hop, hop + history = window, history >= taps - 1, an
    overlap-add block whose tail fits behind its hop, and on 16384-frame windows an EVEN history of at least 2 floor(taps / 2) frames — the
    tile stores frames in pairs from an even window position on (test_emu_tile.py::test_emulated_16384_tile_needs_an_even_history).  The 8192-
    frame tile and the overlap-add tile take any hop (test_emu_tile.py::test_emulated_8192_tile_at_any_hop; odd histories of the overlap-add
    tile: test_emu_ola.py::test_emulated_overlap_add_history_carry).  An HRIR the window cannot hold
    goes to the partitioned path, whose hop is 4096 whatever the knob says."""
    for C in (1, 2, 7, 8, 14, 16, 17):
        for taps in HOP_TAPS:
            for ola in (None, "1"):
                env = {"AW_WINDOW": str(window), **({"AW_OLA": ola} if ola else {})}
                p = pp.Plan(C, taps, 2, env, hop_align=hop_align)
                what = (window, hop_align, C, taps, ola, p.hop, p.hist_len)
                if p.path == 1:
                    assert taps > 6145 and p.hop == 4096 and p.hist_len == p.partitions * 4096 >= taps, what
                    continue
                # (an HRIR that only the other window holds runs on that one)
                assert p.fft == window or taps > 6145 or 2 * (taps // 2) > 12288, what
                assert p.hop > 0 and p.hop + p.hist_len == p.fft and p.hist_len >= taps - 1, what
                if p.fft == 8192:
                    assert p.hop == align_hop(hop_align, 8192 - (taps - 1)), what
                    assert p.ola_h == 0 or (6 <= p.ola_h <= 8 and p.hist_len <= 8192 - 512 * p.ola_h), what
                else:
                    natural = 16384 - 2 * (taps // 2)
                    assert p.hop == align_hop(hop_align, natural) // 2 * 2 and p.hist_len % 2 == 0 and p.hist_len >= 2 * (taps // 2), what
                    assert p.n_pairs == C and p.ola_h == 0, what


def test_the_default_alignment_never_needs_the_even_rounding():
    """At 64 (and at every even value) the 16384-frame plans are what they were: the rounding to an even hop only ever acts on an odd AW_HOP_ALIGN."""
    for hop_align in (64, 2, 48, 100):
        for taps in range(1, 12290, 7):
            natural = 16384 - 2 * (taps // 2)
            assert align_hop(hop_align, natural) % 2 == 0
            p = pp.Plan(2, taps, 2, {"AW_WINDOW": "16384"}, hop_align=hop_align)
            assert (p.path, p.hop) == (0, align_hop(hop_align, natural)), (hop_align, taps, p.hop)
    p = pp.Plan(2, 4320, 2, {"AW_WINDOW": "16384"}, hop_align=3)
    assert (p.hop, p.hist_len) == (12062, 4322)                 # 12 063 = 3 x 4021 rounded down to an even hop
