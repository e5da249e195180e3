"""The sample-rate converter's tile geometries: one table of (pair, channels, why) that the emulated suite (tests/test_emu_rateconv*.py) and
the device suite (tests/test_gpu_rateconv_geometry.py) both run, and the three handles at the refusal boundary of aw_rateconv_create and
aw_tp_rateconv_set.  Every entry exists for one path of airwave_amd/csrc/device/rateconv_tile.hpp, and the property that puts it on that
path is asserted here, at import, with the header's own plan and tile length (tests/emu/emu_rateconv.py): a change of the tile formula or
of the plan that moves a case off its path fails every test that imports this module, and does not pass unnoticed.

Inputs are those of the existing case() helpers (tests/test_gpu_rateconv.py and its PCM and true-peak siblings): 3 streams of two tiles
plus three frames, then 7 frames, then the flush, so three workgroups per stream, the last one ragged."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rateconv as emu  # noqa: E402

MAX_TILE, HALO, SEGMENT, LDS_FLOATS, TP_HISTORY = 4096, 3, 32, 12288, 11


def block(channels):
    """rc_block: the channels one work item owns, which is one LDS read of 16, 8 or 4 bytes."""
    return 4 if channels % 4 == 0 else 2 if channels % 2 == 0 else 1


def row_stride(taps):
    """rc_row_stride: floats between the rows of the device's coefficient table."""
    return (taps + 3) & ~3


def tile_by_the_formula(L, M, T, C):
    """rc_tile restated: the longest tile, up to 4096 outputs, whose input image (segments of 32 frames behind a halo of 3, one halo more,
    rounded up to 4 floats) and gathered outputs fit 12288 floats of LDS; 0 where none does."""
    def floats(n):
        span = -(-n * M // L) + T
        return ((((span - 1) // SEGMENT + 1) * (SEGMENT + HALO) * C + HALO * C + 3) & ~3) + n * C
    lo, hi = 0, MAX_TILE
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if floats(mid) <= LDS_FLOATS else (lo, mid - 1)
    return lo


def geometry(pair, C):
    L, M, T, D = emu.plan(*pair)
    CB = block(C)
    return dict(L=L, M=M, T=T, D=D, C=C, tile=emu.tile(pair[0], pair[1], C), CB=CB, NB=C // CB, row_stride=row_stride(T))


def first_call_frames(pair, C):
    """Input frames of a case's first call: two tiles of output plus three frames."""
    g = geometry(pair, C)
    return emu.input_frames_for(2 * g["tile"], g["L"], g["M"], g["D"]) + 3


def tap_loops(T):
    """(taps of the first group, of the 16-tap loop, of the 4-tap loop, of the tail) of rc_output."""
    sixteen = (T - 4) // 16 * 16
    four = (T - 4 - sixteen) // 4 * 4
    return 4, sixteen, four, T - 4 - sixteen - four


# (pair, channels, why, the property that justifies the entry)
_TABLE = [
    ((44100, 48000), 1, "one channel: a CB = 1 block at stride 1, the tile clamped to 4096",
     lambda g: g["tile"] == MAX_TILE and g["CB"] == 1 and g["NB"] == 1),
    ((44100, 48000), 4, "the 4-channel block, one work item per output", lambda g: g["CB"] == 4 and g["NB"] == 1),
    ((44100, 48000), 12, "the 4-channel block, three work items per output, frames 48 bytes apart",
     lambda g: g["CB"] == 4 and g["NB"] == 3 and 4 * g["C"] == 48),
    ((44100, 48000), 6, "the 2-channel block, three work items per output", lambda g: g["CB"] == 2 and g["NB"] == 3),
    ((44100, 192000), 16, "a tile shorter than L: every output its own phase class and coefficient row",
     lambda g: g["tile"] == 520 and g["L"] == 640 and g["tile"] < g["L"] and g["CB"] == 4),
    ((96000, 48000), 4, "L = 1: one coefficient row shared by every lane", lambda g: g["L"] == 1 and g["M"] == 2 and g["CB"] == 4),
    ((192000, 44100), 4, "M = 640, the bank-conflict case of the 35-frame segments; rows padded, a two-tap tail",
     lambda g: g["M"] == 640 and g["T"] == 418 and g["T"] % 4 == 2 and g["row_stride"] == 420 != g["T"] and g["CB"] == 4),
    ((192000, 44100), 1, "M = 640 at stride 1: the longest input image",
     lambda g: g["M"] == 640 and g["T"] % 4 == 2 and g["row_stride"] != g["T"] and g["CB"] == 1),
    ((48000, 44100), 8, "T = 106: the 16-tap loop, the 4-tap loop and the two-tap tail all run",
     lambda g: g["T"] == 106 and tap_loops(g["T"]) == (4, 96, 4, 2) and g["NB"] == 2),
    ((88200, 48000), 3, "T = 178: the 4-tap loop runs three times behind the 16-tap loop",
     lambda g: g["T"] == 178 and tap_loops(g["T"]) == (4, 160, 12, 2) and g["CB"] == 1 and g["NB"] == 3),
    ((8000, 48000), 16, "upward with M = 1: six consecutive outputs share their input frame",
     lambda g: g["M"] == 1 and g["L"] == 6 and g["NB"] == 4),
]

CASES = [(pair, C, why) for pair, C, why, _ in _TABLE]
IDS = [f"{pair[0]}-{pair[1]}-C{C}" for pair, C, _ in CASES]
CB4 = [(pair, C) for pair, C, _ in CASES if block(C) == 4]
SHORT_TILE = ((44100, 192000), 16)               # tile < L
ONE_ROW = ((96000, 48000), 4)                    # L == 1

for _pair, _C, _why, _holds in _TABLE:
    _g = geometry(_pair, _C)
    assert _holds(_g), f"{_pair} with {_C} channels no longer hits its path ({_why}): {_g}"
    assert _g["tile"] == tile_by_the_formula(_g["L"], _g["M"], _g["T"], _C), (_pair, _C, _g)
assert len(CB4) >= 2 and SHORT_TILE in CB4 and ONE_ROW in CB4
# the largest input of the table is 192000 -> 44100 with one channel, at about 18 000 frames per stream
assert max(first_call_frames(p, C) for p, C, _ in CASES) == first_call_frames((192000, 44100), 1) == 18058

# ---- the refusal boundary ----
# A plan is accepted for coprime L, M <= 640 and 1 .. 16 channels; T = 2 ceil(48 max(1, M / L)).  The tile lengths below follow from the
# formula by hand (floats of the input image of span ceil(n M / L) + T, plus n C gathered floats, against 12288):
#   L = 1, M = 640: T = 61 440 frames alone exceed the LDS at any channel count                                            -> tile 0
#   L = 2, M = 13, T = 624, C = 16: n = 7: span 670, 21 segments, 21 * 560 + 48 + 112 = 11 920; n = 8: 22 segments > 12 288 -> tile 7
#   L = 2, M = 13, T = 624, C = 15: n = 12: span 702, 22 segments, 11 596 + 180 = 11 776; n = 13: 23 segments, 12 315       -> tile 12
NO_TILE = ((64000, 100), 1)                      # aw_rateconv_create refuses: "no tile"
TINY_TILE = ((13000, 2000), 16)                  # created, tile 7: aw_tp_rateconv_set refuses ("leaves none")
SMALLEST_MEASURING = ((13000, 2000), 15)         # tile 12: the smallest that leaves a measuring tile, of 1 output
BOUNDARY_TILES = {NO_TILE: 0, TINY_TILE: 7, SMALLEST_MEASURING: 12}
assert emu.plan(*NO_TILE[0]) == (1, 640, 61440, 30720) and emu.plan(*TINY_TILE[0]) == emu.plan(*SMALLEST_MEASURING[0]) == (2, 13, 624, 312)
