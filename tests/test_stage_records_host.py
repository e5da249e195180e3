"""CPU-side checks of airwave_amd/csrc/host/stage_records.hpp, the layouts of the output stages' device records: the header compiled by plain
g++ into a test-only library, every offset, total and reset range against the arithmetic runtime.cpp spelled out by hand before the header
existed (written out literally below), and the properties that arithmetic had to have: fields contiguous in the stated order, none
overlapping, each aligned to its element size, nothing past size_t at the largest sizes."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "airwave_amd", "csrc", "host")
N_STREAMS = (1, 3, 1024, 65536)
LOUD_CAPS = (1, 600, 10 ** 10)
ATTACKS, HOLDS = (16, 512), (0, 1024)
TABLE_DOUBLES = 706                      # what set_loudness uploads behind the records: 2 x 97 table + 2 x 64 x 4 plane doubles
RECORD = 40                              # sizeof(awl::Record)
TP_HIST = 2 * 11                         # floats per stream and slot: awtp::kHistory frames of two ears

SHIM = r"""
#include "stage_records.hpp"
typedef unsigned long long u64;
// a field as six numbers: offset, element size, elements per stream, slots, and where at(base, stream 2, slot 1) and at(base) point
template <class T> static u64 *put(u64 *o, const awst::Field<T> &f, u64 slots) {
    unsigned char *base = reinterpret_cast<unsigned char *>(4096);
    o[0] = f.off; o[1] = sizeof(T); o[2] = f.per_stream; o[3] = slots;
    o[4] = (u64)(reinterpret_cast<unsigned char *>(f.at(base, 2, slots > 1 ? 1 : 0)) - base);
    o[5] = (u64)(reinterpret_cast<unsigned char *>(f.at(base)) - base);
    o[6] = f.bytes();
    return o + 7;
}
extern "C" {
void levels(u64 n, u64 *o) {
    const awst::Levels L{{n}};
    o = put(o, L.records, 1); o = put(o, L.call_peaks, 1); o = put(o, L.gains, 1);
    o[0] = L.reset_bytes; o[1] = L.total;
}
void loudness(u64 n, u64 cap, u64 tables, u64 *o) {
    const awst::Loudness L{{n}, cap, tables};
    o = put(o, L.state, 1); o = put(o, L.nonfinite, 1); o = put(o, L.hops, 1);
    o[0] = L.reset_bytes; o[1] = L.total; o[2] = L.tables.off; o[3] = L.tables.per_stream;
}
void true_peak(u64 n, u64 *o) {
    const awst::TruePeak L{{n}};
    o = put(o, L.nonfinite, 1); o = put(o, L.peaks, 1); o = put(o, L.call_peaks, 1); o = put(o, L.history, 2);
    o[0] = L.reset_bytes; o[1] = L.total;
}
void limiter(u64 n, int attack, int hold, u64 *o) {
    const awst::Limiter L{{n}, attack, hold};
    o = put(o, L.limited, 1); o = put(o, L.nonfinite, 1); o = put(o, L.min_gain, 1); o = put(o, L.history, 2);
    o[0] = L.reset_bytes; o[1] = L.total; o[2] = L.hist_floats;
}
void sizes(u64 *o) { o[0] = sizeof(awl::Record); o[1] = awtp::kHistory; o[2] = awlo::kFilters; o[3] = sizeof(size_t); }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage_records_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libstage_records_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + HOST, str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    u64, out = ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_ulonglong)
    lib.levels.argtypes = [u64, out]
    lib.loudness.argtypes = [u64, u64, u64, out]
    lib.true_peak.argtypes = [u64, out]
    lib.limiter.argtypes = [u64, ctypes.c_int, ctypes.c_int, out]
    lib.sizes.argtypes = [out]
    return lib


def _call(fn, *args, fields):
    """-> ([(off, elem, per_stream, slots, at_2_1, at_0, slot_bytes) per field], [the numbers behind them])"""
    o = (ctypes.c_ulonglong * (7 * fields + 4))()
    fn(*args, o)
    v = [int(x) for x in o]
    return [tuple(v[7 * i:7 * i + 7]) for i in range(fields)], v[7 * fields:]


def _check_fields(n, fields, total_of_fields):
    """The properties of any layout: in order from byte 0, back to back (so: no overlap, no gap), aligned, inside size_t, and at() of
    stream 2 in the last slot where the field list puts it."""
    end = 0
    for off, elem, per_stream, slots, at_2_1, at_0, slot_bytes in fields:
        assert off == end                                   # contiguous in the stated order: nothing overlaps, nothing is skipped
        assert off % elem == 0                              # aligned to its element size
        assert slot_bytes == n * per_stream * elem
        assert at_0 == off and at_2_1 == off + (slots - 1) * slot_bytes + 2 * per_stream * elem
        end = off + slots * slot_bytes
        assert end < 2 ** 64
    assert end == total_of_fields


def test_the_constants_the_arithmetic_below_uses(shim):
    o = (ctypes.c_ulonglong * 4)()
    shim.sizes(o)
    assert list(o) == [RECORD, TP_HIST // 2, 2, 8]          # (size_t has 64 bits: "inside size_t" below means < 2 ** 64)


@pytest.mark.parametrize("n", N_STREAMS)
def test_levels_layout_is_the_parents(shim, n):
    fields, (reset, total, _, _) = _call(shim.levels, n, fields=3)
    # [n] awl::Record, then [n] uint32 call-local peaks, then [n] float FIXED gains; a reset wrote n * (sizeof(Record) + sizeof(uint32_t))
    assert [f[0] for f in fields] == [0, n * 40, n * 40 + n * 4]
    assert [f[1:4] for f in fields] == [(40, 1, 1), (4, 1, 1), (4, 1, 1)]
    assert total == n * (40 + 4 + 4) and reset == n * (40 + 4)
    _check_fields(n, fields, total)


@pytest.mark.parametrize("n,cap", list(itertools.product(N_STREAMS, LOUD_CAPS)))
def test_loudness_layout_is_the_parents(shim, n, cap):
    fields, (reset, total, tables_off, tables_per_stream) = _call(shim.loudness, n, cap, TABLE_DOUBLES, fields=3)
    # [n][2][4] double filter state, [n] uint64 non-finite counts, [n][cap] double hop energies (what a reset zeroes), then the tables
    record_bytes = n * (2 * 4 + 1 + cap) * 8
    assert [f[0] for f in fields] == [0, n * 2 * 4 * 8, n * 2 * 4 * 8 + n * 8]
    assert [f[1:4] for f in fields] == [(8, 8, 1), (8, 1, 1), (8, cap, 1)]
    assert reset == record_bytes == tables_off and tables_per_stream == 0
    assert total == record_bytes + TABLE_DOUBLES * 8 < 2 ** 64
    _check_fields(n, fields, record_bytes)


@pytest.mark.parametrize("n", N_STREAMS)
def test_true_peak_layout_is_the_parents(shim, n):
    fields, (reset, total, _, _) = _call(shim.true_peak, n, fields=4)
    # [n] uint64 non-finite counts, [n][2] uint32 peaks, [n] uint32 call-local peaks, then two slots of [n][11][2] float history
    record_bytes = n * (8 + 3 * 4)
    assert [f[0] for f in fields] == [0, n * 8, n * 8 + 2 * n * 4, record_bytes]
    assert [f[1:4] for f in fields] == [(8, 1, 1), (4, 2, 1), (4, 1, 1), (4, 22, 2)]
    assert fields[3][4] == record_bytes + 1 * n * 22 * 4 + 2 * 22 * 4                 # history slot 1, stream 2
    assert total == record_bytes + 2 * n * 22 * 4 and reset == total                  # a reset zeroed tp_bytes: all of it
    _check_fields(n, fields, total)


@pytest.mark.parametrize("n,attack,hold", list(itertools.product(N_STREAMS, ATTACKS, HOLDS)))
def test_limiter_layout_is_the_parents(shim, n, attack, hold):
    fields, (reset, total, hist_floats, _) = _call(shim.limiter, n, attack, hold, fields=4)
    # [n] uint64 limited frames, [n] uint64 non-finite counts, [n] uint32 lowest-gain bits, then two slots of [n][halo][2] float history
    halo = (attack + 12 + hold) + attack - 2 + 11            # window + L - 2 frames of q, + the interpolator's 11 frames of history
    assert hist_floats == 2 * halo
    assert [f[0] for f in fields] == [0, n * 8, n * 16, n * 16 + n * 4]
    assert [f[1:4] for f in fields] == [(8, 1, 1), (8, 1, 1), (4, 1, 1), (4, 2 * halo, 2)]
    assert fields[3][4] == n * 20 + 1 * n * 2 * halo * 4 + 2 * 2 * halo * 4           # history slot 1, stream 2
    assert total == n * (8 + 8 + 4 + 2 * 2 * halo * 4) and reset == n * 16            # a reset zeroed the two counters: n * 16
    _check_fields(n, fields, total)
