"""CPU-side checks of the batch entries' equalizer stage (aw_spatializer_set_equalizer): the entry is declared, exported and typed; a
NULL handle is refused (the other refusals need a live handle: tests/test_gpu_eq_stage.py); and awst::Equalizer, the layout of the stage's one device allocation
(airwave_amd/csrc/host/stage_records.hpp), has the offsets written out by hand below — through a small compiled shim, as
tests/test_stage_records_host.py does for the other four stages."""
import ctypes
import os
import re
import subprocess

import pytest

from airwave_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "airwave_amd", "csrc", "host")
HEADER = os.path.join(ROOT, "include", "airwave_hip.h")
AW_ERR_INVALID_ARGUMENT = 1
NAME = "aw_spatializer_set_equalizer"


def test_the_entry_is_declared_exported_and_typed():
    text = open(HEADER).read()
    assert NAME in set(re.findall(r"AW_API\s+[\w\s\*]+?\b(aw_\w+)\s*\(", text))
    assert NAME in _capi.SIGNATURES
    lib = _capi.load()
    assert getattr(lib, NAME).argtypes == _capi.SIGNATURES[NAME][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert NAME in {line.split()[-1] for line in out.splitlines() if line.split()}
    # info 25 / 26 on no handle, like every other index
    assert lib.aw_spatializer_info(None, 25) == -1 and lib.aw_spatializer_info(None, 26) == -1
    # the header says where crossfaded target changes live
    assert "aw_eq_set_target" in text[text.index("Equalizer of the batch entries"):text.index("AW_API aw_status " + NAME)]


def test_a_null_handle_is_refused():
    lib = _capi.load()
    fn = getattr(lib, NAME)
    d = ctypes.c_void_p()
    assert lib.aw_eq_definition_create(3.0, ctypes.byref(d)) == 0
    try:
        one = ctypes.cast((ctypes.c_void_p * 1)(d), _capi.c_void_pp)
        assert fn(None, None, 0, None) == AW_ERR_INVALID_ARGUMENT
        assert fn(None, one, 1, None) == AW_ERR_INVALID_ARGUMENT
        assert lib.aw_last_error_message()
    finally:
        lib.aw_eq_definition_destroy(d)


SHIM = r"""
#include "stage_records.hpp"
typedef unsigned long long u64;
extern "C" void equalizer(u64 n, u64 presets, u64 kmax, u64 table_doubles, u64 *o) {
    const awst::Equalizer L{{n}, presets, kmax, table_doubles};
    unsigned char *base = reinterpret_cast<unsigned char *>(4096);
    o[0] = L.state.off; o[1] = L.state.per_stream; o[2] = L.state.bytes();
    o[3] = (u64)(reinterpret_cast<unsigned char *>(L.state.at(base, 2)) - base);
    o[4] = L.reset_bytes;
    o[5] = L.map.off; o[6] = L.map.per_stream; o[7] = L.map.bytes();
    o[8] = (u64)(reinterpret_cast<unsigned char *>(L.map.at(base, 2)) - base);
    o[9] = L.presets.off; o[10] = sizeof(awk::EqStagePreset);
    o[11] = (u64)(reinterpret_cast<unsigned char *>(L.presets.at(base) + 1) - base);
    o[12] = L.tables.off; o[13] = (u64)(reinterpret_cast<unsigned char *>(L.tables.at(base)) - base);
    o[14] = L.total;
    o[15] = alignof(awk::EqStagePreset);
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("eq_stage_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libeq_stage_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + HOST, str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    u64 = ctypes.c_ulonglong
    lib.equalizer.argtypes = [u64, u64, u64, u64, ctypes.POINTER(u64)]
    return lib


# (streams, presets, kmax, table doubles) -> state bytes, map offset, header offset, table offset, total: by hand.
#   state  [n][kmax][4] doubles from byte 0 — all a reset zeroes;  map  [n] int32 behind it;  headers  [presets] of 32 bytes on the next
#   multiple of 8;  tables behind them.
CASES = [
    ((1, 1, 0, 0),        dict(state=0,     map=0,     headers=8,     tables=40,    total=40)),                      # preamp only: no state at all
    ((5, 3, 64, 24357),   dict(state=10240, map=10240, headers=10264, tables=10360, total=10360 + 194856)),         # 5 * 64 * 32; + 20 -> 10260 -> 10264; + 96
    ((9, 2, 5, 1765),     dict(state=1440,  map=1440,  headers=1480,  tables=1544,  total=1544 + 14120)),           # 9 * 5 * 32; + 36 -> 1476 -> 1480; + 64
]


@pytest.mark.parametrize("args,want", CASES)
def test_equalizer_layout(shim, args, want):
    n, presets, kmax, doubles = args
    o = (ctypes.c_ulonglong * 16)()
    shim.equalizer(n, presets, kmax, doubles, o)
    (state_off, state_per, state_bytes, state_at2, reset, map_off, map_per, map_bytes, map_at2, hdr_off, hdr_size, hdr_at1, tab_off, tab_at,
     total, hdr_align) = [int(v) for v in o]
    assert (state_off, state_per, state_bytes) == (0, kmax * 4, want["state"]) and state_at2 == 2 * kmax * 4 * 8
    assert reset == want["state"]                                  # the reset range is exactly the state
    assert (map_off, map_per, map_bytes) == (want["map"], 1, n * 4) and map_at2 == want["map"] + 8
    assert map_off == state_off + state_bytes                      # back to back
    assert (hdr_off, hdr_size, hdr_align) == (want["headers"], 32, 8) and hdr_at1 == want["headers"] + 32
    assert hdr_off % 8 == 0 and 0 <= hdr_off - (map_off + map_bytes) < 8
    assert tab_off == want["tables"] == hdr_off + presets * 32 == tab_at and tab_off % 8 == 0
    assert total == want["total"] == tab_off + doubles * 8

