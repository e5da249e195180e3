"""TEST-ONLY: ctypes access to the kernel-path planner of the library's host code (tests/emu/emu_path_policy.cpp over
airwave_amd/csrc/host/path_policy.hpp), built with plain g++ like the library's host code: -ffp-contract=fast for baseline x86-64 (no
-march=native), so that the cost comparisons run in the library's arithmetic."""
import ctypes
import os

import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_path_policy.so")
_lib = None

ENV_KNOBS = ("AW_WINDOW", "AW_OLA", "AW_LW")
PLAN_FIELDS = ("path", "fused2", "hop", "hist_len", "partitions", "n_pairs", "ola_h", "cmac_group", "fwd_one_pair", "herm_ok", "lw_mode")


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, [(os.path.join(_HERE, "emu_path_policy.cpp"), [])], compile_flags=("-std=c++17", "-O2", "-ffp-contract=fast"))
        i, ll, p = ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)
        _lib.pp_plan_create.argtypes = [i, i, i, p, p]
        _lib.pp_use_ola_tile.argtypes = [p, i, i, i, ll, i, i]
        _lib.pp_lw_choose.argtypes = [p, i, i, i, i, ll, ctypes.c_uint, ll, i, p]
        _lib.pp_lw_rows.argtypes = [i]
        _lib.pp_ola_max_bytes.restype = ll
    return _lib


def lw_rows():
    out = []
    while lib().pp_lw_rows(len(out)):
        out.append(lib().pp_lw_rows(len(out)))
    return out


class Plan:
    """plan_create() of one spatializer: the environment knobs as {name: text}, the context's as numbers."""

    def __init__(self, channels, taps, streams, env=None, hop_align=64, ola_min_blocks=-1):
        env = env or {}
        assert set(env) <= set(ENV_KNOBS), env          # (the atoi of each, as aw_spatializer_create reads them)
        k = []
        for name in ENV_KNOBS:
            k += [int(name in env), int(env.get(name, 0))]
        k += [0, 0, 0, 0, 0, hop_align, ola_min_blocks]
        self.layout = (channels, taps, streams)
        self.ola_min_blocks = ola_min_blocks
        self._v = (ctypes.c_int * 11)()
        lib().pp_plan_create(channels, taps, streams, (ctypes.c_int * 13)(*k), self._v)
        for name, v in zip(PLAN_FIELDS, self._v):
            setattr(self, name, int(v))
        self.fft = 16384 if self.fused2 else 8192

    def use_ola_tile(self, frames, persistent_wgs):
        return bool(lib().pp_use_ola_tile(self._v, *self.layout, frames, persistent_wgs, self.ola_min_blocks))

    def lw_choose(self, frames, cus, reserved_frames=0, have=0, for_reserve=False):
        """(rows of the first group of windows, rows of the remainder window), 0 where there is none."""
        out = (ctypes.c_int * 5)()
        lib().pp_lw_choose(self._v, *self.layout, cus, reserved_frames, have, frames, int(for_reserve), out)
        return int(out[1]), int(out[3])
