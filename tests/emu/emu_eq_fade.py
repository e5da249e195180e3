"""TEST-ONLY: ctypes access to the thread-emulated target change of the equalizer stage (tests/emu/emu_eq_fade.cpp), and the stage's
bookkeeping around it as the runtime keeps it: one table of presets, the active / faded-to / published maps, two state banks, one clock."""
import ctypes
import os

import numpy as np

import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = os.path.join(_HERE, "libemu_eq_fade.so")
_UNITS = [(os.path.join(_HERE, "emu_eq_fade.cpp"), []), (os.path.join(_ROOT, "airwave_amd/csrc/host/eq.cpp"), [])]
_lib = None
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int32)
lp = ctypes.POINTER(ctypes.c_longlong)
LL = ctypes.c_longlong


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, _UNITS, link_flags=["-pthread"])
        _lib.emu_eq_fade_segment.argtypes = [ctypes.c_void_p, LL, ctypes.c_void_p, ctypes.c_void_p, ip, ip, ctypes.c_int, LL, LL, LL, ctypes.c_int,
                                             ctypes.c_double, dp, ip, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        _lib.emu_eq_fade_length.argtypes = [ctypes.c_double]
        _lib.emu_eq_fade_length.restype = LL
        _lib.emu_eq_fade_plan.argtypes = [lp, LL, lp]
    return _lib


def keep():
    return lib().emu_eq_keep()


def fade_length(rate):
    return int(lib().emu_eq_fade_length(float(rate)))


def plan(clock, frames):
    """clock: [length, frame, fading, pending] -> ([(first, frames, t0, fade, begins, ends)], the clock after the call)."""
    c = (LL * 4)(*[int(v) for v in clock])
    segs = (LL * 18)()
    n = lib().emu_eq_fade_plan(c, int(frames), segs)
    return [tuple(int(segs[i * 6 + k]) for k in range(6)) for i in range(n)], [int(v) for v in c]


class FadeStage:
    """The stage with target changes.  presets: every preset the test will use, [(preamp_db, [(type, fc, gain_db, q)])]; stream_map: the
    installed map (-1: not equalized).  set_target(entries) publishes; process(x) runs one call and returns (y, the call's cuts)."""

    def __init__(self, presets, stream_map, sample_rate, ear_split=False):
        self.rate, self.ear_split = float(sample_rate), bool(ear_split)
        self.map = np.ascontiguousarray(stream_map, dtype=np.int32)
        n = self.map.size
        self.to_map = np.full(n, keep(), np.int32)
        self.pending_map = np.full(n, keep(), np.int32)
        self.preamps = np.ascontiguousarray([p for p, _ in presets], dtype=np.float64)
        self.counts = np.ascontiguousarray([len(f) for _, f in presets], dtype=np.int32)
        self.filters = np.ascontiguousarray(np.asarray([f for _, fl in presets for f in fl], dtype=np.float64).reshape(-1, 4))
        self.kmax = int(self.counts.max())
        self.z = np.zeros((n, self.kmax, 4), np.float64)
        self.z_to = np.zeros((n, self.kmax, 4), np.float64)
        self.clock = [fade_length(sample_rate), 0, 0, 0]

    def set_target(self, entries):
        e = np.asarray(entries, np.int32)
        pick = e != keep()
        self.pending_map[pick] = e[pick]
        if pick.any():
            self.clock[3] = 1

    def reset(self):
        self.z[:] = 0
        self.z_to[:] = 0

    def process(self, x):
        y = np.array(x, dtype=np.float32, order="C")
        n, frames = y.shape[0], y.shape[1]
        segs, after = plan(self.clock, frames)
        for first, count, t0, fade, begins, ends in segs:
            if begins:
                pick = self.pending_map != keep()
                self.to_map[pick] = self.pending_map[pick]
                self.pending_map[pick] = keep()
                self.z_to[pick] = 0
            rc = lib().emu_eq_fade_segment(y.ctypes.data + first * 8, frames, self.z.ctypes.data, self.z_to.ctypes.data, self.map.ctypes.data_as(ip),
                                           self.to_map.ctypes.data_as(ip), n, count, t0, self.clock[0], fade, self.rate, self.preamps.ctypes.data_as(dp),
                                           self.counts.ctypes.data_as(ip), self.filters.ctypes.data_as(dp), self.counts.size, self.kmax, int(self.ear_split))
            assert rc == 0, rc
            if ends:
                pick = self.to_map != keep()
                self.map[pick] = self.to_map[pick]
                self.z[pick] = self.z_to[pick]
                self.to_map[pick] = keep()
        self.clock = after
        return y, segs
