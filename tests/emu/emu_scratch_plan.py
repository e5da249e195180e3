"""TEST-ONLY: ctypes access to the scratch and chunk planner of the library's host code (tests/emu/emu_scratch_plan.cpp over
airwave_amd/csrc/host/scratch_plan.hpp), built with the flags of emu_path_policy.py so that lw_choose's cost comparisons run in the
library's arithmetic."""
import ctypes
import os

import numpy as np

import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_scratch_plan.so")
_lib = None

PART_FIELDS = ("n_blocks", "n_windows", "per_stream", "per_stream_w", "chunk", "need", "wspec_at")
LW_FIELDS = ("chunk", "need", "spec_per_sw0", "per_stream0", "chunk0", "wrows_at0", "spec_per_sw1", "per_stream1", "chunk1", "wrows_at1")
CALL_FIELDS = ("n_groups", "R0", "windows0", "R1", "windows1")
SCRATCH_FIELDS = CALL_FIELDS + tuple("part_" + f for f in PART_FIELDS) + tuple("lw_" + f for f in LW_FIELDS)
GRID_FIELDS = (("channels", "taps", "streams", "budget", "reserve", "frames", "path", "hop", "partitions", "n_pairs", "hist_len") +
               tuple("res_" + f for f in CALL_FIELDS) + ("longest", "res_need", "res_chunk") +
               tuple("in_" + f for f in SCRATCH_FIELDS) + tuple("un_" + f for f in SCRATCH_FIELDS))


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(_LIB, [(os.path.join(_HERE, "emu_scratch_plan.cpp"), [])], compile_flags=("-std=c++17", "-O2", "-ffp-contract=fast"))
        i, ll = ctypes.c_int, ctypes.c_longlong
        pi, pll = ctypes.POINTER(i), ctypes.POINTER(ll)
        for name, args in (("sp_stream_chunk", [ll] * 5), ("sp_part_scratch", [pi, i, i, i, ll, ll, ll, pll]), ("sp_lw_plan_scratch", [i, i, i, pll, ll, ll, pll]),
                           ("sp_default_budget", [i, ll]), ("sp_part_longest_call", [pi, i, i, i, i, ll]), ("sp_reserve_need", [pi, i, i, i, i, pll, ll, ll, pll]),
                           ("sp_host_chunk_streams", [i, i, ll, i, i]), ("sp_staged_chunk_streams", [i, i, ll, i, i, ll, ll]), ("sp_staged_streams", [ll, i]),
                           ("sp_grid", [i, i, i, pi, i, pll, i, pll, i, i, pll, ll]), ("pp_lw_choose", [pi, i, i, i, i, ll, ctypes.c_uint, ll, i, pi])):
            getattr(_lib, name).argtypes = args
            getattr(_lib, name).restype = ll
        assert _lib.sp_grid_fields() == len(GRID_FIELDS)
    return _lib


def _lls(values):
    return (ctypes.c_longlong * len(values))(*values)


def lw_choose(plan, cus, frames, reserved_frames=0, have=0, for_reserve=False):
    """The call plan of emu_path_policy.Plan `plan` as [(R, windows)] of its groups, and `have` with the plan's window lengths added."""
    out = (ctypes.c_int * 5)()
    lib().pp_lw_choose(plan._v, *plan.layout, cus, reserved_frames, have, frames, int(for_reserve), out)
    groups = [(int(out[1 + 2 * g]), int(out[2 + 2 * g])) for g in range(out[0])]
    rows = [lib().pp_lw_rows(k) for k in range(16)]
    for R, _ in groups:
        have |= 1 << rows.index(R)
    return groups, have


def stream_chunk(budget_elems, held_elems, per_stream, streams, cap=-1):
    """cap < 0: none (the long-window path)."""
    return int(lib().sp_stream_chunk(budget_elems, held_elems, per_stream, streams, cap))


def part_scratch(plan, frames, budget, held=0):
    """plan: emu_path_policy.Plan."""
    out = (ctypes.c_longlong * len(PART_FIELDS))()
    lib().sp_part_scratch(plan._v, *plan.layout, frames, budget, held, out)
    return dict(zip(PART_FIELDS, map(int, out)))


def lw_plan_scratch(layout, groups, budget, held=0):
    """groups: [(R, windows)] of one or two groups."""
    call = [len(groups)] + [v for g in groups for v in g] + [0, 0] * (2 - len(groups))
    out = (ctypes.c_longlong * len(LW_FIELDS))()
    lib().sp_lw_plan_scratch(*layout, _lls(call), budget, held, out)
    return dict(zip(LW_FIELDS, map(int, out)))


def default_budget(known, free_bytes):
    return int(lib().sp_default_budget(int(known), free_bytes))


def part_longest_call(plan, cus, max_frames):
    return int(lib().sp_part_longest_call(plan._v, *plan.layout, cus, max_frames))


def reserve_need(plan, cus, groups, reserved_frames, budget):
    """(need, chunk) for the reserve plan `groups` ([(R, windows)], empty: the long-window kernels do not take the reserved length)."""
    call = [len(groups)] + [v for g in groups for v in g] + [0, 0] * (2 - len(groups))
    out = (ctypes.c_longlong * 2)()
    lib().sp_reserve_need(plan._v, *plan.layout, cus, _lls(call), reserved_frames, budget, out)
    return int(out[0]), int(out[1])


def host_chunk_streams(streams, channels, frames, in_bytes, host_chunk_mb):
    return int(lib().sp_host_chunk_streams(streams, channels, frames, in_bytes, host_chunk_mb))


def staged_chunk_streams(streams, channels, frames, in_bytes, host_chunk_mb, reserved_frames, reserved_chunk):
    return int(lib().sp_staged_chunk_streams(streams, channels, frames, in_bytes, host_chunk_mb, reserved_frames, reserved_chunk))


def staged_streams(chunk, streams):
    return int(lib().sp_staged_streams(chunk, streams))


def grid(channels, taps, cus, streams, budgets, reserves, steps):
    """{field: int64 array} over (streams x reserves x budgets x call lengths) of one layout: GRID_FIELDS."""
    capacity = len(streams) * len(budgets) * len(reserves) * (steps + 2)
    out = np.zeros((capacity, len(GRID_FIELDS)), np.int64)
    n = lib().sp_grid(channels, taps, cus, (ctypes.c_int * len(streams))(*streams), len(streams), _lls(budgets), len(budgets), _lls(reserves), len(reserves),
                      steps, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), capacity)
    return {name: out[:n, k] for k, name in enumerate(GRID_FIELDS)}
