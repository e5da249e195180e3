"""The two pure headers under the multi-device handle (aw_multi, airwave_amd/csrc/multi_runtime.cpp), on the CPU with plain g++:
  shard_plan.hpp     shard_streams is airwave_amd/sharding.py's rule; shard_ranges cuts every global stream range into disjoint, ordered
                     pieces that cover it exactly and stay inside their shards (tests/emu/emu_shard_plan.cpp);
  shard_workers.hpp  a stand-alone program (tests/emu/emu_shard_workers.cpp) over the worker core: a few thousand rounds of run() with
                     1 .. 8 workers, a deliberately failing shard per round, create / destroy in a loop — built with -fsanitize=thread
                     and run as a plain process.
Neither header may look at the environment or include the device runtime."""
import ctypes
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _build  # noqa: E402

from airwave_amd import sharding  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
HOST = os.path.join(ROOT, "airwave_amd", "csrc", "host")

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _build.load(os.path.join(EMU, "libemu_shard_plan.so"), [(os.path.join(EMU, "emu_shard_plan.cpp"), [])], compile_flags=("-std=c++17", "-O2"))
        ip = ctypes.POINTER(ctypes.c_int)
        _lib.sp_shard_streams.argtypes = [ctypes.c_int] * 3 + [ip, ip]
        _lib.sp_shard_streams.restype = None
        _lib.sp_shard_ranges.argtypes = [ctypes.c_int] * 4 + [ip]
        _lib.sp_shard_of.argtypes = [ctypes.c_int] * 3
    return _lib


def shard(total, world, rank):
    f, c = ctypes.c_int(), ctypes.c_int()
    lib().sp_shard_streams(total, world, rank, ctypes.byref(f), ctypes.byref(c))
    return f.value, c.value


def test_shard_streams_is_the_python_rule():
    for total in range(0, 201):
        for world in range(1, 18):
            got = [shard(total, world, r) for r in range(world)]
            assert got == [sharding.shard_streams(total, world, r) for r in range(world)], (total, world)
            # contiguous, in order, the first total % world one longer, zero-stream shards allowed
            assert got[0][0] == 0 and sum(c for _, c in got) == total
            assert all(got[r][0] + got[r][1] == got[r + 1][0] for r in range(world - 1))
            assert [c for _, c in got] == [total // world + (1 if r < total % world else 0) for r in range(world)]


def test_shard_ranges_cut_every_range_into_ordered_disjoint_pieces_inside_their_shards():
    out = (ctypes.c_int * (4 * 64))()
    cases = 0
    for total in range(0, 41):
        for world in range(1, 8):
            shards = [sharding.shard_streams(total, world, r) for r in range(world)]
            for first in range(0, total + 1):
                for n in range(0, total - first + 1):
                    k = lib().sp_shard_ranges(total, world, first, n, out)
                    pieces = [tuple(out[4 * j:4 * j + 4]) for j in range(k)]
                    at, last_shard = first, -1
                    for s, g, l, c in pieces:
                        assert c > 0 and g == at and s > last_shard, (total, world, first, n, pieces)             # in order, disjoint, no empty piece
                        sf, sc = shards[s]
                        assert 0 <= l and l + c <= sc and sf + l == g, (total, world, first, n, pieces)           # inside its shard, at the right place
                        at, last_shard = g + c, s
                    assert at == first + n, (total, world, first, n, pieces)                                      # covers exactly the range
                    cases += 1
            for stream in range(total):
                s = lib().sp_shard_of(total, world, stream)
                assert shards[s][0] <= stream < shards[s][0] + shards[s][1]
    assert cases > 80000


def test_the_two_headers_are_pure_host_code():
    for name in ("shard_plan.hpp", "shard_workers.hpp"):
        src = open(os.path.join(HOST, name)).read()
        assert "getenv" not in src, name
        assert not re.search(r"#\s*include\s*[<\"][^>\"]*hip", src), name
        assert "hipError_t" not in src and "hipStream_t" not in src, name


def test_worker_core_under_the_thread_sanitizer(tmp_path):
    """Plain process, own main: statuses, messages, lowest failing index, no job outside run(), create / destroy in a loop."""
    exe = str(tmp_path / "emu_shard_workers")
    r = None
    for sanitizer in ("thread", "address,undefined"):          # the second where the thread sanitizer does not link or its runtime cannot start
        cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all",
                             os.path.join(EMU, "emu_shard_workers.cpp"), "-o", exe], capture_output=True, text=True)
        if cc.returncode != 0 and sanitizer == "thread":
            continue
        assert cc.returncode == 0, cc.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        if sanitizer == "thread" and "FATAL: ThreadSanitizer" in r.stderr:          # (its shadow mapping does not fit this kernel's address layout)
            continue
        print("sanitizer:", sanitizer)
        break
    assert r.returncode == 0 and r.stdout.startswith("ok: "), (r.returncode, r.stdout, r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert int(r.stdout.split()[1]) >= 4000
