"""TEST-ONLY: the build-if-stale loader of the emulation libraries (tests/emu/emu*.py).  The dependencies come from the compiler (-MMD), so
a header nobody listed cannot leave an old library in place: next to libX.so lies libX.so.d, the command lines that built it and every
file they read.  Both are written relative to the library's directory, so a copy of the tree keeps its libraries."""
import ctypes
import json
import os
import shlex
import subprocess
from concurrent.futures import ThreadPoolExecutor

CXX = "g++"
FLAGS = ("-std=c++20", "-O2", "-pthread")
MAX_COMPILERS = 16


def _make_deps(path):
    """The prerequisites of a make-syntax dependency file."""
    text = open(path).read().replace("\\\n", " ")
    return [os.path.normpath(p) for p in shlex.split(text.split(":", 1)[1])]


def _stale(lib_path, commands):
    here = os.path.dirname(lib_path)
    try:
        record = json.load(open(lib_path + ".d"))
        built = os.path.getmtime(lib_path)
        return record["commands"] != commands or any(os.path.getmtime(os.path.join(here, d)) > built for d in record["deps"])
    except (OSError, ValueError, KeyError):          # no library, no (readable) record, or a recorded file that is gone
        return True


def load(lib_path, units, link_flags=(), compile_flags=FLAGS, force=False):
    """ctypes.CDLL(lib_path), built first when it is stale: when it or its record is missing, a recorded file is newer than it or gone, or
    the command lines differ (force: in any case).  units: [(source, extra_flags)], compiled side by side and then linked."""
    lib_path = os.path.abspath(lib_path)
    here, name = os.path.split(lib_path)
    objs = [f"{name}.{i}.o" for i in range(len(units))]
    commands = [[CXX, *compile_flags, "-fPIC", *extra, "-MMD", "-MF", o + ".d", "-c", os.path.relpath(os.path.abspath(src), here), "-o", o]
                for (src, extra), o in zip(units, objs)]
    commands.append([CXX, "-shared", *link_flags, "-o", name] + objs)
    if force or _stale(lib_path, commands):
        try:
            with ThreadPoolExecutor(max_workers=MAX_COMPILERS) as pool:
                if any(rc != 0 for rc in pool.map(lambda c: subprocess.call(c, cwd=here), commands[:-1])):
                    raise RuntimeError(f"{name}: the emulation sources failed to compile")
            deps = sorted({d for o in objs for d in _make_deps(os.path.join(here, o + ".d"))})
            subprocess.run(commands[-1], cwd=here, check=True)
            with open(lib_path + ".d", "w") as f:
                json.dump({"commands": commands, "deps": deps}, f, indent=1)
        finally:
            for o in objs:
                for tmp in (o, o + ".d"):
                    if os.path.exists(os.path.join(here, tmp)):
                        os.remove(os.path.join(here, tmp))
    return ctypes.CDLL(lib_path)
