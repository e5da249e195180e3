"""The build-if-stale loader of the emulation libraries (tests/emu/_build.py): it rebuilds when a file the compiler read has changed or the
command line has, and only then; the limiter binding's record names the headers a hand-written list forgot."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _build  # noqa: E402


def _age(path, seconds):
    """Moves a file's mtime (whole seconds, so that no file system rounds the difference away)."""
    t = int(os.path.getmtime(path)) + seconds
    os.utime(path, (t, t))


def _project(tmp_path):
    """A two-line source and its header, written a quarter of an hour ago: a library may then be made 100 s older and still be current."""
    (tmp_path / "answer.hpp").write_text("#define ANSWER 42\n")
    (tmp_path / "answer.cpp").write_text('#include "answer.hpp"\nextern "C" int answer() { return ANSWER + EXTRA; }\n')
    _age(str(tmp_path / "answer.hpp"), -900)
    _age(str(tmp_path / "answer.cpp"), -900)
    return str(tmp_path / "libanswer.so"), [(str(tmp_path / "answer.cpp"), ["-DEXTRA=0"])]


def test_first_load_builds(tmp_path):
    lib, units = _project(tmp_path)
    assert _build.load(lib, units).answer() == 42
    record = json.load(open(lib + ".d"))
    assert {os.path.basename(d) for d in record["deps"]} == {"answer.cpp", "answer.hpp"}
    assert sorted(os.listdir(tmp_path)) == ["answer.cpp", "answer.hpp", "libanswer.so", "libanswer.so.d"]      # no objects left behind


def test_second_load_does_not_build(tmp_path):
    lib, units = _project(tmp_path)
    _build.load(lib, units)
    _age(lib, -100)                      # a rebuild would bring the time back
    before = os.path.getmtime(lib)
    assert _build.load(lib, units).answer() == 42
    assert os.path.getmtime(lib) == before


def test_newer_header_or_other_flags_rebuild(tmp_path):
    lib, units = _project(tmp_path)
    _build.load(lib, units)
    _age(lib, -100)
    before = os.path.getmtime(lib)
    _age(str(tmp_path / "answer.hpp"), 850)             # 50 s newer than the library now
    _build.load(lib, units)
    assert os.path.getmtime(lib) > before

    _age(lib, -10)                       # (still newer than the header)
    before = os.path.getmtime(lib)
    _build.load(lib, [(units[0][0], ["-DEXTRA=1"])])
    assert os.path.getmtime(lib) > before
    assert "-DEXTRA=1" in json.load(open(lib + ".d"))["commands"][0]

    os.remove(lib + ".d")                # no record: nothing says what the library was built from
    _age(lib, -10)
    before = os.path.getmtime(lib)
    _build.load(lib, [(units[0][0], ["-DEXTRA=1"])])
    assert os.path.getmtime(lib) > before


def test_limiter_record_names_every_header():
    import emu_limiter
    emu_limiter.lib()
    names = {os.path.basename(d) for d in json.load(open(emu_limiter._LIB + ".d"))["deps"]}
    assert {"emu_limiter.cpp", "limiter_tile.hpp", "limiter.hpp", "truepeak.hpp", "levels.hpp", "pcm.hpp", "emu_stage_ctx.hpp"} <= names
