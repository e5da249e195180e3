"""CPU-side check of airwave_amd/csrc/host/device_buf.hpp, the one owner of the library's device and page-locked memory: the real header
compiled by plain g++ against a stand-in for <hip/hip_runtime.h> (tests/harness/hip_stub, first on the include path) into a stand-alone
program with the address and undefined-behaviour sanitizers, which then runs as a child process.  The program
(tests/harness/device_buf_check.cpp) checks the order and number of allocation calls of grow / alloc / reset / upload and the moves, the
page-locked pair of calls, an eight-buffer aggregate whose k-th allocation fails, and awr::Event; it exits non-zero on any mismatch, and
LeakSanitizer fails it for anything still allocated at exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness")


def test_buf_and_event_under_host_sanitizers(tmp_path):
    exe = tmp_path / "device_buf_check"
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(HARNESS, "hip_stub"), "-I" + os.path.join(ROOT, "airwave_amd", "csrc"),
                    os.path.join(HARNESS, "device_buf_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "device_buf_check: ok"


def test_only_the_buffer_type_and_the_four_raw_entries_name_the_allocation_calls():
    """Outside device_buf.hpp, the only code under csrc/ that calls hipMalloc / hipHostMalloc / hipFree / hipHostFree is the four entry
    points that hand the pointer to the caller (comments may mention the calls)."""
    import re
    csrc = os.path.join(ROOT, "airwave_amd", "csrc")
    found = []
    for d, _, files in os.walk(csrc):
        for f in files:
            path = os.path.join(d, f)
            if os.path.relpath(path, csrc) == os.path.join("host", "device_buf.hpp"):
                continue
            for n, line in enumerate(open(path, errors="replace"), 1):
                code = line.split("//")[0]
                if re.search(r"\bhip(Host)?(Malloc|Free)\s*\(", code) and not code.lstrip().startswith(("*", "/*")):
                    found.append((os.path.relpath(path, csrc), code.strip()))
    assert sorted(found) == sorted([
        ("runtime.cpp", "AW_HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));"),                              # aw_device_alloc
        ("runtime.cpp", "if (dptr) AW_HIP_TRY(hipFree(dptr));"),                                         # aw_device_free
        ("runtime.cpp", "AW_HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));"),     # aw_host_alloc_pinned
        ("runtime.cpp", "if (ptr) AW_HIP_TRY(hipHostFree(ptr));"),                                       # aw_host_free_pinned
    ]), found
