"""examples/offline_batch_resample.c — two rate buckets spatialized and converted to 48 kHz on the device, from plain C99.  CPU: it
compiles as strict C99 against include/airwave_hip.h alone (no HIP headers) and fails loudly without a device.  Its GPU run is in
tests/test_gpu_rateconv.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "offline_batch_resample.c")
EXE = os.path.join(ROOT, "examples", "offline_batch_resample")
WAV = os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav")


def build():
    lib_dir = os.path.join(ROOT, "airwave_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib_dir,
                    "-lairwave_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", EXE], check=True)


def test_resample_example_is_strict_c99_and_needs_a_device():
    import torch
    assert "hip/hip_runtime" not in open(SRC).read()
    build()
    if torch.cuda.is_available():
        return                                                      # the no-device half runs where there is none
    r = subprocess.run([EXE, WAV, "2", "0.05"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
