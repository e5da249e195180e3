"""examples/offline_batch_resample_pcm.c — two rate buckets of s16 spatialized and converted to s16 at 48 kHz on the device, with gain,
dither and levels from the converter, from plain C99.  CPU: it compiles as strict C99 against include/airwave_hip.h alone (no HIP headers)
and fails loudly without a device.  Its GPU run is in tests/test_gpu_rateconv_pcm.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "offline_batch_resample_pcm.c")
EXE = os.path.join(ROOT, "examples", "offline_batch_resample_pcm")
WAV = os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav")


def build():
    lib_dir = os.path.join(ROOT, "airwave_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib_dir,
                    "-lairwave_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", EXE], check=True)


def test_pcm_resample_example_is_strict_c99_and_needs_a_device():
    import torch
    text = open(SRC).read()
    assert "hip/hip_runtime" not in text
    for name in ("aw_pcm_rateconv_process", "aw_pcm_rateconv_flush", "aw_pcm_rateconv_set_gain", "aw_pcm_rateconv_set_dither",
                 "aw_pcm_rateconv_set_metering", "aw_pcm_rateconv_get_levels", "aw_spatializer_process_pcm"):
        assert name in text, name
    build()
    if torch.cuda.is_available():
        return                                                      # the no-device half runs where there is none
    r = subprocess.run([EXE, WAV, "2", "0.05"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
