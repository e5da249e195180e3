"""examples/offline_batch_limiter.c — measure loudness, one gain per stream to -16 LUFS, a look-ahead limiter at -1 dBTP, dithered s16,
from plain C99.  CPU: it compiles as strict C99 against include/airwave_hip.h alone and fails loudly without a device.  GPU: its pass-two
output, decoded and measured by the numpy references (loudness_ref.py, true_peak_ref.py), keeps the ceiling, and the streams the limiter
only touches now and then sit at the loudness target — where the fixed-gain example has to give the target up."""
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_ref
import true_peak_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "offline_batch_limiter.c")
EXE = os.path.join(ROOT, "examples", "offline_batch_limiter")


def build():
    lib_dir = os.path.join(ROOT, "airwave_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib_dir,
                    "-lairwave_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", EXE], check=True)


def test_limiter_example_is_strict_c99_and_needs_a_device():
    import torch
    build()
    if torch.cuda.is_available():
        return                                                      # the no-device half runs where there is none
    r = subprocess.run([EXE, os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav"), "2", "0.5"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_limiter_example_keeps_the_ceiling_and_the_target(golden_dir, tmp_path):
    build()
    wav = os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav")
    S, seconds = 5, 2.0
    F = int(seconds * 48000)
    out = str(tmp_path / "out.s16")
    r = subprocess.run([EXE, wav, str(S), str(seconds), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert f"streams {S} frames {F} target -16.0 LUFS ceiling -1.0 dBTP latency 75" in r.stdout
    rows = re.findall(r"stream (\d+): (-?[\d.]+) LUFS gain ([\d.]+) min limiter gain ([\d.]+) limited (\d+) of (\d+) frames clipped (\d+)", r.stdout)
    assert [int(row[0]) for row in rows] == list(range(S))
    y = np.fromfile(out, dtype=np.int16).reshape(S, F, 2).astype(np.float32) / np.float32(32768.0)
    c = ref.coefficients()
    at_target = 0
    for s, (_, lufs, gain, min_gain, limited, frames, clipped) in enumerate(rows):
        got_tp = ref.db(ref.measure(y[s], c)["peak"].max())
        got_lufs = loudness_ref.measure(y[s].astype(np.float64), 48000)["integrated"]
        print(f"stream {s}: pass one {lufs} LUFS, gain {gain}; limiter min gain {min_gain}, {limited} of {frames} frames limited; "
              f"pass two {got_lufs:.3f} LUFS {got_tp:.3f} dBTP, clipped {clipped}")
        # dither and rounding come after the limiter (an LSB or two of s16 at -1 dBTP is 0.001 dB), and on dense material the gain moves
        # between windows: DESIGN.md's overshoot at attack 64 / hold 128 is 4e-5 of the ceiling, 0.0004 dB
        assert got_tp <= -1.0 + 0.01, (s, got_tp)
        assert int(clipped) == 0 and int(frames) == F + 75
        assert got_lufs <= -16.0 + 0.1
        if int(limited) * 100 < F:                                  # under 1 % of the frames turned down, and the click they hold is 0.8 % of the energy: under 0.05 dB lost
            assert abs(got_lufs + 16.0) <= 0.1, (s, got_lufs)
            at_target += 1
    assert at_target >= 1
    assert all(int(row[4]) > 0 and float(row[3]) < 1.0 for row in rows)        # every stream has its click, and the limiter caught it
