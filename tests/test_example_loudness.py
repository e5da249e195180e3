"""examples/offline_batch_loudness.c — measure, aw_loudness_gain to -16 LUFS as fixed gains, dithered s16, from plain C99.  CPU: it
compiles as strict C99 against include/airwave_hip.h alone and fails loudly without a device.  GPU: its pass-two output, decoded and
measured by the numpy reference (loudness_ref.py), sits at the target."""
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "offline_batch_loudness.c")
EXE = os.path.join(ROOT, "examples", "offline_batch_loudness")


def build():
    lib_dir = os.path.join(ROOT, "airwave_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib_dir,
                    "-lairwave_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", EXE], check=True)


def test_loudness_example_is_strict_c99_and_needs_a_device():
    import torch
    build()
    if torch.cuda.is_available():
        return                                                      # the no-device half runs where there is none
    r = subprocess.run([EXE, os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav"), "2", "0.5"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_loudness_example_brings_every_stream_to_the_target(golden_dir, tmp_path):
    build()
    wav = os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav")
    S, seconds = 5, 1.0
    F = int(seconds * 48000)
    out = str(tmp_path / "out.s16")
    r = subprocess.run([EXE, wav, str(S), str(seconds), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert f"streams {S} frames {F} target -16.0 LUFS" in r.stdout
    rows = re.findall(r"stream (\d+): (-?[\d.]+) LUFS gain ([\d.]+) clipped (\d+)", r.stdout)
    assert [int(i) for i, _, _, _ in rows] == list(range(S))
    measured = np.array([float(l) for _, l, _, _ in rows])
    assert np.all(np.diff(measured) > 0) and measured[-1] - measured[0] > 20          # quiet to loud: the gains differ
    y = np.fromfile(out, dtype=np.int16).reshape(S, F, 2).astype(np.float64) / 32768.0
    clean = 0
    for s, (_, _, _, clipped) in enumerate(rows):
        got = ref.measure(y[s], 48000)["integrated"]
        print(f"stream {s}: pass one {measured[s]:.3f} LUFS, pass two {got:.3f} LUFS, clipped {clipped}")
        if int(clipped) == 0:
            assert abs(got + 16.0) <= 0.1, (s, got)
            clean += 1
    assert clean >= 3
