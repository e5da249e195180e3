"""examples/offline_batch_resample_true_peak.c — two rate buckets spatialized, measured behind the converter at 48 kHz, gained to
-1 dBTP and delivered as dithered s16, from plain C99.  CPU: it compiles as strict C99 against include/airwave_hip.h alone (no HIP
headers) and fails loudly without a device.  GPU: its printed figures parse, and its output, decoded and measured by the numpy reference
(true_peak_ref.py), holds the ceiling."""
import os
import re
import subprocess

import numpy as np
import pytest

import true_peak_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "offline_batch_resample_true_peak.c")
EXE = os.path.join(ROOT, "examples", "offline_batch_resample_true_peak")
WAV = os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav")


def build():
    lib_dir = os.path.join(ROOT, "airwave_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib_dir,
                    "-lairwave_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", EXE], check=True)


def test_true_peak_resample_example_is_strict_c99_and_needs_a_device():
    import torch
    text = open(SRC).read()
    assert "hip/hip_runtime" not in text
    for name in ("aw_tp_rateconv_set", "aw_tp_rateconv_measure", "aw_tp_rateconv_measure_flush", "aw_tp_rateconv_get", "aw_tp_rateconv_reset_records",
                 "aw_pcm_rateconv_set_gain", "aw_pcm_rateconv_process", "aw_pcm_rateconv_flush", "aw_spatializer_process_pcm"):
        assert name in text, name
    build()
    if torch.cuda.is_available():
        return                                                      # the no-device half runs where there is none
    r = subprocess.run([EXE, WAV, "2", "0.05"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_true_peak_resample_example_holds_the_ceiling(golden_dir, tmp_path):
    build()
    wav = os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav")
    S, seconds = 3, 0.05
    F = 2400                                                        # 0.05 s at 48 kHz from either bucket
    out = str(tmp_path / "out.s16")
    r = subprocess.run([EXE, wav, str(S), str(seconds), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    buckets = re.findall(r"bucket (\d+) Hz -> 48000 Hz: (\d+) streams, (\d+) frames in, (\d+) frames out, ceiling (-?[\d.]+) dBTP, clipped (\d+)", r.stdout)
    assert [(int(a), int(b), int(c), int(d), e, int(f)) for a, b, c, d, e, f in buckets] == [(44100, S, 2205, F, "-1.000", 0), (96000, S, 4800, F, "-1.000", 0)]
    rows = re.findall(r"stream (\d+) at (\d+) Hz: (-?[\d.]+) dBTP before \(sample peak (-?[\d.]+) dBFS\), gain ([\d.e+-]+), (-?[\d.]+) dBTP after, (\d+) frames", r.stdout)
    assert [(int(row[0]), int(row[1])) for row in rows] == [(i, rate) for rate in (44100, 96000) for i in range(S)]
    y = np.fromfile(out, dtype=np.int16).reshape(2 * S, F, 2).astype(np.float32) / np.float32(32768.0)
    c = ref.coefficients()
    bound = 0
    for k, (_, rate, before, sample, gain, after, frames) in enumerate(rows):
        got = ref.db(ref.measure(y[k], c)["peak"].max())
        print(f"stream {k} at {rate} Hz: {before} dBTP before (sample peak {sample}), gain {gain}; delivered {got:.3f} dBTP (reported {after})")
        assert int(frames) == F and float(before) >= float(sample)
        # dither and rounding come after the gain: an LSB or two of s16 at -1 dBTP is 0.001 dB
        assert got <= -1.0 + 0.01 and abs(got - float(after)) <= 0.01, (k, got)
        assert float(after) <= -1.0 + 0.001
        if float(gain) < 1.0:
            bound += 1
            assert abs(float(after) + 1.0) <= 0.001
        else:
            assert float(gain) == 1.0 and abs(float(after) - float(before)) <= 0.001
    assert bound >= 1
