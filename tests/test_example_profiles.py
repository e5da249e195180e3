"""examples/offline_batch_profiles.c — two headphone presets assigned alternately to the streams (aw_spatializer_set_equalizer), then the
limiter example's chain: measure loudness, one gain per stream to -16 LUFS, a look-ahead limiter at -1 dBTP, dithered s16, from plain C99.
CPU: it compiles as strict C99 against include/airwave_hip.h alone and fails loudly without a device.  GPU: its pass-two output, decoded
and measured by the numpy references (loudness_ref.py, true_peak_ref.py), keeps the ceiling and the target although the equalizer ran —
it ran in front of the meters and the limiter — and the two presets left their mark on the spectrum of the streams they were given."""
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_ref
import true_peak_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "offline_batch_profiles.c")
EXE = os.path.join(ROOT, "examples", "offline_batch_profiles")
PRESETS = [os.path.join(ROOT, "tests", "golden", "eq", name) for name in ("Bass Booster.txt", "Treble Reducer.txt")]


def build():
    lib_dir = os.path.join(ROOT, "airwave_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib_dir,
                    "-lairwave_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", EXE], check=True)


def test_profiles_example_is_strict_c99_and_needs_a_device():
    import torch
    build()
    if torch.cuda.is_available():
        return                                                      # the no-device half runs where there is none
    r = subprocess.run([EXE, os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav"), *PRESETS, "2", "0.5"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_profiles_example_equalizes_in_front_of_the_meters_and_the_limiter(golden_dir, tmp_path):
    build()
    wav = os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav")
    S, seconds = 4, 2.0
    F = int(seconds * 48000)
    out = str(tmp_path / "out.s16")
    r = subprocess.run([EXE, wav, *PRESETS, str(S), str(seconds), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "presets 2 (3 and 2 filters, at most 3 enabled)" in r.stdout
    assert f"streams {S} frames {F} target -16.0 LUFS ceiling -1.0 dBTP latency 75" in r.stdout
    rows = re.findall(r"stream (\d+): preset (\d) (-?[\d.]+) LUFS gain ([\d.]+) min limiter gain ([\d.]+) limited (\d+) of (\d+) frames clipped (\d+)", r.stdout)
    assert [(int(row[0]), int(row[1])) for row in rows] == [(s, s & 1) for s in range(S)]
    y = np.fromfile(out, dtype=np.int16).reshape(S, F, 2).astype(np.float32) / np.float32(32768.0)
    c = ref.coefficients()
    lows, highs = [], []
    for s, (_, _, lufs, gain, min_gain, limited, frames, clipped) in enumerate(rows):
        got_tp = ref.db(ref.measure(y[s], c)["peak"].max())
        got_lufs = loudness_ref.measure(y[s].astype(np.float64), 48000)["integrated"]
        spec = np.abs(np.fft.rfft(y[s, :, 0].astype(np.float64))) ** 2
        hz = np.fft.rfftfreq(F, 1 / 48000.0)
        mids = spec[(hz > 400) & (hz < 1200)].mean()                 # neither preset reaches here
        lows.append(10 * np.log10(spec[(hz > 20) & (hz < 100)].mean() / mids))
        highs.append(10 * np.log10(spec[(hz > 8000) & (hz < 16000)].mean() / mids))
        print(f"stream {s}: pass one {lufs} LUFS, gain {gain}; limiter min gain {min_gain}, {limited} of {frames} frames limited; "
              f"pass two {got_lufs:.3f} LUFS {got_tp:.3f} dBTP, clipped {clipped}; over 400 - 1200 Hz: 20 - 100 Hz {lows[-1]:+.2f} dB, 8 - 16 kHz {highs[-1]:+.2f} dB")
        # as tests/test_example_limiter.py: dither and rounding come after the limiter, the overshoot at attack 64 / hold 128 is 0.0004 dB
        assert got_tp <= -1.0 + 0.01, (s, got_tp)
        assert int(clipped) == 0 and int(frames) == F + 75
        assert got_lufs <= -16.0 + 0.1
        if int(limited) * 100 < F:                                  # the loudness was measured on the equalized signal: the target holds behind it
            assert abs(got_lufs + 16.0) <= 0.1, (s, got_lufs)
    # white noise through one HRIR: the streams' spectra differ by their preset alone.  Bass Booster (even streams) lifts 20 - 100 Hz by
    # 5 to 7 dB (low shelf at 105 Hz, +5 dB, and +2 dB at 60 Hz) and leaves the highs alone; Treble Reducer (odd streams) leaves the lows
    # alone and takes about 4 dB off 8 - 16 kHz (high shelf at 6 kHz, -4 dB).  160, 1600 and 16 000 bins a band: the estimate of a band's
    # mean moves by a few tenths of a dB.
    assert min(lows[0], lows[2]) - max(lows[1], lows[3]) > 4.0, lows
    assert min(highs[0], highs[2]) - max(highs[1], highs[3]) > 3.0, highs
