"""examples/offline_batch_profile_switch.c — a programme rendered in calls of one second whose odd streams change their headphone preset
at a cue second (aw_spatializer_set_equalizer_target: a 20 ms fade inside the batch entries) while the even ones keep theirs
(AW_EQ_KEEP), from plain C99.  CPU: it compiles as strict C99 against include/airwave_hip.h alone and fails loudly without a device.
GPU: against a run of the same programme without the cue, switched and unswitched streams differ only from the cue second on, and behind
the fade the switched streams carry preset B's mark on the spectrum (the band method of tests/test_example_profiles.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "offline_batch_profile_switch.c")
EXE = os.path.join(ROOT, "examples", "offline_batch_profile_switch")
PRESETS = [os.path.join(ROOT, "tests", "golden", "eq", name) for name in ("Bass Booster.txt", "Treble Reducer.txt")]


def build():
    lib_dir = os.path.join(ROOT, "airwave_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib_dir,
                    "-lairwave_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", EXE], check=True)


def test_profile_switch_example_is_strict_c99_and_needs_a_device():
    import torch
    build()
    if torch.cuda.is_available():
        return                                                      # the no-device half runs where there is none
    r = subprocess.run([EXE, os.path.join(ROOT, "tests", "golden", "hrtf", "RoomSH1.0.wav"), *PRESETS, "2", "2", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)


def bands(y):
    """20 - 100 Hz and 8 - 16 kHz over 400 - 1200 Hz, in dB, of one ear."""
    spec = np.abs(np.fft.rfft(y.astype(np.float64))) ** 2
    hz = np.fft.rfftfreq(y.size, 1 / 48000.0)
    mids = spec[(hz > 400) & (hz < 1200)].mean()                     # neither preset reaches here
    return 10 * np.log10(spec[(hz > 20) & (hz < 100)].mean() / mids), 10 * np.log10(spec[(hz > 8000) & (hz < 16000)].mean() / mids)


@pytest.mark.gpu
def test_profile_switch_example_switches_the_odd_streams_at_the_cue(golden_dir, tmp_path):
    build()
    wav = os.path.join(golden_dir, "hrtf", "RoomSH1.0.wav")
    S, seconds, cue, rate = 4, 3, 1, 48000
    out = str(tmp_path / "out.f32")
    r = subprocess.run([EXE, wav, *PRESETS, str(S), str(seconds), str(cue), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "second 1: target published (pending 1)" in r.stdout
    assert "second 0: presets held 1, fade frames left 0, pending 0" in r.stdout
    assert "second 1: presets held 2, fade frames left 0, pending 0" in r.stdout          # the fade's 960 frames lie inside the second
    y = np.fromfile(out, dtype=np.float32).reshape(S, seconds * rate, 2)
    at = cue * rate
    for s in range(S):
        lo0, hi0 = bands(y[s, :at, 0])
        lo1, hi1 = bands(y[s, at + 960:, 0])                         # behind cue + 20 ms
        print(f"stream {s}: before the cue 20 - 100 Hz {lo0:+.2f} dB, 8 - 16 kHz {hi0:+.2f} dB; after it {lo1:+.2f} dB, {hi1:+.2f} dB")
        if s & 1:
            # Bass Booster lifts 20 - 100 Hz by 5 to 7 dB and leaves the highs alone; Treble Reducer leaves the lows alone and takes about
            # 4 dB off 8 - 16 kHz (tests/test_example_profiles.py): the switch takes both steps
            assert lo0 - lo1 > 4.0 and hi0 - hi1 > 3.0, (s, lo0, lo1, hi0, hi1)
        else:
            assert abs(lo0 - lo1) < 1.0 and abs(hi0 - hi1) < 1.0, (s, lo0, lo1, hi0, hi1)
    # Against a run without the cue: every stream is the same, bit for bit, up to the cue.  From there the even streams went through the
    # same filters cut at the fade's two ends (the kernel's chunk boundaries move: Float64 reassociation, the last bit of the float32
    # output at most), the odd ones through another preset.
    out2 = str(tmp_path / "never.f32")
    r2 = subprocess.run([EXE, wav, *PRESETS, str(S), str(seconds), str(seconds), out2], capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr
    never = np.fromfile(out2, dtype=np.float32).reshape(S, seconds * rate, 2)
    for s in range(S):
        assert np.array_equal(y[s, :at].view(np.uint32), never[s, :at].view(np.uint32)), s
        peak = np.abs(never[s]).max()
        diff = np.abs(y[s, at:].astype(np.float64) - never[s, at:]).max()
        print(f"stream {s}: from the cue on, max difference to the run without a cue {diff:.3e} at a peak of {peak:.3f}")
        if s & 1:
            assert diff > 1e-2 * peak, (s, diff, peak)
        else:
            assert diff <= 2.0 ** -23 * max(peak, 1.0), (s, diff, peak)
