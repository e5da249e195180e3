"""True peak of the limiter's output over its ceiling, measured with the library's own rules on the CPU: awlim::sequential
(device/limiter.hpp) limits, awtp::sequential (device/truepeak.hpp) measures, both compiled by g++ through tests/emu/emu_limiter.cpp.
Material: white noise and low-passed noise at 2.4 - 2.5 x full scale and an isolated fs/4 burst, ceiling 0.891 (-1 dBTP).  No GPU.

    python tools/limiter_overshoot.py [--frames 96000]

One JSON line per (material, attack, hold): DESIGN.md's limiter table."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import emu_limiter as emu  # noqa: E402

C = 0.891
SETTINGS = [(16, 0), (64, 0), (64, 128), (256, 256), (512, 1024)]


def materials(frames):
    rng = np.random.default_rng(2024)
    white = rng.uniform(-2.5, 2.5, (frames, 2))
    k = np.hanning(9)
    low = np.stack([np.convolve(rng.standard_normal(frames), k / k.sum(), mode="same") for _ in range(2)], axis=1)
    low *= 2.4 / np.abs(low).max()
    i = np.arange(400)
    burst = np.zeros((1200, 2))
    burst[300:700] = (1.2 * (0.5 - 0.5 * np.cos(2 * np.pi * i / 400)) * np.sin(np.pi / 2 * i + np.pi / 4))[:, None]
    return {"white noise": white, "low-passed noise": low, "fs/4 burst": burst}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96000)
    a = ap.parse_args()
    for name, y in materials(a.frames).items():
        for L, H in SETTINGS:
            x = np.concatenate([y, np.zeros((emu.delay(L), 2))]).astype(np.float32)[None]
            lim = emu.Limiter(1, L, H, C)
            z = lim.process(x)
            print(json.dumps({"material": name, "attack": L, "hold": H, "input_true_peak": round(float(emu.true_peak(x[0])), 4),
                              "output_true_peak_over_ceiling": round(float(emu.true_peak(z[0])) / float(np.float32(C)), 8),
                              "output_sample_peak_over_ceiling": round(float(np.abs(z).max()) / float(np.float32(C)), 8),
                              "min_gain": round(float(lim.min_gain.view(np.float32)[0]), 4)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
