"""Host entry in integer PCM against float32 (aw_spatializer_process_host_pcm): G stereo frames/s and bytes moved per call for f32/f32,
s16/s16 and s24/s24 (with --dither also s16/s16 under TPDF and high-pass TPDF dither, aw_spatializer_set_dither), alternating (the order
rotates every repetition), on page-locked and optionally pageable buffers; then one profiled call per format for the decode / encode kernel
times (HIP events around each launch: aw_spatializer_stage_time).

    python tools/pcm_host_entry.py [--channels 8] [--taps 4320] [--streams 128] [--seconds 10] [--reps 3] [--pageable] [--dither]

One JSON line per measurement and a summary line per format (min / median / max over the repetitions, and the ratio to f32/f32)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import airwave_amd as aw  # noqa: E402

FORMATS = (("f32", np.float32, 4), ("s16", np.int16, 2), ("s24", np.uint8, 3))
DITHERED = (("s16+tpdf", "s16", "tpdf"), ("s16+tpdf_hp", "s16", "tpdf_hp"))      # (label, format, aw_dither mode)


def fill(buf, fmt, base):
    """Tile a few streams of random input over the batch in the format's layout (values matter little: the path is bandwidth-bound)."""
    S = buf.shape[0]
    if fmt == "f32":
        src = base
    elif fmt == "s16":
        src = np.clip(np.rint(base * 32768), -32768, 32767).astype(np.int16)
    else:
        s = np.clip(np.rint(base.astype(np.float64) * 8388608), -8388608, 8388607).astype(np.int64) & 0xFFFFFF
        src = np.stack([s & 0xFF, (s >> 8) & 0xFF, (s >> 16) & 0xFF], axis=-1).astype(np.uint8)
    for i in range(S):
        buf[i] = src[i % src.shape[0]]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--taps", type=int, default=4320)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pageable", action="store_true", help="also time pageable numpy buffers (bounced through page-locked chunks)")
    ap.add_argument("--dither", action="store_true", help="also time s16/s16 with TPDF and high-pass TPDF dither")
    a = ap.parse_args()
    C, S, F = a.channels, a.streams, int(round(a.seconds * 48000))
    rng = np.random.default_rng(1)
    h = (rng.standard_normal((14, a.taps)) * np.exp(-np.arange(a.taps) / (a.taps / 6.0)) * 0.05).astype(np.float32)
    lt = (np.arange(C) % 14).astype(np.int32)
    rt = ((np.arange(C) + 7) % 14).astype(np.int32)
    base = (rng.standard_normal((4, F, C)) * 0.1).astype(np.float32)
    ctx = aw.Context(0)
    sp = aw.Spatializer(aw.HRIR(h, ctx=ctx), lt, rt, n_streams=S, ctx=ctx)
    kinds = ["pinned"] + (["pageable"] if a.pageable else [])
    bufs = {}
    for kind in kinds:
        for fmt, dt, b in FORMATS:
            shp_in, shp_out = ((S, F, C, 3), (S, F, 2, 3)) if fmt == "s24" else ((S, F, C), (S, F, 2))
            if kind == "pinned":
                x, y = ctx.pinned_empty(shp_in, dt), ctx.pinned_empty(shp_out, dt)
            else:
                x, y = np.empty(shp_in, dt), np.empty(shp_out, dt)
            fill(x, fmt, base)
            bufs[(kind, fmt)] = (x, y)
    for fmt, _, _ in FORMATS:
        sp.reserve_pcm(F, fmt, fmt)
    # (label, format, bytes per sample, dither mode)
    runs = [(fmt, fmt, b, "none") for fmt, _, b in FORMATS] + ([(lab, fmt, 2, mode) for lab, fmt, mode in DITHERED] if a.dither else [])

    def call(kind, fmt, mode="none"):
        x, y = bufs[(kind, fmt)]
        sp.set_dither(mode)
        return sp.process_host_into(x, y, in_format=fmt, out_format=fmt)

    for kind in kinds:                              # warm-up: pipeline objects, tables, first-touch of every buffer
        for _, fmt, _, mode in runs:
            call(kind, fmt, mode)
    rates = {}
    for kind in kinds:
        for rep in range(a.reps):
            order = runs[rep % len(runs):] + runs[:rep % len(runs)]
            for lab, fmt, b, mode in order:
                t = time.perf_counter()
                call(kind, fmt, mode)
                dt_s = time.perf_counter() - t
                gfs = S * F / dt_s / 1e9
                rates.setdefault((kind, lab), []).append(gfs)
                moved = S * F * (C + 2) * b
                print(json.dumps({"kind": kind, "format": f"{lab}/{fmt}" if mode != "none" else f"{fmt}/{fmt}", "rep": rep, "channels": C, "taps": a.taps, "streams": S, "frames": F,
                                  "seconds": round(dt_s, 4), "g_frames_per_s": round(gfs, 4), "bytes_moved": moved,
                                  "gb_per_s": round(moved / dt_s / 1e9, 2), "chunk_streams": sp.info()["host_chunk_streams"]}), flush=True)
    # the conversion kernels' own time: one profiled call per format (events around every launch of the call)
    kernels = {}
    for lab, fmt, _, mode in runs:
        sp.set_profiling(True)
        call("pinned", fmt, mode)
        stages = {name: (ms, n) for name, ms, n in sp.stage_times()}
        sp.set_profiling(False)
        kernels[lab] = {k: {"ms": round(stages[k][0], 3), "launches": stages[k][1]} for k in ("aw_pcm_decode_kernel", "aw_pcm_encode_kernel") if k in stages}
    sp.set_dither("none")
    for kind in kinds:
        f32 = float(np.median(rates[(kind, "f32")]))
        for lab, fmt, b, mode in runs:
            r = rates[(kind, lab)]
            print(json.dumps({"summary": kind, "format": f"{fmt}/{fmt}", "dither": mode, "channels": C, "taps": a.taps, "bytes_per_frame": (C + 2) * b,
                              "g_frames_per_s_min": round(min(r), 4), "median": round(float(np.median(r)), 4), "max": round(max(r), 4),
                              "vs_f32_median": round(float(np.median(r)) / f32, 3), "conversion_kernels": kernels[lab] if kind == "pinned" else None}),
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
