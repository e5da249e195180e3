"""What the batch entries launch, case by case: for every (entry, sample formats, meter / gain state, dither, shape) below, one call on a
fresh handle with profiling on, and the (stage name, launches) list of stage_times() afterwards.  The context runs the overlap-add tile
on calls of every size (AW_OLA_MIN_BLOCKS=0) and stages host batches in 1 MB chunks (AW_HOST_CHUNK_MB=1), so that 24 streams of 9001
frames go through the chunk loops and 6 streams of 1777 frames through the one-piece paths.

    python tools/batch_launches.py            # JSON: the launch lists (tests/golden/batch_launch_sequences.json is this output)
    python tools/batch_launches.py --hash     # ... plus, per case: sha256 of the output bytes, clipped count, integer fields of levels()
                                              #     and, in the NEW_STATES, of loudness() / true_peak() / limiter() (+ sha256 of the hop energies)

tests/test_gpu_batch_launches.py loads this file by path and holds the lists against the recorded ones.  Run on the GPU box."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"AW_OLA_MIN_BLOCKS": "0", "AW_HOST_CHUNK_MB": "1"}
TAPS = 300
FORMATS = {"f32": 0, "s16": 1, "s24": 2, "s32": 3}
PAIRS = (("f32", "f32"), ("s16", "f32"), ("f32", "s16"), ("s24", "s24"), ("f32", "s32"))
STATES = ("off", "meter", "gain", "ceiling")
NEW_STATES = ("loudness", "true_peak", "true_peak_ceiling", "limiter")          # the later stages: recorded without dither only
DITHERS = ("none", "tpdf")
LOUDNESS_SECONDS = 1.0                                                          # 10 hops of 4800 frames per stream
# shape name -> (streams, frames, channels, reserve first)
SHAPES = {"one_piece": (6, 1777, 8, False),           # every entry's unchunked path
          "chunked": (24, 9001, 8, False),            # 288 KB per float32 stream: 3 streams per chunk, 8 chunks (s16 input: 7 and 4)
          "single": (1, 1024, 8, True),               # the page-locked single-stream path of the host entries (reserved)
          "planar": (1, 1024, 2, True),               # ... and of the planar entry
          "planar_staged": (1, 1024, 2, False)}       # the planar entry through its device staging (not reserved)
KEY = ("entry", "in", "out", "state", "dither", "shape")


def cases(later=False):
    """The recorded cases, as dicts over KEY: STATES x DITHERS — the matrix of the first recording, which a caller that knows no other
    still gets — and, with later, NEW_STATES behind them (appended, so the earlier cases keep their lines)."""
    out = []
    for states, dithers in ((STATES, DITHERS), (NEW_STATES, DITHERS[:1]))[:2 if later else 1]:
        for entry, pairs, shapes in (("process", PAIRS[:1], ("one_piece", "chunked")),
                                     ("process_host", PAIRS[:1], ("one_piece", "chunked", "single")),
                                     ("process_pcm", PAIRS, ("one_piece", "chunked")),
                                     ("process_host_pcm", PAIRS, ("one_piece", "chunked", "single")),
                                     ("process_planar", PAIRS[:1], ("planar", "planar_staged"))):
            for fin, fout in pairs:
                for shape in shapes:
                    for state in states:
                        for dither in dithers:
                            out.append(dict(zip(KEY, (entry, fin, fout, state, dither, shape))))
    return out


def key(case):
    return tuple(case[k] for k in KEY)


def _pack_s24(s):
    u = (s.astype(np.int64) & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def _input(fmt, S, F, C):
    """Noise whose level rises from stream to stream (the loud streams clip an integer output), in fmt's host layout."""
    rng = np.random.default_rng(S * 100003 + F * 17 + C)
    x = rng.standard_normal((S, F, C)).astype(np.float32) * np.geomspace(0.02, 1.5, S).astype(np.float32)[:, None, None]
    if fmt == "f32":
        return x
    top = 2 ** ({"s16": 16, "s24": 24, "s32": 32}[fmt] - 1)
    s = np.clip(np.rint(x.astype(np.float64) * 0.3 * top), -top, top - 1).astype(np.int64)
    return {"s16": lambda: s.astype(np.int16), "s24": lambda: _pack_s24(s), "s32": lambda: s.astype(np.int32)}[fmt]()


def _output(fmt, S, F):
    return {"f32": lambda: np.zeros((S, F, 2), np.float32), "s16": lambda: np.zeros((S, F, 2), np.int16),
            "s24": lambda: np.zeros((S, F, 2, 3), np.uint8), "s32": lambda: np.zeros((S, F, 2), np.int32)}[fmt]()


def make_context(aw):
    old = {k: os.environ.get(k) for k in ENV}
    try:
        os.environ.update(ENV)                               # knobs are read once, at context creation
        return aw.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _records(sp, state, S):
    """The order-independent fields of the later stages' records (sums that atomics add up in floating point are left out)."""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32).ravel().tolist()
    if state == "loudness":
        ld = sp.loudness()
        hops = np.stack([sp.loudness_hops(s, 0, int(round(10 * LOUDNESS_SECONDS))) for s in range(S)])
        return {"loudness": {k: ld[k].tolist() for k in ("blocks", "blocks_above_absolute", "blocks_gated", "frames", "frames_dropped", "nonfinite")},
                "hops_sha256": hashlib.sha256(hops.tobytes()).hexdigest()}
    if state in ("true_peak", "true_peak_ceiling"):
        tp = sp.true_peak()
        return {"true_peak": {"true_peak_bits": bits(tp["true_peak"]), "call_true_peak_bits": bits(tp["call_true_peak"]),
                              "frames": tp["frames"].tolist(), "nonfinite": tp["nonfinite"].tolist()}}
    if state == "limiter":
        lm = sp.limiter()
        return {"limiter": {"min_gain_bits": bits(lm["min_gain"]), "frames": lm["frames"].tolist(),
                            "limited_frames": lm["limited_frames"].tolist(), "nonfinite": lm["nonfinite"].tolist()}}
    return None


def run_case(aw, ctx, hrirs, case, want_hash=False):
    """One call of the case on a fresh handle -> {"launches": [[name, n], ...]} (+ "sha256", "clipped", "levels", "records" with want_hash)."""
    from airwave_amd.api import _check
    S, F, C, reserve = SHAPES[case["shape"]]
    if C not in hrirs:
        rng = np.random.default_rng(41)
        h = (rng.standard_normal((14, TAPS)) * np.exp(-np.arange(TAPS) / (TAPS / 6.0))).astype(np.float32)
        hrirs[C] = aw.HRIR(h, ctx=ctx)
    lt, rt = (np.arange(C) % 14).astype(np.int32), ((np.arange(C) * 3 + 7) % 14).astype(np.int32)
    sp = aw.Spatializer(hrirs[C], lt, rt, n_streams=S, ctx=ctx)
    if case["dither"] != "none":
        sp.set_dither(case["dither"], seed=7)
    if case["state"] == "meter":
        sp.set_metering(True)
    elif case["state"] == "gain":
        sp.set_gain("fixed", gains=np.linspace(0.3, 1.1, S).astype(np.float32))
    elif case["state"] == "ceiling":
        sp.set_gain("peak_ceiling", ceiling=0.5)
    elif case["state"] == "loudness":
        sp.set_loudness(True, max_seconds=LOUDNESS_SECONDS)
    elif case["state"] == "true_peak":
        sp.set_true_peak(True)
    elif case["state"] == "true_peak_ceiling":
        sp.set_gain("true_peak_ceiling", ceiling=0.5)
    elif case["state"] == "limiter":
        sp.set_gain("fixed", gains=np.linspace(0.3, 1.1, S).astype(np.float32))
        sp.set_limiter(True, ceiling=0.5, attack_frames=64, hold_frames=128)
    if reserve:
        sp.reserve(F)
    x, y = _input(case["in"], S, F, C), _output(case["out"], S, F)
    fi, fo = FORMATS[case["in"]], FORMATS[case["out"]]
    clipped = 0
    sp.set_profiling(True)
    entry = case["entry"]
    if entry in ("process", "process_pcm"):
        dx, dy, dc = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes), ctx.alloc(8)
        try:
            ctx.h2d(dx, x)
            ctx.h2d(dy, y)
            ctx.h2d(dc, np.zeros(1, np.uint64))
            if entry == "process":
                sp.process_device(dx, dy, F)
            else:
                sp.process_pcm_device(dx, fi, dy, fo, F, dc)
            ctx.synchronize()
            ctx.d2h(y, dy)
            n = np.zeros(1, np.uint64)
            ctx.d2h(n, dc)
            clipped = int(n[0])
        finally:
            for p in (dx, dy, dc):
                ctx.free(p)
    elif entry == "process_host":
        sp.process_host_into(x, y)
    elif entry == "process_host_pcm":
        n = ctypes.c_uint64(0)
        _check(sp._lib.aw_spatializer_process_host_pcm(sp._h, ctypes.c_void_p(x.ctypes.data), fi, ctypes.c_void_p(y.ctypes.data), fo, F,
                                                       ctypes.byref(n)))
        clipped = int(n.value)
    else:
        ol, orr = sp.process_planar(x[0, :, 0], x[0, :, 1])
        y = np.stack([ol, orr], axis=-1)
    ctx.synchronize()
    res = {"launches": [[name, int(k)] for name, _, k in sp.stage_times()]}
    if want_hash:
        res["sha256"] = hashlib.sha256(np.ascontiguousarray(y).view(np.uint8).tobytes()).hexdigest()
        res["clipped"] = clipped
        res["levels"] = None
        if case["state"] in ("meter", "gain", "ceiling", "true_peak_ceiling", "limiter"):      # (energy left out: its atomic adds have no fixed order)
            lv = sp.levels()
            res["levels"] = {"peak_bits": lv["peak"].view(np.uint32).tolist(), "gain_bits": lv["gain"].view(np.uint32).tolist(),
                             "frames": lv["frames"].tolist(), "clipped": lv["clipped"].tolist(), "nonfinite": lv["nonfinite"].tolist()}
        res["records"] = _records(sp, case["state"], S)
    return res


def run_all(want_hash=False, entry=None, later=False):
    """[case + result] for every case (of one entry, if named; with the later stages' states, if asked), in cases() order."""
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import airwave_amd as aw
    ctx = make_context(aw)
    hrirs = {}
    return [dict(c, **run_case(aw, ctx, hrirs, c, want_hash)) for c in cases(later) if entry in (None, c["entry"])]


def dumps(rows):
    """The recorded form: every distinct launch list once, then one line per case — its key, the index of its list and, from a --hash
    run, [sha256, clipped, levels] (+ the later stages' records in the NEW_STATES)."""
    seqs, lines = [], []
    for r in rows:
        if r["launches"] not in seqs:
            seqs.append(r["launches"])
        extra = [[r["sha256"], r["clipped"], r["levels"]] + ([r["records"]] if r["records"] else [])] if "sha256" in r else []
        lines.append(json.dumps(list(key(r)) + [seqs.index(r["launches"])] + extra))
    return ('{"env": ' + json.dumps(ENV) + ', "key": ' + json.dumps(list(KEY)) + ',\n"sequences": [\n' + ",\n".join(json.dumps(s) for s in seqs) +
            '\n],\n"cases": [\n' + ",\n".join(lines) + "\n]}")


def loads(text):
    """dumps() back: {key tuple: launch list}."""
    doc = json.loads(text)
    assert doc["key"] == list(KEY)
    return {tuple(row[:len(KEY)]): doc["sequences"][row[len(KEY)]] for row in doc["cases"]}


if __name__ == "__main__":
    print(dumps(run_all("--hash" in sys.argv[1:], later=True)))
