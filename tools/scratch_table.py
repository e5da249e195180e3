"""The scratch the built library holds and the stream chunks it runs, row by row, as compact JSON — through the public Python API only.

    python tools/scratch_table.py > new.json          (well under a minute on the GPU box)

Every row is one fresh context and one fresh spatializer created with AW_SPEC_SCRATCH_MB (and the row's other knobs) set, optionally
reserved, then calls of ascending length with profiling on.  Recorded per device row: Context.scratch_bytes after the reserve, and per
call [frames, scratch_bytes, launches of the partitioned forward kernels, of the partitioned inverse kernel (one per stream chunk), of
the long-window split kernels (stream chunks x groups of windows), info()'s long_window_rows and long_window_rows_rest].  Host rows run
the host entry on a context with AW_HOST_CHUNK_MB=1 and record [frames, info()'s host_chunk_streams, scratch_bytes] per call.
tests/golden/scratch_plan_parent.json is this output; tests/test_scratch_plan_host.py replays it on the CPU through
airwave_amd/csrc/host/scratch_plan.hpp, tests/test_gpu_scratch_plan.py holds the built library against it.  Buffers are zeros: nothing
is timed and no sample is looked at."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("AW_SPEC_SCRATCH_MB", "AW_HOST_CHUNK_MB", "AW_WINDOW", "AW_LW", "AW_OLA", "AW_PART_CMAC", "AW_PART_FWD")
DEVICE_COLUMNS = ["frames", "scratch_bytes", "part_forward_launches", "part_inverse_launches", "lw_split_launches", "long_window_rows", "long_window_rows_rest"]
HOST_COLUMNS = ["frames", "host_chunk_streams", "scratch_bytes"]
PART_FRAMES = [1000, 4097, 9000, 50000, 120000]


def _device(name, channels, taps, streams, mb, reserve, frames, **env):
    return {"name": name, "entry": "device", "channels": channels, "taps": taps, "streams": streams, "env": dict(env, AW_SPEC_SCRATCH_MB=str(mb)),
            "reserve": reserve, "frames": list(frames)}


def _host(name, fmt, reserve, frames):
    return {"name": name, "entry": "host", "channels": 8, "taps": 300, "streams": 24, "env": {"AW_SPEC_SCRATCH_MB": "64", "AW_HOST_CHUNK_MB": "1"},
            "format": fmt, "reserve": reserve, "frames": list(frames)}


def rows():
    out = []
    # partitioned path, marched CMAC (7 channels: 4 pairs, 5 partitions; 166 windows' worth of 8192 elements per stream at 120 000 frames)
    for mb, what in ((64, "one-chunk"), (30, "ragged-chunks"), (8, "one-stream")):
        out.append(_device(f"march-{what}", 7, 20000, 5, mb, 0, PART_FRAMES, AW_LW="0"))
        out.append(_device(f"march-{what}-reserved", 7, 20000, 5, mb, 120000, PART_FRAMES, AW_LW="0"))
    out.append(_device("march-policy", 7, 20000, 5, 24, 0, PART_FRAMES))                        # the policy's own choice per call
    out.append(_device("march-policy-reserved", 7, 20000, 5, 24, 120000, PART_FRAMES))
    # partitioned path, block-group CMAC with the one-pair forward kernel (14 channels: 7 pairs, 10 partitions)
    for mb, what in ((64, "one-chunk"), (40, "ragged-chunks"), (8, "one-stream")):
        out.append(_device(f"group-{what}", 14, 40000, 3, mb, 0, PART_FRAMES, AW_LW="0", AW_PART_CMAC="group"))
        out.append(_device(f"group-{what}-reserved", 14, 40000, 3, mb, 120000, PART_FRAMES, AW_LW="0", AW_PART_CMAC="group"))
    # a path-0 spatializer whose long calls take the long-window kernels (8 channels x 8640 taps, 20 streams: 2 x CUs row tiles from
    # 200 000 frames on); the shorter calls of the reserved rows have the reserve plan's tables only: 56 rows, one window or the fused tiles
    lw_frames = [3000, 210000, 330000, 420000]
    for mb, what in ((512, "one-chunk"), (160, "ragged-chunks"), (16, "one-stream")):
        out.append(_device(f"longwin-{what}", 8, 8640, 20, mb, 0, lw_frames))
        out.append(_device(f"longwin-{what}-reserved", 8, 8640, 20, mb, 420000, lw_frames))
    # the long-window kernels of a partitioned spatializer with streams enough to pay for a second group of windows: 48 + 40 rows
    out.append(_device("longwin-two-groups", 2, 20000, 128, 96, 0, [20000, 150000, 310000]))
    out.append(_device("longwin-two-groups-reserved", 2, 20000, 128, 96, 310000, [20000, 150000, 310000]))
    # the host entry: 24 streams x 9001 frames x 8 channels in 1 MB chunks: 3 streams a chunk from float32, 7 from 16-bit input
    for fmt in ("f32", "s16"):
        out.append(_host(f"host-{fmt}", fmt, 0, [1777, 5000, 9001]))
        out.append(_host(f"host-{fmt}-reserved", fmt, 9001, [1777, 5000, 9001]))
    return out


def _context(aw, torch, env):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)          # the library reads these when the context and the spatializer are created
    return aw.Context(0, stream=torch.cuda.current_stream().cuda_stream), old


def _restore(old):
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _launches(sp, prefix):
    return sum(n for name, _, n in sp.stage_times() if name.startswith(prefix))


def run_row(aw, np, torch, row):
    """The recorded form of one row: {"name", "after_reserve", "calls"}."""
    C, S, frames = row["channels"], row["streams"], row["frames"]
    ctx, old = _context(aw, torch, row["env"])
    try:
        sp = aw.Spatializer(aw.HRIR(np.zeros((2, row["taps"]), np.float32), ctx=ctx), np.zeros(C, np.int32), np.ones(C, np.int32), n_streams=S, ctx=ctx)
    finally:
        _restore(old)
    calls = []
    if row["entry"] == "host":
        dtype = {"f32": np.float32, "s16": np.int16}[row["format"]]
        if row["reserve"]:
            sp.reserve_pcm(row["reserve"], row["format"], row["format"])
        after_reserve = ctx.scratch_bytes
        for f in frames:
            sp.process_host_into(np.zeros((S, f, C), dtype), np.zeros((S, f, 2), dtype))
            calls.append([f, sp.info()["host_chunk_streams"], ctx.scratch_bytes])
        return {"name": row["name"], "after_reserve": after_reserve, "calls": calls}
    x = torch.zeros(S * max(frames) * C + 64, dtype=torch.float32, device="cuda")          # (+ 64 floats: whole-frame vector loads run up to 3 floats past a frame)
    y = torch.zeros(S * max(frames) * 2 + 64, dtype=torch.float32, device="cuda")
    if row["reserve"]:
        sp.reserve(row["reserve"])
    after_reserve = ctx.scratch_bytes
    sp.set_profiling(True)
    seen = [0, 0, 0]
    for f in frames:
        sp.process_device(x.data_ptr(), y.data_ptr(), f)
        ctx.synchronize()
        now = [_launches(sp, "aw_part_forward"), _launches(sp, "aw_part_inverse"), _launches(sp, "aw_lw_split")]
        i = sp.info()
        calls.append([f, ctx.scratch_bytes] + [a - b for a, b in zip(now, seen)] + [i["long_window_rows"], i["long_window_rows_rest"]])
        seen = now
    return {"name": row["name"], "after_reserve": after_reserve, "calls": calls}


def run_all():
    import numpy as np
    import torch  # first: INTEGRATION.md "Coexisting with PyTorch"
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import airwave_amd as aw
    header = {"cus": torch.cuda.get_device_properties(0).multi_processor_count, "device_columns": DEVICE_COLUMNS, "host_columns": HOST_COLUMNS}
    return header, [run_row(aw, np, torch, r) for r in rows()]


def dumps(header, results):
    j = lambda o: json.dumps(o, separators=(",", ":"))
    return '{"header":' + j(header) + ',\n"rows":[\n' + ",\n".join(j(r) for r in results) + "\n]}\n"


if __name__ == "__main__":
    sys.stdout.write(dumps(*run_all()))
