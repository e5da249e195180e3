"""The kernel-path decisions the built library makes over a grid, as compact JSON — through the public Python API only.

    python tools/policy_table.py > new.json          (a minute or two on the GPU box)

The grid is placed around every value of the table in airwave_amd/csrc/host/path_policy.hpp (--table: another copy of that header, e.g.
when the tool runs on a tree that predates it): (value - 1, value) taps or streams, the window limits, the overlap-add block edges,
every overlap-save hop the overlap-add ratio is compared with, and the pinned points of tests/policy_points.py under every knob set.
  create rows   (channels, taps, streams, knob set) -> info() of a fresh spatializer
  call rows     one spatializer, optionally reserve(RESERVE), then process_device() per call length on uninitialised device buffers
                (contents do not matter, nothing is timed) -> the last call's long-window rows, both groups, and overlap-add rows
After a re-measurement: edit one row of the table, run this again with the rebuilt library, and read the diff of the decisions against
tests/golden/path_policy_parent.json (tests/test_path_policy_host.py replays that file on the CPU).
Every step that touches the GPU is a child process under its own time limit; after one that fails nothing more is started."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from policy_points import LONG_HRIR_PATHS, LONG_HRIR_STREAMS, WINDOW_POLICY  # noqa: E402

TABLE = os.path.join(ROOT, "airwave_amd", "csrc", "host", "path_policy.hpp")
KNOB_SETS = [{}, {"AW_WINDOW": "4096"}, {"AW_WINDOW": "8192"}, {"AW_WINDOW": "16384"}, {"AW_OLA": "0"}, {"AW_OLA": "1"}, {"AW_LW": "0"}, {"AW_LW": "64"}]
OLA0, LW_SETS = 4, (4, 5, 6, 7)
CREATE_COLUMNS = ["channels", "taps", "streams", "knob_set", "path", "fft", "hop", "partitions", "history", "overlap_add_rows_policy"]
CALL_COLUMNS = ["channels", "taps", "streams", "knob_set", "reserved", "frames", "long_window_rows", "long_window_rows_rest", "overlap_add_rows"]
RESERVE = 480000
CALL_FRAMES = (1000, 16384, 32768, 49152, 65536, 131072, 480000)
WINDOW_LIMITS = (6145, 6146, 12288, 12289, 12290)
OLA_EDGES = (3585, 4097, 4098, 4609, 4610, 5121, 5122)
STEP_SECONDS = 420
NEVER = 1 << 30


def read_table(path):
    """{channels: (ola_need, fused2_from, fused2_upto, fused2_min_streams, lw_crossover_taps)} and (channels_upto, min_blocks, min_blocks_wide)."""
    src = open(path).read()
    rows = {}
    for m in re.finditer(r"^\s*/\*\s*(\d+)\s*\*/\s*\{([^}]*)\},", src, re.M):
        v = [x.strip() for x in m.group(2).split(",")]
        rows[int(m.group(1))] = (float(v[0]),) + tuple(NEVER if x == "kNever" else int(x) for x in v[1:])
    assert sorted(rows) == list(range(17)), sorted(rows)
    m = re.search(r"ola_min_blocks_default\(int channels\) \{ return channels <= (\d+) \? (\d+) : (\d+); \}", src)
    return rows, tuple(int(x) for x in m.groups())


def grid(table, min_blocks, wgs):
    create, calls = [], []          # create: (C, taps, S, knob set); calls: (C, taps, S, knob set, reserved, [frames])
    for C in range(1, 17):
        _, frm, upto, min_streams, lw = table[C]
        taps = set(WINDOW_LIMITS) | set(OLA_EDGES) | {lw - 1, lw, 5999, 6000}
        if 0 < frm < NEVER:
            taps |= {frm - 1, frm}
        if upto > 0:
            taps |= {upto - 1, upto, upto + 1}
        create += [(C, t, 128, 0) for t in sorted(taps)]
        # the stream counts from which the overlap-add tile decides the window, and from which 16384-frame tiles fill the chip
        create += [(C, t, S, 0) for t in (4320,) + OLA_EDGES for S in (1, 47, 48)]
        if frm < NEVER and max(frm, 4320) <= 6145:
            create += [(C, max(frm, 4320), S, 0) for S in (min_streams - 1, min_streams)]
        # every overlap-save hop (8192 - 64 k at 64 k + 1 taps) the overlap-add block is compared with
        create += [(C, 64 * k + 1, 128, 0) for k in range(16, 81)]
        # the long-window crossover of path 0, with and without the overlap-add tile in its way
        calls += [(C, t, 128, ks, 0, [RESERVE]) for t in (lw - 1, lw) for ks in (0, OLA0)]
    points = [(c, t, s) for c, t, s, _ in WINDOW_POLICY] + [(c, t, LONG_HRIR_STREAMS) for t, c, _, _ in LONG_HRIR_PATHS]
    create += [(c, t, s, ks) for ks in range(len(KNOB_SETS)) for c, t, s in points]
    for C in (2, 7, 8, 14, 16):
        for t in (4320, 8640, 32768):
            calls += [(C, t, S, 0, r, list(CALL_FRAMES)) for S in (1, 16, 128) for r in (0, 1)]
            calls += [(C, t, 128, ks, 0, list(CALL_FRAMES)) for ks in LW_SETS]
    # calls a little longer than what the largest window holds: two groups of windows where the batch amortises the second one's launches
    calls += [(C, 32768, S, 0, 0, [300000, 128 * 4096 - 32768 + 50000, 672000]) for C in (7, 14) for S in (1, 16, 128)]
    # overlap-add tile per call: the blocks per workgroup it needs, one block either side (blocks of 8 rows = 4096 frames at 3969 taps)
    for C in range(4, 17):
        per_stream = {-(-mb * wgs // 128) for mb in min_blocks[1:]}
        calls.append((C, 3969, 128, 0, 0, sorted(4096 * (k - 1) + d for k in per_stream for d in (0, 1))))
    seen, out = set(), []
    for r in create:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out, calls


# ---- child steps (each one process, the GPU opened once) ------------------------------------------------------------------------------
def _env(ks):
    for k in ("AW_WINDOW", "AW_OLA", "AW_LW"):
        os.environ.pop(k, None)
    os.environ.update(KNOB_SETS[ks])


def _spatializer(aw, np, ctx, C, taps, S, ks):
    _env(ks)          # the library reads these when the spatializer is created
    hrir = aw.HRIR(np.zeros((2, taps), np.float32), ctx=ctx)
    return aw.Spatializer(hrir, np.zeros(C, np.int32), np.ones(C, np.int32), n_streams=S, ctx=ctx)


def step_header():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wgs = int(os.environ.get("AW_PERSISTENT_WGS", "0"))
    return {"cus": cus, "persistent_wgs": max(8, wgs if wgs > 0 else cus)}


def step_create(rows):
    import numpy as np
    import torch  # noqa: F401  (first: INTEGRATION.md "Coexisting with PyTorch")
    import airwave_amd as aw
    ctx = aw.Context(0)
    out = []
    for C, taps, S, ks in rows:
        i = _spatializer(aw, np, ctx, C, taps, S, ks).info()
        out.append([C, taps, S, ks, i["path"], i["fft"], i["hop"], i["partitions"], i["history"], i["overlap_add_rows_policy"]])
    return out


def step_calls(rows):
    import numpy as np
    import torch
    import airwave_amd as aw
    ctx = aw.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    # allocated once: the largest shape of the step (+ 64 floats: whole-frame vector loads run up to 3 floats past a frame)
    x = torch.empty(max(S * max(fr) * C for C, _, S, _, _, fr in rows) + 64, dtype=torch.float32, device="cuda")
    y = torch.empty(max(S * max(fr) * 2 for _, _, S, _, _, fr in rows) + 64, dtype=torch.float32, device="cuda")
    out = []
    for C, taps, S, ks, reserved, frames in rows:
        sp = _spatializer(aw, np, ctx, C, taps, S, ks)
        if reserved:
            sp.reserve(RESERVE)
        for f in frames:
            sp.process_device(x.data_ptr(), y.data_ptr(), f)
            ctx.synchronize()
            i = sp.info()
            out.append([C, taps, S, ks, reserved, f, i["long_window_rows"], i["long_window_rows_rest"], i["overlap_add_rows"]])
        del sp
    return out


def run_step(name, payload=None):
    """One GPU step as a child under its own time limit; a failure ends the run (nothing more is started on the device)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name]
    r = subprocess.run(cmd, input=json.dumps(payload), capture_output=True, text=True, timeout=STEP_SECONDS)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"policy_table: step {name} failed with status {r.returncode}")
    return json.loads(r.stdout.splitlines()[-1])


def main():
    if "--step" in sys.argv:
        name = sys.argv[sys.argv.index("--step") + 1]
        payload = json.loads(sys.stdin.read())
        res = step_header() if name == "header" else step_create(payload) if name == "create" else step_calls(payload)
        print(json.dumps(res, separators=(",", ":")))
        return
    table_path = sys.argv[sys.argv.index("--table") + 1] if "--table" in sys.argv else TABLE
    table, min_blocks = read_table(table_path)
    header = {"persistent_wgs": 256} if "--count" in sys.argv else run_step("header")
    create, calls = grid(table, min_blocks, header["persistent_wgs"])
    n_calls = sum(len(c[5]) for c in calls)
    assert len(create) + n_calls <= 4000, (len(create), n_calls)
    if "--count" in sys.argv:
        print(len(create), n_calls)
        return
    create_rows = []
    for i in range(0, len(create), 800):
        create_rows += run_step("create", create[i:i + 800])
        sys.stderr.write(f"create {len(create_rows)} / {len(create)}\n")
    call_rows = []
    for C in sorted({c[0] for c in calls}):
        call_rows += run_step("calls", [c for c in calls if c[0] == C])
        sys.stderr.write(f"calls {len(call_rows)} / {n_calls}\n")
    header.update({"knob_sets": KNOB_SETS, "reserve": RESERVE, "create_columns": CREATE_COLUMNS, "call_columns": CALL_COLUMNS})
    j = lambda o: json.dumps(o, separators=(",", ":"))
    body = lambda rows: "[\n" + ",\n".join(j(r) for r in rows) + "\n]"
    sys.stdout.write('{"header":' + j(header) + ',\n"create":' + body(create_rows) + ',\n"calls":' + body(call_rows) + "}\n")


if __name__ == "__main__":
    main()
