"""The scratch and chunk planner (airwave_amd/csrc/host/scratch_plan.hpp) on the CPU, compiled with plain g++ (tests/emu/emu_scratch_plan.cpp):
  replay       tests/golden/scratch_plan_parent.json — the pool sizes, launch counts and chunkings the library showed on the MI355X before
               the arithmetic moved into the header, recorded by tools/scratch_table.py — every row, every field;
  restatement  the arithmetic as runtime.cpp had it, written out below, field by field over a grid of ~1.15 M (layout, budget, reserve,
               call) cases — the C++ side walks the grid, numpy restates it;
  properties   what the launches rely on (regions end inside the pool, chunk bounds) and SURVEY §8b's "process must not allocate after
               reserve" on the same grid: it holds wherever the reserve plan's stream chunk is at least 2, and has a gap below that
               (strict xfail + one pinned instance; the fix of aw_spatializer_reserve flips both)."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_path_policy as pp  # noqa: E402
import emu_scratch_plan as sp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB, GiB = 1 << 20, 1 << 30
CUS = 256
CHANNELS = (1, 2, 3, 7, 8, 9, 14, 16)
TAPS = (300, 4320, 5200, 6146, 8640, 12289, 20000, 32768, 40000)
STREAMS = (1, 2, 3, 5, 16, 128, 1024)
BUDGETS = (1 * MiB, 3 * MiB, 20 * MiB, 96 * MiB, 6 * GiB, 64 * GiB)
RESERVES = (4096, 9000, 50000, 70000, 120000, 200001, 480000, 777777, 1000000, 3000000)
STEPS = 36          # call lengths 1 + (reserve - 1) k / 36 (every ninth of the reserve among them), then reserve - 1 and reserve
N, LW_M, PART_CAP = 8192, 4096, 65535


@pytest.fixture(scope="module")
def grid():
    """{field: int64 array} over the whole grid (emu_scratch_plan.GRID_FIELDS)."""
    parts = [sp.grid(c, t, CUS, STREAMS, BUDGETS, RESERVES, STEPS) for c in CHANNELS for t in TAPS]
    g = {f: np.concatenate([p[f] for p in parts]) for f in sp.GRID_FIELDS}
    assert len(g["frames"]) == len(CHANNELS) * len(TAPS) * len(STREAMS) * len(BUDGETS) * len(RESERVES) * (STEPS + 2)
    return g


# ---- replay --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("_scratch_table_under_test", os.path.join(ROOT, "tools", "scratch_table.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "scratch_plan_parent.json")))


def replay_device(row, cus):
    """What runtime.cpp does around the header for one device row: (pool bytes after the reserve, [per call: frames, pool bytes, stream
    chunks on the partitioned kernels, stream chunks x groups on the long-window kernels, rows, rows of the rest])."""
    plan = pp.Plan(row["channels"], row["taps"], row["streams"], {k: v for k, v in row["env"].items() if k in pp.ENV_KNOBS})
    budget, S = int(row["env"]["AW_SPEC_SCRATCH_MB"]) << 20, row["streams"]
    pool = reserved = have = 0
    if row["reserve"]:
        groups, have = sp.lw_choose(plan, cus, row["reserve"], for_reserve=True)
        reserved = row["reserve"]
        pool = sp.reserve_need(plan, cus, groups, reserved, budget)[0]
    after_reserve, calls = pool * 8, []
    for f in row["frames"]:
        groups, have = sp.lw_choose(plan, cus, f, reserved, have)          # (a call builds the tables it lacks)
        held = pool if f <= reserved else 0
        part = lw = 0
        if groups:
            sc = sp.lw_plan_scratch(plan.layout, groups, budget, held)
            pool, lw = max(pool, sc["need"]), -(-S // sc["chunk"]) * len(groups)
        elif plan.path == 1:
            sc = sp.part_scratch(plan, f, budget, held)
            pool, part = max(pool, sc["need"]), -(-S // sc["chunk"])
        calls.append([f, pool * 8, part, lw] + [g[0] for g in groups] + [0] * (2 - len(groups)))
    return after_reserve, calls


def replay_host(row):
    S, C, b = row["streams"], row["channels"], {"f32": 4, "s16": 2}[row["format"]]
    mb = int(row["env"]["AW_HOST_CHUNK_MB"])
    reserved_chunk = sp.host_chunk_streams(S, C, row["reserve"], b, mb) if row["reserve"] else 0
    return [[f, sp.staged_chunk_streams(S, C, f, b, mb, row["reserve"], reserved_chunk), 0] for f in row["frames"]]


def test_replay_of_the_recorded_rows(tool, recorded):
    head = recorded["header"]
    assert head["device_columns"] == tool.DEVICE_COLUMNS and head["host_columns"] == tool.HOST_COLUMNS
    rows = tool.rows()
    assert [r["name"] for r in rows] == [r["name"] for r in recorded["rows"]]
    wrong = []
    for row, rec in zip(rows, recorded["rows"]):
        if row["entry"] == "host":
            if rec["after_reserve"] != 0 or replay_host(row) != rec["calls"]:
                wrong.append((row["name"], replay_host(row), rec))
            continue
        after_reserve, calls = replay_device(row, head["cus"])
        # the forward transform of one stream chunk is one to three launches (interior, head and boundary windows), the same for every chunk
        got = [[f, pool, chunks, lw, r0, r1] for f, pool, _, chunks, lw, r0, r1 in rec["calls"]]
        forward_ok = all(chunks == 0 and fwd == 0 or chunks > 0 and fwd % chunks == 0 and 1 <= fwd // chunks <= 3 for _, _, fwd, chunks, *_ in rec["calls"])
        if after_reserve != rec["after_reserve"] or calls != got or not forward_ok:
            wrong.append((row["name"], after_reserve, calls, rec))
    assert not wrong, wrong


def test_the_recorded_rows_cover_what_they_should(tool, recorded):
    """Both partitioned forms and the long-window kernels of a path-0 spatializer, each with everything in one chunk, chunks that do not
    divide the stream count and one stream per chunk, reserved and not; two groups of windows; a clamp to the held pool; the host entry."""
    rows = {r["name"]: r for r in tool.rows()}
    rec = {r["name"]: r["calls"] for r in recorded["rows"]}
    for kind, col, S in (("march", 3, 5), ("group", 3, 3), ("longwin", 4, 20)):          # col: the column that counts the stream chunks
        for suffix in ("", "-reserved"):
            assert {c[col] for c in rec[f"{kind}-one-chunk{suffix}"]} - {0} == {1}, kind
            assert any(1 < c[col] < S and S % c[col] for c in rec[f"{kind}-ragged-chunks{suffix}"]), kind
            assert any(c[col] == S for c in rec[f"{kind}-one-stream{suffix}"]), kind
    assert pp.Plan(8, 8640, 20).path == 0 and all(c[5] > 0 for c in rec["longwin-one-chunk"][1:])
    assert pp.Plan(7, 20000, 5).cmac_group == 0 and pp.Plan(14, 40000, 3).fwd_one_pair == 1 and rows["group-one-chunk"]["env"]["AW_PART_CMAC"] == "group"
    assert any(c[5] and c[6] for c in rec["longwin-two-groups"]) and any(c[5] and c[6] for c in rec["longwin-two-groups-reserved"])
    # a call shorter than the reserve whose chunk is the held pool's, not the budget's: more chunks than the unreserved handle runs
    clamped = [(n, a[0]) for n in rows if rows[n]["entry"] == "device" and n + "-reserved" in rec
               for a, b in zip(rec[n + "-reserved"], rec[n]) if a[3] + a[4] > b[3] + b[4]]
    assert clamped and all(f < rows[n]["frames"][-1] for n, f in clamped), clamped
    assert [c[1] for c in rec["host-f32"]] == [0, 6, 3] and [c[1] for c in rec["host-f32-reserved"]] == [3, 3, 3]
    assert [c[1] for c in rec["host-s16"]][-1] == 7 and [c[1] for c in rec["host-s16-reserved"]] == [7, 7, 7]


# ---- restatement ---------------------------------------------------------------------------------------------------------------------
def _chunk(budget_bytes, held, per_stream, streams, cap=None):
    """The five-line clamp both paths had: budget / per_stream, at most what the held pool holds (if it holds one), at least 1, at most
    the stream count (and the grid limit)."""
    chunk = budget_bytes // (per_stream * 8)
    held_chunk = held // per_stream
    chunk = np.where((held_chunk >= 1) & (chunk > held_chunk), held_chunk, chunk)
    chunk = np.minimum(np.maximum(chunk, 1), streams)
    return chunk if cap is None else np.minimum(chunk, cap)


def _part(g, frames, budget, held):
    """part_plan of runtime.cpp."""
    n_blocks = (frames + g["hop"] - 1) // g["hop"]
    n_windows = n_blocks + g["partitions"] - 1
    per_stream, per_stream_w = n_windows * g["n_pairs"] * N, n_blocks * N
    chunk = _chunk(budget, held, per_stream + per_stream_w, g["streams"], PART_CAP)
    return {"n_blocks": n_blocks, "n_windows": n_windows, "per_stream": per_stream, "per_stream_w": per_stream_w, "chunk": chunk,
            "need": (per_stream + per_stream_w) * chunk, "wspec_at": per_stream * chunk}


def _lw(g, R, windows, budget, held):
    """lw_scratch and lw_plan_scratch of runtime.cpp for the groups (R[i], windows[i]) (R == 0: no such group)."""
    C, S = g["channels"], g["streams"]
    real_last, n_pairs = C & 1, (C + 1) // 2
    out, chunks = {}, []
    for i in range(2):
        Nw = R[i] * LW_M
        spec_per_sw = (n_pairs - real_last) * Nw + np.where(real_last == 1, Nw // 2, 0)
        per_stream = windows[i] * (spec_per_sw + Nw)
        chunk = np.where(R[i] > 0, _chunk(budget, held, np.maximum(per_stream, 1), S), S)
        out.update({f"spec_per_sw{i}": spec_per_sw, f"per_stream{i}": per_stream, f"chunk{i}": np.where(R[i] > 0, chunk, 0)})
        chunks.append(chunk)
    out["chunk"] = np.minimum(np.minimum(chunks[0], chunks[1]), S)
    out["need"] = np.maximum(out["per_stream0"], out["per_stream1"]) * out["chunk"]
    for i in range(2):
        out[f"wrows_at{i}"] = out["chunk"] * windows[i] * out[f"spec_per_sw{i}"]
    return out


def _call(g, prefix, held):
    """The scratch of the grid's calls `prefix` ("in_": inside the reserve, "un_": never reserved) restated: {field: (restated, emulated)}."""
    lw_runs, part_runs = g[prefix + "n_groups"] > 0, (g[prefix + "n_groups"] == 0) & (g["path"] == 1)
    part = _part(g, g["frames"], g["budget"], held)
    lw = _lw(g, (g[prefix + "R0"], g[prefix + "R1"]), (g[prefix + "windows0"], g[prefix + "windows1"]), g["budget"], held)
    out = {"part_" + f: (np.where(part_runs, v, 0), g[prefix + "part_" + f]) for f, v in part.items()}
    out.update({"lw_" + f: (np.where(lw_runs, v, 0), g[prefix + "lw_" + f]) for f, v in lw.items()})
    return out


def test_restatement_of_the_calls(grid):
    g = grid
    assert len(g["frames"]) > 1_100_000
    for prefix, held in (("in_", g["res_need"]), ("un_", np.zeros_like(g["res_need"]))):
        fields = _call(g, prefix, held)
        assert set(fields) == {f for f in sp.SCRATCH_FIELDS if f not in sp.CALL_FIELDS}
        for f, (want, got) in fields.items():
            bad = np.flatnonzero(want != got)
            assert bad.size == 0, (prefix + f, bad.size, {k: int(g[k][bad[0]]) for k in sp.GRID_FIELDS}, int(want[bad[0]]))


def test_restatement_of_the_reserve(grid):
    """The sizing block of aw_spatializer_reserve: the reserve plan's scratch; on the partitioned path also the longest call the policy
    leaves to the partitioned kernels and ONE stream of the reserved length."""
    g = grid
    zero = np.zeros_like(g["budget"])
    lw = _lw(g, (g["res_R0"], g["res_R1"]), (g["res_windows0"], g["res_windows1"]), g["budget"], zero)
    need = np.where(g["res_n_groups"] > 0, lw["need"], 0)
    chunk = np.where(g["res_n_groups"] > 0, lw["chunk"], g["streams"])
    longest = _part(g, np.maximum(g["longest"], 1), g["budget"], zero)
    one = _part(g, g["reserve"], g["budget"], zero)
    part = g["path"] == 1
    need = np.where(part & (g["longest"] > 0), np.maximum(need, longest["need"]), need)
    need = np.where(part, np.maximum(need, one["per_stream"] + one["per_stream_w"]), need)
    chunk = np.where(part & (g["res_n_groups"] == 0), one["chunk"], chunk)
    assert np.array_equal(need, g["res_need"]) and np.array_equal(chunk, g["res_chunk"])
    assert np.all(g["longest"][~part] == 0) and np.all(g["longest"] <= g["reserve"])


@pytest.mark.parametrize("channels,taps,streams,reserve", [(7, 20000, 5, 120000), (7, 32768, 128, 480000), (2, 12289, 16, 70000), (14, 40000, 3, 3000000),
                                                           (16, 6146, 1024, 9000), (8, 8640, 128, 200001)])
def test_restatement_of_the_longest_partitioned_call(channels, taps, streams, reserve):
    """part_longest_call of runtime.cpp: the strided scan over whole blocks, one lw_choose per step."""
    plan = pp.Plan(channels, taps, streams)
    longest = 0
    if plan.path == 1:
        B = plan.hop
        n_blocks = (reserve + B - 1) // B
        stride = max(1, n_blocks // 2048)
        nb = 1
        while True:
            f = min(min(nb, n_blocks) * B, reserve)
            if not sp.lw_choose(plan, CUS, f, for_reserve=True)[0]:
                longest = min(f + (stride - 1) * B, reserve)
            if nb >= n_blocks:
                break
            nb += stride
    assert sp.part_longest_call(plan, CUS, reserve) == longest


def test_stream_chunk_restated():
    rng = np.random.default_rng(5)
    for _ in range(20000):
        per_stream = int(rng.integers(1, 1 << int(rng.integers(1, 36))))
        budget = int(rng.integers(0, 1 << int(rng.integers(1, 40))))
        held = int(rng.integers(0, 1 << int(rng.integers(1, 40)))) * int(rng.integers(0, 2))
        streams = int(rng.integers(1, 1 << int(rng.integers(1, 18))))
        for cap in (None, PART_CAP):
            want = int(_chunk(np.int64(budget * 8), np.int64(held), np.int64(per_stream), np.int64(streams), cap))
            assert sp.stream_chunk(budget, held, per_stream, streams, -1 if cap is None else cap) == want


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def test_chunk_bounds_and_regions(grid):
    g = grid
    for prefix in ("in_", "un_"):
        part, lw = g[prefix + "part_chunk"] > 0, g[prefix + "n_groups"] > 0
        assert not np.any(part & lw) and np.all((part | lw) == ((g["path"] == 1) | lw))
        for runs, chunk, need, per_stream in ((part, g[prefix + "part_chunk"], g[prefix + "part_need"], g[prefix + "part_per_stream"] + g[prefix + "part_per_stream_w"]),
                                              (lw, g[prefix + "lw_chunk"], g[prefix + "lw_need"], np.maximum(g[prefix + "lw_per_stream0"], g[prefix + "lw_per_stream1"]))):
            assert np.all(chunk[runs] >= 1) and np.all(chunk[runs] <= g["streams"][runs])
            assert np.array_equal(need[runs], (per_stream * chunk)[runs])
            assert np.all((need * 8 <= g["budget"])[runs & (chunk > 1)])
        assert np.all(g[prefix + "part_chunk"] <= PART_CAP)
        # the partitioned W region and every group's rows + s1/s2 end inside the pool the call asked for
        assert np.array_equal((g[prefix + "part_wspec_at"] + g[prefix + "part_per_stream_w"] * g[prefix + "part_chunk"])[part], g[prefix + "part_need"][part])
        for i in ("0", "1"):
            windows, R = g[prefix + "windows" + i], g[prefix + "R" + i]
            end = g[prefix + "lw_wrows_at" + i] + g[prefix + "lw_chunk"] * windows * R * LW_M
            assert np.all((end <= g[prefix + "lw_need"])[lw]) and np.all((g[prefix + "lw_wrows_at" + i] >= g[prefix + "lw_chunk"] * windows * g[prefix + "lw_spec_per_sw" + i])[lw])


def test_default_budget():
    last = 0
    for free in [0, 1, 100 * MiB, 160 * MiB - 1, 160 * MiB, 161 * MiB, 1 * GiB, 15 * GiB, 159 * GiB, 160 * GiB, 160 * GiB + 5, 288 * GiB, 1 << 50]:
        b = sp.default_budget(True, free)
        assert b == max(min(64 * GiB, free // 5 * 2), 64 * MiB) and 64 * MiB <= b <= 64 * GiB and b >= last
        last = b
    assert sp.default_budget(False, 0) == sp.default_budget(False, 1 << 50) == 6 * GiB


def _over(g):
    return np.maximum(g["in_part_need"], g["in_lw_need"]) > g["res_need"]


def test_no_call_inside_the_reserve_outgrows_it_from_two_streams_a_chunk_on(grid):
    """On the tables of the reserve plan and with the pool the reserve sized: no shorter call needs more, wherever the reserve plan runs at
    least two streams per chunk."""
    assert not np.any(_over(grid) & (grid["res_chunk"] >= 2))


@pytest.mark.xfail(strict=True, reason="reserve gap: where the budget holds fewer than two streams of the reserve plan, a shorter call of a path-0 spatializer on the "
                                       "long-window kernels picks another window grouping from the reserve's tables whose ONE stream is larger than everything "
                                       "aw_spatializer_reserve sized; the held clamp (held / per_stream == 0) does not apply and the pool grows inside process")
def test_no_call_inside_the_reserve_outgrows_it(grid):
    over = _over(grid)
    assert not np.any(over), (int(over.sum()), sorted(set(grid["path"][over].tolist())), int(grid["res_chunk"][over].max()))


def test_the_reserve_gap_pinned():
    """16 channels x 5200 taps x 128 streams on 256 CUs, 96 MiB, reserve(1 000 000), then 810 887 frames: one group of 4 windows of 56 rows,
    8 257 536 elements against 7 077 888 reserved.  (The pull request that fixes the reserve turns `>` into `<=`.)"""
    plan = pp.Plan(16, 5200, 128)
    assert plan.path == 0
    res, have = sp.lw_choose(plan, 256, 1000000, for_reserve=True)
    need, chunk = sp.reserve_need(plan, 256, res, 1000000, 96 * MiB)
    call, _ = sp.lw_choose(plan, 256, 810887, 1000000, have)
    assert call == [(56, 4)] and chunk == 1
    got = sp.lw_plan_scratch(plan.layout, call, 96 * MiB, need)
    assert (got["need"], need) == (8257536, 7077888) and got["need"] > need


# ---- host entry ----------------------------------------------------------------------------------------------------------------------
def test_host_chunks_restated_and_inside_a_host_reserve():
    def restated(S, C, frames, b, mb):          # host_chunk_streams of runtime.cpp
        chunk_bytes, per_stream = mb << 20, frames * C * b
        if S < 4 or per_stream * S < 2 * chunk_bytes:
            return 0
        return min(max(max(1, chunk_bytes // per_stream), 2), (S + 1) // 2)
    assert sp.host_chunk_streams(24, 8, 9001, 4, 1) == 3 and sp.host_chunk_streams(24, 8, 9001, 2, 1) == 7
    n = 0
    for S in (1, 3, 4, 5, 24, 128, 1024):
        for C in (1, 2, 7, 8, 14, 16):
            for b in (2, 3, 4):
                for mb in (1, 8, 64):
                    for reserve in (4096, 9001, 70000, 480000):
                        rc = sp.host_chunk_streams(S, C, reserve, b, mb)
                        assert rc == restated(S, C, reserve, b, mb)
                        sized = sp.staged_streams(rc, S) * reserve          # frames the staging holds (x channels x bytes: the same both sides)
                        assert sp.staged_streams(rc, S) == (2 * rc if rc > 0 else S)
                        for frames in sorted({1, 64, reserve // 9, reserve // 3, reserve // 2, reserve - 1, reserve, reserve + 1, 3 * reserve}):
                            cs = sp.staged_chunk_streams(S, C, frames, b, mb, reserve, rc)
                            own = restated(S, C, frames, b, mb)
                            inside = frames <= reserve
                            assert cs == ((min(own, rc) if own > 0 else rc) if rc > 0 else 0) if inside else cs == own
                            if inside:          # the same formats as the reserve: never more streams a chunk, never more staging
                                assert cs <= rc and sp.staged_streams(cs, S) * frames <= sized
                            n += 1
    assert n > 10000
