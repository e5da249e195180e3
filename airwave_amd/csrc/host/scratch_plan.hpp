// scratch_plan.hpp — how much scratch a call needs and how many streams run per chunk: the sizing of the context's pool (partitioned and
// long-window kernels), of aw_spatializer_reserve() and of the host entry's staged chunks, as pure functions.
// Plain C++ like path_policy.hpp: no device call, no environment lookup, no allocation, no handle — runtime.cpp asks the device for its
// free memory, reads the knobs, calls these and keeps the side effects (pool_grow, timers, reserved_pool); tests/test_scratch_plan_host.py
// checks them on the CPU against a literal restatement and against what the built library did (tests/golden/scratch_plan_parent.json,
// written by tools/scratch_table.py).  Units: complex elements of 8 bytes for the pool, bytes for budgets.
//   stream_chunk()          streams per chunk: what the budget holds; inside what reserve sized (held_elems > 0) at most what the pool that
//                           is already there holds — a short call would otherwise pick a larger chunk whose rounding can exceed it; at
//                           least one stream, whatever the budget says
//   part_scratch()          the partitioned kernels' scratch of a call;  lw_scratch() / lw_plan_scratch(): the long-window kernels'
//   default_budget()        where AW_SPEC_SCRATCH_MB is not set: min(64 GiB, 40 % of the device memory free when first needed) — sized for
//                           288 GB of HBM: cfg 3 (1024 streams x 10 s, 4 pairs, 8 partitions) needs 40 GB and runs as one chunk
//   reserve_need()          what aw_spatializer_reserve() sizes the pool for, and the stream chunk of its plan
//   host_chunk_streams()    host entry: streams per staged chunk (0: the whole batch in one piece, serial — small batches, plug-in shaped
//                           calls); AW_HOST_CHUNK_MB counts input bytes as they cross PCIe, so a 16-bit batch moves twice the streams per
//                           chunk of a float32 one;  staged_chunk_streams(): ... or, inside what a host reserve sized, its chunking
// SURVEY §8b, "process must not allocate after reserve": a call inside the reserved length clamps its stream chunk to the pool that is
// there.  Known gap (the test pins it): where the budget holds fewer than two streams of the reserve plan, a shorter call of a path-0
// spatializer can pick another window grouping whose ONE stream is larger than everything reserve_need() sized, and the pool grows.
#pragma once
#include <climits>
#include "path_policy.hpp"

namespace awp {

constexpr size_t kElemBytes = 8;                                                   // one complex float of the pool
constexpr long long kPartChunkCap = 65535, kNoChunkCap = LLONG_MAX;               // grid.y / grid.z of the CMAC launches; the long-window path has none

inline long long stream_chunk(size_t budget_elems, size_t held_elems, size_t per_stream, long long streams, long long cap) {
    long long chunk = (long long)(budget_elems / per_stream);
    const long long held_chunk = (long long)(held_elems / per_stream);
    if (held_chunk >= 1 && chunk > held_chunk) chunk = held_chunk;
    return std::min(std::min(std::max(chunk, 1LL), streams), cap);
}

// Partitioned path, calls of `frames` frames: window spectra (per_stream) + accumulated W (per_stream_w) of one stream chunk.
struct PartScratch {
    int n_blocks; long long n_windows; size_t per_stream, per_stream_w; long long chunk; size_t need;
    size_t wspec_at() const { return per_stream * (size_t)chunk; }          // where W starts inside the pool
};
inline PartScratch part_scratch(const Layout &l, const CreatePlan &p, int64_t frames, size_t budget_bytes, size_t held_elems = 0) {
    PartScratch s{};
    s.n_blocks = (int)((frames + p.hop - 1) / p.hop);
    s.n_windows = (long long)s.n_blocks + p.partitions - 1;
    s.per_stream = (size_t)s.n_windows * p.n_pairs * awk::kN;
    s.per_stream_w = (size_t)s.n_blocks * awk::kN;
    s.chunk = stream_chunk(budget_bytes / kElemBytes, held_elems, s.per_stream + s.per_stream_w, l.streams, kPartChunkCap);
    s.need = (s.per_stream + s.per_stream_w) * (size_t)s.chunk;
    return s;
}

// Long-window path, one group of windows: rows of every (stream, window) + s1/s2 of one stream chunk.
struct LwScratch {
    long long n_windows; size_t per_stream; long long chunk; size_t need; long long spec_per_sw;
    size_t wrows_at(long long call_chunk) const { return (size_t)call_chunk * n_windows * spec_per_sw; }      // where the group's rows start
};
inline LwScratch lw_scratch(const Layout &l, int R, long long n_windows, size_t budget_bytes, size_t held_elems) {
    LwScratch r{};
    const long long N = (long long)R * awk::kLwM;
    const int real_last = l.channels & 1, n_pairs = (l.channels + 1) / 2;          // (a fused2 spatializer's n_pairs counts pseudo-pairs)
    r.n_windows = n_windows;
    r.spec_per_sw = (long long)(n_pairs - real_last) * N + (real_last ? N / 2 : 0);
    r.per_stream = (size_t)r.n_windows * (size_t)(r.spec_per_sw + N);
    r.chunk = stream_chunk(budget_bytes / kElemBytes, held_elems, r.per_stream, l.streams, kNoChunkCap);
    r.need = r.per_stream * (size_t)r.chunk;
    return r;
}
// ... and a whole call plan: every group of the plan runs on the same chunk of streams
struct LwPlanScratch { long long chunk; size_t need; LwScratch g[2]; };
inline LwPlanScratch lw_plan_scratch(const Layout &l, const LwCallPlan &plan, size_t budget_bytes, size_t held_elems) {
    LwPlanScratch all{l.streams, 0, {}};
    for (int i = 0; i < plan.n_groups; ++i) {
        all.g[i] = lw_scratch(l, plan.g[i].R, plan.g[i].n_windows, budget_bytes, held_elems);
        all.chunk = std::min(all.chunk, all.g[i].chunk);
    }
    for (int i = 0; i < plan.n_groups; ++i) all.need = std::max(all.need, all.g[i].per_stream * (size_t)all.chunk);
    return all;
}

inline size_t default_budget(bool known, size_t free_bytes) {          // known: hipMemGetInfo succeeded
    const size_t b = known ? std::min<size_t>((size_t)64 << 30, free_bytes / 5 * 2) : (size_t)6 << 30;
    return std::max<size_t>(b, (size_t)64 << 20);
}

// The longest call of at most max_frames frames that the policy (lw_choose with every window length available) leaves to the partitioned
// kernels (0: none; a path-0 spatializer never runs them).  A reserved spatializer only has the window lengths of its reserve() plan, so a
// call well short of max_frames may still come to the partitioned kernels beyond this length: it then runs in stream chunks clamped to the
// pool, correct and a little slower — what reserve() buys is no allocation, and the full rate at the length it was asked for.  Scanned in
// steps of whole blocks; with more than 2048 candidate lengths the scan strides and answers one stride longer, i.e. never too short.
inline int64_t part_longest_call(const LwInputs &in, int64_t max_frames) {
    if (in.plan.path != 1) return 0;
    const int64_t B = in.plan.hop, n_blocks = (max_frames + B - 1) / B;
    const int64_t stride = std::max<int64_t>(1, n_blocks / 2048);
    int64_t longest = 0;
    for (int64_t nb = 1;; nb += stride) {
        const int64_t f = std::min<int64_t>(std::min(nb, n_blocks) * B, max_frames);
        if (!lw_choose(in, f, true).n_groups) longest = std::min<int64_t>(f + (stride - 1) * B, max_frames);
        if (nb >= n_blocks) break;
    }
    return longest;
}

// lw_res: lw_choose(in, the frames asked for, true), whose tables the reserve builds; reserved_frames: the longest length reserved so far
struct ReserveNeed { size_t need; long long chunk; };
inline ReserveNeed reserve_need(const LwInputs &in, const LwCallPlan &lw_res, int64_t reserved_frames, size_t budget_bytes) {
    ReserveNeed r{0, in.layout.streams};
    const LwPlanScratch lw = lw_plan_scratch(in.layout, lw_res, budget_bytes, 0);
    if (lw_res.n_groups) r = ReserveNeed{lw.need, lw.chunk};
    if (in.plan.path == 1) {
        // Shorter calls may still run on the partitioned kernels: size for the longest call lw_choose() leaves to them (cfg 3: 45 056
        // of 480 000 frames, 4 GB — round 4 sized for max_frames on BOTH kernel sets: 41.5 GB where the long-window kernels need 19),
        // and for ONE stream of reserved_frames whatever the policy says (a call inside the reserved size clamps its stream chunk to the
        // buffer that is there, stream_chunk: it never reallocates).
        const int64_t longest = part_longest_call(in, reserved_frames);
        if (longest > 0) r.need = std::max(r.need, part_scratch(in.layout, in.plan, longest, budget_bytes).need);
        const PartScratch one = part_scratch(in.layout, in.plan, reserved_frames, budget_bytes);
        r.need = std::max(r.need, one.per_stream + one.per_stream_w);
        if (!lw_res.n_groups) r.chunk = one.chunk;
    }
    return r;
}

inline int64_t host_chunk_streams(int streams, int channels, int64_t frames, size_t in_bytes, int host_chunk_mb) {          // in_bytes: per input sample
    const size_t chunk_bytes = (size_t)host_chunk_mb << 20;
    const size_t per_stream = (size_t)frames * channels * in_bytes;
    if (streams < 4 || per_stream * streams < 2 * chunk_bytes) return 0;
    const int64_t cs = std::max<int64_t>((int64_t)(chunk_bytes / per_stream), 2);
    return std::min<int64_t>(cs, (streams + 1) / 2);
}
inline int64_t staged_chunk_streams(int streams, int channels, int64_t frames, size_t in_bytes, int host_chunk_mb, int64_t reserved_frames, int64_t reserved_chunk) {
    const int64_t cs = host_chunk_streams(streams, channels, frames, in_bytes, host_chunk_mb);
    if (frames > reserved_frames) return cs;
    return reserved_chunk > 0 ? (cs > 0 ? std::min(cs, reserved_chunk) : reserved_chunk) : 0;
}
// streams the staging buffers hold: two chunks in flight each way, or the whole batch
inline size_t staged_streams(int64_t chunk, int streams) { return chunk > 0 ? 2 * (size_t)chunk : (size_t)streams; }

}  // namespace awp
