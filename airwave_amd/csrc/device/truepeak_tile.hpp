// truepeak_tile.hpp — device code of the true-peak kernel (rules: truepeak.hpp): one workgroup of kTpThreads threads measures one tile of
// kTpTile frames of one stream.  Plain C++ over an execution context (stage_gpu_ctx.hpp: the GPU's; tests/emu/emu_stage_ctx.hpp:
// threads on the CPU), so the code hipcc compiles is the code the emulation runs.
//
// A tile goes from global memory into LDS once, in 16-byte words whatever the stream's alignment (a dense [streams][frames][2] chunk
// puts every other stream 8 bytes off when `frames` is odd; a caller's buffer may start on any float).  Non-finite samples are replaced
// and counted on the way.  The LDS image is rows of 8 frames (16 floats) kTpRowStride floats apart: a thread owns one row and reads it,
// the row before and the last three frames of the row before that — its 8 frames and their 11 predecessors — with 16-byte LDS reads that
// the row stride keeps free of bank conflicts (16 lanes x 20 dwords cover the 64 banks once).  Two rows in front of the tile hold its
// halo: the 16 frames before it from global memory, or, in a stream's first tile, the carried history behind zeros.  After the 576 FMAs
// of its row a thread holds one peak per ear; a wave reduces them and lane 0 issues one atomic per quantity (a tile lies in one stream,
// so every wave does).  The tile that holds the stream's last frame writes the next call's history from the same LDS image, into the
// other slot: no tile reads what another writes.
#pragma once
#include <cstdint>

#include "truepeak.hpp"

namespace awk {

constexpr int kTpThreads = 256;
constexpr int kTpRowFrames = 8;                                   // frames per thread
constexpr int kTpTile = kTpThreads * kTpRowFrames;                // frames per workgroup tile: 2048
constexpr int kTpHaloRows = 2;                                    // 16 >= awtp::kHistory frames in front of the tile
constexpr int kTpRowFloats = 2 * kTpRowFrames, kTpRowStride = kTpRowFloats + 4;
constexpr int kTpLdsFloats = (kTpThreads + kTpHaloRows) * kTpRowStride;      // 20,640 bytes
constexpr int kTpWordsPerThread = kTpTile * 2 / 4 / kTpThreads;   // 16-byte words of a tile per thread: 4 (+ 1 ragged word per tile)
static_assert(kTpHaloRows * kTpRowFrames >= awtp::kHistory && kTpThreads >= 2 * kTpHaloRows * kTpRowFrames, "halo");

struct TruePeakParams {
    const float *in;                 // [n_streams][frames][2], dense, 4-byte aligned: the chunk's float32 output before the gain
    long long frames;
    int n_streams;
    const float *hist_in;            // [n_streams][kHistory][2] cleaned frames before this call (oldest first)
    float *hist_out;                 // ... before the next call (another buffer)
    uint32_t *tp_bits;               // [n_streams][2] cumulative, or NULL (only the call-local peak is wanted)
    unsigned long long *nonfinite;   // [n_streams], or NULL with tp_bits
    uint32_t *call_tp;               // [n_streams], zeroed by the caller at the start of the call
    float c[awtp::kCoefficients];
};

// LDS position of float k of the tile (k = 2 * frame + ear; down to -2 * 16 for the halo)
AWP_HD int tp_lds_at(int k) { return ((k + kTpHaloRows * kTpRowFloats) >> 4) * kTpRowStride + ((k + kTpHaloRows * kTpRowFloats) & 15); }

template <class Ctx> AWP_HD void truepeak_tile(const Ctx &ctx, const TruePeakParams &p, long long s, long long tile) {
    float *L = ctx.lds();
    const int t = ctx.tid();
    const long long f0 = tile * kTpTile;
    const int valid = (int)(p.frames - f0 < kTpTile ? p.frames - f0 : kTpTile);          // frames of this tile, >= 1
    const long long e0 = (s * p.frames + f0) * 2, n_total = (long long)p.n_streams * p.frames * 2;
    const int q = (int)((reinterpret_cast<uintptr_t>(p.in + e0) >> 2) & 3u);              // floats between the 16-byte boundary below and the tile
    const int n_floats = 2 * valid, n_words = (n_floats + q + 3) >> 2;
    unsigned nf = 0;
    for (int i = 0; i <= kTpWordsPerThread; ++i) {
        const int w = i * kTpThreads + t;
        if (w >= n_words) break;
        const long long e = e0 - q + 4ll * w;
        const int k0 = 4 * w - q;
        float x[4];
        if (e >= 0 && e + 4 <= n_total) {
            ctx.ld16(p.in + e, x);
        } else {                                           // a word that reaches past the chunk: its floats one by one
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = (e + j >= 0 && e + j < n_total) ? p.in[e + j] : 0.0f;
        }
        if (q == 0 && k0 + 4 <= n_floats) {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = awtp::filter_input(x[j], nf);
            ctx.st16(L + tp_lds_at(k0), x);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + j >= 0 && k0 + j < n_floats) L[tp_lds_at(k0 + j)] = awtp::filter_input(x[j], nf);
        }
    }
    if (t < 2 * kTpHaloRows * kTpRowFrames) {              // the halo: float t of the 16 frames before the tile
        const long long g = f0 - kTpHaloRows * kTpRowFrames + (t >> 1);     // frame of the stream
        const int ear = t & 1;
        float v = 0.0f;
        unsigned ignored = 0;                              // (counted by the tile that owns the frame)
        if (g >= 0) v = awtp::filter_input(p.in[(s * p.frames + g) * 2 + ear], ignored);
        else if (g + awtp::kHistory >= 0) v = p.hist_in[(s * awtp::kHistory + (g + awtp::kHistory)) * 2 + ear];
        L[(t >> 4) * kTpRowStride + (t & 15)] = v;
    }
    ctx.barrier();
    uint32_t pk[2] = {0u, 0u};
    if (t * kTpRowFrames < valid) {
        // win[i] = float 16 t - 22 + i of the tile: the thread's 8 frames behind their 11 predecessors
        float win[2 * (awtp::kHistory + kTpRowFrames)];
        const float *r = L + t * kTpRowStride;            // (row t - 2 of the tile)
        ctx.ld_lds8(r + 10, win);                          // floats 10 .. 11 of it, then 12 .. 15
        ctx.ld_lds16(r + 12, win + 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ctx.ld_lds16(r + kTpRowStride + 4 * i, win + 6 + 4 * i);
            ctx.ld_lds16(r + 2 * kTpRowStride + 4 * i, win + 22 + 4 * i);
        }
#pragma unroll
        for (int j = 0; j < kTpRowFrames; ++j)
            if (t * kTpRowFrames + j < valid) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const uint32_t m = awtp::frame_peak_bits(p.c, win + 2 * awtp::kHistory + 2 * j + e, -2);
                    pk[e] = m > pk[e] ? m : pk[e];
                }
            }
    }
    if (f0 + valid == p.frames && t < 2 * awtp::kHistory)  // the stream's last tile: the last 11 frames of (history ++ call)
        p.hist_out[s * (2 * awtp::kHistory) + t] = L[tp_lds_at(2 * (valid - awtp::kHistory) + t)];
    pk[0] = ctx.wave_max(pk[0]);
    pk[1] = ctx.wave_max(pk[1]);
    nf = ctx.wave_sum(nf);
    if ((t & 63) == 0) {
        if (p.tp_bits) {
            if (pk[0]) ctx.atomic_max(p.tp_bits + 2 * s, pk[0]);
            if (pk[1]) ctx.atomic_max(p.tp_bits + 2 * s + 1, pk[1]);
            if (nf) ctx.atomic_add(p.nonfinite + s, (unsigned long long)nf);
        }
        const uint32_t m = pk[0] > pk[1] ? pk[0] : pk[1];
        if (m) ctx.atomic_max(p.call_tp + s, m);
    }
}

}  // namespace awk
