// limiter_tile.hpp — device code of the limiter kernel (rules: limiter.hpp): one workgroup of kLimThreads threads produces one tile of
// kLimTile output frames of one stream.  Plain C++ over an execution context (stage_gpu_ctx.hpp: the GPU's; tests/emu/emu_stage_ctx.hpp:
// threads on the CPU), so the code hipcc compiles is the code the emulation runs.
//
// LDS holds three images (49,440 bytes: three workgroups per CU):
//   U  the raw u of the tile behind its halo of halo(L, H) frames, as [frame][2] floats.  Read from global memory once, in 16-byte words
//      whatever the stream's alignment (truepeak_tile.hpp), times the stream's pre-gain; the halo is earlier frames of the call or, in a
//      stream's first tiles, the carried history.
//   Q  q of the tile and of the q_halo(L, H) frames before it: a thread takes rows of four frames, reads their 15-frame window with
//      16-byte LDS reads (lanes 8 dwords apart: conflict-free per group of eight), cleans it and runs truepeak.hpp's 72 FMAs per frame.
//      The sliding minimum over W frames is then formed in place by window doubling: a pass with reach d turns minima over s frames
//      into minima over s + d <= 2 s; min is idempotent, so the last pass may overlap and ceil(log2 W) passes suffice.
//   P  the exclusive prefix sums of m over the tile and the L - 1 frames before it, in uint64_t (six entries per thread, a wave scan,
//      four wave totals): S[n] = P[n + L] - P[n].
// The store multiplies the delayed u by g and writes z with 16-byte stores where a word lies inside the tile.  Records take one atomic
// per wave and quantity.  The tile that holds the stream's last frame writes the next call's history from U, into the other slot: no
// tile reads what another writes, and the kernel is out of place (neighbouring tiles read each other's input).
#pragma once
#include <cstdint>

#include "limiter.hpp"

namespace awk {

constexpr int kLimThreads = 256;
constexpr int kLimTile = 1024;                                    // output frames per workgroup
constexpr int kLimRowFrames = 4;                                  // frames a thread's detector step covers
constexpr int kLimUBase = 2072;                                   // frames in front of the tile in U: the halo and the 3 a first row may reach past it
constexpr int kLimQBase = 2064;                                   // ... in Q: q_halo rounded up to whole rows, and a multiple of 4
constexpr int kLimPPerThread = 6;
constexpr int kLimPEntries = kLimThreads * kLimPPerThread;        // 1536 >= kLimTile + kMaxAttack
constexpr int kLimQPerThread = (kLimQBase + kLimTile + kLimThreads - 1) / kLimThreads;      // 13
constexpr int kLimPBytes = (kLimPEntries + kLimThreads / 64) * 8;
constexpr int kLimUFloats = (kLimUBase + kLimTile) * 2;
constexpr int kLimLdsBytes = kLimPBytes + kLimUFloats * 4 + (kLimQBase + kLimTile) * 4;
static_assert(kLimUBase >= awlim::kMaxHalo + kLimRowFrames - 1 && kLimUBase % 2 == 0, "U");
static_assert(kLimQBase >= awlim::kMaxHalo - awtp::kHistory + kLimRowFrames - 1 && kLimQBase % kLimRowFrames == 0, "Q");
static_assert(kLimPEntries >= kLimTile + awlim::kMaxAttack && kLimPBytes % 16 == 0 && kLimLdsBytes <= 65536, "P");

struct LimiterParams {
    const float *in;                 // [n_streams][frames][2], dense, 4-byte aligned: the chunk's float32 output y before the gain
    float *out;                      // the same shape, another buffer: z
    long long frames;
    int n_streams;
    const float *gain;               // [n_streams] pre-gains, or NULL (every one 1)
    const float *hist_in;            // [n_streams][halo(L, H)][2] raw u before this call (oldest first)
    float *hist_out;                 // ... before the next call (another buffer)
    uint32_t *min_gain;              // [n_streams] bits, lowered
    unsigned long long *limited;     // [n_streams], added to
    unsigned long long *nonfinite;   // [n_streams], added to
    int L, H;
    float ceiling;
    float c[awtp::kCoefficients];
};

template <class Ctx> AWP_HD void limiter_tile(const Ctx &ctx, const LimiterParams &p, long long s, long long tile) {
    unsigned char *lds = ctx.lds();
    unsigned long long *P = reinterpret_cast<unsigned long long *>(lds);
    unsigned long long *wave_total = P + kLimPEntries;
    float *U = reinterpret_cast<float *>(lds + kLimPBytes);
    uint32_t *Q = reinterpret_cast<uint32_t *>(U + kLimUFloats);
    const int t = ctx.tid();
    const int L = p.L, W = awlim::window(p.L, p.H), D = awlim::delay(p.L), QH = awlim::q_halo(p.L, p.H), HL = awlim::halo(p.L, p.H);
    const long long f0 = tile * kLimTile;
    const int valid = (int)(p.frames - f0 < kLimTile ? p.frames - f0 : kLimTile);          // frames of this tile, >= 1
    const long long e0 = (s * p.frames + f0) * 2, n_total = (long long)p.n_streams * p.frames * 2;
    const float g_s = p.gain ? p.gain[s] : 1.0f;

    // ---- load: float k of the image is float 2 * f0 + k of the stream; the call's own floats start at k_call
    const int k_call = f0 >= HL ? -2 * HL : (int)(-2 * f0);
    unsigned nf = 0;
    {
        const int q = (int)((reinterpret_cast<uintptr_t>(p.in + e0 + k_call) >> 2) & 3u);   // floats between the 16-byte boundary below and k_call
        const int n_floats = 2 * valid - k_call, n_words = (n_floats + q + 3) >> 2;
        for (int w = t; w < n_words; w += kLimThreads) {
            const int k0 = k_call - q + 4 * w;
            const long long e = e0 + k0;
            float x[4];
            if (e >= 0 && e + 4 <= n_total) {
                ctx.ld16(p.in + e, x);
            } else {                                       // a word that reaches past the chunk: its floats one by one
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = (e + j >= 0 && e + j < n_total) ? p.in[e + j] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + j;
                if (k < k_call || k >= 2 * valid) continue;
                const float u = awlim::pre_gain(x[j], g_s);
                unsigned ignored = 0;                      // (a halo frame is counted by the tile that owns it)
                (void)awtp::filter_input(u, k >= 0 ? nf : ignored);
                U[k + 2 * kLimUBase] = u;
            }
        }
        const float *h = p.hist_in + s * (2ll * HL) + 2 * (f0 + HL);                       // float k of the image, for k < k_call
        for (int k = -2 * HL + t; k < k_call; k += kLimThreads) U[k + 2 * kLimUBase] = h[k];
    }
    ctx.barrier();

    // ---- detector: rows of four frames from frame -QHr of the image on
    {
        const int QHr = (QH + kLimRowFrames - 1) & ~(kLimRowFrames - 1), n_rows = (QHr + valid + kLimRowFrames - 1) / kLimRowFrames;
        for (int i = t; i < n_rows; i += kLimThreads) {
            const int fr = -QHr + kLimRowFrames * i;
            // win[j] = float 2 * (fr - 11) + j of the image: the row's 4 frames behind their 11 predecessors
            float win[2 * (awtp::kHistory + kLimRowFrames)];
            const float *r = U + 2 * (fr - awtp::kHistory) + 2 * kLimUBase;
            ctx.ld_lds8(r, win);
#pragma unroll
            for (int j = 0; j < 7; ++j) ctx.ld_lds16(r + 2 + 4 * j, win + 2 + 4 * j);
            unsigned ignored = 0;
#pragma unroll
            for (int j = 0; j < 2 * (awtp::kHistory + kLimRowFrames); ++j) win[j] = awtp::filter_input(win[j], ignored);
#pragma unroll
            for (int j = 0; j < kLimRowFrames; ++j)
                if (fr + j >= -QH && fr + j < valid) {
                    const uint32_t a = awtp::frame_peak_bits(p.c, win + 2 * awtp::kHistory + 2 * j, -2);
                    const uint32_t b = awtp::frame_peak_bits(p.c, win + 2 * awtp::kHistory + 2 * j + 1, -2);
                    Q[fr + j + kLimQBase] = awlim::required_q(a > b ? a : b, p.ceiling);
                }
        }
    }
    ctx.barrier();

    // ---- sliding minimum over W frames, in place: Q[i] = min(q[i - (W - 1)] .. q[i]) for i >= lo + W - 1
    {
        const int lo = kLimQBase - QH, hi = kLimQBase + valid;
        for (int span = 1; span < W;) {
            const int d = span < W - span ? span : W - span;
            uint32_t x[kLimQPerThread];
#pragma unroll
            for (int j = 0; j < kLimQPerThread; ++j) {
                const int i = lo + t + kLimThreads * j;
                x[j] = 0;
                if (i < hi) {
                    x[j] = Q[i];
                    if (i - d >= lo) { const uint32_t o = Q[i - d]; x[j] = o < x[j] ? o : x[j]; }
                }
            }
            ctx.barrier();
#pragma unroll
            for (int j = 0; j < kLimQPerThread; ++j) {
                const int i = lo + t + kLimThreads * j;
                if (i < hi) Q[i] = x[j];
            }
            ctx.barrier();
            span += d;
        }
    }

    // ---- exclusive prefix sums of m from frame -(L - 1) on: P[j] = m[-(L - 1)] + .. + m[-(L - 1) + j - 1], j = 0 .. L - 1 + valid
    {
        const int n_m = L - 1 + valid, j0 = kLimPPerThread * t;
        const uint32_t *M = Q + kLimQBase - (L - 1);
        unsigned long long v[kLimPPerThread], tot = 0;
#pragma unroll
        for (int i = 0; i < kLimPPerThread; ++i) { v[i] = tot; tot += j0 + i < n_m ? (unsigned long long)M[j0 + i] : 0ull; }
        const unsigned long long before = ctx.wave_exclusive_sum(tot);
        if ((t & 63) == 63) wave_total[t >> 6] = before + tot;
        ctx.barrier();
        unsigned long long base = before;
        for (int w = 0; w < (t >> 6); ++w) base += wave_total[w];
#pragma unroll
        for (int i = 0; i < kLimPPerThread; ++i)
            if (j0 + i <= n_m) P[j0 + i] = base + v[i];
    }
    ctx.barrier();

    // ---- store: z of the tile in 16-byte words of the output buffer
    uint32_t g_min = awlim::kOneBits;
    unsigned limited = 0;
    {
        float *o = p.out + e0;
        const int q = (int)((reinterpret_cast<uintptr_t>(o) >> 2) & 3u);
        const int n_floats = 2 * valid, n_words = (n_floats + q + 3) >> 2;
        for (int w = t; w < n_words; w += kLimThreads) {
            const int k0 = 4 * w - q;
            float x[4];
            float g = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + j, fr = k >> 1;
                x[j] = 0.0f;
                if (k < 0 || k >= n_floats) continue;
                if (j == 0 || (k & 1) == 0) g = awlim::ramp_gain(P[fr + L] - P[fr], L);
                if ((k & 1) == 0) {
                    const uint32_t gb = awl::float_bits(g);
                    g_min = gb < g_min ? gb : g_min;
                    limited += gb < awlim::kOneBits ? 1u : 0u;
                }
                x[j] = awlim::limit(U[k - 2 * D + 2 * kLimUBase], g);
            }
            if (k0 >= 0 && k0 + 4 <= n_floats) {
                ctx.st16(o + k0, x);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + j >= 0 && k0 + j < n_floats) o[k0 + j] = x[j];
            }
        }
    }
    if (f0 + valid == p.frames) {                          // the stream's last tile: the last HL frames of (history ++ call)
        float *h = p.hist_out + s * (2ll * HL);
        for (int i = t; i < 2 * HL; i += kLimThreads) h[i] = U[2 * (valid - HL) + i + 2 * kLimUBase];
    }
    g_min = ctx.wave_min(g_min);
    limited = ctx.wave_sum(limited);
    nf = ctx.wave_sum(nf);
    if ((t & 63) == 0) {
        if (g_min < awlim::kOneBits) ctx.atomic_min(p.min_gain + s, g_min);
        if (limited) ctx.atomic_add(p.limited + s, (unsigned long long)limited);
        if (nf) ctx.atomic_add(p.nonfinite + s, (unsigned long long)nf);
    }
}

}  // namespace awk
