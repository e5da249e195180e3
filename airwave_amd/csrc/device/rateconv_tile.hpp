// rateconv_tile.hpp — device code of the sample-rate converter (rules: rateconv.hpp): one workgroup of kRcThreads threads converts one tile
// of output frames of one stream.  Plain C++ over an execution context (stage_gpu_ctx.hpp: the GPU's; tests/emu/emu_stage_ctx.hpp: threads
// on the CPU), so the code hipcc compiles is the code the emulation runs.
//
// A tile of `tile` outputs needs the input frames i(first) + D - (T - 1) .. i(last) + D, at most ceil(tile M / L) + T of them.  They go
// from global memory into LDS once, in 16-byte words whatever the stream's alignment (a dense [streams][frames][channels] buffer puts a
// stream on any float); frames before the call come from the carried history instead.  The LDS image is the span in segments of 32
// frames, each behind a copy of the 3 frames before it.  That makes a segment 35 frames long: the windows of two outputs of one phase lie
// M frames apart, and M = 160, 320 or 640 frames of a dense image would put a whole wave's reads on one bank, while 175, 350 or 700 do
// not (an odd multiple of 8 bytes, or 2 or 4 lanes per bank at the worst).  And it makes the four frames of four consecutive taps
// contiguous wherever the first one lies, so a group of four taps costs one position and four reads.  A thread owns one output and one
// block of 1, 2 or 4 channels (whatever divides the channel count, so a block is one LDS read).  Work items are ordered by phase first:
// outputs n and n + L share the coefficient row, so the lanes of a wave read a few rows between them, not 64, and a row's 16-byte words
// come through the caches once per wave.  The T multiply-adds run k = 0, 1, .., T - 1 as the rule has them.  Results are gathered in a second LDS region and leave in frame order, so the
// stores are dense although a wave's outputs lie L frames apart.  The last tile of a stream also writes the next call's history — the last
// T - 1 frames of (history ++ call), straight from global memory — into the other slot, and the stream's counts: no tile reads what
// another writes.  Positions in a stream are 64-bit; inside a tile they are offsets from the tile's first output and fit 32 bits.
#pragma once
#include <cstdint>

#include "rateconv.hpp"

namespace awk {

constexpr int kRcThreads = 256;
constexpr int kRcLdsFloats = 12288;                               // 48 KB, static: input image + output image
constexpr int kRcMaxTile = 4096;
constexpr int kRcSegmentShift = 5, kRcSegment = 1 << kRcSegmentShift;      // the input image lies in segments of 32 frames ...
constexpr int kRcHalo = 3;                                        // ... each behind a copy of the 3 frames before it

struct RateconvParams {
    const float *in;                 // [n_streams][in_frames][channels], dense, 4-byte aligned; NULL: in_frames frames of zeros (flush)
    long long in_frames;             // > 0
    float *out;                      // [n_streams][out_frames][channels]
    long long out_frames;            // what this call produces; 0: only the history and the counts move
    int n_streams, channels;
    int L, M, taps, latency;
    int tile;                        // rc_tile(L, M, taps, channels)
    int row_stride;                  // floats between the rows of c: taps rounded up to a multiple of 4
    const float *c;                  // [L][row_stride], 16-byte aligned
    const float *hist_in;            // [n_streams][taps - 1][channels] frames before this call (oldest first)
    float *hist_out;                 // ... before the next call (another buffer)
    long long consumed, produced;    // the streams' counts before this call
    long long *counts;               // [n_streams][2]: consumed, produced after it
};

AWP_HD int rc_block(int channels) { return channels % 4 == 0 ? 4 : channels % 2 == 0 ? 2 : 1; }
AWP_HD int rc_row_stride(int taps) { return (taps + 3) & ~3; }
// LDS position of channel 0 of frame f of the input image: segment f / 32 starts with its halo of kRcHalo frames
AWP_HD int rc_lds_at(int f, int channels) { return (f + kRcHalo * (f >> kRcSegmentShift) + kRcHalo) * channels; }
// floats of an input image of `span` frames (the halo of the segment behind the last one included), a multiple of 4
AWP_HD int rc_image_floats(int span, int channels) {
    return ((((span - 1) >> kRcSegmentShift) + 1) * (kRcSegment + kRcHalo) * channels + kRcHalo * channels + 3) & ~3;
}
// the most input frames a tile of `tile` outputs reads
AWP_HD int rc_span(int tile, int L, int M, int taps) { return (int)(((long long)tile * M + L - 1) / L) + taps; }
// The tile length of a handle: the longest, up to kRcMaxTile, whose two images fit kRcLdsFloats.  A function of (L, M, T, channels) only.
inline int rc_tile(int L, int M, int taps, int channels) {
    int lo = 0, hi = kRcMaxTile;                                   // lo fits (0: nothing does), hi + 1 does not
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (rc_image_floats(rc_span(mid, L, M, taps), channels) + mid * channels <= kRcLdsFloats) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <int CB, class Ctx> AWP_HD void rc_read(const Ctx &ctx, const float *l, float (&x)[CB]) {
    if constexpr (CB == 4) ctx.ld_lds16(l, x);
    else if constexpr (CB == 2) ctx.ld_lds8(l, x);
    else x[0] = l[0];
}

// One frame of the call or of the history into the image, and into the halo of the next segment when it is one of a segment's last 3.
AWP_HD void rc_store(float *image, int f, int ch, int channels, float v) {
    const int at = rc_lds_at(f, channels) + ch;
    image[at] = v;
    if ((f & (kRcSegment - 1)) >= kRcSegment - kRcHalo) image[at + kRcHalo * channels] = v;
}

// Taps k .. k + 3 of one output and channel block: cw their coefficients, f the image frame of tap k.  Tap k + j reads frame f - j, which
// lies j frames below f in the image whether or not a segment ends between them: that is what the halo is for.
template <int CB, bool FIRST, class Ctx>
AWP_HD void rc_taps4(const Ctx &ctx, const float *image, int f, int channels, const float (&cw)[4], float (&acc)[CB]) {
    const float *top = image + rc_lds_at(f, channels);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x[CB];
        rc_read<CB>(ctx, top - j * channels, x);
#pragma unroll
        for (int e = 0; e < CB; ++e) acc[e] = (FIRST && j == 0) ? cw[0] * x[e] : __builtin_fmaf(cw[j], x[e], acc[e]);
    }
}

// One output of one channel block: row = c[p_n], `image` the input image at the block's first channel, f0 the image frame of tap 0.
// The coefficients come sixteen taps at a time, so that four loads are in flight before the first is waited for.
template <int CB, class Ctx>
AWP_HD void rc_output(const Ctx &ctx, const float *image, const float *row, int f0, int channels, int taps, float *y) {
    float acc[CB], cw[4][4];
    ctx.ld16(row, cw[0]);
    rc_taps4<CB, true>(ctx, image, f0, channels, cw[0], acc);
    int k = 4;
    for (; k + 16 <= taps; k += 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ctx.ld16(row + k + 4 * i, cw[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) rc_taps4<CB, false>(ctx, image, f0 - k - 4 * i, channels, cw[i], acc);
    }
    for (; k + 4 <= taps; k += 4) {
        ctx.ld16(row + k, cw[0]);
        rc_taps4<CB, false>(ctx, image, f0 - k, channels, cw[0], acc);
    }
    for (; k < taps; ++k) {                                        // (T = 2 D: two taps at most)
        float x[CB];
        rc_read<CB>(ctx, image + rc_lds_at(f0 - k, channels), x);
#pragma unroll
        for (int e = 0; e < CB; ++e) acc[e] = __builtin_fmaf(row[k], x[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < CB; ++e) y[e] = acc[e];
}

// `tile` counts the tiles of this call; a call without outputs runs tile 0 for the history alone.
template <class Ctx> AWP_HD void rateconv_tile(const Ctx &ctx, const RateconvParams &p, long long s, long long tile) {
    float *image = ctx.lds();
    const int t = ctx.tid();
    const int C = p.channels, T = p.taps, D = p.latency, CB = rc_block(C);
    const long long o0 = tile * p.tile;                                                    // the tile's first output within the call
    const int valid = (int)(p.out_frames - o0 < p.tile ? p.out_frames - o0 : p.tile);      // outputs of this tile (0: none at all)
    if (valid > 0) {
        const long long n0 = p.produced + o0;                                              // absolute output index
        const int p0 = awrc::phase(n0, p.L, p.M);
        const long long lo = awrc::input_index(n0, p.L, p.M) + D - (T - 1);                // absolute input frames lo .. hi
        const long long hi = awrc::input_index(n0 + valid - 1, p.L, p.M) + D;
        const int span = (int)(hi - lo + 1);                                               // <= rc_span(p.tile, ..)
        const long long rel = lo - p.consumed;                                             // frame of the call; >= -(T - 1)
        const int n_hist = rel < 0 ? (int)(-rel < span ? -rel : span) : 0;                 // frames the history supplies
        for (int k = t; k < n_hist * C; k += kRcThreads) {         // (rel < 0 here)
            const int f = k / C;
            rc_store(image, f, k - f * C, C, p.hist_in[(s * (T - 1) + (rel + (T - 1))) * C + k]);
        }
        const int n_floats = (span - n_hist) * C;                                          // floats of the call's own frames
        if (!p.in) {
            for (int k = t; k < n_floats; k += kRcThreads) {
                const int f = k / C;
                rc_store(image, n_hist + f, k - f * C, C, 0.0f);
            }
        } else if (n_floats > 0) {
            const long long e0 = (s * p.in_frames + (rel + n_hist)) * C, n_total = (long long)p.n_streams * p.in_frames * C;
            const int q = (int)((reinterpret_cast<uintptr_t>(p.in + e0) >> 2) & 3u);       // floats between the 16-byte boundary below and the span
            const int n_words = (n_floats + q + 3) >> 2;
            for (int w = t; w < n_words; w += kRcThreads) {
                const long long e = e0 - q + 4ll * w;
                const int k0 = 4 * w - q;
                float x[4];
                if (e >= 0 && e + 4 <= n_total) {
                    ctx.ld16(p.in + e, x);
                } else {                                           // a word that reaches past the buffer: its floats one by one
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j] = (e + j >= 0 && e + j < n_total) ? p.in[e + j] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + j >= 0 && k0 + j < n_floats) {
                        const int f = (k0 + j) / C;
                        rc_store(image, n_hist + f, k0 + j - f * C, C, x[j]);
                    }
            }
        }
        ctx.barrier();
        // work items: (phase class r, member g of the class, channel block b), b fastest, then g
        float *gathered = image + rc_image_floats(rc_span(p.tile, p.L, p.M, T), C);        // [valid][C]
        const int NB = C / CB, G = (valid + p.L - 1) / p.L, classes = valid < p.L ? valid : p.L;
        for (int item = t; item < classes * G * NB; item += kRcThreads) {
            const int b = item % NB, g = (item / NB) % G, r = item / (NB * G);
            const int o = r + p.L * g;
            if (o >= valid) continue;
            // (n0 + o) M = i(n0) L + p(n0) + o M: inside the tile the position is 32-bit arithmetic, p(n0) + o M < 640 + 4096 * 640
            const unsigned v = (unsigned)p0 + (unsigned)o * (unsigned)p.M;
            const int f0 = (int)(v / (unsigned)p.L) + (T - 1);                             // i(n0 + o) + D - lo
            const float *row = p.c + (long long)(v % (unsigned)p.L) * p.row_stride;
            float *y = gathered + o * C + b * CB;
            if (CB == 4) rc_output<4>(ctx, image + b * 4, row, f0, C, T, y);
            else if (CB == 2) rc_output<2>(ctx, image + b * 2, row, f0, C, T, y);
            else rc_output<1>(ctx, image + b, row, f0, C, T, y);
        }
        ctx.barrier();
        float *out = p.out + (s * p.out_frames + o0) * C;
        for (int k = t; k < valid * C; k += kRcThreads) out[k] = gathered[k];
    }
    const long long tiles = (p.out_frames + p.tile - 1) / p.tile;
    if (tile == (tiles > 0 ? tiles - 1 : 0)) {                     // the stream's last tile: the last T - 1 frames of (history ++ call)
        for (int k = t; k < (T - 1) * C; k += kRcThreads) {
            const long long f = p.in_frames - (T - 1) + k / C;     // frame of the call
            p.hist_out[s * (T - 1) * C + k] = f >= 0 ? (p.in ? p.in[(s * p.in_frames + f) * C + k % C] : 0.0f)
                                                     : p.hist_in[(s * (T - 1) + (f + (T - 1))) * C + k % C];
        }
        if (t == 0) {
            p.counts[2 * s] = p.consumed + p.in_frames;
            p.counts[2 * s + 1] = p.produced + p.out_frames;
        }
    }
}

}  // namespace awk
