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
//
// The PCM form (rateconv_tile_pcm; rule: rateconv.hpp, "integer PCM in and out") is the same tile with a decode in the LDS fill and an
// encode in the pass that leaves the gathered image.  The float32 form above is the code it always was (PCM is a template argument, so no
// branch of the PCM form is compiled into it); inside the PCM form the two formats, the dither mode, the gain and the records are uniform
// run-time branches, for they stand outside the tap loop.  Input of any byte alignment is read in aligned 16-byte words where the whole
// word lies inside the call's buffer and byte by byte elsewhere; an element belongs to the word that holds its first byte, and the up to
// three bytes it may have in the next word are read singly (with the byte behind them where the buffer holds it).  On the way out a thread encodes whole elements once, in place in the gathered
// image (so every count is taken once), and behind a barrier the tile's bytes leave as aligned 4-byte words put together from those codes,
// with single bytes at the tile's ragged ends: no word shared with a neighbouring tile or stream is read or rewritten.
//
// The measuring forms (rateconv_tile_pcm_tp, rateconv_tile_tp_measure; rule: rateconv.hpp, "true peak of the converted output") are the PCM
// form with the true-peak rule of truepeak.hpp applied to the gathered image between the tap loop and the encode, which overwrites that
// image.  A frame needs its 11 predecessors: the gathered image is [11 + valid][channels], and its first 11 frames are the stream's
// carried history for the first tile of a call and outputs o0 - 11 .. o0 - 1, computed again, for every later one (tiles run in parallel;
// where a tile is shorter than 11 and o0 - 11 < 0, the history supplies the frames before the call: no input before history ++ call is
// needed).  A measuring tile is therefore 11 outputs shorter,
// rc_tp_tile, inside the same LDS layout.  The tile that holds the stream's last output writes the last 11 cleaned frames of its image
// into the other history slot.  TP is a template argument beside PCM, so neither earlier form carries a branch of it.
#pragma once
#include <cstdint>

#include "rateconv.hpp"

namespace awk {

constexpr int kRcThreads = 256;
constexpr int kRcLdsFloats = 12288;                               // 48 KB, static: input image + output image
constexpr int kRcMaxTile = 4096;
constexpr int kRcSegmentShift = 5, kRcSegment = 1 << kRcSegmentShift;      // the input image lies in segments of 32 frames ...
constexpr int kRcHalo = 3;                                        // ... each behind a copy of the 3 frames before it

// One stream's record (aw_rateconv_levels): every field is a max or an integer sum.
struct RateconvLevels {
    uint32_t peak_bits;              // the bits of max |y| over finite samples, before gain (a float >= 0 orders as its bits do)
    uint32_t reserved;
    unsigned long long frames, clipped, nonfinite;
};

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
    // ---- the PCM form only (rateconv_tile_pcm, launch_rateconv_pcm); all zero: F32 in and out, no dither, no gain, no records ----
    int in_format, out_format;       // awp::Format of in and out, which then are byte buffers of any alignment
    int dither;                      // awp::Dither of an s16 / s24 encode
    unsigned long long dither_seed, first_stream;      // global stream = first_stream + s
    const float *gains;              // [n_streams], or NULL: no gain
    RateconvLevels *levels;          // [n_streams], or NULL: not metered
    unsigned long long *clipped;     // NULL, or the word every tile adds its clipped count to
};

using RateconvTruePeak = awrc::TruePeakRecord;                    // one stream's true-peak record (aw_rateconv_true_peak)

// What the measuring forms take beside RateconvParams.
struct RateconvTp {
    const float *hist_in;            // [n_streams][11][channels] cleaned output frames before this call (oldest first)
    float *hist_out;                 // ... before the next call (another buffer); written only by a call that produces frames
    RateconvTruePeak *records;       // [n_streams]
    int tile;                        // rc_tp_tile(L, M, taps, channels)
    float c[awtp::kCoefficients];    // awtp::filter
};

constexpr int kRcTpOff = 0, kRcTpOn = 1, kRcTpOnly = 2;           // TP of rateconv_tile_form: not measured; measured and written; measured only

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

// The tile length of the measuring forms: 11 gathered frames and their span go to the predecessors.  A function of (L, M, T, channels)
// only; 0 or less: this handle has no measuring tile.
inline int rc_tp_tile(int L, int M, int taps, int channels) { return rc_tile(L, M, taps, channels) - awtp::kHistory; }

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

// ---- the PCM form's element helpers ----
AWP_HD uint32_t rc_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
// 32 bits at byte `o` (0 .. 15) of the little-endian words x0 .. x4; scalars and selects, so that nothing here is an indexed array
AWP_HD uint32_t rc_bytes_at(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t x4, int o) {
    const int i = o >> 2, sh = (o & 3) * 8;
    const uint32_t lo = i == 0 ? x0 : i == 1 ? x1 : i == 2 ? x2 : x3;
    const uint32_t hi = i == 0 ? x1 : i == 1 ? x2 : i == 2 ? x3 : x4;
    return (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh);
}
// the up to four bytes at `at` .. `at` + 3 of a buffer of `total` bytes as a little-endian word; bytes outside the buffer are not read
AWP_HD uint32_t rc_word_bytewise(const unsigned char *base, long long at, long long total) {
    uint32_t u = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (at + j >= 0 && at + j < total) u |= (uint32_t)base[at + j] << (8 * j);
    return u;
}
// awp::decode_at of an element whose little-endian bytes are the low bytes of u
AWP_HD float rc_decode(int fmt, uint32_t u) {
    if (fmt == awp::kS16) return awp::decode_s16((int16_t)(uint16_t)u);
    if (fmt == awp::kS24) return awp::decode_s24(u & 0xFFu, (u >> 8) & 0xFFu, (u >> 16) & 0xFFu);
    if (fmt == awp::kS32) return awp::decode_s32((int32_t)u);
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// awp::encode_dithered_at as the integer it would write (its low format_bytes bytes); F32: the float's bits
AWP_HD uint32_t rc_encode(int fmt, int mode, float x, uint64_t key, uint64_t n, int e, unsigned *clip) {
    if (fmt == awp::kS32) return (uint32_t)awp::encode_s32(x, clip);
    if (fmt == awp::kS16 || fmt == awp::kS24) {
        if (mode == awp::kDitherNone) return (uint32_t)(fmt == awp::kS16 ? awp::encode_s16(x, clip) : awp::encode_s24(x, clip));
        const float d = awp::dither_value(mode, key, n, e);
        return (uint32_t)(fmt == awp::kS16 ? awp::encode_s16_dithered(x, d, clip) : awp::encode_s24_dithered(x, d, clip));
    }
    return rc_bits(x);
}
// element e of the call's buffer (flat over [streams][frames][channels]), one element at a time: the history write
template <bool PCM> AWP_HD float rc_input(const RateconvParams &p, long long e) {
    if constexpr (PCM) return awp::decode_at(p.in_format, reinterpret_cast<const unsigned char *>(p.in) + e * awp::format_bytes(p.in_format));
    else return p.in[e];
}
// byte b of a tile's output: byte b % bytes of the code of element b / bytes
AWP_HD uint32_t rc_out_byte(const float *codes, int b, int bytes) {
    const int k = bytes == 2 ? b >> 1 : bytes == 3 ? b / 3 : b >> 2;
    return (rc_bits(codes[k]) >> (8 * (b - k * bytes))) & 0xFFu;
}

// The PCM form's LDS fill: elements e0 .. e0 + n - 1 of the call's buffer (flat over [streams][frames][channels]) decoded into image
// frames first_frame ..; nothing outside [p.in, p.in + bytes of the call) is read.
template <class Ctx> AWP_HD void rc_fill_pcm(const Ctx &ctx, const RateconvParams &p, float *image, long long e0, int n, int first_frame) {
    const int C = p.channels, fi = p.in_format, bi = awp::format_bytes(fi);
    const unsigned char *base = reinterpret_cast<const unsigned char *>(p.in);
    const long long total = (long long)p.n_streams * p.in_frames * C * bi, b0 = e0 * bi;   // bytes of the call; byte of the span's first element
    const int q = (int)(reinterpret_cast<uintptr_t>(base + b0) & 15u);                    // bytes between the 16-byte boundary below and the span
    const bool straddles = bi == 3 || (reinterpret_cast<uintptr_t>(base) & (uintptr_t)(bi - 1)) != 0;      // elements may cross a word's end
    const int n_words = (n * bi + q + 15) >> 4;
    for (int w = ctx.tid(); w < n_words; w += kRcThreads) {
        const int r0 = 16 * w - q;                                 // byte of the span the word starts at
        const long long wb = b0 + r0;                              // ... of the buffer
        uint32_t x0, x1, x2, x3;
        if (wb >= 0 && wb + 16 <= total) {
            float v[4];
            ctx.ld16(reinterpret_cast<const float *>(base + wb), v);
            x0 = rc_bits(v[0]); x1 = rc_bits(v[1]); x2 = rc_bits(v[2]); x3 = rc_bits(v[3]);
        } else {                                                   // a word that reaches past the buffer: its bytes one by one
            x0 = rc_word_bytewise(base, wb, total); x1 = rc_word_bytewise(base, wb + 4, total);
            x2 = rc_word_bytewise(base, wb + 8, total); x3 = rc_word_bytewise(base, wb + 12, total);
        }
        const uint32_t x4 = straddles ? rc_word_bytewise(base, wb + 16, total) : 0u;      // what an element that starts here has over there
        int k = r0 <= 0 ? 0 : (r0 + bi - 1) / bi;                  // the first element that starts in this word
#pragma unroll
        for (int j = 0; j < 8; ++j, ++k) {                         // (at most 8 elements start in 16 bytes)
            const int o = k * bi - r0;
            if (o < 16 && k < n) {
                const int f = k / C;
                rc_store(image, first_frame + f, k - f * C, C, rc_decode(fi, rc_bytes_at(x0, x1, x2, x3, x4, o)));
            }
        }
    }
}

// The PCM form's way out of the gathered image [valid][C]: gain, dither, encode and the records, then the tile's own bytes.
template <class Ctx> AWP_HD void rc_leave_pcm(const Ctx &ctx, const RateconvParams &p, float *gathered, long long s, long long o0, int valid) {
    const int t = ctx.tid(), C = p.channels, fo = p.out_format, bo = awp::format_bytes(fo);
    const float g = p.gains ? p.gains[s] : 1.0f;
    const uint64_t key0 = awp::dither_key(p.dither_seed, p.first_stream + (uint64_t)s);
    const uint64_t n0 = (uint64_t)(p.produced + o0);
    uint32_t peak = 0u;
    unsigned nonfinite = 0u, clipped = 0u;
    for (int k = t; k < valid * C; k += kRcThreads) {              // element k: read, encoded and put back by this thread alone
        const int f = k / C, ch = k - f * C;
        const float y = gathered[k];
        const uint32_t a = rc_bits(y) & 0x7FFFFFFFu;
        if (a >= 0x7F800000u) ++nonfinite; else peak = a > peak ? a : peak;
        const float u = p.gains ? y * g : y;
        unsigned clip = 0u;
        const uint32_t code = rc_encode(fo, p.dither, u, key0 + (uint64_t)(ch >> 1) * 0xA0761D6478BD642Full, n0 + (uint64_t)f, ch & 1, &clip);
        __builtin_memcpy(&gathered[k], &code, 4);                  // (the image stays an array of float: its elements now carry the codes' bits)
        clipped += clip;
    }
    if (p.levels || p.clipped) {                                   // (uniform: every wave is whole at the wave operations)
        const unsigned c = ctx.wave_sum(clipped);
        if ((t & 63) == 0 && c) {
            if (p.levels) ctx.atomic_add(&p.levels[s].clipped, (unsigned long long)c);
            if (p.clipped) ctx.atomic_add(p.clipped, (unsigned long long)c);
        }
    }
    if (p.levels) {
        const uint32_t m = ctx.wave_max(peak);
        const unsigned nf = ctx.wave_sum(nonfinite);
        if ((t & 63) == 0) {
            if (m) ctx.atomic_max(&p.levels[s].peak_bits, m);
            if (nf) ctx.atomic_add(&p.levels[s].nonfinite, (unsigned long long)nf);
        }
        if (t == 0) ctx.atomic_add(&p.levels[s].frames, (unsigned long long)valid);
    }
    ctx.barrier();
    unsigned char *out = reinterpret_cast<unsigned char *>(p.out) + (s * p.out_frames + o0) * C * bo;
    const int n = valid * C * bo;                                  // the tile's bytes
    int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(out) & 3u)) & 3u);       // ... in front of its first whole word
    head = head < n ? head : n;
    const int n_words = (n - head) >> 2, tail = head + 4 * n_words;
    if (bo == 4 && head == 0) {
        for (int w = t; w < n_words; w += kRcThreads) reinterpret_cast<uint32_t *>(out)[w] = rc_bits(gathered[w]);
    } else {
        for (int w = t; w < n_words; w += kRcThreads) {
            const int b = head + 4 * w;
            *reinterpret_cast<uint32_t *>(out + b) = rc_out_byte(gathered, b, bo) | (rc_out_byte(gathered, b + 1, bo) << 8) |
                                                     (rc_out_byte(gathered, b + 2, bo) << 16) | (rc_out_byte(gathered, b + 3, bo) << 24);
        }
    }
    if (t < head) out[t] = (unsigned char)rc_out_byte(gathered, t, bo);
    if (t >= 64 && t - 64 < n - tail) out[tail + t - 64] = (unsigned char)rc_out_byte(gathered, tail + t - 64, bo);
}

// The measuring forms' pass over the gathered image [11 + valid][C], whose first 11 frames are the predecessors: the contribution of
// every frame and channel of the tile to the stream's record, and (last: the tile holds the stream's last output) the next history.
// Reads the image only.
template <class Ctx> AWP_HD void rc_measure(const Ctx &ctx, const RateconvParams &p, const RateconvTp &tp, const float *gathered, long long s, int valid, bool last) {
    const int t = ctx.tid(), C = p.channels, H = awtp::kHistory;
    uint32_t true_peak = 0u, sample_peak = 0u;
#pragma unroll 1
    for (int k = t; k < valid * C; k += kRcThreads) {              // element k of the tile: frame k / C, channel k % C
        const float *top = gathered + H * C + k;
        float w[awtp::kTaps];                                      // w[j] = v[n - j]
        unsigned nonfinite = 0u;
#pragma unroll
        for (int j = 0; j < awtp::kTaps; ++j) w[j] = awtp::filter_input(top[-j * C], nonfinite);
        const uint32_t a = awtp::float_bits(w[0]) & 0x7FFFFFFFu, m = awtp::frame_peak_bits(tp.c, w, 1);
        sample_peak = a > sample_peak ? a : sample_peak;
        true_peak = m > true_peak ? m : true_peak;
    }
    const uint32_t wt = ctx.wave_max(true_peak), ws = ctx.wave_max(sample_peak);       // (uniform: every wave is whole here)
    if ((t & 63) == 0) {
        if (wt) ctx.atomic_max(&tp.records[s].true_peak_bits, wt);
        if (ws) ctx.atomic_max(&tp.records[s].sample_peak_bits, ws);
    }
    if (t == 0) ctx.atomic_add(&tp.records[s].frames, (unsigned long long)valid);
    if (last) {
        unsigned nonfinite = 0u;
        for (int k = t; k < H * C; k += kRcThreads) tp.hist_out[s * H * C + k] = awtp::filter_input(gathered[valid * C + k], nonfinite);
    }
}

// `tile` counts the tiles of this call; a call without outputs runs tile 0 for the history alone.  PCM: p.in and p.out are byte buffers of
// p.in_format and p.out_format, and the gain, the dither and the records of p apply; else the float32 form, which reads none of those.
// TP (kRcTpOn, kRcTpOnly; PCM only): tiles of tp->tile outputs, measured into tp->records; kRcTpOnly writes no output, no levels record and
// no clip count.
template <bool PCM, int TP, class Ctx>
AWP_HD void rateconv_tile_form(const Ctx &ctx, const RateconvParams &p, const RateconvTp *tp, long long s, long long tile) {
    static_assert(TP == kRcTpOff || PCM, "the measuring forms are forms of the PCM form");
    float *image = ctx.lds();
    const int t = ctx.tid();
    const int C = p.channels, T = p.taps, D = p.latency, CB = rc_block(C);
    int step = p.tile;
    if constexpr (TP != kRcTpOff) step = tp->tile;
    const long long o0 = tile * step;                                                      // the tile's first output within the call
    const int valid = (int)(p.out_frames - o0 < step ? p.out_frames - o0 : step);          // outputs of this tile (0: none at all)
    if (valid > 0) {
        // the measuring forms compute the outputs before a later tile again, up to 11 and as many as the call has: `lead` of them, `made` in all
        const int lead = TP != kRcTpOff ? (int)(o0 < awtp::kHistory ? o0 : awtp::kHistory) : 0, made = valid + lead;
        const long long n0 = p.produced + o0 - lead;                                       // absolute output index
        const int p0 = awrc::phase(n0, p.L, p.M);
        const long long lo = awrc::input_index(n0, p.L, p.M) + D - (T - 1);                // absolute input frames lo .. hi
        const long long hi = awrc::input_index(n0 + made - 1, p.L, p.M) + D;
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
        } else if constexpr (PCM) {
            if (n_floats > 0) rc_fill_pcm(ctx, p, image, (s * p.in_frames + (rel + n_hist)) * C, n_floats, n_hist);
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
        float *gathered = image + rc_image_floats(rc_span(p.tile, p.L, p.M, T), C);        // [made][C]; measuring: [11 + valid][C]
        float *computed = gathered;                                                        // where output n0 goes
        if constexpr (TP != kRcTpOff) {                            // the predecessors from before the call: history frames o0 .. 10
            for (int k = t; k < (awtp::kHistory - lead) * C; k += kRcThreads) gathered[k] = tp->hist_in[(s * awtp::kHistory + o0) * C + k];
            computed += (awtp::kHistory - lead) * C;
        }
        const int NB = C / CB, G = (made + p.L - 1) / p.L, classes = made < p.L ? made : p.L;
        for (int item = t; item < classes * G * NB; item += kRcThreads) {
            const int b = item % NB, g = (item / NB) % G, r = item / (NB * G);
            const int o = r + p.L * g;
            if (o >= made) continue;
            // (n0 + o) M = i(n0) L + p(n0) + o M: inside the tile the position is 32-bit arithmetic, p(n0) + o M < 640 + 4096 * 640
            const unsigned v = (unsigned)p0 + (unsigned)o * (unsigned)p.M;
            const int f0 = (int)(v / (unsigned)p.L) + (T - 1);                             // i(n0 + o) + D - lo
            const float *row = p.c + (long long)(v % (unsigned)p.L) * p.row_stride;
            float *y = computed + o * C + b * CB;
            if (CB == 4) rc_output<4>(ctx, image + b * 4, row, f0, C, T, y);
            else if (CB == 2) rc_output<2>(ctx, image + b * 2, row, f0, C, T, y);
            else rc_output<1>(ctx, image + b, row, f0, C, T, y);
        }
        ctx.barrier();
        if constexpr (TP != kRcTpOff) {
            rc_measure(ctx, p, *tp, gathered, s, valid, o0 + valid == p.out_frames);
            if constexpr (TP == kRcTpOn) {
                ctx.barrier();                                     // (the encode below overwrites what the measurement reads)
                rc_leave_pcm(ctx, p, gathered + awtp::kHistory * C, s, o0, valid);
            }
        } else if constexpr (PCM) {
            rc_leave_pcm(ctx, p, gathered, s, o0, valid);
        } else {
            float *out = p.out + (s * p.out_frames + o0) * C;
            for (int k = t; k < valid * C; k += kRcThreads) out[k] = gathered[k];
        }
    }
    const long long tiles = (p.out_frames + step - 1) / step;
    if (tile == (tiles > 0 ? tiles - 1 : 0)) {                     // the stream's last tile: the last T - 1 frames of (history ++ call)
        for (int k = t; k < (T - 1) * C; k += kRcThreads) {
            const long long f = p.in_frames - (T - 1) + k / C;     // frame of the call
            p.hist_out[s * (T - 1) * C + k] = f >= 0 ? (p.in ? rc_input<PCM>(p, (s * p.in_frames + f) * C + k % C) : 0.0f)
                                                     : p.hist_in[(s * (T - 1) + (f + (T - 1))) * C + k % C];
        }
        if (t == 0) {
            p.counts[2 * s] = p.consumed + p.in_frames;
            p.counts[2 * s + 1] = p.produced + p.out_frames;
        }
    }
}

template <class Ctx> AWP_HD void rateconv_tile(const Ctx &ctx, const RateconvParams &p, long long s, long long tile) {
    rateconv_tile_form<false, kRcTpOff>(ctx, p, nullptr, s, tile);
}
template <class Ctx> AWP_HD void rateconv_tile_pcm(const Ctx &ctx, const RateconvParams &p, long long s, long long tile) {
    rateconv_tile_form<true, kRcTpOff>(ctx, p, nullptr, s, tile);
}
// The PCM form, measured: also adds to tp.records and carries tp.hist_in to tp.hist_out.
template <class Ctx> AWP_HD void rateconv_tile_pcm_tp(const Ctx &ctx, const RateconvParams &p, const RateconvTp &tp, long long s, long long tile) {
    rateconv_tile_form<true, kRcTpOn>(ctx, p, &tp, s, tile);
}
// The measurement alone: the input history, the counts, tp.records and tp.hist_out move; p.out, p.gains, p.levels and p.clipped are not used.
template <class Ctx> AWP_HD void rateconv_tile_tp_measure(const Ctx &ctx, const RateconvParams &p, const RateconvTp &tp, long long s, long long tile) {
    rateconv_tile_form<true, kRcTpOnly>(ctx, p, &tp, s, tile);
}

}  // namespace awk
