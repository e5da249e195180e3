// pcm_kernels.hip — integer PCM <-> float32 streaming passes of the PCM entries (aw_spatializer_process_pcm / _process_host_pcm).
//
// Both kernels are bandwidth-bound: one thread per group of G elements whose PCM side spans a whole number of 16-byte words (s16: 8
// elements, 16 B; s24: 16 elements, 48 B = three dwords per four samples; s32: 4 elements, 16 B), so every load and store of the body
// is 16 B wide and coalesced.  The body starts where the ALIGNED side (decode: the float destination; encode: the PCM destination) meets a
// 16-byte boundary; the other side then sits at the same offset Q * 4 + b inside its 16-byte word for every group (G elements span whole
// words on both sides), so each thread loads the aligned words covering its group — one more when the offset is not zero, a word that
// still holds a byte of the group, so nothing past the buffer is touched — and funnels them into place (v_alignbyte).  Q is a template
// argument, so the funnel indexes registers.  The unaligned head (at most 15 elements) and the ragged tail (fewer than G) are one element
// per thread, byte by byte (pcm.hpp).  The dithered encode (s16 / s24, aw_spatializer_set_dither) is the same pass with the group's dither
// values computed in registers from the element index (group_dither); the undithered kernel is unchanged.
//
// Levels and gain (aw_spatializer_set_metering / _set_gain; rules: levels.hpp): aw_levels_kernel reads a chunk's float32 output once and
// adds every stream's peak, energy and non-finite count to its record, one atomic per wave and quantity; aw_scale_kernel multiplies
// float32 output by its stream's gain in place; the gained encode (aw_pcm_encode_gain_kernel) is the encode pass with the group's gains
// looked up the way its dither is, and with the clipped samples also counted per stream.  None of them runs, and the kernels above run as
// they always have, while the meter is off and no gain is set.
// One launcher serves the three encode kernels (launch_pcm_encode: a gain struct selects the gained kernel, a dither struct alone the
// dithered one, neither the plain one); the batch entries' one chunk step calls it (runtime.cpp: batch_chunk).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "levels.hpp"
#include "pcm.hpp"
#include "pcm_kernels.hpp"

namespace {

constexpr int kThreads = 256;

template <int FMT> struct Group;
template <> struct Group<awp::kS16> { static constexpr int G = 8, words = 1; };     // words: 16-B words of PCM per group
template <> struct Group<awp::kS24> { static constexpr int G = 16, words = 3; };
template <> struct Group<awp::kS32> { static constexpr int G = 4, words = 1; };

__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t b) { return b ? __builtin_amdgcn_alignbyte(hi, lo, b) : lo; }

// element index of the idx-th one-element thread: the head [0, head), then the tail after the body
__device__ __forceinline__ int64_t edge_element(int64_t idx, int64_t head, int64_t body_end) { return idx < head ? idx : body_end + (idx - head); }

// ---- decode: PCM -> float ----------------------------------------------------------------------------------------------------------
// Q, b: the body's first PCM byte lies at 16 * k + 4 * Q + b
template <int FMT, int Q>
__global__ __launch_bounds__(kThreads) void aw_pcm_decode_kernel(const unsigned char *__restrict__ src, float *__restrict__ dst, int64_t n,
                                                                 int64_t head, int64_t n_body, uint32_t b) {
    constexpr int G = Group<FMT>::G, W = Group<FMT>::words, BYTES = FMT == awp::kS24 ? 3 : FMT == awp::kS16 ? 2 : 4;
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < n_body) {
        const int64_t e = head + t * G;
        const uint4 *w = reinterpret_cast<const uint4 *>(src + e * BYTES - (4 * Q + b));
        uint32_t d[4 * (W + 1)];
#pragma unroll
        for (int i = 0; i < W; ++i) { const uint4 v = w[i]; d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w; }
        if (Q != 0 || b != 0) { const uint4 v = w[W]; d[4 * W] = v.x; d[4 * W + 1] = v.y; d[4 * W + 2] = v.z; d[4 * W + 3] = v.w; }
        else { d[4 * W] = d[4 * W + 1] = d[4 * W + 2] = d[4 * W + 3] = 0u; }
        uint32_t s[4 * W];                                   // the group's PCM bytes as dwords
#pragma unroll
        for (int i = 0; i < 4 * W; ++i) s[i] = funnel(d[Q + i + 1], d[Q + i], b);
        float4 *o = reinterpret_cast<float4 *>(dst + e);
        if constexpr (FMT == awp::kS16) {
            o[0] = make_float4(awp::decode_s16((int16_t)(s[0] & 0xFFFFu)), awp::decode_s16((int16_t)(s[0] >> 16)),
                               awp::decode_s16((int16_t)(s[1] & 0xFFFFu)), awp::decode_s16((int16_t)(s[1] >> 16)));
            o[1] = make_float4(awp::decode_s16((int16_t)(s[2] & 0xFFFFu)), awp::decode_s16((int16_t)(s[2] >> 16)),
                               awp::decode_s16((int16_t)(s[3] & 0xFFFFu)), awp::decode_s16((int16_t)(s[3] >> 16)));
        } else if constexpr (FMT == awp::kS24) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {                    // three dwords -> four samples
                const uint32_t x = s[3 * q], y = s[3 * q + 1], z = s[3 * q + 2];
                const uint32_t u0 = x & 0xFFFFFFu, u1 = (x >> 24) | ((y & 0xFFFFu) << 8), u2 = (y >> 16) | ((z & 0xFFu) << 16), u3 = z >> 8;
                o[q] = make_float4(awp::decode_s24(u0 & 0xFF, (u0 >> 8) & 0xFF, u0 >> 16), awp::decode_s24(u1 & 0xFF, (u1 >> 8) & 0xFF, u1 >> 16),
                                   awp::decode_s24(u2 & 0xFF, (u2 >> 8) & 0xFF, u2 >> 16), awp::decode_s24(u3 & 0xFF, (u3 >> 8) & 0xFF, u3 >> 16));
            }
        } else {
            o[0] = make_float4(awp::decode_s32((int32_t)s[0]), awp::decode_s32((int32_t)s[1]), awp::decode_s32((int32_t)s[2]), awp::decode_s32((int32_t)s[3]));
        }
    } else {
        const int64_t idx = t - n_body, body_end = head + n_body * G;
        if (idx < n - n_body * G) {
            const int64_t e = edge_element(idx, head, body_end);
            dst[e] = awp::decode_at(FMT, src + e * BYTES);
        }
    }
}

// ---- encode: float -> PCM, clipped samples counted -----------------------------------------------------------------------------------
// The dither of a launch (aw_spatializer_set_dither): the launch covers whole streams of spf = 2 * frames samples, the first of them global
// stream g0, of a call that began at frame position pos.
struct DitherLaunch { uint64_t seed, g0, pos, spf; };

// Dither values of the G elements from element e on.  (stream, sample in stream) comes from one division per group, then steps in
// registers: r reaches spf where the group enters the next stream (several times in one group when spf < G).  spf is even, so r's
// parity is the ear and r = 0 starts a frame.  TPDF: one hash per element (counter K + 2p + ear = K + 2 pos + r).  TPDF_HP: one per
// frame, plus the hash of p - 1 at the group's start and at each stream it enters.
template <int MODE, int G>
__device__ __forceinline__ void group_dither(const DitherLaunch &dl, uint64_t e, float (&d)[G]) {
    uint64_t s = e / dl.spf, r = e - s * dl.spf;
    uint64_t key = awp::dither_key(dl.seed, dl.g0 + s);
    if constexpr (MODE == awp::kDitherTpdf) {
        uint64_t base = key + 2 * dl.pos;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            if (j > 0 && ++r == dl.spf) { r = 0; key = awp::dither_key(dl.seed, dl.g0 + ++s); base = key + 2 * dl.pos; }
            d[j] = awp::tpdf_from_hash(awp::splitmix64(base + r));
        }
    } else {
        uint64_t p = dl.pos + (r >> 1);
        uint64_t h = awp::splitmix64(key + p), h_prev = awp::splitmix64(key + p - 1);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            if (j > 0) {
                if (++r == dl.spf) {
                    r = 0; key = awp::dither_key(dl.seed, dl.g0 + ++s); p = dl.pos;
                    h = awp::splitmix64(key + p); h_prev = awp::splitmix64(key + p - 1);
                } else if (!(r & 1)) {
                    ++p; h_prev = h; h = awp::splitmix64(key + p);
                }
            }
            d[j] = awp::tpdf_hp_from_hashes(h, h_prev, (int)(r & 1));
        }
    }
}

template <int MODE> __device__ __forceinline__ int32_t enc_s16(float x, float d, unsigned *k) {
    if constexpr (MODE == awp::kDitherNone) return awp::encode_s16(x, k); else return awp::encode_s16_dithered(x, d, k);
}
template <int MODE> __device__ __forceinline__ int32_t enc_s24(float x, float d, unsigned *k) {
    if constexpr (MODE == awp::kDitherNone) return awp::encode_s24(x, k); else return awp::encode_s24_dithered(x, d, k);
}

// The gain of a launch (aw_spatializer_set_gain) and its per-stream clip counts: the launch covers whole streams of spf samples; gain,
// call_peak and rec point at the entry of its first stream.
struct GainLaunch {
    int mode;                         // awl::GainMode; kGainNone: every gain is 1 (a metered encode without gain)
    float ceiling;                    // kGainPeakCeiling
    const float *gain;                // kGainFixed: the streams' gains
    const uint32_t *call_peak;        // kGainPeakCeiling: bits of the streams' peaks over this call (aw_levels_kernel wrote them)
    awl::Record *rec;                 // NULL, or the streams' records: clipped samples are counted per stream too
    uint64_t spf;
};

__device__ __forceinline__ float stream_gain(const GainLaunch &gl, uint64_t s) {
    if (gl.mode == awl::kGainFixed) return gl.gain[s];
    if (gl.mode == awl::kGainPeakCeiling) return awl::auto_gain(awl::bits_float(gl.call_peak[s]), gl.ceiling);
    return 1.0f;
}

// Gains of the G elements from element e on: group_dither's stepping, one division per group.  s / r: stream and sample in stream of e;
// s_last: the stream of the group's last element.
template <int G>
__device__ __forceinline__ void group_gain(const GainLaunch &gl, uint64_t e, float (&g)[G], uint64_t &s, uint64_t &r, uint64_t &s_last) {
    s = e / gl.spf; r = e - s * gl.spf;
    uint64_t si = s, ri = r;
    float gs = stream_gain(gl, si);
#pragma unroll
    for (int j = 0; j < G; ++j) {
        if (j > 0 && ++ri == gl.spf) { ri = 0; gs = stream_gain(gl, ++si); }
        g[j] = gs;
    }
    s_last = si;
}

// The encode kernels' body.  Q: the body's first float lies at 16 * k + 4 * Q.  MODE kDitherNone is aw_pcm_encode_kernel as it always
// was (dl unused); the dithered forms (s16 / s24) add the group's dither values before the rounding.  GM (gain / meter, gl) multiplies
// every sample by its stream's gain first and counts the clipped samples per stream as well; without it gl is unused and the code is
// what it was.
template <int FMT, int Q, int MODE, bool GM = false>
__device__ __forceinline__ void encode_body(const float *__restrict__ src, unsigned char *__restrict__ dst, int64_t n, int64_t head,
                                            int64_t n_body, unsigned long long *clipped, const DitherLaunch &dl, const GainLaunch &gl = {}) {
    constexpr int G = Group<FMT>::G, W = Group<FMT>::words, BYTES = FMT == awp::kS24 ? 3 : FMT == awp::kS16 ? 2 : 4;
    constexpr int FW = G / 4;                                 // 16-B words of floats per group
    static_assert(MODE == awp::kDitherNone || FMT == awp::kS16 || FMT == awp::kS24, "only s16 and s24 are dithered");
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned c = 0;                                           // clipped samples of this lane
    unsigned cm = 0, lane_count = 0;                          // GM: clip flags of the group's elements; clipped samples this lane reports for
    uint32_t lane_stream = 0;                                 //     stream lane_stream at the end (a group inside one stream, or an edge element)
    if (t < n_body) {
        const int64_t e = head + t * G;
        const float4 *w = reinterpret_cast<const float4 *>(src + e - Q);
        float f[4 * (FW + 1)];
#pragma unroll
        for (int i = 0; i < FW; ++i) { const float4 v = w[i]; f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w; }
        if (Q != 0) { const float4 v = w[FW]; f[4 * FW] = v.x; f[4 * FW + 1] = v.y; f[4 * FW + 2] = v.z; f[4 * FW + 3] = v.w; }
        else { f[4 * FW] = f[4 * FW + 1] = f[4 * FW + 2] = f[4 * FW + 3] = 0.0f; }
        uint64_t gs0 = 0, gr0 = 0, gs1 = 0;
        if constexpr (GM) {
            float g[G];
            group_gain<G>(gl, (uint64_t)e, g, gs0, gr0, gs1);
#pragma unroll
            for (int j = 0; j < G; ++j) f[Q + j] = awl::apply_gain(f[Q + j], g[j]);
        }
        float d[G];
        if constexpr (MODE != awp::kDitherNone) group_dither<MODE, G>(dl, (uint64_t)e, d);
        else {
#pragma unroll
            for (int j = 0; j < G; ++j) d[j] = 0.0f;
        }
        uint32_t s[4 * W];
        if constexpr (FMT == awp::kS16) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned c0 = 0, c1 = 0;
                const uint32_t lo = (uint32_t)enc_s16<MODE>(f[Q + 2 * i], d[2 * i], &c0) & 0xFFFFu;
                const uint32_t hi = (uint32_t)enc_s16<MODE>(f[Q + 2 * i + 1], d[2 * i + 1], &c1) & 0xFFFFu;
                s[i] = lo | (hi << 16);
                c += c0 + c1;
                if constexpr (GM) cm |= (c0 << (2 * i)) | (c1 << (2 * i + 1));
            }
        } else if constexpr (FMT == awp::kS24) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {                    // four samples -> three dwords
                unsigned k[4] = {0, 0, 0, 0};
                uint32_t u[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) u[j] = (uint32_t)enc_s24<MODE>(f[Q + 4 * q + j], d[4 * q + j], &k[j]) & 0xFFFFFFu;
                s[3 * q] = u[0] | (u[1] << 24);
                s[3 * q + 1] = (u[1] >> 8) | (u[2] << 16);
                s[3 * q + 2] = (u[2] >> 16) | (u[3] << 8);
                c += k[0] + k[1] + k[2] + k[3];
                if constexpr (GM) cm |= (k[0] | (k[1] << 1) | (k[2] << 2) | (k[3] << 3)) << (4 * q);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned k = 0;
                s[i] = (uint32_t)awp::encode_s32(f[Q + i], &k);
                c += k;
                if constexpr (GM) cm |= k << i;
            }
        }
        uint4 *o = reinterpret_cast<uint4 *>(dst + e * BYTES);
#pragma unroll
        for (int i = 0; i < W; ++i) o[i] = make_uint4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
        if constexpr (GM) {
            if (gl.rec && cm) {
                if (gs0 == gs1) { lane_stream = (uint32_t)gs0; lane_count = (unsigned)__popc(cm); }
                else {                                        // the group crosses streams: one add per clipped element
#pragma unroll
                    for (int j = 0; j < G; ++j) {
                        if (j > 0 && ++gr0 == gl.spf) { gr0 = 0; ++gs0; }
                        if ((cm >> j) & 1u) atomicAdd(&gl.rec[gs0].clipped, 1ull);
                    }
                }
            }
        }
    } else {
        const int64_t idx = t - n_body, body_end = head + n_body * G;
        if (idx < n - n_body * G) {
            const int64_t e = edge_element(idx, head, body_end);
            if constexpr (GM) {
                const uint64_t s = (uint64_t)e / gl.spf, r = (uint64_t)e - s * gl.spf;
                unsigned k = 0;
                awl::encode_gained_at(FMT, MODE, src[e], stream_gain(gl, s), MODE == awp::kDitherNone ? 0 : awp::dither_key(dl.seed, dl.g0 + s),
                                      dl.pos + (r >> 1), (int)(r & 1), dst + e * BYTES, &k);
                c = k;
                if (gl.rec) { lane_stream = (uint32_t)s; lane_count = k; }
            } else if constexpr (MODE == awp::kDitherNone) {
                awp::encode_at(FMT, src[e], dst + e * BYTES, &c);
            } else {
                const uint64_t s = (uint64_t)e / dl.spf, r = (uint64_t)e - s * dl.spf;
                awp::encode_dithered_at(FMT, MODE, src[e], awp::dither_key(dl.seed, dl.g0 + s), dl.pos + (r >> 1), (int)(r & 1), dst + e * BYTES, &c);
            }
        }
    }
    if constexpr (GM) {
        // per stream: one ballot-summed add where every reporting lane of the wave lies in one stream, else one add per lane
        if (lane_count) {
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)lane_stream);
            const unsigned long long lanes = __ballot(1);
            if (__ballot(lane_stream != first) == 0) {
                unsigned long long sum = 0;
#pragma unroll
                for (int bit = 0; bit < 5; ++bit) sum += (unsigned long long)__popcll(__ballot((lane_count >> bit) & 1u)) << bit;
                if ((int)__lane_id() == __ffsll((long long)lanes) - 1) atomicAdd(&gl.rec[first].clipped, sum);
            } else {
                atomicAdd(&gl.rec[lane_stream].clipped, (unsigned long long)lane_count);
            }
        }
    }
    if (!clipped) return;
    // wave-level sum of the lanes' counts (at most G each, five bits): one ballot + popcount per bit, one global atomic per wave
    unsigned long long total = 0;
#pragma unroll
    for (int bit = 0; bit < 5; ++bit) total += (unsigned long long)__popcll(__ballot((c >> bit) & 1u)) << bit;
    const unsigned long long active = __ballot(1);
    if (total && (int)__lane_id() == __ffsll((long long)active) - 1) atomicAdd(clipped, total);
}

template <int FMT, int Q>
__global__ __launch_bounds__(kThreads) void aw_pcm_encode_kernel(const float *__restrict__ src, unsigned char *__restrict__ dst, int64_t n,
                                                                 int64_t head, int64_t n_body, unsigned long long *clipped) {
    encode_body<FMT, Q, awp::kDitherNone>(src, dst, n, head, n_body, clipped, DitherLaunch{});
}

template <int FMT, int Q, int MODE>
__global__ __launch_bounds__(kThreads) void aw_pcm_encode_dither_kernel(const float *__restrict__ src, unsigned char *__restrict__ dst, int64_t n,
                                                                        int64_t head, int64_t n_body, unsigned long long *clipped, DitherLaunch dl) {
    encode_body<FMT, Q, MODE>(src, dst, n, head, n_body, clipped, dl);
}

template <int FMT, int Q, int MODE>
__global__ __launch_bounds__(kThreads) void aw_pcm_encode_gain_kernel(const float *__restrict__ src, unsigned char *__restrict__ dst, int64_t n,
                                                                      int64_t head, int64_t n_body, unsigned long long *clipped, DitherLaunch dl,
                                                                      GainLaunch gl) {
    encode_body<FMT, Q, MODE, true>(src, dst, n, head, n_body, clipped, dl, gl);
}

// ---- levels: peak, energy and non-finite count of every stream of a chunk's float32 output ---------------------------------------------
// The launch covers whole streams of spf samples; rec (NULL: the meter is off and only the automatic gain wants the peaks) and call_peak
// point at the entry of its first stream.
struct LevelsLaunch { awl::Record *rec; uint32_t *call_peak; uint64_t spf; };

constexpr int kLevelsIter = 8;                                // 16-B words per lane: a wave covers 8 KB, one set of atomics where it lies in one stream

// adds one lane's (or one reduced wave's) sums of stream s; ears as given
__device__ __forceinline__ void levels_add(const LevelsLaunch &ll, uint64_t s, uint32_t pk0, uint32_t pk1, double en0, double en1, unsigned nf) {
    if (ll.rec) {
        awl::Record *r = ll.rec + s;
        if (pk0) atomicMax(&r->peak_bits[0], pk0);
        if (pk1) atomicMax(&r->peak_bits[1], pk1);
        if (en0 != 0.0) atomicAdd(&r->energy[0], en0);
        if (en1 != 0.0) atomicAdd(&r->energy[1], en1);
        if (nf) atomicAdd(&r->nonfinite, (unsigned long long)nf);
    }
    const uint32_t m = pk0 > pk1 ? pk0 : pk1;
    if (m) atomicMax(&ll.call_peak[s], m);
}

// the whole wave's sums of stream s (every lane calls; a[0] / a[1]: even / odd elements, swapped = the launch's body starts on a right ear)
__device__ __forceinline__ void levels_wave_add(const LevelsLaunch &ll, uint64_t s, bool swapped, uint32_t (&pk)[2], double (&en)[2], unsigned &nf) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t p0 = __shfl_xor(pk[0], m), p1 = __shfl_xor(pk[1], m);
        pk[0] = p0 > pk[0] ? p0 : pk[0];
        pk[1] = p1 > pk[1] ? p1 : pk[1];
        en[0] += __shfl_xor(en[0], m);
        en[1] += __shfl_xor(en[1], m);
        nf += __shfl_xor(nf, m);
    }
    if (__lane_id() == 0) {
        if (swapped) levels_add(ll, s, pk[1], pk[0], en[1], en[0], nf);
        else levels_add(ll, s, pk[0], pk[1], en[0], en[1], nf);
    }
    pk[0] = pk[1] = 0u; en[0] = en[1] = 0.0; nf = 0u;
}

// src: n floats, 4-byte aligned; the body of n_body 16-B words starts at element head; the at most 6 elements before and after it are
// one thread each in workgroup 0.  Every wave is launched whole and keeps its lanes together, so the shuffles see all 64 lanes.
__global__ __launch_bounds__(kThreads) void aw_levels_kernel(const float *__restrict__ src, int64_t n, int64_t head, int64_t n_body, LevelsLaunch ll) {
    const int lane = (int)(threadIdx.x & 63u);
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < n - 4 * n_body) {
        const uint64_t e = (uint64_t)edge_element((int64_t)threadIdx.x, head, head + 4 * n_body), s = e / ll.spf;
        uint32_t pk[2] = {0u, 0u}; double en[2] = {0.0, 0.0}; unsigned nf = 0;
        const int ear = (int)((e - s * ll.spf) & 1u);
        awl::contribute(src[e], pk[ear], en[ear], nf);
        levels_add(ll, s, pk[0], pk[1], en[0], en[1], nf);
    }
    const float4 *w = reinterpret_cast<const float4 *>(src + head);
    const bool swapped = (head & 1) != 0;
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int64_t w0 = wave * (64 * kLevelsIter);
    if (w0 >= n_body) return;
    // stream and sample in stream of the wave's first element: one division per wave, then steps of 256 samples
    uint64_t s0 = ((uint64_t)head + 4 * (uint64_t)w0) / ll.spf, r0 = (uint64_t)head + 4 * (uint64_t)w0 - s0 * ll.spf;
    uint32_t pk[2] = {0u, 0u}; double en[2] = {0.0, 0.0}; unsigned nf = 0;
    bool open = false;                                        // the registers hold sums of stream cur
    uint64_t cur = 0;
    for (int i = 0; i < kLevelsIter && w0 < n_body; ++i, w0 += 64) {
        const int64_t w_last = w0 + 63 < n_body ? w0 + 63 : n_body - 1;
        const bool one_stream = r0 + (uint64_t)(4 * (w_last - w0) + 3) < ll.spf;
        const int64_t wi = w0 + lane;
        const bool valid = wi < n_body;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (valid) v = w[wi];
        if (one_stream) {
            if (open && cur != s0) { levels_wave_add(ll, cur, swapped, pk, en, nf); open = false; }
            open = true; cur = s0;
            if (valid) {
                awl::contribute(v.x, pk[0], en[0], nf); awl::contribute(v.y, pk[1], en[1], nf);
                awl::contribute(v.z, pk[0], en[0], nf); awl::contribute(v.w, pk[1], en[1], nf);
            }
        } else {                                              // the wave's 256 samples cross streams: every lane adds its own
            if (open) { levels_wave_add(ll, cur, swapped, pk, en, nf); open = false; }
            if (valid) {
                const float y[4] = {v.x, v.y, v.z, v.w};
                const uint64_t e = (uint64_t)head + 4 * (uint64_t)wi;
                uint64_t s = e / ll.spf, r = e - s * ll.spf;
                uint32_t lp[2] = {0u, 0u}; double le[2] = {0.0, 0.0}; unsigned ln = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j > 0 && ++r == ll.spf) {
                        levels_add(ll, s, lp[0], lp[1], le[0], le[1], ln);
                        lp[0] = lp[1] = 0u; le[0] = le[1] = 0.0; ln = 0u; r = 0; ++s;
                    }
                    awl::contribute(y[j], lp[r & 1u], le[r & 1u], ln);
                }
                levels_add(ll, s, lp[0], lp[1], le[0], le[1], ln);
            }
        }
        r0 += 256;
        while (r0 >= ll.spf) { r0 -= ll.spf; ++s0; }
    }
    if (open) levels_wave_add(ll, cur, swapped, pk, en, nf);
}

// ---- scale: float32 output times its stream's gain, in place ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void aw_scale_kernel(float *__restrict__ buf, int64_t n, int64_t head, int64_t n_body, GainLaunch gl) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < n_body) {
        const int64_t e = head + 4 * t;
        float4 *w = reinterpret_cast<float4 *>(buf + e);
        const float4 v = *w;
        float g[4];
        uint64_t s, r, s_last;
        group_gain<4>(gl, (uint64_t)e, g, s, r, s_last);
        *w = make_float4(awl::apply_gain(v.x, g[0]), awl::apply_gain(v.y, g[1]), awl::apply_gain(v.z, g[2]), awl::apply_gain(v.w, g[3]));
    } else {
        const int64_t idx = t - n_body;
        if (idx < n - 4 * n_body) {
            const int64_t e = edge_element(idx, head, head + 4 * n_body);
            buf[e] = awl::apply_gain(buf[e], stream_gain(gl, (uint64_t)e / gl.spf));
        }
    }
}

// element count of the unaligned head: 16-B alignment of the address + head * bytes; n (all one-element threads) when there is none
int64_t head_to_align(uintptr_t addr, int bytes, int64_t n) {
    const unsigned m = (unsigned)(addr & 15u), need = (16u - m) & 15u;
    int64_t h;
    if (bytes == 3) h = (int64_t)((need * 11u) & 15u);      // 3 * 11 = 1 (mod 16)
    else if (need % (unsigned)bytes) h = n;
    else h = need / (unsigned)bytes;
    return h < n ? h : n;
}

template <int FMT>
hipError_t decode_fmt(const unsigned char *src, float *dst, int64_t n, hipStream_t stream) {
    constexpr int G = Group<FMT>::G, BYTES = FMT == awp::kS24 ? 3 : FMT == awp::kS16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(dst) & 3u) return hipErrorInvalidValue;
    const int64_t head = head_to_align(reinterpret_cast<uintptr_t>(dst), 4, n);
    const int64_t n_body = (n - head) / G;
    const int64_t threads = n_body + (n - n_body * G);      // body groups + head + tail elements
    const unsigned sh = (unsigned)((reinterpret_cast<uintptr_t>(src) + (uintptr_t)head * BYTES) & 15u);
    const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads));
    switch (sh >> 2) {
        case 0: hipLaunchKernelGGL((aw_pcm_decode_kernel<FMT, 0>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, sh & 3u); break;
        case 1: hipLaunchKernelGGL((aw_pcm_decode_kernel<FMT, 1>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, sh & 3u); break;
        case 2: hipLaunchKernelGGL((aw_pcm_decode_kernel<FMT, 2>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, sh & 3u); break;
        default: hipLaunchKernelGGL((aw_pcm_decode_kernel<FMT, 3>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, sh & 3u); break;
    }
    return hipGetLastError();
}

template <int FMT, int Q, int MODE>
void encode_launch(dim3 grid, hipStream_t stream, const float *src, unsigned char *dst, int64_t n, int64_t head, int64_t n_body,
                   unsigned long long *clipped, const DitherLaunch &dl, const GainLaunch *gl) {
    if (gl)
        hipLaunchKernelGGL((aw_pcm_encode_gain_kernel<FMT, Q, MODE>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, clipped, dl, *gl);
    else if constexpr (MODE == awp::kDitherNone)
        hipLaunchKernelGGL((aw_pcm_encode_kernel<FMT, Q>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, clipped);
    else
        hipLaunchKernelGGL((aw_pcm_encode_dither_kernel<FMT, Q, MODE>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, clipped, dl);
}

template <int FMT, int MODE>
hipError_t encode_fmt(const float *src, unsigned char *dst, int64_t n, unsigned long long *clipped, hipStream_t stream, const DitherLaunch &dl,
                      const GainLaunch *gl) {
    constexpr int G = Group<FMT>::G, BYTES = FMT == awp::kS24 ? 3 : FMT == awp::kS16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(src) & 3u) return hipErrorInvalidValue;
    const int64_t head = head_to_align(reinterpret_cast<uintptr_t>(dst), BYTES, n);
    const int64_t n_body = (n - head) / G;
    const int64_t threads = n_body + (n - n_body * G);
    const unsigned q = (unsigned)(((reinterpret_cast<uintptr_t>(src) + (uintptr_t)head * 4) & 15u) >> 2);
    const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads));
    switch (q) {
        case 0: encode_launch<FMT, 0, MODE>(grid, stream, src, dst, n, head, n_body, clipped, dl, gl); break;
        case 1: encode_launch<FMT, 1, MODE>(grid, stream, src, dst, n, head, n_body, clipped, dl, gl); break;
        case 2: encode_launch<FMT, 2, MODE>(grid, stream, src, dst, n, head, n_body, clipped, dl, gl); break;
        default: encode_launch<FMT, 3, MODE>(grid, stream, src, dst, n, head, n_body, clipped, dl, gl); break;
    }
    return hipGetLastError();
}

}  // namespace

namespace awk {

hipError_t launch_pcm_decode(int fmt, const void *src, float *dst, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const unsigned char *s = static_cast<const unsigned char *>(src);
    switch (fmt) {
        case awp::kS16: return decode_fmt<awp::kS16>(s, dst, n, stream);
        case awp::kS24: return decode_fmt<awp::kS24>(s, dst, n, stream);
        case awp::kS32: return decode_fmt<awp::kS32>(s, dst, n, stream);
        default: return hipErrorInvalidValue;
    }
}

static GainLaunch gain_launch(const PcmGain &gain, int64_t frames) {
    return GainLaunch{gain.mode, gain.ceiling, gain.gain, gain.call_peak, gain.rec, 2 * (uint64_t)frames};
}
static bool gain_ok(const PcmGain &gain) {
    if (gain.mode == awl::kGainFixed) return gain.gain != nullptr;
    if (gain.mode == awl::kGainPeakCeiling) return gain.call_peak != nullptr;
    return gain.mode == awl::kGainNone;
}

hipError_t launch_pcm_encode(int fmt, const float *src, void *dst, int64_t n, unsigned long long *clipped, const PcmDither *dither,
                             const PcmGain *gain, hipStream_t stream) {
    int mode = dither ? dither->mode : awp::kDitherNone;
    if (gain) {
        if (!dither || !gain_ok(*gain)) return hipErrorInvalidValue;
        if (fmt == awp::kS32) mode = awp::kDitherNone;
    } else if (dither && mode != awp::kDitherTpdf && mode != awp::kDitherTpdfHp) {
        return hipErrorInvalidValue;
    }
    if (dither && (dither->frames <= 0 || n < 0 || n % (2 * dither->frames))) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    unsigned char *d = static_cast<unsigned char *>(dst);
    const DitherLaunch dl = dither ? DitherLaunch{dither->seed, dither->first_stream, dither->position, 2 * (uint64_t)dither->frames} : DitherLaunch{};
    const GainLaunch gl = gain ? gain_launch(*gain, dither->frames) : GainLaunch{};
    const GainLaunch *g = gain ? &gl : nullptr;
    switch (fmt * 4 + mode) {
        case awp::kS16 * 4 + awp::kDitherNone: return encode_fmt<awp::kS16, awp::kDitherNone>(src, d, n, clipped, stream, dl, g);
        case awp::kS16 * 4 + awp::kDitherTpdf: return encode_fmt<awp::kS16, awp::kDitherTpdf>(src, d, n, clipped, stream, dl, g);
        case awp::kS16 * 4 + awp::kDitherTpdfHp: return encode_fmt<awp::kS16, awp::kDitherTpdfHp>(src, d, n, clipped, stream, dl, g);
        case awp::kS24 * 4 + awp::kDitherNone: return encode_fmt<awp::kS24, awp::kDitherNone>(src, d, n, clipped, stream, dl, g);
        case awp::kS24 * 4 + awp::kDitherTpdf: return encode_fmt<awp::kS24, awp::kDitherTpdf>(src, d, n, clipped, stream, dl, g);
        case awp::kS24 * 4 + awp::kDitherTpdfHp: return encode_fmt<awp::kS24, awp::kDitherTpdfHp>(src, d, n, clipped, stream, dl, g);
        case awp::kS32 * 4 + awp::kDitherNone: return encode_fmt<awp::kS32, awp::kDitherNone>(src, d, n, clipped, stream, dl, g);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_levels(const float *src, int64_t n, int64_t frames, awl::Record *rec, uint32_t *call_peak, hipStream_t stream) {
    if (!call_peak || frames <= 0 || n < 0 || n % (2 * frames) || (reinterpret_cast<uintptr_t>(src) & 3u)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const int64_t head = head_to_align(reinterpret_cast<uintptr_t>(src), 4, n), n_body = (n - head) / 4;
    const int64_t per_block = (int64_t)(kThreads / 64) * 64 * kLevelsIter;               // 16-B words per workgroup
    const dim3 grid((unsigned)std::max<int64_t>(1, (n_body + per_block - 1) / per_block));
    hipLaunchKernelGGL(aw_levels_kernel, grid, dim3(kThreads), 0, stream, src, n, head, n_body, LevelsLaunch{rec, call_peak, 2 * (uint64_t)frames});
    return hipGetLastError();
}

hipError_t launch_scale(float *buf, int64_t n, int64_t frames, const PcmGain &gain, hipStream_t stream) {
    if (!gain_ok(gain) || frames <= 0 || n < 0 || n % (2 * frames) || (reinterpret_cast<uintptr_t>(buf) & 3u)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const int64_t head = head_to_align(reinterpret_cast<uintptr_t>(buf), 4, n), n_body = (n - head) / 4;
    const int64_t threads = n_body + (n - 4 * n_body);
    const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(aw_scale_kernel, grid, dim3(kThreads), 0, stream, buf, n, head, n_body, gain_launch(gain, frames));
    return hipGetLastError();
}

}  // namespace awk
