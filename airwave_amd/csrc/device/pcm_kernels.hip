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
#include <hip/hip_runtime.h>

#include <cstdint>

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

// The encode kernels' body.  Q: the body's first float lies at 16 * k + 4 * Q.  MODE kDitherNone is aw_pcm_encode_kernel as it always
// was (dl unused); the dithered forms (s16 / s24) add the group's dither values before the rounding.
template <int FMT, int Q, int MODE>
__device__ __forceinline__ void encode_body(const float *__restrict__ src, unsigned char *__restrict__ dst, int64_t n, int64_t head,
                                            int64_t n_body, unsigned long long *clipped, const DitherLaunch &dl) {
    constexpr int G = Group<FMT>::G, W = Group<FMT>::words, BYTES = FMT == awp::kS24 ? 3 : FMT == awp::kS16 ? 2 : 4;
    constexpr int FW = G / 4;                                 // 16-B words of floats per group
    static_assert(MODE == awp::kDitherNone || FMT == awp::kS16 || FMT == awp::kS24, "only s16 and s24 are dithered");
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned c = 0;                                           // clipped samples of this lane
    if (t < n_body) {
        const int64_t e = head + t * G;
        const float4 *w = reinterpret_cast<const float4 *>(src + e - Q);
        float f[4 * (FW + 1)];
#pragma unroll
        for (int i = 0; i < FW; ++i) { const float4 v = w[i]; f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w; }
        if (Q != 0) { const float4 v = w[FW]; f[4 * FW] = v.x; f[4 * FW + 1] = v.y; f[4 * FW + 2] = v.z; f[4 * FW + 3] = v.w; }
        else { f[4 * FW] = f[4 * FW + 1] = f[4 * FW + 2] = f[4 * FW + 3] = 0.0f; }
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
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) { unsigned k = 0; s[i] = (uint32_t)awp::encode_s32(f[Q + i], &k); c += k; }
        }
        uint4 *o = reinterpret_cast<uint4 *>(dst + e * BYTES);
#pragma unroll
        for (int i = 0; i < W; ++i) o[i] = make_uint4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
    } else {
        const int64_t idx = t - n_body, body_end = head + n_body * G;
        if (idx < n - n_body * G) {
            const int64_t e = edge_element(idx, head, body_end);
            if constexpr (MODE == awp::kDitherNone) {
                awp::encode_at(FMT, src[e], dst + e * BYTES, &c);
            } else {
                const uint64_t s = (uint64_t)e / dl.spf, r = (uint64_t)e - s * dl.spf;
                awp::encode_dithered_at(FMT, MODE, src[e], awp::dither_key(dl.seed, dl.g0 + s), dl.pos + (r >> 1), (int)(r & 1), dst + e * BYTES, &c);
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
                   unsigned long long *clipped, const DitherLaunch &dl) {
    if constexpr (MODE == awp::kDitherNone)
        hipLaunchKernelGGL((aw_pcm_encode_kernel<FMT, Q>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, clipped);
    else
        hipLaunchKernelGGL((aw_pcm_encode_dither_kernel<FMT, Q, MODE>), grid, dim3(kThreads), 0, stream, src, dst, n, head, n_body, clipped, dl);
}

template <int FMT, int MODE = awp::kDitherNone>
hipError_t encode_fmt(const float *src, unsigned char *dst, int64_t n, unsigned long long *clipped, hipStream_t stream, const DitherLaunch &dl = {}) {
    constexpr int G = Group<FMT>::G, BYTES = FMT == awp::kS24 ? 3 : FMT == awp::kS16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(src) & 3u) return hipErrorInvalidValue;
    const int64_t head = head_to_align(reinterpret_cast<uintptr_t>(dst), BYTES, n);
    const int64_t n_body = (n - head) / G;
    const int64_t threads = n_body + (n - n_body * G);
    const unsigned q = (unsigned)(((reinterpret_cast<uintptr_t>(src) + (uintptr_t)head * 4) & 15u) >> 2);
    const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads));
    switch (q) {
        case 0: encode_launch<FMT, 0, MODE>(grid, stream, src, dst, n, head, n_body, clipped, dl); break;
        case 1: encode_launch<FMT, 1, MODE>(grid, stream, src, dst, n, head, n_body, clipped, dl); break;
        case 2: encode_launch<FMT, 2, MODE>(grid, stream, src, dst, n, head, n_body, clipped, dl); break;
        default: encode_launch<FMT, 3, MODE>(grid, stream, src, dst, n, head, n_body, clipped, dl); break;
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

hipError_t launch_pcm_encode(int fmt, const float *src, void *dst, int64_t n, unsigned long long *clipped, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    unsigned char *d = static_cast<unsigned char *>(dst);
    switch (fmt) {
        case awp::kS16: return encode_fmt<awp::kS16>(src, d, n, clipped, stream);
        case awp::kS24: return encode_fmt<awp::kS24>(src, d, n, clipped, stream);
        case awp::kS32: return encode_fmt<awp::kS32>(src, d, n, clipped, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_pcm_encode_dithered(int fmt, const PcmDither &dither, const float *src, void *dst, int64_t n, unsigned long long *clipped,
                                      hipStream_t stream) {
    if (dither.mode != awp::kDitherTpdf && dither.mode != awp::kDitherTpdfHp) return hipErrorInvalidValue;
    if (dither.frames <= 0 || n < 0 || n % (2 * dither.frames)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    unsigned char *d = static_cast<unsigned char *>(dst);
    const DitherLaunch dl{dither.seed, dither.first_stream, dither.position, 2 * (uint64_t)dither.frames};
    const int key = fmt * 4 + dither.mode;
    switch (key) {
        case awp::kS16 * 4 + awp::kDitherTpdf: return encode_fmt<awp::kS16, awp::kDitherTpdf>(src, d, n, clipped, stream, dl);
        case awp::kS16 * 4 + awp::kDitherTpdfHp: return encode_fmt<awp::kS16, awp::kDitherTpdfHp>(src, d, n, clipped, stream, dl);
        case awp::kS24 * 4 + awp::kDitherTpdf: return encode_fmt<awp::kS24, awp::kDitherTpdf>(src, d, n, clipped, stream, dl);
        case awp::kS24 * 4 + awp::kDitherTpdfHp: return encode_fmt<awp::kS24, awp::kDitherTpdfHp>(src, d, n, clipped, stream, dl);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace awk
