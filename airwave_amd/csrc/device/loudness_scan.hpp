// loudness_scan.hpp — the K-weighted hop energies of batches of stereo streams (rules: loudness.hpp), device code shared between hipcc
// (loudness_kernels.hip over scan_gpu_ctx.hpp's context, the EQ kernels' too) and the CPU thread-emulation harness
// (tests/emu/emu_loudness.cpp over emu_ctx.hpp's).
//
// The K-weighting is a cascade of two Float64 biquads, a time recurrence over the whole stream, so the time axis is parallelised the
// way the parametric EQ's is, with the machinery of eq_cascade.hpp as it stands: one workgroup per stream walks the call in spans of
// kEqThreads x kEqChunk frames; every thread runs both filters over its chunk of both ears from a zero state, the chunk recurrence is
// scanned inside the wave with DPP moves and chained over the waves through LDS, and the zero-input response of the entering state is
// added (steps (1) - (3) of eq_cascade.hpp; the tables are the EQ's, built by the same double-double builder for the two fixed sections).
// What differs is the end of a span: nothing is stored as float32.  Each thread squares and sums its chunk of both ears into the one or
// two hops the chunk lies in (a hop is rate / 10 frames: at 44.1 kHz a 32-frame chunk can straddle a hop edge, at 48 and 96 kHz never),
// the workgroup reduces per hop in a fixed order (in-wave DPP sum, then the wave totals through LDS in wave order), and one thread adds
// the span's sum to E[stream][hop] with a plain read-modify-write: one workgroup owns a stream, so there are no atomics and a given
// split of the timeline into calls gives the same bits every time.
//
// Carried across calls per stream: the filter state (8 doubles, [filter][lz1 lz2 rz1 rz2]); the frame count since the last reset, which
// fixes the hop index, is the same for every stream of a handle and comes with the launch (frame0).  Hops at or past `cap_hops` are not
// recorded.  The state is not flushed to zero as the EQ's is: a decaying tail stays what the recurrence makes of it.
#pragma once
#include "eq_cascade.hpp"
#include "loudness.hpp"

namespace awk {

constexpr int kLdFilters = awlo::kFilters;
// LDS map (bytes): the EQ's stage and wave totals, a carry of two filters, and the per-hop wave sums of one span
constexpr int kLdMaxSpanHops = kEqThreads + 1;                          // a hop is at least kEqChunk frames (launch_loudness): a span touches at most this many
constexpr int kLdCarryBytes = 2 * kLdFilters * 4 * 8;                   // ping-pong [filter][4]
constexpr int kLdPartBytes = (kLdMaxSpanHops + 1) * (kEqThreads / 64) * 8;   // [hop of the span | the non-finite count][wave]
constexpr int kLdLdsBytes = eq_stage_bytes(2) + kEqTotalsBytes + kLdCarryBytes + kLdPartBytes;   // 78,240: two workgroups per CU

struct LoudnessParams {
    const float *in;          // [stream][stride_frames][2] interleaved L,R: the float32 output before the gain
    double *z;                // [stream][kLdFilters][4]  lz1 lz2 rz1 rz2
    double *hops;             // [stream][cap_hops]  E
    unsigned long long *nonfinite;   // [stream]
    const double *tab;        // [kLdFilters][kEqTabDoubles]   (EqTables::tab)
    const double *plane;      // [kLdFilters][64][4]           (EqTables::plane)
    long long frames;         // frames this launch measures per stream
    long long stride_frames;  // distance between streams, in frames
    long long frame0;         // frames measured before this launch since the last reset
    long long hop;            // frames per hop
    long long cap_hops;       // hops recorded per stream
};

// Inclusive sum over the wave in a fixed order: lane 63 ends with the total (rows of 16 lanes, then the row totals).
template <class Ctx> AW_HD double ld_wave_sum(Ctx &ctx, double v) {
    v += ctx.template row_shr<1>(v);
    v += ctx.template row_shr<2>(v);
    v += ctx.template row_shr<4>(v);
    v += ctx.template row_shr<8>(v);
    v += ctx.row_bcast15(v);
    v += ctx.row_bcast31(v);
    return v;
}

// One workgroup walks one stream's timeline, both ears in every thread.  p.frames must be a multiple of kEqChunk and p.hop >= kEqChunk.
template <class Ctx> AW_HD void loudness_stream(Ctx &ctx, const LoudnessParams &p, long long stream) {
    constexpr int E = 2, S = 4, K = kLdFilters;
    typedef EqRaw<2> Raw;
    const int tid = ctx.tid();
    const int lane = tid & 63;
    char *lds = reinterpret_cast<char *>(ctx.lds());
    float *stage = reinterpret_cast<float *>(lds);                         // [chunk][kEqChunk * 2 + 4] floats
    double *totals = reinterpret_cast<double *>(lds + eq_stage_bytes(2));
    double *carry = reinterpret_cast<double *>(lds + eq_stage_bytes(2) + kEqTotalsBytes);
    double *part = reinterpret_cast<double *>(lds + eq_stage_bytes(2) + kEqTotalsBytes + kLdCarryBytes);
    constexpr int kStride = kEqChunk * E + 4, kWaves = kEqThreads / 64;
    const int wave = ctx.wave();
    double *zs = p.z + stream * (long long)K * 4;
    const float *in = p.in + stream * p.stride_frames * 2;
    double *hops = p.hops + stream * p.cap_hops;

    for (int i = tid; i < K * S; i += kEqThreads) carry[i] = zs[i];
    int par = 0;
    unsigned nonfinite = 0;

    constexpr int kPer = Raw::kFrames, kLoads = kEqChunk / kPer;
    EqF4 raw[kLoads];
    for (long long base = 0; base < p.frames; base += kEqSpan) {
        const long long rem = p.frames - base;
        const int nfr = rem < kEqSpan ? (int)rem : kEqSpan;
        const int nchunks = nfr / kEqChunk;
        // the span's frames: kEqChunk / 2 independent coalesced loads per lane, all in flight at once; the last, partial span is guarded
        if (nfr == kEqSpan) {
#pragma unroll
            for (int j = 0; j < kLoads; ++j) raw[j] = Raw::load(in + (base + (long long)(j * kEqThreads + tid) * kPer) * 2);
        } else {
#pragma unroll
            for (int j = 0; j < kLoads; ++j) {
                const int f = (j * kEqThreads + tid) * kPer;
                raw[j] = Raw::zero();
                if (f + kPer <= nfr) raw[j] = Raw::load(in + (base + f) * 2);       // (nfr is even: no half pair)
            }
        }
        ctx.barrier();   // the part reads of the previous span and the carry writes are complete
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const int f = (j * kEqThreads + tid) * kPer;
            Raw::lds_store(stage + (f / kEqChunk) * kStride + (f % kEqChunk) * E, raw[j]);
        }
        ctx.barrier();
        double x[E][kEqChunk];
#pragma unroll
        for (int j = 0; j < kEqChunk; ++j)
#pragma unroll
            for (int e = 0; e < E; ++e) x[e][j] = awlo::filter_input(stage[tid * kStride + j * E + e], nonfinite);

        for (int k = 0; k < K; ++k) {
            const double *c = p.tab + (long long)k * kEqTabDoubles;        // uniform: scalar loads
            double ck[5], pp[20];
#pragma unroll
            for (int i = 0; i < 5; ++i) ck[i] = c[i];
#pragma unroll
            for (int i = 0; i < 16; ++i) pp[i] = c[5 + kEqChunk * 2 + i];
#pragma unroll
            for (int i = 0; i < 4; ++i) pp[16 + i] = c[5 + kEqChunk * 2 + 6 * 4 + i];
            const double b0 = ck[0], b1 = ck[1], b2 = ck[2], na1 = -ck[3], na2 = -ck[4];
            const double *dk = p.plane + (long long)k * 64 * 4;
            double d16[4], d32[4], d64[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { d16[i] = dk[(lane & 15) * 4 + i]; d32[i] = dk[(lane & 31) * 4 + i]; d64[i] = dk[lane * 4 + i]; }
            // (1) zero-state response of this chunk, in place
            double st[S];
#pragma unroll
            for (int i = 0; i < S; ++i) st[i] = 0.0;
#pragma unroll
            for (int j = 0; j < kEqChunk; ++j)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const double t1 = __builtin_fma(b1, x[e][j], st[2 * e + 1]), t2 = b2 * x[e][j];
                    ctx.fma_in_place(x[e][j], b0, st[2 * e], t1, t2);
                    st[2 * e] = __builtin_fma(na1, x[e][j], t1);
                    st[2 * e + 1] = __builtin_fma(na2, x[e][j], t2);
                }
            // (2a) inclusive scan of s[c+1] = P s[c] + e[c] inside the wave
            double q[S];
#pragma unroll
            for (int i = 0; i < S; ++i) q[i] = ctx.template row_shr<1>(st[i]);
            eq_apply<E>(pp + 0, q, st);
#pragma unroll
            for (int i = 0; i < S; ++i) q[i] = ctx.template row_shr<2>(st[i]);
            eq_apply<E>(pp + 4, q, st);
#pragma unroll
            for (int i = 0; i < S; ++i) q[i] = ctx.template row_shr<4>(st[i]);
            eq_apply<E>(pp + 8, q, st);
#pragma unroll
            for (int i = 0; i < S; ++i) q[i] = ctx.template row_shr<8>(st[i]);
            eq_apply<E>(pp + 12, q, st);
#pragma unroll
            for (int i = 0; i < S; ++i) q[i] = ctx.row_bcast15(st[i]);
            eq_apply<E>(d16, q, st);
#pragma unroll
            for (int i = 0; i < S; ++i) q[i] = ctx.row_bcast31(st[i]);
            eq_apply<E>(d32, q, st);
            // wave totals -> LDS (ping-pong by filter parity)
            double *tot = totals + (k & 1) * kWaves * 4;
            if (lane == 63) {
#pragma unroll
                for (int i = 0; i < S; ++i) tot[wave * 4 + i] = st[i];
            }
            ctx.barrier();
            // (2b) state entering this wave: W_0 = carried state, W_w = P^64 W_{w-1} + T_{w-1}
            const double *cin = carry + par * K * 4 + k * S;
            double w[S];
#pragma unroll
            for (int i = 0; i < S; ++i) w[i] = cin[i];
            double tw[kWaves - 1][S];
#pragma unroll
            for (int i = 0; i < kWaves - 1; ++i)
#pragma unroll
                for (int m = 0; m < S; ++m) tw[i][m] = tot[i * 4 + m];
#pragma unroll
            for (int i = 0; i < kWaves - 1; ++i)
                if (i < wave) {                    // wave-uniform
                    eq_apply<E>(pp + 16, w, tw[i]);
#pragma unroll
                    for (int m = 0; m < S; ++m) w[m] = tw[i][m];
                }
            // (2c) state leaving this chunk; the state entering it is the one leaving the lane below (lane 0: W_w itself)
            eq_apply<E>(d64, w, st);
            if (tid == nchunks - 1) {   // state after the last active chunk -> next span / next call
                double *cout = carry + (par ^ 1) * K * 4 + k * S;
#pragma unroll
                for (int i = 0; i < S; ++i) cout[i] = st[i];
            }
            double sin_[S];
#pragma unroll
            for (int i = 0; i < S; ++i) sin_[i] = ctx.wave_shr1(st[i], w[i]);
            // (3) zero-input response of the entering state
            const double *g = c + 5;
#pragma unroll
            for (int j = 0; j < kEqChunk; ++j) {
                const double g0 = g[2 * j], g1 = g[2 * j + 1];
#pragma unroll
                for (int e = 0; e < E; ++e) x[e][j] = __builtin_fma(g1, sin_[2 * e + 1], __builtin_fma(g0, sin_[2 * e], x[e][j]));
            }
        }
        par ^= 1;

        // x is the K-weighted signal.  This chunk's frames lie in hop h0 (the first n0 of them) and, past a hop edge, in h0 + 1.
        const long long g0 = p.frame0 + base + (long long)tid * kEqChunk;
        const long long hfirst = (p.frame0 + base) / p.hop, hlast = (p.frame0 + base + nfr - 1) / p.hop;
        const long long h0 = g0 / p.hop;
        const long long to_edge = (h0 + 1) * p.hop - g0;
        const int n0 = to_edge < kEqChunk ? (int)to_edge : kEqChunk;
        double ea = 0.0, eb = 0.0;
#pragma unroll
        for (int j = 0; j < kEqChunk; ++j) {
            const double sq = __builtin_fma(x[1][j], x[1][j], x[0][j] * x[0][j]);
            ea += j < n0 ? sq : 0.0;
            eb += j < n0 ? 0.0 : sq;
        }
        if (tid >= nchunks) { ea = 0.0; eb = 0.0; }      // (past the call's end: zero input, but the zero-input response is not zero)
        const int slot = (int)(h0 - hfirst), nh = (int)(hlast - hfirst) + 1;
        for (int k = 0; k < nh; ++k) {                   // workgroup-uniform trip count
            const double v = ld_wave_sum(ctx, (slot == k ? ea : 0.0) + (slot + 1 == k ? eb : 0.0));
            if (lane == 63) part[k * kWaves + wave] = v;
        }
        ctx.barrier();
        for (int k = tid; k < nh; k += kEqThreads) {
            const long long h = hfirst + k;
            if (h < p.cap_hops) {
                double sum = part[k * kWaves];
#pragma unroll
                for (int i = 1; i < kWaves; ++i) sum += part[k * kWaves + i];
                hops[h] += sum;
            }
        }
    }
    // the call's non-finite samples, through the same reduction (exact: counts below 2^53)
    const double nf = ld_wave_sum(ctx, (double)nonfinite);
    ctx.barrier();       // the part reads of the last span
    if (lane == 63) part[wave] = nf;
    ctx.barrier();
    if (tid == 0) {
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) sum += part[i];
        if (sum > 0.0) p.nonfinite[stream] += (unsigned long long)sum;
    }
    for (int i = tid; i < K * S; i += kEqThreads) zs[i] = carry[par * K * 4 + i];
}

// The recurrence itself, one thread per stream: calls shorter than a chunk, the tail of a call, and rates whose hop is shorter than a
// chunk.  eq_sequential's arithmetic (non-contracted Float64) without its float32 store and its flush.
AW_HD void loudness_sequential(const LoudnessParams &p, long long stream) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double *zs = p.z + stream * (long long)kLdFilters * 4;
    const float *in = p.in + stream * p.stride_frames * 2;
    double *hops = p.hops + stream * p.cap_hops;
    double c[kLdFilters][5], z[kLdFilters][4];
    for (int k = 0; k < kLdFilters; ++k) {
        for (int i = 0; i < 5; ++i) c[k][i] = p.tab[(long long)k * kEqTabDoubles + i];
        for (int i = 0; i < 4; ++i) z[k][i] = zs[k * 4 + i];
    }
    unsigned nonfinite = 0;
    long long h = p.frame0 / p.hop, left = (h + 1) * p.hop - p.frame0;     // frames of hop h still to come
    double acc = 0.0;
    for (long long f = 0; f < p.frames; ++f) {
        double sq = 0.0;
        for (int e = 0; e < 2; ++e) {
            double v = awlo::filter_input(in[2 * f + e], nonfinite);
            for (int k = 0; k < kLdFilters; ++k) {
                const double lo = c[k][0] * v + z[k][2 * e];
                const double z1 = c[k][1] * v - c[k][3] * lo + z[k][2 * e + 1];
                const double z2 = c[k][2] * v - c[k][4] * lo;
                z[k][2 * e] = z1;
                z[k][2 * e + 1] = z2;
                v = lo;
            }
            sq += v * v;
        }
        acc += sq;
        if (--left == 0 || f + 1 == p.frames) {
            if (h < p.cap_hops) hops[h] += acc;
            acc = 0.0;
            if (left == 0) { h += 1; left = p.hop; }
        }
    }
    for (int k = 0; k < kLdFilters; ++k)
        for (int i = 0; i < 4; ++i) zs[k * 4 + i] = z[k][i];
    if (nonfinite) p.nonfinite[stream] += nonfinite;
}

}  // namespace awk
