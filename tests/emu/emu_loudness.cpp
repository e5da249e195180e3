// emu_loudness.cpp — TEST-ONLY: the loudness kernels (airwave_amd/csrc/device/loudness_scan.hpp, the code hipcc compiles) under the CPU
// thread emulation of emu_ctx.hpp: one emulated workgroup of kEqThreads per stream for the chunk-aligned part, loudness_sequential for the
// tail — the split launch_loudness makes.  Tables: the library's own builder (host/eq.cpp) over the coefficients of loudness.hpp.
#include "emu_ctx.hpp"

#include "../../airwave_amd/csrc/device/loudness_scan.hpp"

extern "C" {

// in: [stream][frames][2]; z: [stream][2][4], hops: [stream][cap_hops], nonfinite: [stream] — carried in and out.  Returns frames per hop,
// or 0 for a rate that has none.
long long emu_loudness(const float *in, int n_streams, long long frames, double rate, long long frame0, double *z, double *hops,
                       long long cap_hops, unsigned long long *nonfinite) {
    using namespace awk;
    const long long hop = awlo::hop_frames(rate);
    if (hop <= 0) return 0;
    double kw[awlo::kFilters][5];
    awlo::k_weighting(rate, kw);
    std::vector<double> tab((size_t)kLdFilters * kEqTabDoubles), plane((size_t)kLdFilters * awh::kEqSectionPlaneDoubles);
    for (int k = 0; k < kLdFilters; ++k)
        awh::eq_section_tables(awh::Biquad{kw[k][0], kw[k][1], kw[k][2], kw[k][3], kw[k][4]}, &tab[(size_t)k * kEqTabDoubles],
                               &plane[(size_t)k * awh::kEqSectionPlaneDoubles]);
    LoudnessParams p{};
    p.in = in; p.z = z; p.hops = hops; p.nonfinite = nonfinite;
    p.tab = tab.data(); p.plane = plane.data();
    p.stride_frames = frames; p.frame0 = frame0; p.hop = hop; p.cap_hops = cap_hops;
    const long long body = hop >= kEqChunk ? frames - frames % kEqChunk : 0;
    if (body > 0) {
        p.frames = body;
        EmuShared sh(kEqThreads, (size_t)(kLdLdsBytes + sizeof(cf) - 1) / sizeof(cf));
        for (int s = 0; s < n_streams; ++s)
            emu_workgroup(kEqThreads, [&](int t) { EmuCtx ctx{t, &sh}; loudness_stream(ctx, p, s); });
    }
    if (frames > body) {
        p.in = in + body * 2; p.frames = frames - body; p.frame0 = frame0 + body;
        for (int s = 0; s < n_streams; ++s) loudness_sequential(p, s);
    }
    return hop;
}

// The two sections' host-built tables: coef [2][5], tab [2][kEqTabDoubles], plane [2][64][4]; returns kEqTabDoubles.
int emu_loudness_tables(double rate, double *coef, double *tab, double *plane) {
    double kw[awlo::kFilters][5];
    awlo::k_weighting(rate, kw);
    for (int k = 0; k < awlo::kFilters; ++k) {
        for (int i = 0; i < 5; ++i) coef[k * 5 + i] = kw[k][i];
        awh::eq_section_tables(awh::Biquad{kw[k][0], kw[k][1], kw[k][2], kw[k][3], kw[k][4]}, tab + (size_t)k * awk::kEqTabDoubles,
                               plane + (size_t)k * awh::kEqSectionPlaneDoubles);
    }
    return awk::kEqTabDoubles;
}

}
