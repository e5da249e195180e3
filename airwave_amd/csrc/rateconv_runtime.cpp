// rateconv_runtime.cpp — C ABI of the batch sample-rate converter (aw_rateconv_*, include/airwave_hip.h): the rules are
// device/rateconv.hpp, the kernel device/rateconv_tile.hpp.  Audio-rate conversion has no counterpart in the reference, whose two-point
// linear interpolation (Resampler.swift:31-68, aw_resample) is for an HRIR at activation and images and aliases at about -30 dB on audio.
// The aw_pcm_rateconv_* entries run the same handle through the kernel's PCM form (integer PCM in and out, dither, gain, records), and
// the aw_tp_rateconv_* entries add the true peak of the converted output: the PCM form's measuring forms.
// One owner thread per handle, like every other handle of this library; the handle goes as aw_eq does: device current, stream idle, then
// its members.
#include <cmath>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "device/rateconv_kernels.hpp"
#include "runtime.hpp"

using awr::fail;

namespace {

aw_status plan_checked(double in_rate, double out_rate, awrc::Plan &p) {
    switch (awrc::plan(in_rate, out_rate, p)) {
        case awrc::kPlanNotIntegral: return fail(AW_ERR_INVALID_ARGUMENT, "sample rates must be positive integers in Hz");
        case awrc::kPlanEqual: return fail(AW_ERR_INVALID_ARGUMENT, "the rates are equal: there is nothing to convert");
        case awrc::kPlanTooLarge:
            return fail(AW_ERR_INVALID_ARGUMENT, "the reduced ratio out / in has a term above " + std::to_string(awrc::kMaxTerm) + ": not approximated");
        default: return AW_OK;
    }
}

}  // namespace

struct aw_rateconv {
    aw_context *ctx = nullptr;
    int n_streams = 0, n_channels = 0, tile = 0;
    awrc::Plan plan;
    awrc::Counts counts;                       // the same for every stream
    awr::Buf<float> d_c;                       // [L][row_stride]
    awr::Buf<float> d_hist[2];                 // [streams][taps - 1][channels]: a call reads slot cur and writes the other
    awr::Buf<long long> d_counts;              // [streams][2], written by each call's last tiles
    int cur = 0;
    // the aw_pcm_rateconv_* entries' settings; aw_rateconv_process / _flush / _reset ignore them
    int dither = AW_DITHER_NONE;
    uint64_t dither_seed = 0, first_stream = 0;
    int gain_mode = AW_GAIN_NONE;
    int metering = 0;
    awr::Buf<float> d_gains;                   // [streams], made by set_gain(AW_GAIN_FIXED)
    awr::Buf<awk::RateconvLevels> d_levels;    // [streams], made by set_metering(on); aw_rateconv_levels is its layout
    // the aw_tp_rateconv_* entries' state, one allocation made by aw_tp_rateconv_set(on): the records [streams] (aw_rateconv_true_peak is
    // their layout), then two history slots [streams][11][channels]; a call that produces frames reads slot tp_cur and writes the other
    int true_peak = 0, tp_tile = 0, tp_cur = 0;
    awr::Buf<float> d_tp;
    float tp_c[awtp::kCoefficients];
    awk::RateconvTruePeak *tp_records() const { return reinterpret_cast<awk::RateconvTruePeak *>(d_tp.get()); }
    size_t tp_hist_floats() const { return (size_t)n_streams * awtp::kHistory * n_channels; }
    float *tp_hist(int slot) const { return d_tp.get() + (size_t)n_streams * (sizeof(awk::RateconvTruePeak) / sizeof(float)) + (size_t)slot * tp_hist_floats(); }
};

static_assert(sizeof(aw_rateconv_levels) == 32 && sizeof(awk::RateconvLevels) == 32, "aw_rateconv_levels is the kernel's record");
static_assert(sizeof(aw_rateconv_true_peak) == 16 && sizeof(awk::RateconvTruePeak) == 16, "aw_rateconv_true_peak is the kernel's record");
static_assert(AW_SAMPLE_F32 == awp::kF32 && AW_SAMPLE_S16 == awp::kS16 && AW_SAMPLE_S24 == awp::kS24 && AW_SAMPLE_S32 == awp::kS32, "formats");
static_assert(AW_DITHER_NONE == awp::kDitherNone && AW_DITHER_TPDF == awp::kDitherTpdf && AW_DITHER_TPDF_HP == awp::kDitherTpdfHp, "dither modes");

namespace {

aw_status reset_state(aw_rateconv *rc) {
    AW_HIP_TRY(hipMemsetAsync(rc->d_hist[rc->cur].get(), 0, rc->d_hist[rc->cur].bytes(), rc->ctx->stream));
    AW_HIP_TRY(hipMemsetAsync(rc->d_counts.get(), 0, rc->d_counts.bytes(), rc->ctx->stream));
    if (rc->d_tp) AW_HIP_TRY(hipMemsetAsync(rc->tp_hist(rc->tp_cur), 0, rc->tp_hist_floats() * sizeof(float), rc->ctx->stream));      // v = 0 before the next frame
    rc->counts = awrc::Counts{};
    return AW_OK;
}

// What an aw_pcm_rateconv_* call adds to the float32 form.
struct PcmCall {
    aw_sample_format in_format, out_format;
    uint64_t *clipped;
    bool measure_only;                         // aw_tp_rateconv_measure / _measure_flush: no output buffer, no capacity
};

// in NULL: in_frames frames of zeros; pcm NULL: the float32 form
aw_status run(aw_rateconv *rc, const void *in, long long in_frames, void *out, long long capacity, int64_t *out_frames, const PcmCall *pcm = nullptr) {
    const awrc::Plan &pl = rc->plan;
    const long long n_out = awrc::outputs_after(rc->counts.consumed + in_frames, pl.L, pl.M, pl.latency) - rc->counts.produced;
    const bool measure_only = pcm && pcm->measure_only;
    if (!measure_only && capacity < n_out)
        return fail(AW_ERR_INVALID_ARGUMENT, "out_capacity_frames " + std::to_string(capacity) + " is below the " + std::to_string(n_out) +
                                                 " frames this call produces (aw_rateconv_output_frames)");
    if (!measure_only && n_out > 0 && !out) return fail(AW_ERR_INVALID_ARGUMENT, "out_device is NULL");
    if (out_frames) *out_frames = n_out;
    if (in_frames == 0) return AW_OK;
    AW_HIP_TRY(hipSetDevice(rc->ctx->device));
    awk::RateconvParams p{};
    p.in = static_cast<const float *>(in); p.in_frames = in_frames; p.out = static_cast<float *>(out); p.out_frames = n_out;
    p.n_streams = rc->n_streams; p.channels = rc->n_channels;
    p.L = pl.L; p.M = pl.M; p.taps = pl.taps; p.latency = pl.latency;
    p.tile = rc->tile; p.row_stride = awk::rc_row_stride(pl.taps); p.c = rc->d_c.get();
    p.hist_in = rc->d_hist[rc->cur].get(); p.hist_out = rc->d_hist[rc->cur ^ 1].get();
    p.consumed = rc->counts.consumed; p.produced = rc->counts.produced; p.counts = rc->d_counts.get();
    if (pcm) {
        p.in_format = pcm->in_format; p.out_format = pcm->out_format;
        p.dither = rc->dither; p.dither_seed = rc->dither_seed; p.first_stream = rc->first_stream;
        p.gains = rc->gain_mode == AW_GAIN_FIXED ? rc->d_gains.get() : nullptr;
        p.levels = rc->metering ? rc->d_levels.get() : nullptr;
        p.clipped = reinterpret_cast<unsigned long long *>(pcm->clipped);
        if (rc->true_peak) {
            awk::RateconvTp tp{};
            tp.hist_in = rc->tp_hist(rc->tp_cur); tp.hist_out = rc->tp_hist(rc->tp_cur ^ 1);
            tp.records = rc->tp_records(); tp.tile = rc->tp_tile;
            for (int i = 0; i < awtp::kCoefficients; ++i) tp.c[i] = rc->tp_c[i];
            AW_HIP_TRY(measure_only ? awk::launch_rateconv_tp_measure(p, tp, rc->ctx->stream) : awk::launch_rateconv_pcm_tp(p, tp, rc->ctx->stream));
            if (n_out > 0) rc->tp_cur ^= 1;                     // (a call without frames leaves the carried v history where it is)
        } else {
            AW_HIP_TRY(awk::launch_rateconv_pcm(p, rc->ctx->stream));
        }
    } else {
        AW_HIP_TRY(awk::launch_rateconv(p, rc->ctx->stream));
    }
    rc->cur ^= 1;
    rc->counts.consumed += in_frames;
    rc->counts.produced += n_out;
    return AW_OK;
}

}  // namespace

extern "C" {

aw_status aw_rateconv_plan(double in_rate, double out_rate, int32_t *L, int32_t *M, int32_t *taps, int32_t *latency) try {
    awrc::Plan p;
    const aw_status st = plan_checked(in_rate, out_rate, p);
    if (st != AW_OK) return st;
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (taps) *taps = p.taps;
    if (latency) *latency = p.latency;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_rateconv_filter(double in_rate, double out_rate, float *c, int64_t capacity_floats) try {
    if (!c) return fail(AW_ERR_INVALID_ARGUMENT, "c is NULL");
    awrc::Plan p;
    const aw_status st = plan_checked(in_rate, out_rate, p);
    if (st != AW_OK) return st;
    if (capacity_floats < (int64_t)p.L * p.taps)
        return fail(AW_ERR_INVALID_ARGUMENT, "capacity_floats is below L * taps = " + std::to_string((long long)p.L * p.taps));
    awrc::filter(p, c);
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_rateconv_create(aw_context *ctx, double in_rate, double out_rate, int32_t n_streams, int32_t n_channels, aw_rateconv **out) try {
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!ctx) return fail(AW_ERR_NO_DEVICE, "no context (no HIP device): there is no CPU fallback");
    if (n_streams <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "n_streams must be > 0");
    if (n_channels < 1 || n_channels > awrc::kMaxChannels) return fail(AW_ERR_INVALID_ARGUMENT, "n_channels must be in 1..16");
    awrc::Plan pl;
    const aw_status planned = plan_checked(in_rate, out_rate, pl);
    if (planned != AW_OK) return planned;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(AW_ERR_NO_DEVICE, "hipSetDevice failed");
    awr::Owner<aw_rateconv> rc(new (std::nothrow) aw_rateconv(), aw_rateconv_destroy);
    if (!rc) return fail(AW_ERR_OUT_OF_MEMORY, "allocation failed");
    rc->ctx = ctx; rc->n_streams = n_streams; rc->n_channels = n_channels; rc->plan = pl;
    rc->tile = awk::rc_tile(pl.L, pl.M, pl.taps, n_channels);
    rc->tp_tile = awk::rc_tp_tile(pl.L, pl.M, pl.taps, n_channels);
    if (rc->tile < 1) return fail(AW_ERR_INVALID_ARGUMENT, "no tile of this converter fits the kernel's LDS");
    // the table, rows padded to 16-byte words (the pad is never read as a tap)
    const int stride = awk::rc_row_stride(pl.taps);
    std::vector<float> dense((size_t)pl.L * pl.taps), rows((size_t)pl.L * stride, 0.0f);
    awrc::filter(pl, dense.data());
    for (int ph = 0; ph < pl.L; ++ph)
        for (int k = 0; k < pl.taps; ++k) rows[(size_t)ph * stride + k] = dense[(size_t)ph * pl.taps + k];
    awr::Counter *const allocs = &ctx->device_allocs;
    AW_HIP_TRY(rc->d_c.upload(rows.data(), rows.size(), allocs, &ctx->sync_copies));
    const size_t hist = (size_t)n_streams * (pl.taps - 1) * n_channels;
    AW_HIP_TRY(rc->d_hist[0].alloc(hist, allocs));
    AW_HIP_TRY(rc->d_hist[1].alloc(hist, allocs));
    AW_HIP_TRY(rc->d_counts.alloc((size_t)n_streams * 2, allocs));
    const aw_status zeroed = reset_state(rc.get());
    if (zeroed != AW_OK) return zeroed;
    *out = rc.release();
    return AW_OK;
} AW_NOEXCEPT_TAIL

void aw_rateconv_destroy(aw_rateconv *rc) {
    if (!rc) return;
    (void)hipSetDevice(rc->ctx->device);
    (void)hipStreamSynchronize(rc->ctx->stream);
    delete rc;
}

int64_t aw_rateconv_info(const aw_rateconv *rc, int32_t what) {
    if (!rc) return -1;
    switch (what) {
        case 0: return rc->plan.L;
        case 1: return rc->plan.M;
        case 2: return rc->plan.taps;
        case 3: return rc->plan.latency;
        case 4: return rc->tile;
        case 5: return rc->counts.consumed;
        case 6: return rc->counts.produced;
        case 7: return rc->dither;
        case 8: return rc->gain_mode;
        case 9: return rc->metering;
        case 10: return rc->true_peak;
        case 11: return rc->tp_tile > 0 ? rc->tp_tile : 0;
        default: return -1;
    }
}

int64_t aw_rateconv_output_frames(const aw_rateconv *rc, int64_t in_frames) {
    if (!rc || in_frames < 0) return -1;
    return awrc::outputs_after(rc->counts.consumed + in_frames, rc->plan.L, rc->plan.M, rc->plan.latency) - rc->counts.produced;
}

aw_status aw_rateconv_process(aw_rateconv *rc, const float *in_device, int64_t in_frames, float *out_device, int64_t out_capacity_frames,
                              int64_t *out_frames) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (in_frames < 0) return fail(AW_ERR_INVALID_ARGUMENT, "in_frames must be >= 0");
    if (in_frames > 0 && !in_device) return fail(AW_ERR_INVALID_ARGUMENT, "in_device is NULL");
    if ((reinterpret_cast<uintptr_t>(in_device) | reinterpret_cast<uintptr_t>(out_device)) & 3u)
        return fail(AW_ERR_INVALID_ARGUMENT, "buffers must be 4-byte aligned");
    return run(rc, in_device, in_frames, out_device, out_capacity_frames, out_frames);
} AW_NOEXCEPT_TAIL

aw_status aw_rateconv_flush(aw_rateconv *rc, float *out_device, int64_t out_capacity_frames, int64_t *out_frames) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (reinterpret_cast<uintptr_t>(out_device) & 3u) return fail(AW_ERR_INVALID_ARGUMENT, "buffers must be 4-byte aligned");
    const aw_status st = run(rc, nullptr, rc->plan.latency, out_device, out_capacity_frames, out_frames);
    if (st != AW_OK) return st;
    return reset_state(rc);
} AW_NOEXCEPT_TAIL

aw_status aw_rateconv_reset(aw_rateconv *rc) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    AW_HIP_TRY(hipSetDevice(rc->ctx->device));
    return reset_state(rc);
} AW_NOEXCEPT_TAIL

aw_status aw_pcm_rateconv_process(aw_rateconv *rc, const void *in_device, aw_sample_format in_format, int64_t in_frames, void *out_device,
                                  aw_sample_format out_format, int64_t out_capacity_frames, int64_t *out_frames, uint64_t *clipped_device) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!awp::format_bytes(in_format) || !awp::format_bytes(out_format)) return fail(AW_ERR_INVALID_ARGUMENT, "unknown sample format");
    if (in_frames < 0) return fail(AW_ERR_INVALID_ARGUMENT, "in_frames must be >= 0");
    if (in_frames > 0 && !in_device) return fail(AW_ERR_INVALID_ARGUMENT, "in_device is NULL");
    const PcmCall call{in_format, out_format, clipped_device, false};
    return run(rc, in_device, in_frames, out_device, out_capacity_frames, out_frames, &call);
} AW_NOEXCEPT_TAIL

aw_status aw_pcm_rateconv_flush(aw_rateconv *rc, void *out_device, aw_sample_format out_format, int64_t out_capacity_frames, int64_t *out_frames,
                                uint64_t *clipped_device) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!awp::format_bytes(out_format)) return fail(AW_ERR_INVALID_ARGUMENT, "unknown sample format");
    const PcmCall call{AW_SAMPLE_F32, out_format, clipped_device, false};
    const aw_status st = run(rc, nullptr, rc->plan.latency, out_device, out_capacity_frames, out_frames, &call);
    if (st != AW_OK) return st;
    return reset_state(rc);
} AW_NOEXCEPT_TAIL

aw_status aw_pcm_rateconv_set_dither(aw_rateconv *rc, aw_dither mode, uint64_t seed, uint64_t first_stream) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (mode != AW_DITHER_NONE && mode != AW_DITHER_TPDF && mode != AW_DITHER_TPDF_HP) return fail(AW_ERR_INVALID_ARGUMENT, "unknown dither mode");
    rc->dither = mode; rc->dither_seed = seed; rc->first_stream = first_stream;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_pcm_rateconv_set_gain(aw_rateconv *rc, aw_gain_mode mode, const float *gains_host, int32_t n) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (mode == AW_GAIN_NONE) { rc->gain_mode = AW_GAIN_NONE; return AW_OK; }
    if (mode == AW_GAIN_PEAK_CEILING || mode == AW_GAIN_TRUE_PEAK_CEILING)
        return fail(AW_ERR_INVALID_ARGUMENT, "the ceiling gains are per-call functions of a peak, which the one-pass converter does not have: meter, then set AW_GAIN_FIXED");
    if (mode != AW_GAIN_FIXED) return fail(AW_ERR_INVALID_ARGUMENT, "unknown gain mode");
    if (!gains_host || (n != 1 && n != rc->n_streams)) return fail(AW_ERR_INVALID_ARGUMENT, "AW_GAIN_FIXED takes 1 gain or one per stream");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(gains_host[i])) return fail(AW_ERR_INVALID_ARGUMENT, "gain " + std::to_string(i) + " is not finite");
    std::vector<float> g((size_t)rc->n_streams);
    for (int s = 0; s < rc->n_streams; ++s) g[(size_t)s] = gains_host[n == 1 ? 0 : s];
    AW_HIP_TRY(hipSetDevice(rc->ctx->device));
    AW_HIP_TRY(hipStreamSynchronize(rc->ctx->stream));          // (no call still reads the gains this one replaces)
    awr::Buf<float> fresh;
    AW_HIP_TRY(fresh.upload(g.data(), g.size(), &rc->ctx->device_allocs, &rc->ctx->sync_copies));
    rc->d_gains = std::move(fresh);
    rc->gain_mode = AW_GAIN_FIXED;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_pcm_rateconv_set_metering(aw_rateconv *rc, int32_t on) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (on && !rc->d_levels) {
        AW_HIP_TRY(hipSetDevice(rc->ctx->device));
        awr::Buf<awk::RateconvLevels> fresh;
        AW_HIP_TRY(fresh.alloc((size_t)rc->n_streams, &rc->ctx->device_allocs));
        AW_HIP_TRY(hipMemsetAsync(fresh.get(), 0, fresh.bytes(), rc->ctx->stream));
        rc->d_levels = std::move(fresh);
    }
    rc->metering = on ? 1 : 0;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_pcm_rateconv_get_levels(aw_rateconv *rc, int32_t first_stream, int32_t n, aw_rateconv_levels *out_host) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!out_host) return fail(AW_ERR_INVALID_ARGUMENT, "out_host is NULL");
    if (first_stream < 0 || n < 0 || (long long)first_stream + n > rc->n_streams) return fail(AW_ERR_INVALID_ARGUMENT, "stream range outside the handle");
    if (!rc->d_levels) return fail(AW_ERR_INVALID_ARGUMENT, "aw_pcm_rateconv_set_metering was never called on this handle");
    AW_HIP_TRY(hipSetDevice(rc->ctx->device));
    if (n > 0)
        AW_HIP_TRY(hipMemcpyAsync(out_host, rc->d_levels.get() + first_stream, (size_t)n * sizeof(aw_rateconv_levels), hipMemcpyDeviceToHost, rc->ctx->stream));
    AW_HIP_TRY(hipStreamSynchronize(rc->ctx->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_pcm_rateconv_reset_levels(aw_rateconv *rc) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!rc->d_levels) return AW_OK;
    AW_HIP_TRY(hipSetDevice(rc->ctx->device));
    AW_HIP_TRY(hipMemsetAsync(rc->d_levels.get(), 0, rc->d_levels.bytes(), rc->ctx->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_tp_rateconv_set(aw_rateconv *rc, int32_t on) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!on) { rc->true_peak = 0; return AW_OK; }
    if (rc->tp_tile < 1)
        return fail(AW_ERR_INVALID_ARGUMENT, "the measuring form needs 11 output frames beside a tile, and this converter's tile of " +
                                                 std::to_string(rc->tile) + " leaves none");
    if (rc->true_peak) return AW_OK;
    AW_HIP_TRY(hipSetDevice(rc->ctx->device));
    if (!rc->d_tp) {
        awr::Buf<float> fresh;
        const size_t floats = (size_t)rc->n_streams * (sizeof(awk::RateconvTruePeak) / sizeof(float)) + 2 * rc->tp_hist_floats();
        AW_HIP_TRY(fresh.alloc(floats, &rc->ctx->device_allocs));
        AW_HIP_TRY(hipMemsetAsync(fresh.get(), 0, fresh.bytes(), rc->ctx->stream));
        rc->d_tp = std::move(fresh);
        awtp::filter(rc->tp_c);
    } else {                                   // switched on again: what the meter did not see counts as v = 0
        AW_HIP_TRY(hipMemsetAsync(rc->tp_hist(rc->tp_cur), 0, rc->tp_hist_floats() * sizeof(float), rc->ctx->stream));
    }
    rc->true_peak = 1;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_tp_rateconv_get(aw_rateconv *rc, int32_t first_stream, int32_t n, aw_rateconv_true_peak *out_host) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!out_host) return fail(AW_ERR_INVALID_ARGUMENT, "out_host is NULL");
    if (first_stream < 0 || n < 0 || (long long)first_stream + n > rc->n_streams) return fail(AW_ERR_INVALID_ARGUMENT, "stream range outside the handle");
    if (!rc->d_tp) return fail(AW_ERR_INVALID_ARGUMENT, "aw_tp_rateconv_set was never switched on on this handle");
    AW_HIP_TRY(hipSetDevice(rc->ctx->device));
    if (n > 0)
        AW_HIP_TRY(hipMemcpyAsync(out_host, rc->tp_records() + first_stream, (size_t)n * sizeof(aw_rateconv_true_peak), hipMemcpyDeviceToHost, rc->ctx->stream));
    AW_HIP_TRY(hipStreamSynchronize(rc->ctx->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_tp_rateconv_reset_records(aw_rateconv *rc) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!rc->d_tp) return AW_OK;
    AW_HIP_TRY(hipSetDevice(rc->ctx->device));
    AW_HIP_TRY(hipMemsetAsync(rc->tp_records(), 0, (size_t)rc->n_streams * sizeof(awk::RateconvTruePeak), rc->ctx->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_tp_rateconv_measure(aw_rateconv *rc, const void *in_device, aw_sample_format in_format, int64_t in_frames, int64_t *out_frames) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!awp::format_bytes(in_format)) return fail(AW_ERR_INVALID_ARGUMENT, "unknown sample format");
    if (in_frames < 0) return fail(AW_ERR_INVALID_ARGUMENT, "in_frames must be >= 0");
    if (in_frames > 0 && !in_device) return fail(AW_ERR_INVALID_ARGUMENT, "in_device is NULL");
    if (!rc->true_peak) return fail(AW_ERR_INVALID_ARGUMENT, "measuring is off: aw_tp_rateconv_set(rc, 1) first");
    const PcmCall call{in_format, AW_SAMPLE_F32, nullptr, true};
    return run(rc, in_device, in_frames, nullptr, 0, out_frames, &call);
} AW_NOEXCEPT_TAIL

aw_status aw_tp_rateconv_measure_flush(aw_rateconv *rc, int64_t *out_frames) try {
    if (!rc) return fail(AW_ERR_INVALID_ARGUMENT, "rc is NULL");
    if (!rc->true_peak) return fail(AW_ERR_INVALID_ARGUMENT, "measuring is off: aw_tp_rateconv_set(rc, 1) first");
    const PcmCall call{AW_SAMPLE_F32, AW_SAMPLE_F32, nullptr, true};
    const aw_status st = run(rc, nullptr, rc->plan.latency, nullptr, 0, out_frames, &call);
    if (st != AW_OK) return st;
    return reset_state(rc);
} AW_NOEXCEPT_TAIL

}  // extern "C"
