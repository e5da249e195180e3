// multi_runtime.cpp — device enumeration and aw_multi, the batch spatializer over several devices behind ONE handle (include/airwave_hip.h,
// "multi-device batch spatializer").  No device code of its own: a shard is an aw_context + aw_hrir + aw_spatializer driven through the
// single-handle entries, the process path on one persistent worker thread per shard (host/shard_workers.hpp), everything else on the
// caller's thread.  Which streams a shard owns, and how a global stream range is cut, is host/shard_plan.hpp.  Compiled by hipcc as host C++.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "runtime.hpp"

#include "device/pcm.hpp"
#include "host/shard_plan.hpp"
#include "host/shard_workers.hpp"

using awr::fail;

struct aw_multi {
    struct ShardObj {
        int32_t ordinal = 0;
        awsh::Shard range;                       // (count 0: nothing below exists)
        aw_context *ctx = nullptr;
        aw_hrir *hrir = nullptr;
        aw_spatializer *sp = nullptr;
        uint64_t clipped = 0;                    // the last process call's count, written by the shard's worker
    };
    int32_t n_streams = 0, n_channels = 0;
    std::vector<ShardObj> shards;                // one per entry of device_ordinals
    std::vector<awsh::Piece> pieces;             // one slot per shard: what a getter or a sliced setter walks (no allocation on a call)
    std::unique_ptr<awsh::Workers> workers;      // one thread per non-empty shard
    int32_t world() const { return (int32_t)shards.size(); }
    ShardObj *first_live() { for (ShardObj &s : shards) if (s.sp) return &s; return nullptr; }
};

namespace {

std::string shard_prefix(const aw_multi *m, int32_t i) { return "shard " + std::to_string(i) + " (device " + std::to_string(m->shards[(size_t)i].ordinal) + "): "; }

// a failing single-handle call on the caller's thread: its status, its message prefixed with the shard
aw_status shard_fail(const aw_multi *m, int32_t i, aw_status st) { return fail(st, shard_prefix(m, i) + aw_last_error_message()); }

// what a worker runs: a single-handle call on the shard's objects; on failure the text of the worker's thread-local message goes into the
// worker's buffer, from where run()'s caller takes it to its own thread-local message
template <class Call> struct ShardJob {
    aw_multi *m;
    Call call;
    int operator()(int shard, char *message, size_t capacity) {
        const aw_status st = call(m->shards[(size_t)shard]);
        if (st != AW_OK) std::snprintf(message, capacity, "%s", aw_last_error_message());
        return (int)st;
    }
};
template <class Call> aw_status run_on_workers(aw_multi *m, Call call) {
    ShardJob<Call> job{m, call};
    const awsh::Workers::Result r = m->workers->run(job);
    return r.status == 0 ? AW_OK : fail((aw_status)r.status, shard_prefix(m, r.shard) + r.message);
}

// every live shard in turn on the caller's thread; stops at the first failure
template <class Call> aw_status each_shard(aw_multi *m, Call call) {
    for (int32_t i = 0; i < m->world(); ++i) {
        aw_multi::ShardObj &s = m->shards[(size_t)i];
        if (!s.sp) continue;
        const aw_status st = call(s);
        if (st != AW_OK) return shard_fail(m, i, st);
    }
    return AW_OK;
}

// the prologue of the range getters: the handle, the range, n == 0 (*pieces = 0: the call is over), the output
aw_status range_begin(aw_multi *m, int32_t first_stream, int32_t n, const void *out, int32_t *pieces) {
    *pieces = 0;
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    if (first_stream < 0 || n < 0 || (int64_t)first_stream + n > m->n_streams) return fail(AW_ERR_INVALID_ARGUMENT, "streams out of range");
    if (n == 0) return AW_OK;
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out_host is NULL");
    *pieces = awsh::shard_ranges(m->n_streams, m->world(), first_stream, n, m->pieces.data());
    return AW_OK;
}

template <class Record, class Get> aw_status gather(aw_multi *m, int32_t first_stream, int32_t n, Record *out, Get get) {
    int32_t k = 0;
    const aw_status st = range_begin(m, first_stream, n, out, &k);
    if (st != AW_OK) return st;
    for (int32_t j = 0; j < k; ++j) {
        const awsh::Piece &p = m->pieces[(size_t)j];
        const aw_status s = get(m->shards[(size_t)p.shard].sp, p.local_first, p.count, out + (p.global_first - first_stream));
        if (s != AW_OK) return shard_fail(m, p.shard, s);
    }
    return AW_OK;
}

// The equalizer setters' whole-argument check (the single handle's own, over every stream of the multi handle), so that a refused call has
// changed no shard
aw_status eq_args(const aw_multi *m, const aw_eq_definition *const *definitions, int32_t n_definitions, const int32_t *stream_definition, int32_t lowest,
                  bool check_without_definitions) {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    return awr::eq_map_args(definitions, n_definitions, stream_definition, m->n_streams, lowest, check_without_definitions);
}

void multi_free(aw_multi *m) {
    if (!m) return;
    m->workers.reset();                          // the threads first: nothing runs on a shard that is being torn down
    for (aw_multi::ShardObj &s : m->shards) {
        aw_spatializer_destroy(s.sp);
        aw_hrir_destroy(s.hrir);
        aw_context_destroy(s.ctx);
    }
    delete m;
}

}  // namespace

extern "C" {

/* ---- device enumeration ---------------------------------------------------------------------- */
int32_t aw_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return count > 0 ? count : 0;
}

aw_status aw_device_info(int32_t ordinal, struct aw_device_info *out) try {
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out is NULL");
    std::memset(out, 0, sizeof *out);
    const int32_t count = aw_device_count();
    if (count <= 0) return fail(AW_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (ordinal < 0 || ordinal >= count) return fail(AW_ERR_NO_DEVICE, "device ordinal out of range");
    hipDeviceProp_t prop;
    AW_HIP_TRY(hipGetDeviceProperties(&prop, ordinal));
    std::snprintf(out->name, sizeof out->name, "%s", prop.name);
    std::snprintf(out->arch, sizeof out->arch, "%s", prop.gcnArchName);
    out->compute_units = prop.multiProcessorCount;
    out->total_bytes = (uint64_t)prop.totalGlobalMem;
    int previous = 0;                            // free memory is asked of the current device: put the caller's back afterwards
    AW_HIP_TRY(hipGetDevice(&previous));
    AW_HIP_TRY(hipSetDevice(ordinal));
    size_t free_b = 0, total_b = 0;
    const hipError_t e = hipMemGetInfo(&free_b, &total_b);
    (void)hipSetDevice(previous);
    AW_HIP_TRY(e);
    out->free_bytes = (uint64_t)free_b;
    return AW_OK;
} AW_NOEXCEPT_TAIL

/* ---- the handle ------------------------------------------------------------------------------ */
aw_status aw_multi_create(const int32_t *device_ordinals, int32_t n_devices, const float *tracks, int32_t n_tracks, int32_t taps, double sample_rate,
                          int32_t n_in_channels, const int32_t *left_track, const int32_t *right_track, int32_t n_streams, int32_t block_hint,
                          aw_multi **out) try {
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64) return fail(AW_ERR_INVALID_ARGUMENT, "n_devices must lie in 1 .. 64");
    if (!device_ordinals) return fail(AW_ERR_INVALID_ARGUMENT, "device_ordinals is NULL");
    if (n_streams < 1) return fail(AW_ERR_INVALID_ARGUMENT, "n_streams must be >= 1");
    // what aw_hrir_create and aw_spatializer_create would refuse, answered here with their statuses: before any HIP call
    if (!tracks) return fail(AW_ERR_INVALID_ARGUMENT, "tracks is NULL");
    if (n_tracks <= 0) return fail(AW_ERR_INVALID_CHANNEL_COUNT, "HRIR needs at least one track");
    if (taps <= 0) return fail(AW_ERR_WAV_EMPTY_FILE, "HRIR has no taps");
    if (!left_track || !right_track) return fail(AW_ERR_INVALID_ARGUMENT, "left_track or right_track is NULL");
    if (n_in_channels <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "n_in_channels must be positive");
    int mapped = 0;
    for (int32_t c = 0; c < n_in_channels; ++c) {
        const int32_t l = left_track[c], r = right_track[c];
        if (l < 0 || r < 0) continue;
        if (l >= n_tracks || r >= n_tracks)
            return fail(AW_ERR_INVALID_CHANNEL_MAPPING, "HRIR indices (" + std::to_string(l) + ", " + std::to_string(r) + ") out of range for " + std::to_string(n_tracks) + " channels");
        ++mapped;
    }
    if (mapped == 0) return fail(AW_ERR_CONVOLUTION_SETUP_FAILED, "No valid renderers created");

    awr::Owner<aw_multi> owner(new (std::nothrow) aw_multi(), multi_free);          // destroys what was built on every early return below
    aw_multi *m = owner.get();
    if (!m) return fail(AW_ERR_OUT_OF_MEMORY, "multi handle");
    m->n_streams = n_streams; m->n_channels = n_in_channels;
    m->shards.resize((size_t)n_devices);
    m->pieces.resize((size_t)n_devices);
    std::vector<int> live;
    for (int32_t i = 0; i < n_devices; ++i) {
        m->shards[(size_t)i].ordinal = device_ordinals[i];
        m->shards[(size_t)i].range = awsh::shard_streams(n_streams, n_devices, i);
        if (m->shards[(size_t)i].range.count > 0) live.push_back(i);
    }
    for (int i : live) {
        aw_multi::ShardObj &s = m->shards[(size_t)i];
        aw_status st = awr::context_create_divided(s.ordinal, (int32_t)live.size(), &s.ctx);
        if (st == AW_OK) st = aw_hrir_create(s.ctx, tracks, n_tracks, taps, sample_rate, &s.hrir);
        if (st == AW_OK) st = aw_spatializer_create(s.ctx, s.hrir, n_in_channels, left_track, right_track, s.range.count, block_hint, &s.sp);
        if (st != AW_OK) return shard_fail(m, i, st);
    }
    m->workers.reset(new awsh::Workers(live, AW_ERR_INVALID_ARGUMENT));
    *out = owner.release();
    return AW_OK;
} AW_NOEXCEPT_TAIL

void aw_multi_destroy(aw_multi *m) { multi_free(m); }

int32_t aw_multi_shard_count(const aw_multi *m) { return m ? m->world() : 0; }
int32_t aw_multi_stream_count(const aw_multi *m) { return m ? m->n_streams : 0; }
int32_t aw_multi_channel_count(const aw_multi *m) { return m ? m->n_channels : 0; }

aw_status aw_multi_shard(const aw_multi *m, int32_t shard, int32_t *device_ordinal, int32_t *first_stream, int32_t *count) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    if (shard < 0 || shard >= m->world()) return fail(AW_ERR_INVALID_ARGUMENT, "shard out of range");
    const aw_multi::ShardObj &s = m->shards[(size_t)shard];
    if (device_ordinal) *device_ordinal = s.ordinal;
    if (first_stream) *first_stream = s.range.first;
    if (count) *count = s.range.count;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_spatializer *aw_multi_spatializer(const aw_multi *m, int32_t shard) { return m && shard >= 0 && shard < m->world() ? m->shards[(size_t)shard].sp : nullptr; }
aw_context *aw_multi_context(const aw_multi *m, int32_t shard) { return m && shard >= 0 && shard < m->world() ? m->shards[(size_t)shard].ctx : nullptr; }

/* ---- process path: on the workers ------------------------------------------------------------ */
aw_status aw_multi_reserve_pcm(aw_multi *m, int64_t max_frames, aw_sample_format in_format, aw_sample_format out_format) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    if (awp::format_bytes(in_format) <= 0 || awp::format_bytes(out_format) <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "unknown sample format");
    return run_on_workers(m, [=](aw_multi::ShardObj &s) { return aw_spatializer_reserve_pcm(s.sp, max_frames, in_format, out_format); });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_process_host_pcm(aw_multi *m, const void *in_host, aw_sample_format in_format, void *out_host, aw_sample_format out_format,
                                    int64_t frames, uint64_t *clipped) try {
    if (!m || !in_host || !out_host) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    const int in_b = awp::format_bytes(in_format), out_b = awp::format_bytes(out_format);
    if (in_b <= 0 || out_b <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "unknown sample format");
    if (clipped) *clipped = 0;
    if (frames <= 0) return frames == 0 ? AW_OK : fail(AW_ERR_INVALID_ARGUMENT, "frames must be >= 0");
    // one handle's layouts: shard i's slice starts at its first stream
    const size_t in_psb = (size_t)frames * (size_t)m->n_channels * (size_t)in_b, out_psb = (size_t)frames * 2 * (size_t)out_b;
    const unsigned char *in = static_cast<const unsigned char *>(in_host);
    unsigned char *o = static_cast<unsigned char *>(out_host);
    const bool plain = in_format == AW_SAMPLE_F32 && out_format == AW_SAMPLE_F32;
    const aw_status st = run_on_workers(m, [=](aw_multi::ShardObj &s) {
        const unsigned char *si = in + (size_t)s.range.first * in_psb;
        unsigned char *so = o + (size_t)s.range.first * out_psb;
        s.clipped = 0;
        if (plain) return aw_spatializer_process_host(s.sp, reinterpret_cast<const float *>(si), reinterpret_cast<float *>(so), frames);
        return aw_spatializer_process_host_pcm(s.sp, si, in_format, so, out_format, frames, &s.clipped);
    });
    if (st != AW_OK) return st;
    uint64_t total = 0;
    for (const aw_multi::ShardObj &s : m->shards) total += s.clipped;
    if (clipped) *clipped = total;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_multi_reset(aw_multi *m) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    return each_shard(m, [](aw_multi::ShardObj &s) { return aw_spatializer_reset(s.sp); });
} AW_NOEXCEPT_TAIL

/* ---- page-locked buffers every device of the handle can DMA ---------------------------------- */
aw_status aw_multi_alloc_pinned(aw_multi *m, size_t bytes, void **ptr) try {
    if (!m || !ptr) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    *ptr = nullptr;
    aw_multi::ShardObj *s = m->first_live();
    AW_HIP_TRY(hipSetDevice(s->ctx->device));
    AW_HIP_TRY(awr::host_alloc_raw(ptr, bytes ? bytes : 1, hipHostMallocPortable));
    s->ctx->device_allocs += 1;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_multi_free_pinned(aw_multi *m, void *ptr) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    if (ptr) AW_HIP_TRY(awr::host_free_raw(ptr));
    return AW_OK;
} AW_NOEXCEPT_TAIL

/* ---- settings: serially on the caller's thread, sliced with shard_ranges --------------------- */
aw_status aw_multi_set_dither(aw_multi *m, aw_dither mode, uint64_t seed, uint64_t first_stream) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    if (mode != AW_DITHER_NONE && mode != AW_DITHER_TPDF && mode != AW_DITHER_TPDF_HP) return fail(AW_ERR_INVALID_ARGUMENT, "unknown dither mode");
    return each_shard(m, [=](aw_multi::ShardObj &s) { return aw_spatializer_set_dither(s.sp, mode, seed, first_stream + (uint64_t)s.range.first); });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_set_metering(aw_multi *m, int32_t on) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    return each_shard(m, [=](aw_multi::ShardObj &s) { return aw_spatializer_set_metering(s.sp, on); });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_reset_levels(aw_multi *m) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    return each_shard(m, [](aw_multi::ShardObj &s) { return aw_spatializer_reset_levels(s.sp); });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_set_gain(aw_multi *m, aw_gain_mode mode, const float *gains_host, int32_t n, float ceiling) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    if (const aw_status args = awr::gain_args(mode, gains_host, n, m->n_streams, ceiling)) return args;          // the whole array first: a refused call has changed no shard
    const bool sliced = mode == AW_GAIN_FIXED && n != 1;
    return each_shard(m, [=](aw_multi::ShardObj &s) {
        return aw_spatializer_set_gain(s.sp, mode, sliced ? gains_host + s.range.first : gains_host, sliced ? s.range.count : n, ceiling);
    });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_set_loudness(aw_multi *m, int32_t on, double max_seconds) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    return each_shard(m, [=](aw_multi::ShardObj &s) { return aw_spatializer_set_loudness(s.sp, on, max_seconds); });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_set_true_peak(aw_multi *m, int32_t on) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    return each_shard(m, [=](aw_multi::ShardObj &s) { return aw_spatializer_set_true_peak(s.sp, on); });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_set_limiter(aw_multi *m, int32_t on, float ceiling, int32_t attack_frames, int32_t hold_frames) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    return each_shard(m, [=](aw_multi::ShardObj &s) { return aw_spatializer_set_limiter(s.sp, on, ceiling, attack_frames, hold_frames); });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_set_equalizer(aw_multi *m, const aw_eq_definition *const *definitions, int32_t n_definitions, const int32_t *stream_definition) try {
    const aw_status st = eq_args(m, definitions, n_definitions, stream_definition, -1, false);
    if (st != AW_OK) return st;
    return each_shard(m, [=](aw_multi::ShardObj &s) {
        return aw_spatializer_set_equalizer(s.sp, definitions, n_definitions, stream_definition ? stream_definition + s.range.first : nullptr);
    });
} AW_NOEXCEPT_TAIL

aw_status aw_multi_set_equalizer_target(aw_multi *m, const aw_eq_definition *const *definitions, int32_t n_definitions, const int32_t *stream_definition) try {
    const aw_status st = eq_args(m, definitions, n_definitions, stream_definition, AW_EQ_KEEP, true);
    if (st != AW_OK) return st;
    if (!stream_definition && n_definitions == 0) return fail(AW_ERR_INVALID_ARGUMENT, "stream_definition is NULL (every stream takes definition 0) and there is no definition");
    return each_shard(m, [=](aw_multi::ShardObj &s) {
        return aw_spatializer_set_equalizer_target(s.sp, definitions, n_definitions, stream_definition ? stream_definition + s.range.first : nullptr);
    });
} AW_NOEXCEPT_TAIL

/* ---- getters: a global stream range, gathered across the shard boundaries -------------------- */
aw_status aw_multi_get_levels(aw_multi *m, int32_t first_stream, int32_t n, aw_stream_levels *out_host) try {
    return gather(m, first_stream, n, out_host, aw_spatializer_get_levels);
} AW_NOEXCEPT_TAIL

aw_status aw_multi_get_loudness(aw_multi *m, int32_t first_stream, int32_t n, aw_stream_loudness *out_host) try {
    return gather(m, first_stream, n, out_host, aw_spatializer_get_loudness);
} AW_NOEXCEPT_TAIL

aw_status aw_multi_get_true_peak(aw_multi *m, int32_t first_stream, int32_t n, aw_stream_true_peak *out_host) try {
    return gather(m, first_stream, n, out_host, aw_spatializer_get_true_peak);
} AW_NOEXCEPT_TAIL

aw_status aw_multi_get_limiter(aw_multi *m, int32_t first_stream, int32_t n, aw_stream_limiter *out_host) try {
    return gather(m, first_stream, n, out_host, aw_spatializer_get_limiter);
} AW_NOEXCEPT_TAIL

aw_status aw_multi_get_loudness_hops(aw_multi *m, int32_t stream, int64_t first_hop, int64_t n, double *out_host) try {
    if (!m) return fail(AW_ERR_INVALID_ARGUMENT, "m is NULL");
    if (stream < 0 || stream >= m->n_streams) return fail(AW_ERR_INVALID_ARGUMENT, "stream out of range");
    const int32_t i = awsh::shard_of(m->n_streams, m->world(), stream);
    const aw_multi::ShardObj &s = m->shards[(size_t)i];
    const aw_status st = aw_spatializer_get_loudness_hops(s.sp, stream - s.range.first, first_hop, n, out_host);
    return st == AW_OK ? AW_OK : shard_fail(m, i, st);
} AW_NOEXCEPT_TAIL

}  // extern "C"
