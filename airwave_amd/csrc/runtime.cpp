// runtime.cpp — device-side objects of the C ABI: context, HRIR set, batch spatializer, the mono
// engine trio and the callback-size adapter.  Compiled by hipcc as host C++.
#include "runtime.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <new>
#include <stdexcept>
#include <thread>

#include "device/eq_kernels.hpp"
#include "device/limiter_kernels.hpp"
#include "device/loudness_kernels.hpp"
#include "device/pcm.hpp"
#include "device/pcm_kernels.hpp"
#include "device/truepeak_kernels.hpp"
#include "host/eq.hpp"
#include "host/path_policy.hpp"
#include "host/scratch_plan.hpp"
#include "host/tables.hpp"

// table sets a spatializer can hold: one per long-window length (awp::kLwRowChoices); lw_plans reserves this many at create
static constexpr size_t kLwPlanSlots = 16;

// Host threads that copy slices of ONE buffer at a time: the multi-stream host entry bounces pageable caller memory through page-locked
// chunks with them (one thread copies ~10 GB/s, PCIe Gen5 moves 57 GB/s each way).  copy() blocks; the caller copies a slice too.
struct aw_context::CopyPool {
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    char *dst = nullptr; const char *src = nullptr;
    size_t bytes = 0, slice = 0;
    int n_slices = 0, next = 0, done = 0;
    unsigned long long gen = 0;
    bool stop = false;
    explicit CopyPool(int n) {
        for (int i = 0; i < n; ++i) {
            try { workers.emplace_back([this] { run(); }); } catch (...) { break; }          // fewer threads: the caller's own slice loop still finishes the job
        }
    }
    ~CopyPool() {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv_work.notify_all();
        for (auto &w : workers) if (w.joinable()) w.join();
    }
    bool take(int &i) { if (next >= n_slices) return false; i = next++; return true; }       // under m
    void slice_copy(int i) {
        const size_t off = (size_t)i * slice, n = std::min(slice, bytes - off);
        std::memcpy(dst + off, src + off, n);
    }
    void run() {
        unsigned long long seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv_work.wait(lk, [&] { return stop || (gen != seen && next < n_slices); });
            if (stop) return;
            seen = gen;
            int i;
            while (take(i)) {
                lk.unlock();
                slice_copy(i);
                lk.lock();
                if (++done == n_slices) cv_done.notify_all();
            }
        }
    }
    // start() hands a buffer to the workers and returns; wait() blocks until it is copied (a pool with no worker copies in wait()).  One
    // job at a time per pool: the host entry uses a second, smaller pool for the output direction so that the copy OUT of chunk k-1 runs
    // beside the copy IN of chunk k+1 instead of after it on the driver thread (round 6).
    void start(void *d, const void *s_, size_t n) {
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return done == n_slices; });
        if (n == 0) return;
        dst = static_cast<char *>(d); src = static_cast<const char *>(s_); bytes = n;
        const int parts = (int)std::min<size_t>(std::max<size_t>(workers.size(), 1), std::max<size_t>(1, n >> 20));
        slice = ((n + parts - 1) / parts + 4095) & ~(size_t)4095;
        n_slices = (int)((n + slice - 1) / slice); next = 0; done = 0; ++gen;
        cv_work.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        int i;
        while (workers.empty() && take(i)) {          // no thread could be started: the waiter does the work
            lk.unlock();
            slice_copy(i);
            lk.lock();
            ++done;
        }
        cv_done.wait(lk, [&] { return done == n_slices; });
    }
    void copy(void *d, const void *s_, size_t n) {
        if (n == 0) return;
        std::unique_lock<std::mutex> lk(m);
        dst = static_cast<char *>(d); src = static_cast<const char *>(s_); bytes = n;
        const int parts = (int)std::min<size_t>(workers.size() + 1, std::max<size_t>(1, n >> 20));      // slices of >= 1 MiB
        slice = ((n + parts - 1) / parts + 4095) & ~(size_t)4095;
        n_slices = (int)((n + slice - 1) / slice); next = 0; done = 0; ++gen;
        cv_work.notify_all();
        int i;
        while (take(i)) {
            lk.unlock();
            slice_copy(i);
            lk.lock();
            ++done;
        }
        cv_done.wait(lk, [&] { return done == n_slices; });
    }
};

namespace awr {

static thread_local std::string g_last_error;
// the structured part of AW_ERR_EQ_INVALID_FILTER (aw_last_eq_filter_error): valid until the thread's next failing call
static thread_local struct { bool valid; int index, kind, line; } g_eq_filter_error = {false, 0, 0, 0};

void set_error(const std::string &msg) { g_last_error = msg; }
aw_status fail(aw_status code, const std::string &msg) {
    g_last_error = msg;
    g_eq_filter_error.valid = false;
    return code;
}
aw_status fail_eq_filter(int enabled_index, int kind, int source_line, const std::string &msg) {
    g_last_error = msg;
    g_eq_filter_error = {true, enabled_index, kind, source_line};
    return AW_ERR_EQ_INVALID_FILTER;
}
aw_status hip_fail(hipError_t e, const char *what) {
    g_eq_filter_error.valid = false;
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? AW_ERR_OUT_OF_MEMORY : AW_ERR_HIP;
}

bool context_literal_resampler(const aw_context *ctx) { return ctx && ctx->literal_resampler; }

aw_status caught() noexcept {
    aw_status code = AW_ERR_INVALID_ARGUMENT;
    try {
        try { throw; }
        catch (const std::bad_alloc &) { code = AW_ERR_OUT_OF_MEMORY; g_last_error = "host memory exhausted"; }
        catch (const std::length_error &) { code = AW_ERR_OUT_OF_MEMORY; g_last_error = "host container size limit"; }
        catch (const std::exception &e) { g_last_error = std::string("internal error: ") + e.what(); }
        catch (...) { g_last_error = "internal error"; }
    } catch (...) {          // (the message itself could not be stored)
    }
    return code;
}

}  // namespace awr

using awr::fail;

// awr::Buf::grow of one of a spatializer's grow-only buffers as a status; every such allocation counts in device_allocs.
template <class B> static aw_status grow_buf(aw_spatializer *sp, B *buf, size_t need) {
    AW_HIP_TRY(buf->grow(need, &sp->ctx->device_allocs));
    return AW_OK;
}

// The record getters' read-back: field f (host/stage_records.hpp) of the n streams from first_stream on, out of the stage's allocation d.
template <class T> static aw_status get_field(const awst::Field<T> &f, unsigned char *d, int32_t first_stream, int32_t n, std::vector<T> *host) {
    host->resize((size_t)n * f.per_stream);
    AW_HIP_TRY(hipMemcpy(host->data(), f.at(d, (size_t)first_stream), host->size() * sizeof(T), hipMemcpyDeviceToHost));
    return AW_OK;
}

extern "C" {

const char *aw_version(void) { return "airwave-hip 0.1 (gfx950)"; }

const char *aw_last_error_message(void) { return awr::g_last_error.c_str(); }

int32_t aw_last_eq_filter_error(int32_t *enabled_index, int32_t *error_kind, int32_t *source_line) {
    if (!awr::g_eq_filter_error.valid) return 0;
    if (enabled_index) *enabled_index = awr::g_eq_filter_error.index;
    if (error_kind) *error_kind = awr::g_eq_filter_error.kind;
    if (source_line) *source_line = awr::g_eq_filter_error.line;
    return 1;
}

const char *aw_status_string(aw_status s) {
    switch (s) {
        case AW_OK: return "ok";
        case AW_ERR_INVALID_ARGUMENT: return "invalid argument";
        case AW_ERR_OUT_OF_MEMORY: return "out of memory";
        case AW_ERR_HIP: return "HIP runtime error";
        case AW_ERR_NO_DEVICE: return "no HIP device";
        case AW_ERR_INVALID_CHANNEL_MAPPING: return "Invalid channel mapping";            // HRIRManager.swift:754
        case AW_ERR_CONVOLUTION_SETUP_FAILED: return "Failed to set up convolution";      // :752
        case AW_ERR_INVALID_CHANNEL_COUNT: return "Invalid channel count";                // :748, WAVLoader.swift:137
        case AW_ERR_WAV_FILE_READ: return "WAV file read error";                          // WAVLoader.swift:135
        case AW_ERR_WAV_EMPTY_FILE: return "WAV file is empty (0 frames)";                // :139
        case AW_ERR_WAV_UNSUPPORTED_FORMAT: return "Unsupported WAV format";              // :143
        case AW_ERR_BLOCK_SIZE_MISMATCH: return "frame count differs from the engine block size";
        case AW_ERR_EQ_PARSE: return "Could not read the equalizer preset";                // EqualizerAPOParser.swift:19
        case AW_ERR_EQ_INVALID_SAMPLE_RATE: return "Sample rate must be finite and positive.";   // ParametricEqualizerProcessor.swift:106-107
        case AW_ERR_EQ_NON_FINITE_PREAMP: return "Preamp must produce a finite linear gain.";   // :108-109
        case AW_ERR_EQ_TOO_MANY_FILTERS: return "Equalizer supports at most 64 filters";   // :110-111
        case AW_ERR_EQ_INVALID_FILTER: return "Filter is invalid";                          // :112-113
        case AW_ERR_EQ_NOT_FOLDABLE: return "Equalizer response too long to fold into the HRIR";
        default: return "unknown status";
    }
}

/* ---- context ------------------------------------------------------------------------------ */
static aw_status context_create_impl(int32_t device, void *ext_stream, bool use_ext, aw_context **out, int32_t copy_divisor = 1) {
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(AW_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= count) return fail(AW_ERR_NO_DEVICE, "device ordinal out of range");
    AW_HIP_TRY(hipSetDevice(device));
    awr::Owner<aw_context> owner(new (std::nothrow) aw_context(), aw_context_destroy);
    aw_context *c = owner.get();
    if (!c) return fail(AW_ERR_OUT_OF_MEMORY, "context");
    c->device = device;
    c->copy_divisor = std::max(1, copy_divisor);
    if (use_ext) {
        c->stream = reinterpret_cast<hipStream_t>(ext_stream);
        c->owns_stream = false;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { c->stream = nullptr; return awr::hip_fail(e, "hipStreamCreate"); }
        c->owns_stream = true;
    }
    hipError_t e = c->t0.create();
    if (e == hipSuccess) e = c->t1.create();
    if (e == hipSuccess) e = awk::prepare_kernels(&c->cfg);
    if (e == hipSuccess) e = awk::prepare_ola_kernels();
    if (e == hipSuccess) e = awk::prepare_lw_kernels();
    if (e == hipSuccess) e = awk::prepare_eq_kernels();
    if (e == hipSuccess) e = awk::prepare_loudness_kernels();
    if (e == hipSuccess) e = awk::prepare_truepeak_kernels();
    if (e == hipSuccess) e = awk::prepare_limiter_kernels();
    if (e == hipSuccess) e = awk::prepare_prep_kernels();
    awh::Twiddles tw;
    awh::build_twiddles(tw);
    if (e == hipSuccess) e = c->d_tw1.upload(tw.tw1.data(), tw.tw1.size(), nullptr, nullptr);
    if (e == hipSuccess) e = c->d_twa.upload(tw.twa.data(), tw.twa.size(), nullptr, nullptr);
    if (e == hipSuccess) e = c->d_twb.upload(tw.twb.data(), tw.twb.size(), nullptr, nullptr);
    if (e == hipSuccess) e = c->d_zeros.alloc(4096 / sizeof(float), nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_zeros.get(), 0, 4096, c->stream);      // (ordered on the stream its readers, the tile kernels, run on)
    if (e != hipSuccess) return awr::hip_fail(e, "context setup");
    *out = owner.release();
    return AW_OK;
}

aw_status aw_context_create(int32_t device, aw_context **out) try { return context_create_impl(device, nullptr, false, out); } AW_NOEXCEPT_TAIL
aw_status aw_context_create_on_stream(int32_t device, void *hip_stream, aw_context **out) try {
    return context_create_impl(device, hip_stream, true, out);
} AW_NOEXCEPT_TAIL

void aw_context_destroy(aw_context *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c->copy_pool;
    delete c->copy_pool_out;
    if (c->s_h2d) (void)hipStreamDestroy(c->s_h2d);
    if (c->s_d2h) (void)hipStreamDestroy(c->s_d2h);
    if (c->owns_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;          // (the buffers and events: their owners' destructors)
}

aw_status aw_context_synchronize(aw_context *c) try {
    if (!c) return fail(AW_ERR_INVALID_ARGUMENT, "ctx is NULL");
    AW_HIP_TRY(hipStreamSynchronize(c->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_context_set_resampler(aw_context *c, int32_t literal_vgenp) try {
    if (!c) return fail(AW_ERR_INVALID_ARGUMENT, "ctx is NULL");
    c->literal_resampler = literal_vgenp != 0;
    return AW_OK;
} AW_NOEXCEPT_TAIL

void *aw_context_stream(aw_context *c) { return c ? reinterpret_cast<void *>(c->stream) : nullptr; }

aw_status aw_context_timer_start(aw_context *c) try {
    if (!c) return fail(AW_ERR_INVALID_ARGUMENT, "ctx is NULL");
    AW_HIP_TRY(hipEventRecord(c->t0.get(), c->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_context_timer_stop(aw_context *c, float *ms) try {
    if (!c || !ms) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    AW_HIP_TRY(hipEventRecord(c->t1.get(), c->stream));
    AW_HIP_TRY(hipEventSynchronize(c->t1.get()));
    AW_HIP_TRY(hipEventElapsedTime(ms, c->t0.get(), c->t1.get()));
    return AW_OK;
} AW_NOEXCEPT_TAIL

// Grows the context's scratch pool to `need` complex elements (the caller holds launch_mu).  The pool is shared by every handle of the
// context, so a failed growth must not take it away from handles that reserved it earlier (round-5 advice): the old size is allocated
// again before the error is returned — if even that fails the pool is empty and the next process call of any handle allocates again (or
// reports the same error).  hipFree waits for the device: launches of other handles that still read the old buffer have finished.
static aw_status pool_grow(aw_context *c, size_t need) {
    const size_t old = c->d_pool.capacity();
    AW_HIP_TRY(c->d_pool.reset());
    const hipError_t e = c->d_pool.alloc(need, &c->device_allocs);
    if (e == hipSuccess) return AW_OK;
    if (old > 0) (void)c->d_pool.alloc(old, &c->device_allocs);
    return awr::hip_fail(e, "scratch pool");
}

/* The context's scratch pool (runtime.hpp), sized ahead of time: a host that knows its largest batch pays the one large hipMalloc at
 * start-up (its wall time is erratic on these boxes: 0.2 ms ... 3.7 s, profiles/round5_v1/alloc_probe.txt) instead of inside the first
 * aw_spatializer_reserve / process that needs it.  Grow-only; bytes the pool already holds are kept. */
aw_status aw_context_reserve_scratch(aw_context *c, size_t bytes) try {
    if (!c) return fail(AW_ERR_INVALID_ARGUMENT, "ctx is NULL");
    AW_HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->launch_mu);
    const size_t need = (bytes + sizeof(awk::cf) - 1) / sizeof(awk::cf);
    if (c->d_pool.capacity() >= need) return AW_OK;
    return pool_grow(c, need);
} AW_NOEXCEPT_TAIL
size_t aw_context_scratch_bytes(const aw_context *c) { return c ? c->d_pool.bytes() : 0; }

/* Measured ceilings of the device the context runs on ("confirm on the box and also quote a measured copy-kernel
 * ceiling"; bench.py's roofline.measured).  Own buffers, freed before returning; blocks; never on a process path. */
aw_status aw_context_bandwidth_probe(aw_context *c, size_t bytes, int32_t repetitions, double *read_gbs, double *write_gbs, double *copy_gbs) try {
    if (!c || !read_gbs || !write_gbs || !copy_gbs) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (bytes < ((size_t)64 << 20) || repetitions < 1) return fail(AW_ERR_INVALID_ARGUMENT, "probe needs >= 64 MiB and >= 1 repetition");
    AW_HIP_TRY(hipSetDevice(c->device));
    awr::Buf<unsigned char> buf_a, buf_b; awr::Buf<float> buf_sink;
    hipError_t e = buf_a.alloc(bytes, nullptr);
    if (e == hipSuccess) e = buf_b.alloc(bytes, nullptr);
    if (e == hipSuccess) e = buf_sink.alloc(64 / sizeof(float), nullptr);
    void *const a = buf_a.get(), *const b = buf_b.get(); float *const sink = buf_sink.get();
    // the source holds pseudo-random samples, not zeros (all-zero data draws less power and can read faster than real data does)
    if (e == hipSuccess) e = awk::launch_synth_fill(reinterpret_cast<float *>(a), 1, (long long)(bytes / sizeof(float)), 0xA17AEull, 0, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b, 0, bytes, c->stream);
    double best[3] = {0.0, 0.0, 0.0};
    for (int what = 0; what < 3 && e == hipSuccess; ++what)
        for (int nt = 0; nt < 2 && e == hipSuccess; ++nt) {
            size_t moved = 0;
            e = awk::launch_bw_probe(what, nt != 0, a, b, bytes, c->cfg.cus, sink, c->stream, &moved);       // warm-up (clocks, TLB)
            for (int r = 0; r < repetitions && e == hipSuccess; ++r) {
                e = hipEventRecord(c->t0.get(), c->stream);
                if (e == hipSuccess) e = awk::launch_bw_probe(what, nt != 0, a, b, bytes, c->cfg.cus, sink, c->stream, &moved);
                if (e == hipSuccess) e = hipEventRecord(c->t1.get(), c->stream);
                if (e == hipSuccess) e = hipEventSynchronize(c->t1.get());
                float ms = 0.f;
                if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->t0.get(), c->t1.get());
                if (e == hipSuccess && ms > 0.f) best[what] = std::max(best[what], (double)moved / (ms * 1e-3) / 1e9);
            }
        }
    if (e != hipSuccess) return awr::hip_fail(e, "bandwidth probe");
    *read_gbs = best[0]; *write_gbs = best[1]; *copy_gbs = best[2];
    return AW_OK;
} AW_NOEXCEPT_TAIL

/* Host link: page-locked host memory to the device and back with hipMemcpyAsync, each way alone and both ways at once (two streams).
 * The yardstick of the host entry's PCIe-inclusive rate (bench.py's secondary_end_to_end). */
aw_status aw_context_pcie_probe(aw_context *c, size_t bytes, int32_t repetitions, double *h2d_gbs, double *d2h_gbs, double *duplex_gbs) try {
    if (!c || !h2d_gbs || !d2h_gbs || !duplex_gbs) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (bytes < ((size_t)16 << 20) || repetitions < 1) return fail(AW_ERR_INVALID_ARGUMENT, "probe needs >= 16 MiB and >= 1 repetition");
    AW_HIP_TRY(hipSetDevice(c->device));
    awr::Buf<unsigned char, awr::Kind::pinned> buf_h_in, buf_h_out; awr::Buf<unsigned char> buf_d_in, buf_d_out;
    hipStream_t s2 = nullptr;
    hipError_t e = buf_h_in.alloc(bytes, nullptr);
    if (e == hipSuccess) e = buf_h_out.alloc(bytes, nullptr);
    if (e == hipSuccess) e = buf_d_in.alloc(bytes, nullptr);
    if (e == hipSuccess) e = buf_d_out.alloc(bytes, nullptr);
    void *const h_in = buf_h_in.get(), *const h_out = buf_h_out.get(), *const d_in = buf_d_in.get(), *const d_out = buf_d_out.get();
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s2, hipStreamNonBlocking);
    if (e == hipSuccess) { std::memset(h_in, 0, bytes); std::memset(h_out, 0, bytes); e = hipMemsetAsync(d_out, 0, bytes, c->stream); }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    double best[3] = {0.0, 0.0, 0.0};
    for (int what = 0; what < 3 && e == hipSuccess; ++what)
        for (int r = 0; r <= repetitions && e == hipSuccess; ++r) {          // (r = 0: warm-up)
            const auto t0 = std::chrono::steady_clock::now();
            if (what != 1) e = hipMemcpyAsync(d_in, h_in, bytes, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess && what != 0) e = hipMemcpyAsync(h_out, d_out, bytes, hipMemcpyDeviceToHost, what == 2 ? s2 : c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e == hipSuccess && what == 2) e = hipStreamSynchronize(s2);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (r > 0 && sec > 0.0) best[what] = std::max(best[what], (double)bytes * (what == 2 ? 2.0 : 1.0) / sec / 1e9);
        }
    if (s2) (void)hipStreamDestroy(s2);
    if (e != hipSuccess) return awr::hip_fail(e, "pcie probe");
    *h2d_gbs = best[0]; *d2h_gbs = best[1]; *duplex_gbs = best[2];
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_device_alloc(aw_context *c, size_t bytes, void **dptr) try {
    if (!c || !dptr) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    AW_HIP_TRY(hipSetDevice(c->device));
    AW_HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));
    return AW_OK;
} AW_NOEXCEPT_TAIL
aw_status aw_device_free(aw_context *c, void *dptr) try {
    if (!c) return fail(AW_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (dptr) AW_HIP_TRY(hipFree(dptr));
    return AW_OK;
} AW_NOEXCEPT_TAIL
aw_status aw_memcpy_h2d(aw_context *c, void *dst, const void *src, size_t bytes) try {
    if (!c || (bytes && (!dst || !src))) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    AW_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    AW_HIP_TRY(hipStreamSynchronize(c->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL
aw_status aw_memcpy_d2h(aw_context *c, void *dst, const void *src, size_t bytes) try {
    if (!c || (bytes && (!dst || !src))) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    AW_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    AW_HIP_TRY(hipStreamSynchronize(c->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL

/* ---- HRIR set ------------------------------------------------------------------------------- */
aw_status aw_hrir_create(aw_context *ctx, const float *tracks, int32_t n_tracks, int32_t taps, double sample_rate,
                         aw_hrir **out) try {
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!ctx || !tracks) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_tracks <= 0) return fail(AW_ERR_INVALID_CHANNEL_COUNT, "HRIR needs at least one track");
    if (taps <= 0) return fail(AW_ERR_WAV_EMPTY_FILE, "HRIR has no taps");
    awr::Owner<aw_hrir> h(new (std::nothrow) aw_hrir(), aw_hrir_destroy);
    if (!h) return fail(AW_ERR_OUT_OF_MEMORY, "hrir");
    h->ctx = ctx; h->n_tracks = n_tracks; h->taps = taps; h->sample_rate = sample_rate;
    h->tracks.assign(tracks, tracks + (size_t)n_tracks * taps);
    *out = h.release();
    return AW_OK;
} AW_NOEXCEPT_TAIL
void aw_hrir_destroy(aw_hrir *h) { delete h; }
int32_t aw_hrir_track_count(const aw_hrir *h) { return h ? h->n_tracks : 0; }
int32_t aw_hrir_taps(const aw_hrir *h) { return h ? h->taps : 0; }
double aw_hrir_sample_rate(const aw_hrir *h) { return h ? h->sample_rate : 0.0; }

/* ---- spatializer ---------------------------------------------------------------------------- */
static aw_status sp_alloc_hist(aw_spatializer *sp) {
    // + 4 floats: whole-frame vector loads of layouts whose frames are not float4s run up to 3 floats past a frame
    const size_t n = (size_t)sp->n_streams * sp->hist_len * sp->n_channels + 4;
    for (int i = 0; i < 2; ++i) {
        AW_HIP_TRY(sp->d_hist[i].alloc(n, nullptr));
        AW_HIP_TRY(hipMemsetAsync(sp->d_hist[i].get(), 0, n * sizeof(float), sp->ctx->stream));
    }
    sp->hist_cur = 0;
    return AW_OK;
}

// The kernel-path decisions of a spatializer are pure functions of its layout and knobs (host/path_policy.hpp); this file reads the knobs,
// calls them and keeps the side effects.
static awp::Layout sp_layout(const aw_spatializer *sp) { return awp::Layout{sp->n_channels, sp->taps, sp->n_streams}; }
static awp::CreatePlan sp_plan(const aw_spatializer *sp) {          // what plan_create() decided, as aw_spatializer_create copied it into sp
    awp::CreatePlan p;
    p.path = sp->path; p.fused2 = sp->fused2; p.hop = sp->hop; p.hist_len = sp->hist_len; p.partitions = sp->partitions; p.n_pairs = sp->n_pairs;
    p.ola_h = sp->ola_h; p.cmac_group = sp->cmac_group; p.fwd_one_pair = sp->fwd_one_pair; p.herm_ok = sp->herm_ok; p.lw_mode = sp->lw_mode;
    return p;
}
static awp::Knob env_knob(const char *name) {
    awp::Knob k;
    if (const char *e = getenv(name)) { k.set = true; k.value = atoi(e); }
    return k;
}

aw_status aw_spatializer_create(aw_context *ctx, const aw_hrir *hrir, int32_t n_in, const int32_t *left_track,
                                const int32_t *right_track, int32_t n_streams, int32_t block_hint,
                                aw_spatializer **out) try {
    (void)block_hint;
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!ctx || !hrir || !left_track || !right_track) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_in <= 0 || n_streams <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "channel and stream counts must be positive");
    // the per-speaker loop of activatePreset: skip unmapped, bounds-check, need >= 1 renderer
    int mapped = 0;
    for (int c = 0; c < n_in; ++c) {
        const int l = left_track[c], r = right_track[c];
        if (l < 0 || r < 0) continue;                                        // HRIRManager.swift:370-372
        if (l >= hrir->n_tracks || r >= hrir->n_tracks)                      // :375-379
            return fail(AW_ERR_INVALID_CHANNEL_MAPPING,
                        "HRIR indices (" + std::to_string(l) + ", " + std::to_string(r) + ") out of range for " +
                            std::to_string(hrir->n_tracks) + " channels");
        ++mapped;
    }
    if (mapped == 0) return fail(AW_ERR_CONVOLUTION_SETUP_FAILED, "No valid renderers created");   // :420-422
    AW_HIP_TRY(hipSetDevice(ctx->device));

    awr::Owner<aw_spatializer> owner(new (std::nothrow) aw_spatializer(), aw_spatializer_destroy);      // destroyed on every early return below
    aw_spatializer *sp = owner.get();
    if (!sp) return fail(AW_ERR_OUT_OF_MEMORY, "spatializer");
    sp->ctx = ctx; sp->n_channels = n_in; sp->n_pairs = (n_in + 1) / 2; sp->n_streams = n_streams;
    sp->taps = hrir->taps;
    sp->sample_rate = hrir->sample_rate;
    // Path choice (host/path_policy.hpp).  Every tuning knob of it is read here, never on the process path; those of the context's
    // LaunchCfg were read at aw_context_create.
    awp::Knobs knobs;
    knobs.window = env_knob("AW_WINDOW");
    knobs.ola = env_knob("AW_OLA");
    knobs.lw = env_knob("AW_LW");
    if (const char *e = getenv("AW_PART_CMAC")) knobs.part_cmac_group = std::strcmp(e, "group") == 0;
    knobs.part_fwd = env_knob("AW_PART_FWD");
    knobs.part_herm = env_knob("AW_PART_HERM");
    knobs.hop_align = ctx->cfg.hop_align;
    knobs.ola_min_blocks_per_wg = ctx->cfg.ola_min_blocks_per_wg;
    const awp::CreatePlan plan = awp::plan_create(sp_layout(sp), knobs, awk::fused_ola_rows(n_in, hrir->taps));
    sp->path = plan.path; sp->fused2 = plan.fused2;
    sp->hop = plan.hop; sp->hist_len = plan.hist_len; sp->partitions = plan.partitions; sp->n_pairs = plan.n_pairs;
    sp->ola_h = plan.ola_h;
    sp->cmac_group = plan.cmac_group; sp->fwd_one_pair = plan.fwd_one_pair; sp->herm_ok = plan.herm_ok;
    sp->lw_mode = plan.lw_mode;
    // Long calls may run on the long-window kernels (device/tile_lw.hpp) whatever the path above — chosen per call, see awp::lw_choose();
    // they use the same history buffer.
    sp->lw_plans.reserve(kLwPlanSlots);                                                  // one entry per window length: pointers into it stay valid (static_assert at kLwPlanSlots)
    // scratch budget per stream chunk: of the partitioned kernels and of the long-window ones, which also serve path-0 layouts
    if (const char *e = getenv("AW_SPEC_SCRATCH_MB")) sp->scratch_budget = (size_t)atoll(e) << 20;
    if (sp->lw_mode != 0) {
        sp->lw_tracks = hrir->tracks; sp->lw_n_tracks = hrir->n_tracks;
        sp->lw_left.assign(left_track, left_track + n_in); sp->lw_right.assign(right_track, right_track + n_in);
        if (n_in > 8) {                  // 32 floats for the wide split kernel's padded copy of a call's very last frame (tile_lw.hpp)
            hipError_t et = sp->d_tail.alloc(32, nullptr);
            if (et == hipSuccess) et = hipMemsetAsync(sp->d_tail.get(), 0, 32 * sizeof(float), ctx->stream);
            if (et != hipSuccess) return awr::hip_fail(et, "spatializer setup");
        }
    }
    // The tables of the short-call kernels (fused tiles, partitioned delay line) are built in float64 on the host, the analogue of the
    // partition FFTs of ConvolutionEngine.init (ConvolutionEngine.swift:141-175) — the partitions of a long HRIR side by side, one host
    // thread each (round 5; cfg 3: 8 partitions x 4 pairs of 8192-point transforms, 48 ms on one thread).  Nothing throws across the ABI.
    std::vector<awk::cf2> all;
    bool tables_ok = true;
    try {
        if (sp->fused2) {
            std::vector<awk::cf4> t4;
            tables_ok = awh::build_poly_tables(hrir->tracks.data(), hrir->n_tracks, hrir->taps, n_in, left_track, right_track, t4);
            all.resize(t4.size() * 2);
            std::memcpy(all.data(), t4.data(), t4.size() * sizeof(awk::cf4));
            all.resize(all.size() + 2 * (size_t)awk::kN, awk::cf2{awk::mk(0.f, 0.f), awk::mk(0.f, 0.f)});   // the zero pair
        } else {
            const int P = sp->partitions;
            std::vector<std::vector<awk::cf2>> tabs((size_t)P);
            tables_ok = awh::parallel_for(P, [&](int q) {
                const int off = sp->path == 0 ? 0 : q * sp->hop;
                const int cnt = sp->path == 0 ? hrir->taps : sp->hop;
                if (!awh::build_pair_tables(hrir->tracks.data(), hrir->n_tracks, hrir->taps, n_in, left_track, right_track, off, cnt, tabs[(size_t)q],
                                            /*pair_threads=*/P == 1))
                    throw std::bad_alloc();
            });
            for (int q = 0; q < P && tables_ok; ++q) all.insert(all.end(), tabs[(size_t)q].begin(), tabs[(size_t)q].end());
            // fused path: one all-zero pair after the last one — a phantom pair (odd pair count in the runtime-loop
            // kernels; stray lanes of non-float4 frames) multiplies it and contributes nothing
            if (sp->path == 0) all.resize(all.size() + awk::kN, awk::cf2{awk::mk(0.f, 0.f), awk::mk(0.f, 0.f)});
        }
    } catch (...) {
        tables_ok = false;
    }
    if (!tables_ok) return fail(AW_ERR_OUT_OF_MEMORY, "filter tables: host memory");
    hipError_t e = sp->d_tab.upload(all.data(), all.size(), nullptr, nullptr);
    if (e != hipSuccess) return awr::hip_fail(e, "filter tables");
    aw_status st = sp_alloc_hist(sp);
    if (st != AW_OK) return st;
    e = sp->k0.create();
    if (e == hipSuccess) e = sp->k1.create();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return awr::hip_fail(e, "spatializer setup");
    *out = owner.release();
    return AW_OK;
} AW_NOEXCEPT_TAIL

void aw_spatializer_destroy(aw_spatializer *sp) {
    if (!sp) return;
    (void)hipSetDevice(sp->ctx->device);
    (void)hipStreamSynchronize(sp->ctx->stream);
    for (auto &pr : sp->pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto &r : sp->stage_pending) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto ev : sp->event_pool) (void)hipEventDestroy(ev);
    delete sp;          // (every buffer and the two named events: their owners' destructors)
}

int32_t aw_spatializer_stream_count(const aw_spatializer *sp) { return sp ? sp->n_streams : 0; }
int32_t aw_spatializer_channel_count(const aw_spatializer *sp) { return sp ? sp->n_channels : 0; }
int64_t aw_spatializer_info(const aw_spatializer *sp, int32_t what) {
    if (!sp) return -1;
    switch (what) {
        case 0: return sp->fused2 ? awk::kN2 : awk::kN;
        case 1: return sp->hop;
        case 2: return sp->partitions;
        case 3: return sp->path;
        case 4: return sp->hist_len;
        case 5: return sp->dominant_frames;   // output frames covered by the launch aw_spatializer_kernel_time() times (last call)
        case 7: return sp->last_lw_R;         // long-window path: rows R of the last call's windows (N = R x 4096); 0 = the partitioned kernels ran
        case 8: return sp->last_lw_R2;        // rows of the last call's remainder window when it ran as two groups of windows (0: one group)
        case 9: return (int64_t)sp->lw_plans.size();   // long-window table sets built so far (one per window length; reserve builds those of its plan)
        case 6: return (int64_t)(sp->ctx->d_pool.bytes() + sp->d_stage_in.bytes() + sp->d_stage_out.bytes() + sp->lim.d_y.bytes() + sp->d_pcm_in.bytes() + sp->d_pcm_out.bytes());   // grow-only device buffers, bytes (the context's scratch pool + this handle's staging)
        case 10: return sp->reserve_tables_us;    // last aw_spatializer_reserve: float64 table build on host threads, microseconds
        case 11: return sp->reserve_upload_us;    //   table upload (hipMalloc + hipMemcpy)
        case 12: return sp->reserve_scratch_us;   //   scratch pool growth (hipMalloc)
        case 13: return sp->ctx->device_allocs;   // device / pinned allocations made so far on behalf of this context's handles
        case 14: return sp->ctx->sync_copies;     // blocking host-to-device table uploads likewise
        case 15: return sp->host_chunk_streams;   // streams per staged chunk of the host entry (0: the whole batch in one piece)
        case 16: return sp->last_ola_h;           // rows H of the overlap-add blocks (512 H frames) the last call ran on; 0: it ran another tile
        case 17: return sp->ola_h;                // rows H this spatializer's long-enough calls use (0: the overlap-add tile is not used)
        case 18: return (int64_t)sp->position;    // frames processed since create / the last reset (the dither's frame position)
        case 19: return sp->lv.metering ? 1 : 0;  // the level meter is on (aw_spatializer_set_metering)
        case 20: return sp->lv.gain_mode;         // aw_gain_mode of the batch entries (aw_spatializer_set_gain)
        case 21: return sp->ld.on ? 1 : 0;        // the loudness measurement is on (aw_spatializer_set_loudness)
        case 22: return sp->tp.on ? 1 : 0;        // the true-peak measurement is on (aw_spatializer_set_true_peak)
        case 23: return sp->lim.on ? 1 : 0;       // the limiter is on (aw_spatializer_set_limiter)
        case 24: return sp->lim.on ? awlim::delay(sp->lim.attack) : 0;      // its latency in frames
        case 25: return sp->eq.n_presets;         // presets the equalizer stage holds (aw_spatializer_set_equalizer / _set_equalizer_target); 0 and no fade: the stage is off
        case 26: return sp->eq.kmax;              // the largest enabled-filter count among them
        case 27: return sp->eq.clock.fading ? sp->eq.clock.length - sp->eq.clock.frame : 0;      // frames left of the running fade (aw_spatializer_set_equalizer_target)
        case 28: return sp->eq.clock.pending ? 1 : 0;                                            // a target is published and has not begun
        default: return -1;
    }
}

static void sp_drain_stages(aw_spatializer *sp);

aw_status aw_spatializer_set_profiling(aw_spatializer *sp, int32_t enabled) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    sp->profiling = enabled != 0;
    sp->kernel_ms_sum = 0.0;
    sp->kernel_launches = 0;
    sp_drain_stages(sp);
    sp->stage_stats.clear();
    return AW_OK;
} AW_NOEXCEPT_TAIL

static hipEvent_t sp_get_event(aw_spatializer *sp) {
    if (!sp->event_pool.empty()) {
        hipEvent_t e = sp->event_pool.back();
        sp->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// HIP events around single launches on the context stream; drained into per-name sums by sp_drain_stages().
struct SpStageTimer final : awk::StageTimer {
    aw_spatializer *sp;
    hipEvent_t cur = nullptr;
    explicit SpStageTimer(aw_spatializer *s) : sp(s) {}
    void begin() override { cur = sp_get_event(sp); (void)hipEventRecord(cur, sp->ctx->stream); }
    void end(const char *name) override {
        hipEvent_t e1 = sp_get_event(sp);
        (void)hipEventRecord(e1, sp->ctx->stream);
        sp->stage_pending.push_back({name, cur, e1});
        cur = nullptr;
    }
};

static void sp_drain_stages(aw_spatializer *sp) {
    for (auto &r : sp->stage_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
            auto it = std::find_if(sp->stage_stats.begin(), sp->stage_stats.end(), [&](const aw_spatializer::StageStat &s) { return std::strcmp(s.name, r.name) == 0; });
            if (it == sp->stage_stats.end()) sp->stage_stats.push_back({r.name, ms, 1});
            else { it->ms_sum += ms; it->launches += 1; }
        }
        sp->event_pool.push_back(r.e0);
        sp->event_pool.push_back(r.e1);
    }
    sp->stage_pending.clear();
}

int32_t aw_spatializer_stage_time(aw_spatializer *sp, int32_t index, const char **name, double *total_ms, int32_t *launches) {
    if (!sp || index < 0) return 0;
    sp_drain_stages(sp);
    if ((size_t)index >= sp->stage_stats.size()) return 0;
    const auto &s = sp->stage_stats[(size_t)index];
    if (name) *name = s.name;
    if (total_ms) *total_ms = s.ms_sum;
    if (launches) *launches = s.launches;
    return 1;
}

int32_t aw_spatializer_kernel_time(aw_spatializer *sp, double *avg_ms, const char **kernel_name) {
    if (!sp) return 0;
    for (auto &pr : sp->pending) {
        float ms = 0.f;
        if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
            sp->kernel_ms_sum += ms;
            sp->kernel_launches += 1;
        }
        sp->event_pool.push_back(pr.first);
        sp->event_pool.push_back(pr.second);
    }
    sp->pending.clear();
    if (avg_ms) *avg_ms = sp->kernel_launches ? sp->kernel_ms_sum / sp->kernel_launches : 0.0;
    if (kernel_name) *kernel_name = sp->last_lw_R ? "aw_lw_split_kernel + aw_lw_rows_kernel + aw_lw_merge_kernel" : sp->path == 0 ? (sp->fused2 ? awk::fused_ols2_kernel_name(sp->n_channels) : sp->last_ola_h ? awk::fused_ola_kernel_name(sp->n_channels, sp->last_ola_h) : awk::fused_ols_kernel_name(sp->n_channels)) : (sp->cmac_group ? "aw_part_forward_kernel + aw_part_cmac_kernel + aw_part_inverse_kernel" : "aw_part_forward_kernel + aw_part_march_kernel + aw_part_inverse_kernel");
    const int n = sp->kernel_launches;
    sp->kernel_ms_sum = 0.0;
    sp->kernel_launches = 0;
    return n;
}

aw_status aw_spatializer_debug_stamps(aw_spatializer *sp, uint64_t *host_out, int64_t capacity_words,
                                      int64_t *n_workgroups) try {
    if (!sp || !host_out || !n_workgroups) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
#if defined(AW_STAMPS) && AW_STAMPS
    const int64_t words = (int64_t)sp->dbg_nwg * awk::kStamps;
    if (!sp->d_dbg || words <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "no launch recorded");
    if (capacity_words < words) return fail(AW_ERR_INVALID_ARGUMENT, "capacity too small");
    AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));
    AW_HIP_TRY(hipMemcpy(host_out, sp->d_dbg.get(), (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_workgroups = sp->dbg_nwg;
    return AW_OK;
#else
    (void)capacity_words;
    *n_workgroups = 0;
    return fail(AW_ERR_INVALID_ARGUMENT, "library not built with AW_STAMPS");
#endif
} AW_NOEXCEPT_TAIL

// What the fused and the partitioned launches share, for the streams of the spatializer from `first_stream` on (`in` / `out` at its frames).
static awk::TileParams sp_tile_params(const aw_spatializer *sp, long long first_stream, const float *in, float *out, int64_t frames) {
    const awk::LaunchCfg &c = sp->ctx->cfg;
    awk::TileParams p{};
    p.in = in; p.out = out; p.hist = sp->d_hist[sp->hist_cur].get() + (size_t)first_stream * sp->hist_len * sp->n_channels;
    p.tab = sp->d_tab.get(); p.tw1 = sp->ctx->d_tw1.get(); p.twa = sp->ctx->d_twa.get(); p.twb = sp->ctx->d_twb.get(); p.zeros = sp->ctx->d_zeros.get();
    p.frames = frames; p.n_channels = sp->n_channels; p.n_pairs = sp->n_pairs;
    p.hop = sp->hop; p.hist_len = sp->hist_len; p.tiles_per_stream = (int)((frames + sp->hop - 1) / sp->hop);
    p.persistent_wgs = c.persistent_wgs; p.wide_two_pass = c.wide_two_pass; p.debug_occupancy = c.debug_occupancy;
    return p;
}

// The timed unit of the chunked paths is the whole pipeline of one stream chunk: an event pair around its launches (kernel_time) and
// the timer its launchers stamp every kernel with (stage_times).  Both do nothing while profiling is off.
struct SpChunkTimer {
    aw_spatializer *sp; hipEvent_t e0 = nullptr, e1 = nullptr; SpStageTimer tm;
    explicit SpChunkTimer(aw_spatializer *s) : sp(s), tm(s) {}
    awk::StageTimer *stages() { return sp->profiling ? &tm : nullptr; }
    hipError_t begin() {
        if (sp->profiling) { e0 = sp_get_event(sp); e1 = sp_get_event(sp); }
        return sp->profiling ? hipEventRecord(e0, sp->ctx->stream) : hipSuccess;
    }
    hipError_t end() {
        const hipError_t e = sp->profiling ? hipEventRecord(e1, sp->ctx->stream) : hipSuccess;
        if (sp->profiling && e == hipSuccess) sp->pending.emplace_back(e0, e1);
        return e;
    }
};

// Every sp_process_* below runs ONE call's kernels for the streams [s_base, s_base + ns_total) of the spatializer; `in` / `out` point at
// stream s_base's frames (the caller's whole batch with s_base = 0, or one staged chunk of the host-entry pipeline).
static aw_status sp_process_fused(aw_spatializer *sp, int s_base, int ns_total, const float *in, float *out, int64_t frames) {
    awk::TileParams p = sp_tile_params(sp, s_base, in, out, frames);
    p.stamp_thread = sp->ctx->cfg.stamp_thread;
#if defined(AW_STAMPS) && AW_STAMPS
    {
        const long long nwg = (long long)ns_total * p.tiles_per_stream;
        const size_t need = (size_t)nwg * awk::kStamps;
        const aw_status st = grow_buf(sp, &sp->d_dbg, need);
        if (st != AW_OK) return st;
        AW_HIP_TRY(hipMemsetAsync(sp->d_dbg.get(), 0, need * sizeof(unsigned long long), sp->ctx->stream));
        sp->dbg_nwg = nwg;
        p.dbg = sp->d_dbg.get();
    }
#endif
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (sp->profiling) { e0 = sp_get_event(sp); e1 = sp_get_event(sp); }
    long long dom_tiles = 0;
    sp->last_ola_h = 0;
    // Overlap-add tile where the call has the blocks for it (the CALL's block count — every stream of the spatializer — not this chunk's:
    // the staged chunks of a host-entry call run the very tile the device entry runs on the whole batch, so both entries give the same
    // bits); else the overlap-save tile on the same tables and history.
    if (awp::use_ola_tile(sp_plan(sp), sp_layout(sp), frames, sp->ctx->cfg.persistent_wgs, sp->ctx->cfg.ola_min_blocks_per_wg)) {
        const int hop_ola = 512 * sp->ola_h;
        p.hop = hop_ola;
        p.tiles_per_stream = (int)((frames + hop_ola - 1) / hop_ola);
        AW_HIP_TRY(awk::launch_fused_ola(p, sp->ola_h, ns_total, sp->ctx->stream, e0, e1));
        sp->last_ola_h = sp->ola_h;
        sp->dominant_frames = (long long)ns_total * frames;              // one launch covers the whole call
        if (sp->profiling) sp->pending.emplace_back(e0, e1);
        return AW_OK;
    }
    if (sp->fused2) AW_HIP_TRY(awk::launch_fused_ols2(p, ns_total, sp->ctx->stream, e0, e1, &dom_tiles));
    else AW_HIP_TRY(awk::launch_fused_ols(p, ns_total, sp->ctx->stream, e0, e1, &dom_tiles));
    // output frames the timed launch produced (tiles x hop, the last tile of a stream may be short)
    sp->dominant_frames = std::min<long long>(dom_tiles * (long long)sp->hop, (long long)ns_total * frames);
    if (sp->profiling) sp->pending.emplace_back(e0, e1);
    return AW_OK;
}

// The scratch of the partitioned and the long-window kernels is the CONTEXT's pool (runtime.hpp): grow-only, the largest need of any
// spatializer created on the context; aw_spatializer_reserve() sizes it ahead of time so that process never allocates.  What a call needs
// and its streams per chunk: host/scratch_plan.hpp.  Budget: AW_SPEC_SCRATCH_MB (read at create), else of the memory free when first needed.
static size_t sp_scratch_budget(aw_spatializer *sp) {
    size_t free_b = 0, total_b = 0;
    if (sp->scratch_budget == 0) {
        const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
        sp->scratch_budget = awp::default_budget(known, free_b);
    }
    return sp->scratch_budget;
}
static aw_status sp_ensure_scratch(aw_spatializer *sp, size_t need) { return sp->ctx->d_pool.capacity() >= need ? AW_OK : pool_grow(sp->ctx, need); }
// the buffer a call inside what aw_spatializer_reserve() sized may count on (its stream chunk is clamped to it: never a reallocation)
static size_t sp_held_scratch(const aw_spatializer *sp, int64_t frames) { return frames <= sp->reserved_frames ? sp->ctx->d_pool.capacity() : 0; }

static aw_status sp_process_partitioned(aw_spatializer *sp, int s_base, int ns_total, const float *in, float *out, int64_t frames) {
    const awp::PartScratch pl = awp::part_scratch(sp_layout(sp), sp_plan(sp), frames, sp_scratch_budget(sp), sp_held_scratch(sp, frames));
    aw_status st = sp_ensure_scratch(sp, pl.need);
    if (st != AW_OK) return st;
    awk::cf *const d_spec = sp->ctx->d_pool.get();
    sp->dominant_frames = 0;
    for (long long s0 = 0; s0 < ns_total; s0 += pl.chunk) {
        const int ns = (int)std::min<long long>(pl.chunk, ns_total - s0);
        awk::TileParams p = sp_tile_params(sp, s_base + s0, in + (size_t)s0 * frames * sp->n_channels, out + (size_t)s0 * frames * 2, frames);
        p.spec = d_spec; p.wspec = d_spec + pl.wspec_at();
        p.partitions = sp->partitions; p.n_blocks = pl.n_blocks; p.first_valid = awk::kN - sp->hop;
        p.fwd_one_pair = sp->fwd_one_pair ? 1 : 0;
        p.herm_last = (!sp->cmac_group && sp->herm_ok && (sp->n_channels & 1)) ? 1 : 0;
        SpChunkTimer timer(sp);          // (the three-kernel pipeline of one stream chunk)
        AW_HIP_TRY(timer.begin());
        AW_HIP_TRY(awk::launch_part_forward(p, ns, sp->ctx->stream, timer.stages()));
        if (sp->cmac_group) AW_HIP_TRY(awk::launch_part_cmac(p, ns, sp->ctx->stream, timer.stages()));
        else AW_HIP_TRY(awk::launch_part_march(p, ns, sp->ctx->stream, timer.stages()));
        AW_HIP_TRY(awk::launch_part_inverse(p, ns, sp->ctx->stream, timer.stages()));
        AW_HIP_TRY(timer.end());
        sp->dominant_frames = (long long)ns * frames;
    }
    return AW_OK;
}

/* ---- long-window path (device/tile_lw.hpp) ---------------------------------------------------- */
// Per call: windows of N = R x 4096 frames (R = 8 RA rows), hop = N - hist_len; hist_len is the history the spatializer's
// other kernel set keeps too (path 1: P x 4096 >= taps; path 0: the fused window minus its hop, any value >= taps - 1), so both kernel
// sets serve the same spatializer and the choice is free per call.
// The choice is awp::lw_choose (host/path_policy.hpp) over these inputs.
using awp::LwCallPlan;
using awp::LwGroup;
static_assert(awp::kLwRowChoiceCount <= (int)kLwPlanSlots, "aw_spatializer::lw_plans holds one table set per window length and never reallocates (sp_process_longwin keeps pointers into it)");
static awp::LwInputs lw_inputs(const aw_spatializer *sp) {
    awp::LwInputs in{sp_layout(sp), sp_plan(sp), sp->ctx->cfg.cus, sp->reserved_frames, 0u};
    for (int i = 0; i < awp::kLwRowChoiceCount; ++i)
        for (const auto &pl : sp->lw_plans)
            if (pl.R == awp::kLwRowChoices[i]) in.have |= 1u << i;
    return in;
}

static aw_status lw_get_plan(aw_spatializer *sp, int R, const aw_spatializer::LwPlan **out) {
    for (const auto &pl : sp->lw_plans)
        if (pl.R == R) { *out = &pl; return AW_OK; }
    awh::LwTables t;
    const int form = sp->ctx->cfg.lw_rows_form;          // which rows kernel the tables are laid out for (read once per context)
    // The filter tables of the 16-point rows kernel are computed ON THE DEVICE (device/prep_kernels.hip: float64, the analogue of the
    // partition FFTs of ConvolutionEngine.init, ConvolutionEngine.swift:141-175); the host builds only the small twiddle tables then.
    // AW_LW_TABLES=host (read at context creation) or the 8-point kernel forms: the float64 host builder computes everything.
    const bool on_gpu = form == 16 && sp->ctx->cfg.lw_tables_on_gpu != 0;
    const auto t_build = std::chrono::steady_clock::now();
    if (!awh::build_lw_tables(sp->lw_tracks.data(), sp->lw_n_tracks, sp->taps, sp->n_channels, sp->lw_left.data(), sp->lw_right.data(), R, t, form, /*filters=*/!on_gpu))
        return fail(AW_ERR_OUT_OF_MEMORY, "long-window tables: host memory");      // (the caller falls back to the kernels that have always served the spatializer)
    auto t_up = std::chrono::steady_clock::now();
    sp->reserve_tables_us += std::chrono::duration_cast<std::chrono::microseconds>(t_up - t_build).count();
    aw_spatializer::LwPlan pl;
    pl.R = R;
    awr::Counter *const allocs = &sp->ctx->device_allocs, *const copies = &sp->ctx->sync_copies;
    auto up = [&](auto &buf, const auto &host) { return buf.upload(host.data(), host.size(), allocs, copies); };
    hipError_t e = hipSuccess;
    if (on_gpu) {
        const int n_pairs = (sp->n_channels + 1) / 2;
        if (!sp->d_lw_tracks || !sp->d_lw_left || !sp->d_lw_right) {     // the impulse responses and the channel map, once per spatializer
            // all three or none: a failure part way (out of memory) frees what was uploaded, so that the next long call uploads again
            // instead of handing the prep kernel a null or never-written channel map (round-5 advice)
            e = up(sp->d_lw_tracks, sp->lw_tracks);
            if (e == hipSuccess) e = up(sp->d_lw_left, sp->lw_left);
            if (e == hipSuccess) e = up(sp->d_lw_right, sp->lw_right);
            if (e != hipSuccess) { (void)sp->d_lw_tracks.reset(); (void)sp->d_lw_left.reset(); (void)sp->d_lw_right.reset(); }
        }
        awr::Buf<unsigned char> d_tmp;
        if (e == hipSuccess) e = pl.d_tab16.alloc((size_t)(R / 2) * n_pairs * 2 * awk::kLwM, nullptr);
        if (e == hipSuccess) e = d_tmp.alloc(awk::lw_prep_scratch_bytes(sp->n_channels, R), nullptr);
        if (e == hipSuccess) {
            sp->ctx->device_allocs += 2;          // (the two above, counted once both are there)
            e = awk::launch_lw_prep(sp->d_lw_tracks.get(), sp->lw_n_tracks, sp->taps, sp->n_channels, sp->d_lw_left.get(), sp->d_lw_right.get(), R, d_tmp.get(), pl.d_tab16.get(), sp->ctx->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(sp->ctx->stream);
        (void)d_tmp.reset();
        const auto t_gpu = std::chrono::steady_clock::now();
        sp->reserve_tables_us += std::chrono::duration_cast<std::chrono::microseconds>(t_gpu - t_up).count();
        t_up = t_gpu;
        if (e == hipSuccess) e = up(pl.d_tw2, t.tw2);
    } else if (form == 16) {
        e = up(pl.d_tab16, t.tab16);
        if (e == hipSuccess) e = up(pl.d_tw2, t.tw2);
    } else {
        e = up(pl.d_tab, t.tab);
    }
    if (e == hipSuccess) e = up(pl.d_coarse, t.coarse);
    if (e == hipSuccess) e = up(pl.d_fine, t.fine);
    if (e == hipSuccess) e = up(pl.d_step, t.step);
    if (e == hipSuccess) e = up(pl.d_tw_r, t.tw_r);
    if (e == hipSuccess) e = up(pl.d_tw1m, t.tw1m);
    // nothing half-built stays behind (pl goes out of scope): the next call tries again (or takes the partitioned kernels)
    if (e != hipSuccess) return awr::hip_fail(e, "long-window tables");
    sp->reserve_upload_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_up).count();
    sp->lw_plans.push_back(std::move(pl));
    *out = &sp->lw_plans.back();
    return AW_OK;
}

static aw_status sp_process_longwin(aw_spatializer *sp, const LwCallPlan &call, int s_base, int ns_total, const float *in, float *out, int64_t frames) {
    const aw_spatializer::LwPlan *tables[2] = {nullptr, nullptr};
    for (int i = 0; i < call.n_groups; ++i) {
        aw_status st = lw_get_plan(sp, call.g[i].R, &tables[i]);
        if (st != AW_OK) return st;
    }
    const auto sc = awp::lw_plan_scratch(sp_layout(sp), call, sp_scratch_budget(sp), sp_held_scratch(sp, frames));
    aw_status st = sp_ensure_scratch(sp, sc.need);
    if (st != AW_OK) return st;
    awk::cf *const d_spec = sp->ctx->d_pool.get();
    sp->dominant_frames = 0;
    for (long long s0 = 0; s0 < ns_total; s0 += sc.chunk) {
        const int ns = (int)std::min<long long>(sc.chunk, ns_total - s0);
        SpChunkTimer timer(sp);
        AW_HIP_TRY(timer.begin());
        if (sp->n_channels > 8)          // the wide split kernel reads the last frame of the last stream from a padded copy (allocated at create)
            AW_HIP_TRY(hipMemcpyAsync(sp->d_tail.get(), in + ((size_t)(s0 + ns) * frames - 1) * sp->n_channels, sp->n_channels * sizeof(float),
                                      hipMemcpyDefault, sp->ctx->stream));          // (`in` is device memory, or the page-locked staging of a one-stream call)
        for (int gi = 0; gi < call.n_groups; ++gi) {
            const LwGroup &g = call.g[gi];
            const aw_spatializer::LwPlan *plan = tables[gi];
            const long long N = (long long)g.R * awk::kLwM;
            awk::LwParams p{};
            p.in = in + (size_t)s0 * frames * sp->n_channels; p.out = out + (size_t)s0 * frames * 2;
            p.hist = sp->d_hist[sp->hist_cur].get() + (size_t)(s_base + s0) * sp->hist_len * sp->n_channels;
            // the tail carry rides along in the split kernel of the LAST group: its last window spans the last hist_len frames of the call
            p.hist_out = gi == call.n_groups - 1 ? sp->d_hist[sp->hist_cur ^ 1].get() + (size_t)(s_base + s0) * sp->hist_len * sp->n_channels : nullptr;
            p.zeros = sp->ctx->d_zeros.get();
            p.frames = frames; p.frame0 = g.frame0; p.frame_end = g.frame_end;
            p.n_channels = sp->n_channels; p.n_pairs = (sp->n_channels + 1) / 2; p.real_last = sp->n_channels & 1;
            p.hist_len = sp->hist_len; p.hop = (int)(N - sp->hist_len); p.n_windows = g.n_windows;
            p.R = g.R; p.N = (int)N;
            p.spec = d_spec; p.spec_per_sw = sc.g[gi].spec_per_sw;
            p.wrows = d_spec + sc.g[gi].wrows_at(sc.chunk);
            p.tab = plan->d_tab.get(); p.tw_coarse = plan->d_coarse.get(); p.tw_fine = plan->d_fine.get(); p.tw_step = plan->d_step.get(); p.tw_r = plan->d_tw_r.get(); p.tw1m = plan->d_tw1m.get();
            p.twa = sp->ctx->d_twa.get(); p.twb = sp->ctx->d_twb.get();
            p.persistent_wgs = sp->ctx->cfg.persistent_wgs;
            p.rows_pairs_per_batch = sp->ctx->cfg.lw_rows_pb;
            p.rows_form = plan->d_tab16 ? 16 : 8; p.tab16 = plan->d_tab16.get(); p.tw2 = plan->d_tw2.get(); p.rows16_wgs = sp->ctx->cfg.lw_rows16_wgs;
            p.n_streams = ns;
            p.tail = sp->n_channels > 8 ? sp->d_tail.get() : nullptr;
            AW_HIP_TRY(awk::launch_lw_split(p, ns, sp->ctx->stream, timer.stages()));
            AW_HIP_TRY(awk::launch_lw_rows(p, ns, sp->ctx->stream, timer.stages()));
            AW_HIP_TRY(awk::launch_lw_merge(p, ns, sp->ctx->stream, timer.stages()));
        }
        AW_HIP_TRY(timer.end());
        sp->dominant_frames = (long long)ns * frames;
    }
    return AW_OK;
}

// Callback-sized calls of a one-stream spatializer take the zero-copy staging (runtime.hpp) when aw_spatializer_reserve has made it;
// longer calls move by DMA (a fused tile reads every input line about twice: not over PCIe).
static constexpr int64_t kZeroCopyFrames = 16384;
static bool sp_zero_copy(const aw_spatializer *sp, int64_t frames) {
    return sp->n_streams == 1 && frames <= kZeroCopyFrames && sp->h_pin_in.capacity() >= (size_t)frames * sp->n_channels && sp->h_pin_out.capacity() >= (size_t)frames * 2;
}

// Sizes every grow-only device buffer for calls of up to max_frames frames, so that the process entries never
// allocate afterwards ("process must not allocate"; creation may block).
aw_status aw_spatializer_reserve(aw_spatializer *sp, int64_t max_frames) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (max_frames <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "max_frames must be positive");
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    sp->reserve_tables_us = sp->reserve_upload_us = sp->reserve_scratch_us = 0;
    const LwCallPlan lw_res = awp::lw_choose(lw_inputs(sp), max_frames, true);
    if (sp->path == 1 || lw_res.n_groups) {
        for (int i = 0; i < lw_res.n_groups; ++i) {
            const aw_spatializer::LwPlan *plan = nullptr;
            aw_status st = lw_get_plan(sp, lw_res.g[i].R, &plan);
            if (st != AW_OK) return st;
        }
        // From here on a call of up to max_frames frames chooses only among the window lengths whose tables exist (lw_choose).
        const int64_t reserved_before = sp->reserved_frames;
        sp->reserved_frames = std::max<int64_t>(sp->reserved_frames, max_frames);
        const size_t need = awp::reserve_need(lw_inputs(sp), lw_res, sp->reserved_frames, sp_scratch_budget(sp)).need;
        const auto t0 = std::chrono::steady_clock::now();
        aw_status st = sp_ensure_scratch(sp, need);
        if (st == AW_OK) {
            const hipError_t es = hipStreamSynchronize(sp->ctx->stream);
            if (es != hipSuccess) st = awr::hip_fail(es, "hipStreamSynchronize (reserve)");
        }
        sp->reserve_scratch_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        if (st != AW_OK) { sp->reserved_frames = reserved_before; return st; }
        sp->reserved_pool = std::max(sp->reserved_pool, need);
    }
    if (sp->n_streams == 1) {       // plug-in shaped use (host / planar entries): their staging buffers too
        const size_t n = (size_t)max_frames * std::max(sp->n_channels, 4);
        aw_status st = grow_buf(sp, &sp->d_stage_in, n);
        if (st == AW_OK) st = grow_buf(sp, &sp->d_stage_out, (size_t)max_frames * 4);
        // callback-sized calls: page-locked staging the kernels address directly
        const size_t zf = (size_t)std::min<int64_t>(max_frames, kZeroCopyFrames);
        if (st == AW_OK) st = grow_buf(sp, &sp->h_pin_in, zf * sp->n_channels);
        if (st == AW_OK) st = grow_buf(sp, &sp->h_pin_out, zf * 2);
        if (st != AW_OK) return st;
    }
    sp->reserved_frames = std::max<int64_t>(sp->reserved_frames, max_frames);
    if (sp->lim.on) {              // the float32 staging in front of the limiter: every stream of the longest call
        const aw_status st = grow_buf(sp, &sp->lim.d_y, (size_t)sp->n_streams * (size_t)max_frames * 2);
        if (st != AW_OK) return st;
    }
    return AW_OK;
} AW_NOEXCEPT_TAIL

// One call's launches for the streams [s_base, s_base + ns) (`in` / `out` at stream s_base), history carry included; the caller holds
// the context's launch lock and flips hist_cur once every stream of the call has been through here.
static aw_status sp_run_streams(aw_spatializer *sp, const LwCallPlan &lw, int s_base, int ns, const float *in, float *out, int64_t frames) {
    aw_status st = AW_OK;
    bool lw_ran = false;
    if (lw.n_groups && sp->last_lw_R) {
        st = sp_process_longwin(sp, lw, s_base, ns, in, out, frames);
        lw_ran = st == AW_OK;
        if (st == AW_ERR_OUT_OF_MEMORY) {
            // the long-window kernels are an optimisation: without memory for their tables or scratch the call takes the kernels
            // that have always served this spatializer (nothing has been launched yet: allocation comes first)
            (void)hipGetLastError();
            sp->last_lw_R = 0; sp->last_lw_R2 = 0;
            st = AW_OK;
        }
    }
    if (st == AW_OK && !lw_ran) st = sp->path == 0 ? sp_process_fused(sp, s_base, ns, in, out, frames) : sp_process_partitioned(sp, s_base, ns, in, out, frames);
    if (st != AW_OK) return st;
    // carry the convolution tail: next call's history = last hist_len frames of (history ++ input)
    if (!lw_ran) {    // (the long-window split kernel has written it on the way)
        const size_t off = (size_t)s_base * sp->hist_len * sp->n_channels;
        float *h_old = sp->d_hist[sp->hist_cur].get() + off, *h_new = sp->d_hist[sp->hist_cur ^ 1].get() + off;
        SpStageTimer tm(sp);
        if (sp->profiling) tm.begin();
        AW_HIP_TRY(awk::launch_hist_update(in, h_old, h_new, frames, sp->n_channels, sp->hist_len, ns, sp->ctx->stream));
        if (sp->profiling) tm.end("aw_hist_update_kernel");
    }
    return AW_OK;
}

// Once per call of every process entry: the call's kernel plan, and the frame position moves past the call.  *pos0 (optional) receives
// the position of the call's first frame, which every encode of the call keys its dither on.
static LwCallPlan sp_begin_call(aw_spatializer *sp, int64_t frames, uint64_t *pos0 = nullptr) {
    if (pos0) *pos0 = sp->position;
    sp->position += (uint64_t)frames;
    const LwCallPlan lw = awp::lw_choose(lw_inputs(sp), frames);
    sp->last_lw_R = lw.n_groups ? lw.g[0].R : 0;
    sp->last_lw_R2 = lw.n_groups > 1 ? lw.g[1].R : 0;
    return lw;
}

/* ---- level meter and output gain of the batch entries (aw_spatializer_set_metering / _set_gain; rules: device/levels.hpp) ------------- */
static_assert(AW_GAIN_NONE == awl::kGainNone && AW_GAIN_FIXED == awl::kGainFixed && AW_GAIN_PEAK_CEILING == awl::kGainPeakCeiling, "aw_gain_mode");
static_assert(AW_GAIN_TRUE_PEAK_CEILING == 3, "aw_gain_mode");
static_assert(sizeof(aw_stream_levels) == 56 && sizeof(awl::Record) == 40, "aw_stream_levels");
// Every output stage (levels lv_, loudness ld_, true peak tp_, limiter lim_) answers the same calls: its setter makes its one allocation
// (stage_alloc: never the process path), X_begin_call runs once per call before its first launch, PingPong::end_call flips its history
// after a call that ran, lv_reset zeroes the reset range of each, and `d` (an awr::Buf) frees itself with the handle.  Where its bytes lie: X_layout.
static awst::Levels lv_layout(const aw_spatializer *sp) { return awst::Levels{{(size_t)sp->n_streams}}; }
static aw_status stage_zero(aw_spatializer *sp, void *p, size_t bytes) { AW_HIP_TRY(hipMemsetAsync(p, 0, bytes, sp->ctx->stream)); return AW_OK; }
static aw_status stage_alloc(aw_spatializer *sp, awr::Buf<unsigned char> *d, size_t bytes, size_t zeroed) {       // (the first `zeroed` bytes start as zeros)
    AW_HIP_TRY(d->alloc(bytes, &sp->ctx->device_allocs));
    return zeroed ? stage_zero(sp, d->get(), zeroed) : AW_OK;
}
// a batch call has anything to do here; while this is false every entry launches what it always has
static bool lv_active(const aw_spatializer *sp) { return sp->lv.metering || sp->lv.gain_mode != AW_GAIN_NONE; }
// the levels kernel runs: the meter wants the sums, the automatic gain the call's peaks
static bool lv_measures(const aw_spatializer *sp) { return sp->lv.metering || sp->lv.gain_mode == AW_GAIN_PEAK_CEILING; }
static aw_status lv_buffers(aw_spatializer *sp) { return sp->lv.d ? AW_OK : stage_alloc(sp, &sp->lv.d, lv_layout(sp).total, lv_layout(sp).total); }      // (set_metering(1) / set_gain)

// Once per batch call, before its first launch: what the call applies (aw_stream_levels::gain), the frames it meters, and — where the
// levels kernel runs (device) — the call-local peaks start from zero.
static aw_status lv_begin_call(aw_spatializer *sp, int64_t frames, bool device) {
    if (!lv_active(sp)) { sp->lv.applied_mode = AW_GAIN_NONE; return AW_OK; }
    sp->lv.applied_mode = sp->lv.gain_mode;
    sp->lv.applied_ceiling = sp->lv.gain_ceiling;
    sp->lv.applied_on_host = !device;
    if (sp->lv.gain_mode == AW_GAIN_FIXED) sp->lv.applied_gains = sp->lv.gains;
    if (sp->lv.metering) sp->lv.frames += (uint64_t)frames;
    return device && lv_measures(sp) ? stage_zero(sp, lv_layout(sp).call_peaks.at(sp->lv.d.get()), lv_layout(sp).call_peaks.bytes()) : AW_OK;
}

// the true-peak kernel runs (below): the measurement is on, or the gain wants the call's true peaks
static bool tp_runs(const aw_spatializer *sp) { return sp->tp.on || sp->lv.gain_mode == AW_GAIN_TRUE_PEAK_CEILING; }
static awst::TruePeak tp_layout(const aw_spatializer *sp) { return awst::TruePeak{{(size_t)sp->n_streams}}; }

// AW_GAIN_TRUE_PEAK_CEILING is the kernels' peak-ceiling gain over the call-local TRUE peaks
static awk::PcmGain lv_gain_launch(const aw_spatializer *sp, int64_t s0) {
    const awst::Levels L = lv_layout(sp);
    awk::PcmGain g{sp->lv.gain_mode, sp->lv.gain_ceiling, L.gains.at(sp->lv.d.get(), s0), L.call_peaks.at(sp->lv.d.get(), s0), sp->lv.metering ? L.records.at(sp->lv.d.get(), s0) : nullptr};
    if (sp->lim.on) { g.mode = awl::kGainNone; g.ceiling = 0.0f; }      // (the limiter has applied the fixed gain)
    else if (sp->lv.gain_mode == AW_GAIN_TRUE_PEAK_CEILING) { g.mode = awl::kGainPeakCeiling; g.call_peak = tp_layout(sp).call_peaks.at(sp->tp.d.get(), s0); }
    return g;
}

// After the kernels of the streams [s0, s0 + ns) have written their float32 output to f_out: meter it, and — float32 output with a gain
// set — scale it in place (integer output is gained by its encode).
static aw_status lv_after_run(aw_spatializer *sp, float *f_out, int64_t s0, int ns, int64_t frames, bool float_out) {
    if (!lv_active(sp)) return AW_OK;
    const int64_t n = (int64_t)ns * 2 * frames;
    if (lv_measures(sp)) {
        SpStageTimer tm(sp);
        if (sp->profiling) tm.begin();
        const awst::Levels L = lv_layout(sp);
        AW_HIP_TRY(awk::launch_levels(f_out, n, frames, sp->lv.metering ? L.records.at(sp->lv.d.get(), s0) : nullptr, L.call_peaks.at(sp->lv.d.get(), s0), sp->ctx->stream));
        if (sp->profiling) tm.end("aw_levels_kernel");
    }
    if (float_out && sp->lv.gain_mode != AW_GAIN_NONE) {
        SpStageTimer tm(sp);
        if (sp->profiling) tm.begin();
        AW_HIP_TRY(awk::launch_scale(f_out, n, frames, lv_gain_launch(sp, s0), sp->ctx->stream));
        if (sp->profiling) tm.end("aw_scale_kernel");
    }
    return AW_OK;
}

// The single-stream page-locked path: the same rules on the CPU, over the n = 2 * frames output samples y.  Returns the call's gain.
static float lv_host_call(aw_spatializer *sp, const float *y, size_t n) {
    uint32_t pk[2] = {0u, 0u};
    double en[2] = {0.0, 0.0};
    unsigned nf = 0;
    if (lv_measures(sp)) for (size_t i = 0; i < n; ++i) awl::contribute(y[i], pk[i & 1], en[i & 1], nf);
    aw_spatializer::Levels &lv = sp->lv;
    if (lv.metering) {
        for (int e = 0; e < 2; ++e) {
            lv.host.peak_bits[e] = std::max(lv.host.peak_bits[e], pk[e]);
            lv.host.energy[e] += en[e];
        }
        lv.host.nonfinite += nf;
    }
    float g = 1.0f;
    if (lv.gain_mode == AW_GAIN_FIXED) g = lv.gains[0];
    else if (lv.gain_mode == AW_GAIN_PEAK_CEILING) g = awl::auto_gain(awl::bits_float(std::max(pk[0], pk[1])), lv.gain_ceiling);
    else if (lv.gain_mode == AW_GAIN_TRUE_PEAK_CEILING) g = awl::auto_gain(awl::bits_float(sp->tp.pinned_call_bits), lv.gain_ceiling);
    lv.applied_host_gain = g;
    return g;
}

/* ---- integrated loudness of the batch entries (aw_spatializer_set_loudness; rules: device/loudness.hpp, kernels: device/loudness_scan.hpp) -- */
static_assert(sizeof(aw_stream_loudness) == 56, "aw_stream_loudness");
constexpr size_t kLdTabDoubles = (size_t)awk::kLdFilters * awk::kEqTabDoubles, kLdPlaneDoubles = (size_t)awk::kLdFilters * awh::kEqSectionPlaneDoubles;
static awst::Loudness ld_layout(const aw_spatializer *sp) { return awst::Loudness{{(size_t)sp->n_streams}, (size_t)sp->ld.cap, kLdTabDoubles + kLdPlaneDoubles}; }

static uint64_t ld_begin_call(aw_spatializer *sp, int64_t frames) {      // once per call: the count moves past it -> the frames measured before it (its hop index)
    if (sp->ld.on) sp->ld.frames += (uint64_t)frames;
    return sp->ld.frames - (sp->ld.on ? (uint64_t)frames : 0);
}

// The float32 output y of the streams [s0, s0 + ns) of a call (dense: `frames` apart), before any gain; frame0: frames measured before
// this call.  Chunks of streams are independent (one workgroup owns a stream), so chunking changes no bit.
static aw_status ld_measure(aw_spatializer *sp, const float *y, int64_t s0, int ns, int64_t frames, uint64_t frame0) {
    SpStageTimer tm(sp);
    if (sp->profiling) tm.begin();
    awk::LoudnessParams p{};
    const awst::Loudness L = ld_layout(sp);
    p.z = L.state.at(sp->ld.d.get(), s0); p.hops = L.hops.at(sp->ld.d.get(), s0); p.nonfinite = L.nonfinite.at(sp->ld.d.get(), s0);
    p.tab = L.tables.at(sp->ld.d.get()); p.plane = p.tab + kLdTabDoubles;
    p.in = y; p.frames = frames; p.stride_frames = frames; p.frame0 = (long long)frame0;
    p.hop = sp->ld.hop; p.cap_hops = sp->ld.cap;
    AW_HIP_TRY(awk::launch_loudness(p, ns, sp->ctx->stream));
    if (sp->profiling) tm.end("aw_loudness_kernel");
    return AW_OK;
}

/* ---- equalizer of the batch entries (aw_spatializer_set_equalizer; rules: device/eq_stage.hpp, kernels: device/eq_cascade.hpp) ---- */
static awst::Equalizer eq_layout(const aw_spatializer *sp) {
    return awst::Equalizer{{(size_t)sp->n_streams}, (size_t)sp->eq.n_presets, (size_t)sp->eq.kmax, sp->eq.table_doubles};
}

static awst::EqualizerFade eq_fade_layout(const aw_spatializer *sp) { return awst::EqualizerFade{{(size_t)sp->n_streams}, (size_t)sp->eq.kmax}; }

// every filter state: the active one, which a fade fades from, and the one it fades to (applyPendingReset :341-352); the setting, the
// clock and a published target stay
static aw_status eq_reset(aw_spatializer *sp) {
    const size_t bytes = sp->eq.d ? eq_layout(sp).reset_bytes : 0, to_bytes = sp->eq.fade ? eq_fade_layout(sp).reset_bytes : 0;
    aw_status st = bytes ? stage_zero(sp, sp->eq.d.get(), bytes) : AW_OK;
    if (st == AW_OK && to_bytes) st = stage_zero(sp, sp->eq.fade.get(), to_bytes);
    return st;
}

// once per call that runs the stage, before its first launch: where the clock cuts it.  batch_end moves the clock, once per call
// however many chunks of streams ran the cuts.
static void eq_begin_call(aw_spatializer *sp, int64_t frames) {
    sp->eq.plan = awef::plan(sp->eq.clock, frames);
    sp->eq.planned = true;
}
static void eq_end_call(aw_spatializer *sp) {
    if (!sp->eq.planned) return;
    sp->eq.planned = false;
    aw_spatializer::Equalizer &q = sp->eq;
    for (int i = 0; i < q.plan.n; ++i) {
        const awef::Segment &g = q.plan.seg[i];
        for (size_t s = 0; g.begins && s < q.pending_map.size(); ++s)
            if (q.pending_map[s] != awk::kEqKeep) { q.to_map[s] = q.pending_map[s]; q.pending_map[s] = awk::kEqKeep; }
        for (size_t s = 0; g.ends && s < q.to_map.size(); ++s)
            if (q.to_map[s] != awk::kEqKeep) { q.map[s] = q.to_map[s]; q.to_map[s] = awk::kEqKeep; }
    }
    q.clock = q.plan.after;
}

// The float32 output y of the streams [s0, s0 + ns) of a call (dense: `frames` apart), in place, before any meter: the chunk-parallel
// body over the whole chunks and the sequential tail, the split aw_eq_state_process makes.  A workgroup owns a stream and the state is
// per stream, so chunks of streams are independent.  Where the call's plan cuts it (a fade begins, runs or ends) each piece runs so, as a
// call of its own, the fading pieces through the fade kernels; the two ends of a fade are queued between the pieces like everything else.
static aw_status eq_run(aw_spatializer *sp, float *y, int64_t s0, int ns, int64_t frames) {
    SpStageTimer tm(sp);
    const awst::Equalizer L = eq_layout(sp);
    unsigned char *const d = sp->eq.d.get();
    awk::EqFadeParams f{};
    awk::EqStageParams &p = f.s;
    p.z = L.state.at(d, (size_t)s0); p.map = L.map.at(d, (size_t)s0); p.presets = L.presets.at(d); p.tables = L.tables.at(d);
    p.stride_frames = frames; p.kmax = sp->eq.kmax;
    p.cus = sp->ctx->cfg.cus; p.ear_split = sp->ctx->cfg.eq_ear_split;
    int *to_map = nullptr, *pending_map = nullptr;
    if (sp->eq.fade) {
        const awst::EqualizerFade F = eq_fade_layout(sp);
        unsigned char *const df = sp->eq.fade.get();
        f.z_to = F.state_to.at(df, (size_t)s0); f.to_map = to_map = F.to_map.at(df, (size_t)s0); pending_map = F.pending_map.at(df, (size_t)s0);
        f.length = sp->eq.clock.length;
    }
    const awef::Plan &plan = sp->eq.plan;
    for (int i = 0; i < plan.n; ++i) {
        const awef::Segment &g = plan.seg[i];
        const int64_t body = g.frames - g.frames % awk::kEqChunk;
        if (g.begins) {
            if (sp->profiling) tm.begin();
            AW_HIP_TRY(awk::launch_eq_stage_turn(true, const_cast<int *>(p.map), to_map, pending_map, p.z, f.z_to, p.kmax, ns, sp->ctx->stream));
            if (sp->profiling) tm.end("aw_eq_stage_turn_kernel");
        }
        if (body > 0) {
            if (sp->profiling) tm.begin();
            p.y = y + g.first * 2; p.frames = body; f.t0 = g.t0;
            AW_HIP_TRY(g.fade ? awk::launch_eq_stage_fade(f, ns, sp->ctx->stream) : awk::launch_eq_stage(p, ns, sp->ctx->stream));
            if (sp->profiling) tm.end(g.fade ? "aw_eq_stage_fade_kernel" : "aw_eq_stage_kernel");
        }
        if (g.frames > body) {
            if (sp->profiling) tm.begin();
            p.y = y + (g.first + body) * 2; p.frames = g.frames - body; f.t0 = g.t0 + body;
            AW_HIP_TRY(g.fade ? awk::launch_eq_stage_fade_tail(f, ns, sp->ctx->stream) : awk::launch_eq_stage_tail(p, ns, sp->ctx->stream));
            if (sp->profiling) tm.end(g.fade ? "aw_eq_stage_fade_tail_kernel" : "aw_eq_stage_tail_kernel");
        }
        if (g.ends) {
            if (sp->profiling) tm.begin();
            AW_HIP_TRY(awk::launch_eq_stage_turn(false, const_cast<int *>(p.map), to_map, pending_map, p.z, f.z_to, p.kmax, ns, sp->ctx->stream));
            if (sp->profiling) tm.end("aw_eq_stage_turn_kernel");
        }
    }
    return AW_OK;
}

/* ---- true peak of the batch entries (aw_spatializer_set_true_peak, AW_GAIN_TRUE_PEAK_CEILING; rules: device/truepeak.hpp, kernel:
 * device/truepeak_tile.hpp) ---- */
static_assert(sizeof(aw_stream_true_peak) == 32, "aw_stream_true_peak");
// the interpolator's coefficients, shared with the limiter: whichever setter runs first builds them
static void tp_filter_once(aw_spatializer *sp) { if (!sp->tp_filter_built) { awtp::filter(sp->tp_filter); sp->tp_filter_built = true; } }
// (set_true_peak(1) / set_gain(AW_GAIN_TRUE_PEAK_CEILING) when the kernel did not run before): the allocation, zeroed, and the coefficients.
// Frames of unmeasured calls are not predecessors: where the allocation is there, the kernel starts again behind silence.
static aw_status tp_buffers(aw_spatializer *sp) {
    const awst::TruePeak L = tp_layout(sp);
    tp_filter_once(sp);
    return sp->tp.d ? stage_zero(sp, L.history.at(sp->tp.d.get()), 2 * L.history.bytes()) : stage_alloc(sp, &sp->tp.d, L.total, L.total);
}

// once per call that runs the kernel, before its first launch
static aw_status tp_begin_call(aw_spatializer *sp, int64_t frames) {
    if (sp->tp.on) sp->tp.frames += (uint64_t)frames;
    return stage_zero(sp, tp_layout(sp).call_peaks.at(sp->tp.d.get()), tp_layout(sp).call_peaks.bytes());
}

// The float32 output y of the streams [s0, s0 + ns) of a call (dense: `frames` apart), before any gain.  A workgroup's tile lies in one
// stream and the history is per stream, so chunks of streams are independent.
static aw_status tp_measure(aw_spatializer *sp, const float *y, int64_t s0, int ns, int64_t frames) {
    SpStageTimer tm(sp);
    if (sp->profiling) tm.begin();
    awk::TruePeakParams p{};
    p.in = y; p.frames = frames; p.n_streams = ns;
    const awst::TruePeak L = tp_layout(sp);
    p.hist_in = L.history.at(sp->tp.d.get(), s0, sp->tp.hist.cur);
    p.hist_out = L.history.at(sp->tp.d.get(), s0, sp->tp.hist.cur ^ 1);
    if (sp->tp.on) { p.tp_bits = L.peaks.at(sp->tp.d.get(), s0); p.nonfinite = L.nonfinite.at(sp->tp.d.get(), s0); }
    p.call_tp = L.call_peaks.at(sp->tp.d.get(), s0);
    std::memcpy(p.c, sp->tp_filter, sizeof(p.c));
    AW_HIP_TRY(awk::launch_truepeak(p, sp->ctx->stream));
    sp->tp.hist.ran = true;
    if (sp->profiling) tm.end("aw_true_peak_kernel");
    return AW_OK;
}

/* ---- look-ahead true-peak limiter of the batch entries (aw_spatializer_set_limiter; rules: device/limiter.hpp, kernel:
 * device/limiter_tile.hpp) ---- */
static_assert(sizeof(aw_stream_limiter) == 32, "aw_stream_limiter");
static awst::Limiter lim_layout(const aw_spatializer *sp) { return awst::Limiter{{(size_t)sp->n_streams}, sp->lim.attack, sp->lim.hold}; }

// records (a reset, a new allocation): the records start over — no frame limited, a lowest gain of 1.  Always (those, and off -> on): the
// history starts over behind silence, on the device and for the single-stream path.
static aw_status lim_reset(aw_spatializer *sp, bool records) {
    const awst::Limiter L = lim_layout(sp);
    if (records) {
        sp->lim.frames = 0;
        sp->lim.host = awlim::Record{};
        AW_HIP_TRY(hipMemsetAsync(sp->lim.d.get(), 0, L.reset_bytes, sp->ctx->stream));
        AW_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(L.min_gain.at(sp->lim.d.get())), (int)awlim::kOneBits, (size_t)sp->n_streams, sp->ctx->stream));
    }
    sp->lim.host_hist.assign(L.hist_floats, 0.0f);
    sp->lim.hist_on_host = false;
    return stage_zero(sp, L.history.at(sp->lim.d.get()), 2 * L.history.bytes());
}

// once per call that runs the kernel, before its first launch: where the single-stream path ran last, its history is the newer one
static aw_status lim_begin_call(aw_spatializer *sp, int64_t frames) {
    sp->lim.frames += (uint64_t)frames;
    if (sp->lim.hist_on_host) {
        const awst::Limiter L = lim_layout(sp);
        AW_HIP_TRY(hipMemcpyAsync(L.history.at(sp->lim.d.get(), 0, sp->lim.hist.cur), sp->lim.host_hist.data(), L.hist_floats * sizeof(float), hipMemcpyHostToDevice, sp->ctx->stream));
        AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));
        sp->lim.hist_on_host = false;
    }
    return AW_OK;
}

// y -> z for the streams [s0, s0 + ns) of a call (dense: `frames` apart; two buffers).  The AW_GAIN_FIXED gain is applied here, in
// front of the detector.  A workgroup's tile lies in one stream and the history is per stream, so chunks of streams are independent.
static aw_status lim_run(aw_spatializer *sp, const float *y, float *z, int64_t s0, int ns, int64_t frames) {
    SpStageTimer tm(sp);
    if (sp->profiling) tm.begin();
    awk::LimiterParams p{};
    p.in = y; p.out = z; p.frames = frames; p.n_streams = ns;
    const awst::Limiter L = lim_layout(sp);
    p.gain = sp->lv.gain_mode == AW_GAIN_FIXED ? lv_layout(sp).gains.at(sp->lv.d.get(), s0) : nullptr;
    p.hist_in = L.history.at(sp->lim.d.get(), s0, sp->lim.hist.cur);
    p.hist_out = L.history.at(sp->lim.d.get(), s0, sp->lim.hist.cur ^ 1);
    p.min_gain = L.min_gain.at(sp->lim.d.get(), s0); p.limited = L.limited.at(sp->lim.d.get(), s0); p.nonfinite = L.nonfinite.at(sp->lim.d.get(), s0);
    p.L = sp->lim.attack; p.H = sp->lim.hold; p.ceiling = sp->lim.ceiling;
    std::memcpy(p.c, sp->tp_filter, sizeof(p.c));
    AW_HIP_TRY(awk::launch_limiter(p, sp->ctx->stream));
    sp->lim.hist.ran = true;
    if (sp->profiling) tm.end("aw_limiter_kernel");
    return AW_OK;
}

// The single-stream page-locked path: the rule itself on the CPU, in place over the n = 2 * frames output samples y (the context's
// stream is idle).  gain: what lv_host_call returned.
static aw_status lim_host_call(aw_spatializer *sp, float *y, int64_t frames, float gain) {
    aw_spatializer::Limiter &lim = sp->lim;
    if (!lim.hist_on_host) {
        const awst::Limiter L = lim_layout(sp);
        AW_HIP_TRY(hipMemcpy(lim.host_hist.data(), L.history.at(lim.d.get(), 0, lim.hist.cur), L.hist_floats * sizeof(float), hipMemcpyDeviceToHost));
        lim.hist_on_host = true;
    }
    lim.frames += (uint64_t)frames;
    awlim::sequential(sp->tp_filter, lim.attack, lim.hold, lim.ceiling, gain, y, frames, lim.host_hist.data(), y, lim.host);
    return AW_OK;
}

/* ---- host entry ------------------------------------------------------------------------------------
 * The reference's callers hand over host buffers (AudioPipeline.swift:3-11: the four planar pointers of a render callback); an offline
 * batch host does too.  A multi-stream batch crosses PCIe in CHUNKS OF STREAMS (streams are independent: state is per stream), double
 * buffered on three HIP streams: H2D of chunk k+1 || kernels of chunk k || D2H of chunk k-1.  Page-locked caller buffers
 * (aw_host_alloc_pinned, hipHostMalloc, hipHostRegister) are read and written by the DMA engines directly; pageable ones are bounced
 * through page-locked chunks by the context's copy threads (below).  aw_spatializer_reserve_host() sizes the device-side chunk buffers
 * and the bounce chunks ahead of time; without it they grow on the first call.  The kernels of a chunk are the batch entries' one chunk
 * step (batch_chunk, below): the host entry adds the copies and the events around it. */
// Page-locked (hipHostMalloc / hipHostRegister) memory moves by DMA as it is; anything else is bounced.
static bool host_ptr_is_pinned(const void *p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }     // (plain malloc'ed memory: invalid value)
    return a.type == hipMemoryTypeHost;
}

static aw_status host_pipeline_objects(aw_context *c) {
    if (c->s_h2d && c->s_d2h && c->ev_d2h[1]) return AW_OK;           // (ev_d2h[1] is the last object made below)
    if (!c->copy_pool) {
        const unsigned hw = std::thread::hardware_concurrency();
        const unsigned div = (unsigned)c->copy_divisor;          // (1 unless a multi-device handle made the context)
        c->copy_pool = new (std::nothrow) aw_context::CopyPool((int)std::max(1u, std::min(12u, std::max(1u, hw / 4)) / div));
        if (!c->copy_pool) return fail(AW_ERR_OUT_OF_MEMORY, "copy threads");
        // the output direction moves a quarter or less of the input's bytes (8 against 4 C per frame): a few threads of its own
        c->copy_pool_out = new (std::nothrow) aw_context::CopyPool((int)std::max(1u, std::min(4u, std::max(1u, hw / 8)) / div));
        if (!c->copy_pool_out) return fail(AW_ERR_OUT_OF_MEMORY, "copy threads");
    }
    // (a failure half-way leaves what exists in place: the next call makes the rest, the context's destructor frees whatever is there)
    if (!c->s_h2d) AW_HIP_TRY(hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking));
    if (!c->s_d2h) AW_HIP_TRY(hipStreamCreateWithFlags(&c->s_d2h, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        if (!c->ev_h2d[i]) AW_HIP_TRY(c->ev_h2d[i].create(hipEventDisableTiming));
        if (!c->ev_run[i]) AW_HIP_TRY(c->ev_run[i].create(hipEventDisableTiming));
        if (!c->ev_d2h[i]) AW_HIP_TRY(c->ev_d2h[i].create(hipEventDisableTiming));
    }
    return AW_OK;
}

// the clipped-sample counter of the host entry (made once, with the first integer output)
static aw_status sp_clip_counter(aw_spatializer *sp) {
    if (sp->d_clip) return AW_OK;
    AW_HIP_TRY(sp->d_clip.alloc(1, &sp->ctx->device_allocs));
    return AW_OK;
}

// float32 staging of every entry that stages (two chunks of streams in flight each way, or the whole batch); host: also the device PCM
// slots of integer formats and the integer output's clip counter; bounce: the page-locked chunks that pageable caller buffers go through
// (aw_spatializer_reserve_host / _reserve_pcm make them; a call on pageable memory that was not reserved for makes them on its first use)
static aw_status host_stage_buffers(aw_spatializer *sp, int64_t frames, int64_t cs, bool bounce_in = false, bool bounce_out = false,
                                    int in_fmt = AW_SAMPLE_F32, int out_fmt = AW_SAMPLE_F32, bool host = true) {
    const size_t streams = awp::staged_streams(cs, sp->n_streams);
    const size_t in_n = streams * frames * sp->n_channels, out_n = streams * frames * 2;   // elements
    const size_t in_b = (size_t)awp::format_bytes(in_fmt), out_b = (size_t)awp::format_bytes(out_fmt);
    aw_status st = grow_buf(sp, &sp->d_stage_in, in_n);
    if (st == AW_OK) st = grow_buf(sp, &sp->d_stage_out, out_n);
    if (st == AW_OK && host && in_fmt != AW_SAMPLE_F32) st = grow_buf(sp, &sp->d_pcm_in, in_n * in_b);
    if (st == AW_OK && host && out_fmt != AW_SAMPLE_F32) st = grow_buf(sp, &sp->d_pcm_out, out_n * out_b);
    if (st == AW_OK && host && out_fmt != AW_SAMPLE_F32) st = sp_clip_counter(sp);
    if (st == AW_OK && host && cs > 0 && bounce_in) st = grow_buf(sp, &sp->h_bounce_in, in_n * in_b);
    if (st == AW_OK && host && cs > 0 && bounce_out) st = grow_buf(sp, &sp->h_bounce_out, out_n * out_b);
    return st;
}

static bool pcm_format_ok(aw_sample_format f) { return awp::format_bytes(f) > 0; }

// the chunking of a staged call (host/scratch_plan.hpp): what the formats ask for (in_bytes per input sample, LaunchCfg::host_chunk_mb per
// chunk), or — inside what a reserve sized — the chunking its buffers were sized for (never a reallocation on this path)
static int64_t staged_chunk_streams(const aw_spatializer *sp, int64_t frames, size_t in_bytes) {
    return awp::staged_chunk_streams(sp->n_streams, sp->n_channels, frames, in_bytes, sp->ctx->cfg.host_chunk_mb, sp->host_reserved_frames, sp->host_chunk_reserved);
}

static aw_status reserve_staged(aw_spatializer *sp, int64_t max_frames, aw_sample_format in_fmt, aw_sample_format out_fmt) {
    aw_status st = aw_spatializer_reserve(sp, max_frames);
    if (st != AW_OK) return st;
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    const int64_t cs = awp::host_chunk_streams(sp->n_streams, sp->n_channels, max_frames, (size_t)awp::format_bytes(in_fmt), sp->ctx->cfg.host_chunk_mb);
    if (cs > 0) { st = host_pipeline_objects(sp->ctx); if (st != AW_OK) return st; }
    st = host_stage_buffers(sp, max_frames, cs, /*bounce_in=*/true, /*bounce_out=*/true, in_fmt, out_fmt);
    if (st == AW_OK) { sp->host_chunk_streams = cs; sp->host_chunk_reserved = cs; sp->host_reserved_frames = std::max(sp->host_reserved_frames, max_frames); }
    return st;
}

aw_status aw_spatializer_reserve_host(aw_spatializer *sp, int64_t max_frames) try {
    return reserve_staged(sp, max_frames, AW_SAMPLE_F32, AW_SAMPLE_F32);
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_reserve_pcm(aw_spatializer *sp, int64_t max_frames, aw_sample_format in_format, aw_sample_format out_format) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (!pcm_format_ok(in_format) || !pcm_format_ok(out_format)) return fail(AW_ERR_INVALID_ARGUMENT, "unknown sample format");
    return reserve_staged(sp, max_frames, in_format, out_format);
} AW_NOEXCEPT_TAIL

int32_t aw_sample_format_bytes(aw_sample_format f) { return awp::format_bytes(f); }

// decode n samples of in_fmt at src into floats at dst / encode n floats into out_fmt, on the context's stream (profiled as stages)
static aw_status pcm_decode(aw_spatializer *sp, int in_fmt, const void *src, float *dst, int64_t n) {
    SpStageTimer tm(sp);
    if (sp->profiling) tm.begin();
    AW_HIP_TRY(awk::launch_pcm_decode(in_fmt, src, dst, n, sp->ctx->stream));
    if (sp->profiling) tm.end("aw_pcm_decode_kernel");
    return AW_OK;
}
static_assert(AW_DITHER_NONE == awp::kDitherNone && AW_DITHER_TPDF == awp::kDitherTpdf && AW_DITHER_TPDF_HP == awp::kDitherTpdfHp, "aw_dither");
// only s16 and s24 are dithered: float32's 24-bit mantissa is coarser than an s32 LSB for nearly every sample
static bool sp_dithers(const aw_spatializer *sp, int out_fmt) {
    return sp->dither != AW_DITHER_NONE && (out_fmt == AW_SAMPLE_S16 || out_fmt == AW_SAMPLE_S24);
}
/* ---- one call plan, one chunk step: batch_args (argument prologue), then under the launch lock batch_formats + batch_begin (the plan),
 * batch_chunk per chunk of streams (decode -> kernels -> meter / gain -> encode) and batch_end (the history flip).  The entries differ in
 * where a chunk's bytes come from and go to; the single-stream page-locked calls run batch_run_pinned and convert on the CPU. */
struct BatchCall {
    int64_t frames;                         // (down to out_psb: batch_formats; the rest: batch_begin)
    int in_fmt, out_fmt;
    bool dec, enc;                          // an integer format on that side: the chunk step converts
    size_t in_b, out_b;                     // bytes per sample
    size_t in_ps, out_ps;                   // samples per stream
    size_t in_psb, out_psb;                 // bytes per stream
    LwCallPlan lw;                          // the call's kernel plan
    uint64_t pos0;                          // position of the call's first frame: every encode of the call keys its dither on it
    unsigned long long *clip;               // NULL, or the device counter this call's encodes add their clipped samples to
    bool metered;                           // metered and gained as the handle is set (the planar entry's inner call is not)
    uint64_t loud0;                         // loudness: frames measured before this call (the hop index of its first frame)
};

// s0: the handle's index of the first of the ns streams encoded.  No dither and neither gain nor meter: the plain encode kernel, as ever.
static aw_status pcm_encode(aw_spatializer *sp, const BatchCall &call, const float *src, void *dst, int64_t s0, int ns) {
    SpStageTimer tm(sp);
    if (sp->profiling) tm.begin();
    const bool lv = lv_active(sp), dithers = sp_dithers(sp, call.out_fmt);
    const awk::PcmDither d{dithers ? sp->dither : awp::kDitherNone, sp->dither_seed, sp->dither_first_stream + (uint64_t)s0, call.pos0, call.frames};
    const awk::PcmGain g = lv ? lv_gain_launch(sp, s0) : awk::PcmGain{};
    AW_HIP_TRY(awk::launch_pcm_encode(call.out_fmt, src, dst, (int64_t)ns * call.out_ps, call.clip, lv || dithers ? &d : nullptr, lv ? &g : nullptr,
                                      sp->ctx->stream));
    if (sp->profiling) tm.end("aw_pcm_encode_kernel");
    return AW_OK;
}

// The argument prologue of every batch entry, answered in this order: a NULL pointer, an unknown format, *zero_clipped = 0 (the host PCM
// entry's count), frames < 0.  frames == 0 is AW_OK with *nothing set (the call is over); otherwise the context's device is made current.
static aw_status batch_args(const aw_spatializer *sp, bool pointers, aw_sample_format in_fmt, aw_sample_format out_fmt, int64_t frames, bool *nothing,
                            uint64_t *zero_clipped = nullptr, const char *negative = "frames must be >= 0") {
    *nothing = true;
    if (!sp || !pointers) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!pcm_format_ok(in_fmt) || !pcm_format_ok(out_fmt)) return fail(AW_ERR_INVALID_ARGUMENT, "unknown sample format");
    if (zero_clipped) *zero_clipped = 0;
    if (frames <= 0) return frames == 0 ? AW_OK : fail(AW_ERR_INVALID_ARGUMENT, negative);
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    *nothing = false;
    return AW_OK;
}

static BatchCall batch_formats(const aw_spatializer *sp, int64_t frames, int in_fmt, int out_fmt) {
    BatchCall b{};
    b.frames = frames; b.in_fmt = in_fmt; b.out_fmt = out_fmt;
    b.dec = in_fmt != AW_SAMPLE_F32; b.enc = out_fmt != AW_SAMPLE_F32;
    b.in_b = (size_t)awp::format_bytes(in_fmt); b.out_b = (size_t)awp::format_bytes(out_fmt);
    b.in_ps = (size_t)frames * sp->n_channels; b.out_ps = (size_t)frames * 2;
    b.in_psb = b.in_ps * b.in_b; b.out_psb = b.out_ps * b.out_b;
    return b;
}

// Once per call, before its first launch.  The kernel plan comes first: the frame position moves past the call even if the call fails
// later.  zero_clip: the counter is the handle's own (host entry) and starts the call at zero.
static aw_status batch_begin(aw_spatializer *sp, BatchCall *call, unsigned long long *clip, bool zero_clip, bool metered) {
    call->lw = sp_begin_call(sp, call->frames, &call->pos0);
    call->clip = clip;
    call->metered = metered;
    if (metered) {
        if (sp->eq.d) eq_begin_call(sp, call->frames);
        aw_status st = lv_begin_call(sp, call->frames, true);
        if (st != AW_OK) return st;
        call->loud0 = ld_begin_call(sp, call->frames);
        if (tp_runs(sp) && (st = tp_begin_call(sp, call->frames)) != AW_OK) return st;
        if (sp->lim.on && (st = lim_begin_call(sp, call->frames)) != AW_OK) return st;
    }
    if (zero_clip) AW_HIP_TRY(hipMemsetAsync(clip, 0, sizeof(unsigned long long), sp->ctx->stream));
    return AW_OK;
}

// every chunk's kernels are queued: the history they wrote is the next call's
static void batch_end(aw_spatializer *sp) {
    sp->hist_cur ^= 1;
    eq_end_call(sp);
    sp->tp.hist.end_call();
    sp->lim.hist.end_call();
}

// The streams [s0, s0 + ns) of a call, on the context's stream: pcm_src -> decode into f_in -> kernels -> meter / gain -> encode of f_out
// into pcm_dst; the equalizer, where one is set, works on the kernels' output in place before the first meter.  A float32 side has no conversion and no staging: the kernels read pcm_src / write pcm_dst, f_in / f_out is not looked at.
// With the limiter on the kernels write y into the limiter's staging instead, the meters tap it there, and the limiter (which applies
// the fixed gain) writes z where y would have gone.
static aw_status batch_chunk(aw_spatializer *sp, const BatchCall &call, int64_t s0, int ns, const void *pcm_src, float *f_in, float *f_out, void *pcm_dst) {
    aw_status st = AW_OK;
    if (call.dec) st = pcm_decode(sp, call.in_fmt, pcm_src, f_in, (int64_t)ns * call.in_ps);
    const float *x = call.dec ? f_in : static_cast<const float *>(pcm_src);
    float *dst = call.enc ? f_out : static_cast<float *>(pcm_dst);
    const bool lim = call.metered && sp->lim.on;
    if (st == AW_OK && lim) st = grow_buf(sp, &sp->lim.d_y, (size_t)ns * call.out_ps);      // (reserved for: nothing happens)
    float *y = lim ? sp->lim.d_y.get() : dst;
    if (st == AW_OK) st = sp_run_streams(sp, call.lw, (int)s0, ns, x, y, call.frames);
    if (st == AW_OK && call.metered && sp->eq.d) st = eq_run(sp, y, s0, ns, call.frames);                        // (every later stage sees the equalized y)
    if (st == AW_OK && call.metered && sp->ld.on) st = ld_measure(sp, y, s0, ns, call.frames, call.loud0);      // (before the gain)
    if (st == AW_OK && call.metered && tp_runs(sp)) st = tp_measure(sp, y, s0, ns, call.frames);                   // (the gain may read its result)
    if (st == AW_OK && call.metered) st = lv_after_run(sp, y, s0, ns, call.frames, !call.enc && !lim);
    if (st == AW_OK && lim) st = lim_run(sp, y, dst, s0, ns, call.frames);
    if (st == AW_OK && call.enc) st = pcm_encode(sp, call, dst, pcm_dst, s0, ns);
    return st;
}

// One stream, a callback's worth of frames (sp_zero_copy): the kernels read h_pin_in and write h_pin_out, page-locked host memory, over
// PCIe, and the call is over when this returns.  metered: the host entry, which then meters, gains and encodes h_pin_out on the CPU.
static aw_status batch_run_pinned(aw_spatializer *sp, int64_t frames, bool metered, uint64_t *pos0) {
    const LwCallPlan lw = sp_begin_call(sp, frames, pos0);
    aw_status st = metered ? lv_begin_call(sp, frames, false) : AW_OK;
    if (metered && sp->eq.d) eq_begin_call(sp, frames);
    if (st == AW_OK) st = sp_run_streams(sp, lw, 0, 1, sp->h_pin_in.get(), sp->h_pin_out.get(), frames);
    if (st == AW_OK && metered && sp->eq.d) st = eq_run(sp, sp->h_pin_out.get(), 0, 1, frames);      // in place over PCIe, like the kernels in front of it
    if (st == AW_OK && metered && sp->ld.on)             // the loudness kernels read the page-locked output as the convolution kernels wrote it
        st = ld_measure(sp, sp->h_pin_out.get(), 0, 1, frames, ld_begin_call(sp, frames));
    const bool tp = metered && tp_runs(sp);
    if (st == AW_OK && tp) st = tp_begin_call(sp, frames);
    if (st == AW_OK && tp) st = tp_measure(sp, sp->h_pin_out.get(), 0, 1, frames);
    if (st != AW_OK) { sp->tp.hist.end_call(false); return st; }       // (the limiter runs on the CPU here: lim_host_call)
    batch_end(sp);
    AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));
    if (tp && sp->lv.gain_mode == AW_GAIN_TRUE_PEAK_CEILING)    // the CPU gains this call: it needs the call's true peak
        AW_HIP_TRY(hipMemcpy(&sp->tp.pinned_call_bits, tp_layout(sp).call_peaks.at(sp->tp.d.get()), sizeof(uint32_t), hipMemcpyDeviceToHost));
    return AW_OK;
}

// The device entry; metered = false: the planar entry's inner call.
static aw_status process_device(aw_spatializer *sp, const float *in, float *out, int64_t frames, bool metered) {
    bool nothing;
    aw_status st = batch_args(sp, in && out, AW_SAMPLE_F32, AW_SAMPLE_F32, frames, &nothing);
    if (st != AW_OK || nothing) return st;
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);       // this call's launches stay together on the stream (the scratch pool is the context's)
    BatchCall call = batch_formats(sp, frames, AW_SAMPLE_F32, AW_SAMPLE_F32);
    st = batch_begin(sp, &call, nullptr, false, metered);
    if (st == AW_OK) st = batch_chunk(sp, call, 0, sp->n_streams, in, nullptr, nullptr, out);
    if (st == AW_OK) batch_end(sp);
    return st;
}

aw_status aw_spatializer_process(aw_spatializer *sp, const float *in, float *out, int64_t frames) try {
    return process_device(sp, in, out, frames, true);
} AW_NOEXCEPT_TAIL

// The host entry's single-stream page-locked call: the CPU converts on the way into and out of the staging (rules: pcm.hpp, levels.hpp).
static aw_status host_process_pinned(aw_spatializer *sp, const BatchCall &call, const unsigned char *in, unsigned char *out, uint64_t *clipped) {
    const int out_fmt = call.out_fmt;
    const size_t out_b = call.out_b, out_ps = call.out_ps;
    float *const h_in = sp->h_pin_in.get(), *const h_out = sp->h_pin_out.get();
    if (call.dec) for (size_t i = 0; i < call.in_ps; ++i) h_in[i] = awp::decode_at(call.in_fmt, in + i * call.in_b);
    else std::memcpy(h_in, in, call.in_psb);
    uint64_t pos0 = 0;
    const aw_status st = batch_run_pinned(sp, call.frames, true, &pos0);
    if (st != AW_OK) return st;
    const bool lv = lv_active(sp);
    float gain = lv ? lv_host_call(sp, h_out, out_ps) : 1.0f;
    if (sp->lim.on) {                   // z replaces y in the staging; the fixed gain went in with it
        const aw_status sl = lim_host_call(sp, h_out, call.frames, gain);
        if (sl != AW_OK) return sl;
        gain = 1.0f;
    }
    if (call.enc) {
        uint64_t n_clip = 0;
        const int mode = sp_dithers(sp, out_fmt) ? sp->dither : awp::kDitherNone;
        const uint64_t key = awp::dither_key(sp->dither_seed, sp->dither_first_stream);
        for (size_t i = 0; i < out_ps; ++i) {
            unsigned k = 0;
            if (lv) awl::encode_gained_at(out_fmt, mode, h_out[i], gain, key, pos0 + i / 2, (int)(i & 1), out + i * out_b, &k);
            else awp::encode_dithered_at(out_fmt, mode, h_out[i], key, pos0 + i / 2, (int)(i & 1), out + i * out_b, &k);
            n_clip += k;
        }
        if (sp->lv.metering) sp->lv.host.clipped += n_clip;
        if (clipped) *clipped = n_clip;
    } else if (sp->lv.gain_mode != AW_GAIN_NONE) {
        float *o = reinterpret_cast<float *>(out);
        for (size_t i = 0; i < out_ps; ++i) o[i] = awl::apply_gain(h_out[i], gain);
    } else {
        std::memcpy(out, h_out, call.out_psb);
    }
    sp->host_chunk_streams = 0;
    return AW_OK;
}

// The host entry for every pair of sample formats.  float32 / float32 (aw_spatializer_process_host) moves the bytes, chunks and launches
// it always has: the device PCM slots of float32 ARE the float staging, and neither conversion kernel runs.  Otherwise each chunk goes
// H2D into its PCM slot -> batch_chunk (decode into the float staging -> kernels -> encode into the PCM out slot) -> D2H, the chunk step
// on the context's stream between the events that already order the slots (ev_run[slot] covers the PCM slots too).
static aw_status host_process(aw_spatializer *sp, const void *in_v, int in_fmt, void *out_v, int out_fmt, int64_t frames, uint64_t *clipped) {
    aw_context *c = sp->ctx;
    const unsigned char *in = static_cast<const unsigned char *>(in_v);
    unsigned char *out = static_cast<unsigned char *>(out_v);
    BatchCall call = batch_formats(sp, frames, in_fmt, out_fmt);
    if (sp_zero_copy(sp, frames)) return host_process_pinned(sp, call, in, out, clipped);
    const bool enc = call.enc;
    const size_t in_ps = call.in_ps, out_ps = call.out_ps, in_psb = call.in_psb, out_psb = call.out_psb;
    const int64_t cs = staged_chunk_streams(sp, frames, call.in_b);
    const bool page_in = cs > 0 && !host_ptr_is_pinned(in), page_out = cs > 0 && !host_ptr_is_pinned(out);
    aw_status st = host_stage_buffers(sp, frames, cs, page_in, page_out, in_fmt, out_fmt);
    if (st == AW_OK && cs > 0) st = host_pipeline_objects(c);
    if (st != AW_OK) return st;
    sp->host_chunk_streams = cs;
    float *const stage_in = sp->d_stage_in.get(), *const stage_out = sp->d_stage_out.get();
    unsigned char *pcm_in = call.dec ? sp->d_pcm_in.get() : reinterpret_cast<unsigned char *>(stage_in);
    unsigned char *pcm_out = enc ? sp->d_pcm_out.get() : reinterpret_cast<unsigned char *>(stage_out);
    if ((st = batch_begin(sp, &call, enc ? sp->d_clip.get() : nullptr, enc, true)) != AW_OK) return st;
    uint64_t n_clip = 0;
    if (cs == 0) {                       // one piece: H2D -> kernels -> D2H on the context's stream
        AW_HIP_TRY(hipMemcpyAsync(pcm_in, in, in_psb * sp->n_streams, hipMemcpyHostToDevice, c->stream));
        if ((st = batch_chunk(sp, call, 0, sp->n_streams, pcm_in, stage_in, stage_out, pcm_out)) != AW_OK) return st;
        batch_end(sp);
        AW_HIP_TRY(hipMemcpyAsync(out, pcm_out, out_psb * sp->n_streams, hipMemcpyDeviceToHost, c->stream));
        if (enc) AW_HIP_TRY(hipMemcpyAsync(&n_clip, sp->d_clip.get(), sizeof(n_clip), hipMemcpyDeviceToHost, c->stream));
        AW_HIP_TRY(hipStreamSynchronize(c->stream));
        if (clipped) *clipped = n_clip;
        return AW_OK;
    }
    // whatever the context's stream still holds (an earlier device-buffer call of this spatializer) comes first
    AW_HIP_TRY(hipEventRecord(c->ev_run[0].get(), c->stream));
    AW_HIP_TRY(hipStreamWaitEvent(c->s_h2d, c->ev_run[0].get(), 0));
    // Pageable caller memory is bounced through page-locked chunks by the context's copy threads: the copy INTO slot k & 1 runs while the
    // DMA engines move chunk k-1, the copy OUT of chunk k-1 while the kernels of chunk k run (round 5; before: hipMemcpyAsync on the
    // pageable pointers themselves, which the HIP runtime stages on one thread).
    int k = 0;
    int64_t prev_s0 = -1; int prev_ns = 0;
    hipError_t he = hipSuccess;
    // chunk k-1's output: wait for its D2H, then hand it to the output copy threads (they work while this thread copies chunk k+1 IN;
    // the bounce slot is waited for before a later D2H is queued into it, and once more at the end)
    auto drain_prev = [&](int slot_prev) {
        if (!page_out || prev_s0 < 0 || he != hipSuccess) return;
        he = hipEventSynchronize(c->ev_d2h[slot_prev].get());
        if (he != hipSuccess) return;
        unsigned char *d = out + (size_t)prev_s0 * out_psb; const unsigned char *b = sp->h_bounce_out.get() + (size_t)slot_prev * cs * out_psb;
        const size_t n = (size_t)prev_ns * out_psb;
        if (c->cfg.host_out_async) c->copy_pool_out->start(d, b, n);
        else c->copy_pool->copy(d, b, n);            // AW_HOST_OUT_ASYNC=0 (A/B): round 5's form, on the driver thread
    };
    for (int64_t s0 = 0; s0 < sp->n_streams && he == hipSuccess; s0 += cs, ++k) {
        const int ns = (int)std::min<int64_t>(cs, sp->n_streams - s0), slot = k & 1;
        unsigned char *d_in = pcm_in + (size_t)slot * cs * in_psb, *d_out = pcm_out + (size_t)slot * cs * out_psb;
        float *f_in = stage_in + (size_t)slot * cs * in_ps, *f_out = stage_out + (size_t)slot * cs * out_ps;   // (float32: d_in / d_out)
        const unsigned char *src = in + (size_t)s0 * in_psb;
        if (page_in) {
            unsigned char *b = sp->h_bounce_in.get() + (size_t)slot * cs * in_psb;
            if (k >= 2) he = hipEventSynchronize(c->ev_h2d[slot].get());                              // chunk k-2's H2D has read this bounce slot
            if (he != hipSuccess) break;
            c->copy_pool->copy(b, src, (size_t)ns * in_psb);
            src = b;
        }
        if (k >= 2) he = hipStreamWaitEvent(c->s_h2d, c->ev_run[slot].get(), 0);                      // chunk k-2's kernels have read this device slot
        if (he == hipSuccess) he = hipMemcpyAsync(d_in, src, (size_t)ns * in_psb, hipMemcpyHostToDevice, c->s_h2d);
        if (he == hipSuccess) he = hipEventRecord(c->ev_h2d[slot].get(), c->s_h2d);
        if (he == hipSuccess) he = hipStreamWaitEvent(c->stream, c->ev_h2d[slot].get(), 0);
        if (he == hipSuccess && k >= 2) he = hipStreamWaitEvent(c->stream, c->ev_d2h[slot].get(), 0); // chunk k-2's output has left this device slot
        if (he != hipSuccess) break;
        if ((st = batch_chunk(sp, call, s0, ns, d_in, f_in, f_out, d_out)) != AW_OK) break;
        he = hipEventRecord(c->ev_run[slot].get(), c->stream);
        if (he == hipSuccess) he = hipStreamWaitEvent(c->s_d2h, c->ev_run[slot].get(), 0);
        if (page_out) c->copy_pool_out->wait();          // chunk k-2's copy-out has left this bounce slot (it had a whole chunk's time)
        unsigned char *dst = page_out ? sp->h_bounce_out.get() + (size_t)slot * cs * out_psb : out + (size_t)s0 * out_psb;
        if (he == hipSuccess) he = hipMemcpyAsync(dst, d_out, (size_t)ns * out_psb, hipMemcpyDeviceToHost, c->s_d2h);
        if (he == hipSuccess) he = hipEventRecord(c->ev_d2h[slot].get(), c->s_d2h);
        drain_prev(slot ^ 1);
        prev_s0 = s0; prev_ns = ns;
    }
    if (enc && st == AW_OK && he == hipSuccess) he = hipMemcpyAsync(&n_clip, sp->d_clip.get(), sizeof(n_clip), hipMemcpyDeviceToHost, c->stream);
    const hipError_t e1 = hipStreamSynchronize(c->s_h2d), e2 = hipStreamSynchronize(c->stream), e3 = hipStreamSynchronize(c->s_d2h);
    if (page_out) c->copy_pool_out->wait();               // no copy thread outlives the call, whatever returns below
    if (st != AW_OK) return st;          // (a failed chunk: the streams are drained, the history has not been flipped)
    AW_HIP_TRY(he); AW_HIP_TRY(e1); AW_HIP_TRY(e2); AW_HIP_TRY(e3);
    drain_prev((k - 1) & 1);             // the last chunk's output
    if (page_out) c->copy_pool_out->wait();
    AW_HIP_TRY(he);
    batch_end(sp);
    if (clipped) *clipped = n_clip;
    return AW_OK;
}

aw_status aw_spatializer_process_host(aw_spatializer *sp, const float *in, float *out, int64_t frames) try {
    bool nothing;
    const aw_status st = batch_args(sp, in && out, AW_SAMPLE_F32, AW_SAMPLE_F32, frames, &nothing);
    if (st != AW_OK || nothing) return st;
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    return host_process(sp, in, AW_SAMPLE_F32, out, AW_SAMPLE_F32, frames, nullptr);
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_process_host_pcm(aw_spatializer *sp, const void *in, aw_sample_format in_format, void *out,
                                          aw_sample_format out_format, int64_t frames, uint64_t *clipped) try {
    bool nothing;
    const aw_status st = batch_args(sp, in && out, in_format, out_format, frames, &nothing, clipped);
    if (st != AW_OK || nothing) return st;
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    return host_process(sp, in, in_format, out, out_format, frames, clipped);
} AW_NOEXCEPT_TAIL

// Device buffers in any pair of formats: the call's streams go in chunks (the host entry's chunking, memory bounded by the chunk) through
// the float staging — batch_chunk straight from and into the caller's buffers.  One kernel choice for the whole call (batch_begin once),
// so the chunks give the bits an unchunked run gives.  float32 / float32 is aw_spatializer_process itself.
aw_status aw_spatializer_process_pcm(aw_spatializer *sp, const void *in_v, aw_sample_format in_fmt, void *out_v, aw_sample_format out_fmt,
                                     int64_t frames, uint64_t *clipped_device) try {
    if (in_fmt == AW_SAMPLE_F32 && out_fmt == AW_SAMPLE_F32)   // (whose prologue answers what this one would)
        return aw_spatializer_process(sp, static_cast<const float *>(in_v), static_cast<float *>(out_v), frames);
    bool nothing;
    aw_status st = batch_args(sp, in_v && out_v, in_fmt, out_fmt, frames, &nothing);
    if (st != AW_OK || nothing) return st;
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    const unsigned char *in = static_cast<const unsigned char *>(in_v);
    unsigned char *out = static_cast<unsigned char *>(out_v);
    BatchCall call = batch_formats(sp, frames, in_fmt, out_fmt);
    int64_t cs = staged_chunk_streams(sp, frames, call.in_b);
    st = host_stage_buffers(sp, frames, cs, false, false, in_fmt, out_fmt, /*host=*/false);
    if (st != AW_OK) return st;
    if (cs == 0) cs = sp->n_streams;
    if ((st = batch_begin(sp, &call, reinterpret_cast<unsigned long long *>(clipped_device), false, true)) != AW_OK) return st;
    for (int64_t s0 = 0; s0 < sp->n_streams; s0 += cs) {
        const int ns = (int)std::min<int64_t>(cs, sp->n_streams - s0);
        const unsigned char *src = in + (size_t)s0 * call.in_psb;
        if ((st = batch_chunk(sp, call, s0, ns, src, sp->d_stage_in.get(), sp->d_stage_out.get(), out + (size_t)s0 * call.out_psb)) != AW_OK) return st;
    }
    batch_end(sp);
    return AW_OK;
} AW_NOEXCEPT_TAIL

/* Page-locked host memory for the host entries (hipHostMalloc): buffers from here cross PCIe by DMA without the runtime's staging copy. */
aw_status aw_host_alloc_pinned(aw_context *ctx, size_t bytes, void **ptr) try {
    if (!ctx || !ptr) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    AW_HIP_TRY(hipSetDevice(ctx->device));
    AW_HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    ctx->device_allocs += 1;
    return AW_OK;
} AW_NOEXCEPT_TAIL
aw_status aw_host_free_pinned(aw_context *ctx, void *ptr) try {
    if (!ctx) return fail(AW_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ptr) AW_HIP_TRY(hipHostFree(ptr));
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_process_planar(aw_spatializer *sp, const float *in_l, const float *in_r, float *out_l,
                                        float *out_r, int32_t frames) try {
    if (!sp || !in_l || !out_l || !out_r) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (sp->n_streams != 1 || sp->n_channels != 2)
        return fail(AW_ERR_INVALID_ARGUMENT, "planar entry needs a 1-stream, 2-channel spatializer");
    bool nothing;
    aw_status st = batch_args(sp, true, AW_SAMPLE_F32, AW_SAMPLE_F32, frames, &nothing, nullptr, "frameCount must be >= 0");
    if (st != AW_OK || nothing) return st;
    hipStream_t s = sp->ctx->stream;
    if (sp_zero_copy(sp, frames)) {
        // The render-callback shape (AudioPipeline.swift:3-11).  Interleave on the way into the page-locked staging (mono duplication,
        // RealtimeAudioProcessor.swift:95-107), let the kernels read and write it in place over PCIe, deinterleave on the way out: two or
        // three kernel launches and one synchronisation per callback (round 4: four copies through the DMA engines and two more kernels).
        std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
        const float *r_src = in_r ? in_r : in_l;
        float *pi = sp->h_pin_in.get();
        for (int i = 0; i < frames; ++i) { pi[2 * (size_t)i] = in_l[i]; pi[2 * (size_t)i + 1] = r_src[i]; }
        if ((st = batch_run_pinned(sp, frames, /*metered=*/false, nullptr)) != AW_OK) return st;
        const float *po = sp->h_pin_out.get();
        for (int i = 0; i < frames; ++i) { out_l[i] = po[2 * (size_t)i]; out_r[i] = po[2 * (size_t)i + 1]; }
        return AW_OK;
    }
    // staging layout: [in interleaved 2F | planar L F | planar R F] and [out interleaved 2F | L F | R F]
    st = grow_buf(sp, &sp->d_stage_in, (size_t)frames * 4);
    if (st == AW_OK) st = grow_buf(sp, &sp->d_stage_out, (size_t)frames * 4);
    if (st != AW_OK) return st;
    float *const d_i = sp->d_stage_in.get(), *const d_o = sp->d_stage_out.get();
    float *d_il = d_i + 2 * (size_t)frames, *d_ir = d_il + frames;
    float *d_ol = d_o + 2 * (size_t)frames, *d_or = d_ol + frames;
    AW_HIP_TRY(hipMemcpyAsync(d_il, in_l, sizeof(float) * frames, hipMemcpyHostToDevice, s));
    AW_HIP_TRY(hipMemcpyAsync(d_ir, in_r ? in_r : in_l, sizeof(float) * frames, hipMemcpyHostToDevice, s));   // mono dup, RealtimeAudioProcessor.swift:95-107
    AW_HIP_TRY(awk::launch_interleave2(d_il, d_ir, d_i, frames, s));
    st = process_device(sp, d_i, d_o, frames, /*metered=*/false);     // (the planar entry is neither metered nor gained)
    if (st != AW_OK) return st;
    AW_HIP_TRY(awk::launch_deinterleave2(d_o, d_ol, d_or, frames, s));
    AW_HIP_TRY(hipMemcpyAsync(out_l, d_ol, sizeof(float) * frames, hipMemcpyDeviceToHost, s));
    AW_HIP_TRY(hipMemcpyAsync(out_r, d_or, sizeof(float) * frames, hipMemcpyDeviceToHost, s));
    AW_HIP_TRY(hipStreamSynchronize(s));
    return AW_OK;
} AW_NOEXCEPT_TAIL

// every stage's records start over (the settings stay)
static aw_status lv_reset(aw_spatializer *sp) {
    sp->lv.host = awl::Record{};
    sp->lv.applied_mode = AW_GAIN_NONE;
    sp->lv.frames = sp->ld.frames = sp->tp.frames = 0;
    sp->tp.pinned_call_bits = 0;
    aw_status st = sp->lv.d ? stage_zero(sp, sp->lv.d.get(), lv_layout(sp).reset_bytes) : AW_OK;
    if (st == AW_OK && sp->ld.d) st = stage_zero(sp, sp->ld.d.get(), ld_layout(sp).reset_bytes);
    if (st == AW_OK && sp->tp.d) st = stage_zero(sp, sp->tp.d.get(), tp_layout(sp).reset_bytes);
    return st == AW_OK && sp->lim.d ? lim_reset(sp, true) : st;
}

// The prologue of the four record getters, answered in this order: a NULL handle, the stream range, n == 0 (AW_OK, *lk left unlocked: the
// call is over), a NULL out, a stage (base: its allocation) whose records were never made; then the device is current, the launch lock held, the stream idle.
static aw_status get_begin(aw_spatializer *sp, int32_t first_stream, int32_t n, const void *out, unsigned char *(*base)(const aw_spatializer *), const char *never, std::unique_lock<std::mutex> *lk) {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (first_stream < 0 || n < 0 || (int64_t)first_stream + n > sp->n_streams) return fail(AW_ERR_INVALID_ARGUMENT, "streams out of range");
    if (n == 0) return AW_OK;
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out_host is NULL");
    if (!base(sp)) return fail(AW_ERR_INVALID_ARGUMENT, never);
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    *lk = std::unique_lock<std::mutex>(sp->ctx->launch_mu);
    AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));
    return AW_OK;
}

aw_status aw_spatializer_reset(aw_spatializer *sp) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    sp->position = 0;
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    const size_t n = (size_t)sp->n_streams * sp->hist_len * sp->n_channels;
    for (int i = 0; i < 2; ++i)
        AW_HIP_TRY(hipMemsetAsync(sp->d_hist[i].get(), 0, std::max<size_t>(n, 1) * sizeof(float), sp->ctx->stream));
    const aw_status st = eq_reset(sp);
    return st == AW_OK ? lv_reset(sp) : st;
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_set_metering(aw_spatializer *sp, int32_t on) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (on) {
        AW_HIP_TRY(hipSetDevice(sp->ctx->device));
        std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
        const aw_status st = lv_buffers(sp);
        if (st != AW_OK) return st;
    }
    sp->lv.metering = on != 0;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_reset_levels(aw_spatializer *sp) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    return lv_reset(sp);
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_get_levels(aw_spatializer *sp, int32_t first_stream, int32_t n, aw_stream_levels *out) try {
    std::unique_lock<std::mutex> lk;
    aw_status st = get_begin(sp, first_stream, n, out, [](const aw_spatializer *s) { return s->lv.d.get(); }, "no levels: neither aw_spatializer_set_metering nor aw_spatializer_set_gain has been called", &lk);
    if (st != AW_OK || !lk) return st;
    std::vector<awl::Record> rec;
    std::vector<uint32_t> peaks;
    if ((st = get_field(lv_layout(sp).records, sp->lv.d.get(), first_stream, n, &rec)) != AW_OK) return st;
    st = sp->lv.applied_mode == AW_GAIN_TRUE_PEAK_CEILING && sp->tp.d ? get_field(tp_layout(sp).call_peaks, sp->tp.d.get(), first_stream, n, &peaks)
                                                                      : get_field(lv_layout(sp).call_peaks, sp->lv.d.get(), first_stream, n, &peaks);
    if (st != AW_OK) return st;
    for (int32_t i = 0; i < n; ++i) {
        awl::Record r = rec[(size_t)i];
        const int32_t s = first_stream + i;
        if (s == 0) {                    // the single-stream path's share (a handle of one stream)
            for (int e = 0; e < 2; ++e) { r.peak_bits[e] = std::max(r.peak_bits[e], sp->lv.host.peak_bits[e]); r.energy[e] += sp->lv.host.energy[e]; }
            r.clipped += sp->lv.host.clipped;
            r.nonfinite += sp->lv.host.nonfinite;
        }
        aw_stream_levels &o = out[i];
        o.peak[0] = awl::bits_float(r.peak_bits[0]); o.peak[1] = awl::bits_float(r.peak_bits[1]);
        o.gain = 1.0f;
        if (sp->lv.applied_mode == AW_GAIN_FIXED && (size_t)s < sp->lv.applied_gains.size()) o.gain = sp->lv.applied_gains[(size_t)s];
        else if (sp->lv.applied_mode == AW_GAIN_PEAK_CEILING || sp->lv.applied_mode == AW_GAIN_TRUE_PEAK_CEILING)
            o.gain = sp->lv.applied_on_host ? sp->lv.applied_host_gain : awl::auto_gain(awl::bits_float(peaks[(size_t)i]), sp->lv.applied_ceiling);
        o.reserved = 0;
        o.energy[0] = r.energy[0]; o.energy[1] = r.energy[1];
        o.frames = sp->lv.frames;
        o.clipped = r.clipped;
        o.nonfinite = r.nonfinite;
    }
    return AW_OK;
} AW_NOEXCEPT_TAIL

// Checks first, then the one allocation and the table upload (here, never on the process path).  A capacity other than the one held
// makes new, empty records.
aw_status aw_spatializer_set_loudness(aw_spatializer *sp, int32_t on, double max_seconds) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (!on) { sp->ld.on = false; return AW_OK; }
    if (!std::isfinite(max_seconds) || !(max_seconds > 0.0) || max_seconds > 1e9) return fail(AW_ERR_INVALID_ARGUMENT, "max_seconds must be finite and positive");
    const long long hop = awlo::hop_frames(sp->sample_rate);
    if (hop <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "loudness needs an HRIR sample rate that is a finite positive multiple of 10 Hz");
    const int64_t cap = (int64_t)std::ceil((double)awlo::kHopsPerSecond * max_seconds);
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    if (!sp->ld.d || cap != sp->ld.cap) {
        double kw[awlo::kFilters][5];
        awlo::k_weighting(sp->sample_rate, kw);
        std::vector<double> tables(kLdTabDoubles + kLdPlaneDoubles);
        for (int k = 0; k < awlo::kFilters; ++k)
            awh::eq_section_tables(awh::Biquad{kw[k][0], kw[k][1], kw[k][2], kw[k][3], kw[k][4]}, &tables[(size_t)k * awk::kEqTabDoubles],
                                   &tables[kLdTabDoubles + (size_t)k * awh::kEqSectionPlaneDoubles]);
        AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));            // whatever still reads the old records
        if (sp->ld.d) { (void)sp->ld.d.reset(); sp->ld.on = false; }
        sp->ld.hop = hop; sp->ld.cap = cap; sp->ld.frames = 0;
        const awst::Loudness L = ld_layout(sp);
        const aw_status st = stage_alloc(sp, &sp->ld.d, L.total, L.reset_bytes);
        if (st != AW_OK) return st;
        AW_HIP_TRY(hipMemcpyAsync(L.tables.at(sp->ld.d.get()), tables.data(), tables.size() * sizeof(double), hipMemcpyHostToDevice, sp->ctx->stream));
        AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));            // (the upload reads `tables`)
    }
    sp->ld.on = true;
    return AW_OK;
} AW_NOEXCEPT_TAIL

// The checks the two equalizer setters share, answered in this order; lowest: the smallest map entry allowed (-1, or AW_EQ_KEEP)
static aw_status eq_setter_args(const aw_spatializer *sp, const aw_eq_definition *const *definitions, int32_t n_definitions, const int32_t *stream_definition,
                                int32_t lowest, bool check_without_definitions) {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    return awr::eq_map_args(definitions, n_definitions, stream_definition, sp->n_streams, lowest, check_without_definitions);
}

static aw_status eq_prepare_all(const aw_spatializer *sp, const aw_eq_definition *const *definitions, int32_t n_definitions, std::vector<awh::EqPrepared> *prep) {
    prep->resize((size_t)n_definitions);
    for (int32_t i = 0; i < n_definitions; ++i) {
        const aw_status st = awr::eq_prepare_checked(&definitions[i]->def, sp->sample_rate, (*prep)[(size_t)i]);
        if (st != AW_OK) {
            awr::set_error(std::string(aw_last_error_message()) + " (definition " + std::to_string(i) + ")");
            return st;
        }
    }
    return AW_OK;
}

// The stage's one allocation for these presets and this map, as awst::Equalizer lays it out: the state zeroed, the map, the headers and every
// preset's tab and plane queued for upload from *image (which stays until the copy has read it).
struct EqBuilt { awr::Buf<unsigned char> d; std::vector<unsigned char> image; int kmax = 0; size_t table_doubles = 0; };
static aw_status eq_build(aw_spatializer *sp, const std::vector<awh::EqPrepared> &prep, const std::vector<int32_t> &stream_map, EqBuilt *b) {
    for (const awh::EqPrepared &q : prep) {
        b->kmax = std::max(b->kmax, q.n_filters);
        b->table_doubles += q.tab.size() + q.plane.size();
    }
    const awst::Equalizer L{{(size_t)sp->n_streams}, prep.size(), (size_t)b->kmax, b->table_doubles};
    // what lies behind the state, as the layout states it: the map, the headers, then every preset's tab and plane
    b->image.assign(L.total - L.map.off, 0);
    auto at = [&](size_t off) { return b->image.data() + (off - L.map.off); };       // (every field starts on a multiple of 8 bytes but the map's end)
    int32_t *const map = reinterpret_cast<int32_t *>(at(L.map.off));
    awk::EqStagePreset *const headers = reinterpret_cast<awk::EqStagePreset *>(at(L.presets.off));
    double *const tables = reinterpret_cast<double *>(at(L.tables.off));
    for (int s = 0; s < sp->n_streams; ++s) map[s] = stream_map[(size_t)s];
    long long off = 0;
    for (size_t i = 0; i < prep.size(); ++i) {
        const awh::EqPrepared &q = prep[i];
        awk::EqStagePreset &h = headers[i];
        h.preamp = q.preamp; h.n_filters = q.n_filters; h.reserved = 0;
        h.tab_off = off; h.plane_off = off + (long long)q.tab.size();
        if (!q.tab.empty()) std::memcpy(tables + h.tab_off, q.tab.data(), q.tab.size() * sizeof(double));
        if (!q.plane.empty()) std::memcpy(tables + h.plane_off, q.plane.data(), q.plane.size() * sizeof(double));
        off += (long long)(q.tab.size() + q.plane.size());
    }
    const aw_status st = stage_alloc(sp, &b->d, L.total, L.reset_bytes);
    if (st != AW_OK) return st;
    AW_HIP_TRY(hipMemcpyAsync(b->d.get() + L.map.off, b->image.data(), b->image.size(), hipMemcpyHostToDevice, sp->ctx->stream));
    return AW_OK;
}

// Checks and the presets' tables first (a refusal leaves the stage as it was), then the one allocation and the upload (here, never on
// the process path).  Every call that installs presets starts the filter state from zero, and ends a running fade and a published target.
aw_status aw_spatializer_set_equalizer(aw_spatializer *sp, const aw_eq_definition *const *definitions, int32_t n_definitions,
                                       const int32_t *stream_definition) try {
    aw_status st = eq_setter_args(sp, definitions, n_definitions, stream_definition, -1, false);
    if (st != AW_OK) return st;
    std::vector<awh::EqPrepared> prep;
    if ((st = eq_prepare_all(sp, definitions, n_definitions, &prep)) != AW_OK) return st;
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));                // whatever still reads the old state, tables or image
    aw_spatializer::Equalizer &q = sp->eq;
    EqBuilt b;
    std::vector<int32_t> map((size_t)sp->n_streams, 0);
    if (n_definitions > 0) {
        for (int s = 0; stream_definition && s < sp->n_streams; ++s) map[(size_t)s] = stream_definition[s];
        if ((st = eq_build(sp, prep, map, &b)) != AW_OK) return st;
    }
    q.d = std::move(b.d);                                             // (no definitions: the stage is off)
    q.image = std::move(b.image);                                     // (the copy may still read it: it stays until the next setter call has synchronised)
    q.n_presets = n_definitions; q.kmax = b.kmax; q.table_doubles = b.table_doubles;
    (void)q.fade.reset();
    q.clock = awef::Clock{}; q.planned = false;
    q.prepared = std::move(prep);
    q.map = std::move(map);
    q.to_map.clear(); q.pending_map.clear();
    if (n_definitions == 0) q.map.clear();
    return AW_OK;
} AW_NOEXCEPT_TAIL

// Publishes a target; rules: device/eq_stage.hpp, host/eq_fade_plan.hpp.  Like an install it checks and prepares first and allocates, uploads
// and synchronises here, never on the process path: the stage's allocation is made anew for the presets still in use (active, faded to,
// published) and the new ones, the states are carried over, and the fade's record is made beside it.  The new entries replace the
// published target's, stream by stream; AW_EQ_KEEP leaves it.
aw_status aw_spatializer_set_equalizer_target(aw_spatializer *sp, const aw_eq_definition *const *definitions, int32_t n_definitions,
                                              const int32_t *stream_definition) try {
    static_assert(AW_EQ_KEEP == awk::kEqKeep, "AW_EQ_KEEP");
    aw_status st = eq_setter_args(sp, definitions, n_definitions, stream_definition, AW_EQ_KEEP, true);
    if (st != AW_OK) return st;
    if (!stream_definition && n_definitions == 0) return fail(AW_ERR_INVALID_ARGUMENT, "stream_definition is NULL (every stream takes definition 0) and there is no definition");
    std::vector<awh::EqPrepared> fresh;
    if ((st = eq_prepare_all(sp, definitions, n_definitions, &fresh)) != AW_OK) return st;
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));                // whatever still reads the old records
    aw_spatializer::Equalizer &q = sp->eq;
    const size_t n = (size_t)sp->n_streams, n_old = q.prepared.size();
    // a stage that is off counts as every stream at -1 (the reference's processor starts at unity)
    std::vector<int32_t> map = q.d ? q.map : std::vector<int32_t>(n, -1);
    std::vector<int32_t> to_map = q.fade ? q.to_map : std::vector<int32_t>(n, awk::kEqKeep);
    std::vector<int32_t> pending_map = q.fade ? q.pending_map : std::vector<int32_t>(n, awk::kEqKeep);
    bool published = q.clock.pending;
    for (size_t s = 0; s < n; ++s) {                                  // (the new presets follow the old ones)
        const int32_t e = stream_definition ? stream_definition[s] : 0;
        if (e == AW_EQ_KEEP) continue;
        pending_map[s] = e < 0 ? -1 : (int32_t)n_old + e;
        published = true;
    }
    // the presets some map still names, in their old order; the maps name them by their new index
    std::vector<int32_t> index(n_old + fresh.size(), -1);
    for (const std::vector<int32_t> *m : {&map, &to_map, &pending_map})
        for (int32_t e : *m) if (e >= 0) index[(size_t)e] = 0;
    std::vector<awh::EqPrepared> prepared;
    for (size_t i = 0; i < index.size(); ++i)
        if (index[i] == 0) {
            index[i] = (int32_t)prepared.size();
            prepared.push_back(i < n_old ? q.prepared[i] : std::move(fresh[i - n_old]));
        }
    for (std::vector<int32_t> *m : {&map, &to_map, &pending_map})
        for (int32_t &e : *m) if (e >= 0) e = index[(size_t)e];
    EqBuilt b;
    if ((st = eq_build(sp, prepared, map, &b)) != AW_OK) return st;
    const awst::Equalizer L{{n}, prepared.size(), (size_t)b.kmax, b.table_doubles};
    const awst::EqualizerFade F{{n}, (size_t)b.kmax};
    awr::Buf<unsigned char> fade;
    if ((st = stage_alloc(sp, &fade, F.total, F.reset_bytes)) != AW_OK) return st;
    // the states go on: a stream's rows are the first of its kmax, before and after
    const size_t row = (size_t)std::min(q.kmax, b.kmax) * 4 * sizeof(double);
    if (q.d && row)
        AW_HIP_TRY(hipMemcpy2DAsync(L.state.at(b.d.get()), (size_t)b.kmax * 32, eq_layout(sp).state.at(q.d.get()), (size_t)q.kmax * 32, row, n, hipMemcpyDeviceToDevice, sp->ctx->stream));
    if (q.fade && row)
        AW_HIP_TRY(hipMemcpy2DAsync(F.state_to.at(fade.get()), (size_t)b.kmax * 32, eq_fade_layout(sp).state_to.at(q.fade.get()), (size_t)q.kmax * 32, row, n, hipMemcpyDeviceToDevice, sp->ctx->stream));
    AW_HIP_TRY(hipMemcpyAsync(F.to_map.at(fade.get()), to_map.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, sp->ctx->stream));
    AW_HIP_TRY(hipMemcpyAsync(F.pending_map.at(fade.get()), pending_map.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, sp->ctx->stream));
    AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));                // (the copies read the old records and the vectors here)
    q.d = std::move(b.d);
    q.image = std::move(b.image);
    q.fade = std::move(fade);
    q.n_presets = (int)prepared.size(); q.kmax = b.kmax; q.table_doubles = b.table_doubles;
    q.prepared = std::move(prepared);
    q.map = std::move(map); q.to_map = std::move(to_map); q.pending_map = std::move(pending_map);
    q.clock.length = awef::fade_length(sp->sample_rate);
    q.clock.pending = published;
    q.planned = false;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_get_loudness(aw_spatializer *sp, int32_t first_stream, int32_t n, aw_stream_loudness *out) try {
    std::unique_lock<std::mutex> lk;
    aw_status st = get_begin(sp, first_stream, n, out, [](const aw_spatializer *s) { return s->ld.d.get(); }, "no loudness: aw_spatializer_set_loudness has not been called", &lk);
    if (st != AW_OK || !lk) return st;
    const awst::Loudness L = ld_layout(sp);
    const uint64_t cap_frames = (uint64_t)sp->ld.cap * (uint64_t)sp->ld.hop;
    const int64_t n_hops = (int64_t)(std::min(sp->ld.frames, cap_frames) / (uint64_t)sp->ld.hop);     // complete hops only
    std::vector<double> e((size_t)n * (size_t)std::max<int64_t>(n_hops, 1));
    std::vector<unsigned long long> nf;
    if (n_hops > 0)                                       // (the complete hops of each stream's row, not the whole field)
        AW_HIP_TRY(hipMemcpy2D(e.data(), (size_t)n_hops * 8, L.hops.at(sp->ld.d.get(), (size_t)first_stream), L.hops.per_stream * 8, (size_t)n_hops * 8, (size_t)n, hipMemcpyDeviceToHost));
    if ((st = get_field(L.nonfinite, sp->ld.d.get(), first_stream, n, &nf)) != AW_OK) return st;
    for (int32_t i = 0; i < n; ++i) {
        const awlo::Gated g = awlo::gate(e.data() + (size_t)i * (size_t)n_hops, n_hops, sp->ld.hop);
        aw_stream_loudness &o = out[i];
        o.integrated_lufs = g.integrated_lufs; o.relative_threshold_lufs = g.relative_threshold_lufs;
        o.blocks = g.blocks; o.blocks_above_absolute = g.blocks_above_absolute; o.blocks_gated = g.blocks_gated;
        o.reserved = 0;
        o.frames = sp->ld.frames;
        o.frames_dropped = sp->ld.frames > cap_frames ? sp->ld.frames - cap_frames : 0;
        o.nonfinite = nf[(size_t)i];
    }
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_get_loudness_hops(aw_spatializer *sp, int32_t stream, int64_t first_hop, int64_t n, double *out) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (stream < 0 || stream >= sp->n_streams) return fail(AW_ERR_INVALID_ARGUMENT, "stream out of range");
    if (first_hop < 0 || n < 0 || first_hop > sp->ld.cap || n > sp->ld.cap - first_hop) return fail(AW_ERR_INVALID_ARGUMENT, "hops out of range");
    if (n == 0) return AW_OK;
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out_host is NULL");
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));
    AW_HIP_TRY(hipMemcpy(out, ld_layout(sp).hops.at(sp->ld.d.get(), (size_t)stream) + (size_t)first_hop, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_loudness_gain(double lufs, double target_lufs, float *gain) try {
    if (!gain) return fail(AW_ERR_INVALID_ARGUMENT, "gain is NULL");
    if (!awlo::gain_to_target(lufs, target_lufs, gain)) return fail(AW_ERR_INVALID_ARGUMENT, "loudness and target must be finite (a silent stream has no gain)");
    return AW_OK;
} AW_NOEXCEPT_TAIL

// The one allocation is made here, never on the process path.  Off -> on: the history is zeroed, the peaks stay.
aw_status aw_spatializer_set_true_peak(aw_spatializer *sp, int32_t on) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (!on) { sp->tp.on = false; return AW_OK; }
    if (sp->tp.on) return AW_OK;
    if (!sp->ctx || sp->n_streams < 1) return fail(AW_ERR_INVALID_ARGUMENT, "the handle has no streams");
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    const aw_status st = tp_buffers(sp);
    if (st == AW_OK) sp->tp.on = true;
    return st;
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_get_true_peak(aw_spatializer *sp, int32_t first_stream, int32_t n, aw_stream_true_peak *out) try {
    std::unique_lock<std::mutex> lk;
    aw_status st = get_begin(sp, first_stream, n, out, [](const aw_spatializer *s) { return s->tp.d.get(); }, "no true peak: neither aw_spatializer_set_true_peak nor AW_GAIN_TRUE_PEAK_CEILING has been used", &lk);
    if (st != AW_OK || !lk) return st;
    const awst::TruePeak L = tp_layout(sp);
    std::vector<unsigned long long> nf;
    std::vector<uint32_t> pk, call;
    if ((st = get_field(L.nonfinite, sp->tp.d.get(), first_stream, n, &nf)) != AW_OK || (st = get_field(L.peaks, sp->tp.d.get(), first_stream, n, &pk)) != AW_OK ||
        (st = get_field(L.call_peaks, sp->tp.d.get(), first_stream, n, &call)) != AW_OK) return st;
    for (int32_t i = 0; i < n; ++i) {
        aw_stream_true_peak &o = out[i];
        o.true_peak[0] = awtp::bits_float(pk[2 * (size_t)i]); o.true_peak[1] = awtp::bits_float(pk[2 * (size_t)i + 1]);
        o.call_true_peak = awtp::bits_float(call[(size_t)i]);
        o.reserved = 0;
        o.frames = sp->tp.frames;
        o.nonfinite = nf[(size_t)i];
    }
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_true_peak_filter(float *out36) try {
    if (!out36) return fail(AW_ERR_INVALID_ARGUMENT, "out36 is NULL");
    float c[awtp::kCoefficients];
    awtp::filter(c);
    std::memcpy(out36, c, sizeof(c));
    return AW_OK;
} AW_NOEXCEPT_TAIL

// Checks first, then every allocation (here, never on the process path); the setting changes only when all of it worked.  Off -> on
// and a change of attack or hold start from empty history; the records stay until a reset unless the allocation is made anew.
aw_status aw_spatializer_set_limiter(aw_spatializer *sp, int32_t on, float ceiling, int32_t attack_frames, int32_t hold_frames) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (!on) { sp->lim.on = false; return AW_OK; }
    if (!sp->ctx || sp->n_streams < 1) return fail(AW_ERR_INVALID_ARGUMENT, "the handle has no streams");
    if (!(ceiling > 0.0f && ceiling <= 1.0f)) return fail(AW_ERR_INVALID_ARGUMENT, "ceiling must lie in (0, 1]");
    if (attack_frames < awlim::kMinAttack || attack_frames > awlim::kMaxAttack) return fail(AW_ERR_INVALID_ARGUMENT, "attack_frames must lie in [16, 512]");
    if (hold_frames < 0 || hold_frames > awlim::kMaxHold) return fail(AW_ERR_INVALID_ARGUMENT, "hold_frames must lie in [0, 1024]");
    if (sp->lv.gain_mode == AW_GAIN_PEAK_CEILING || sp->lv.gain_mode == AW_GAIN_TRUE_PEAK_CEILING)
        return fail(AW_ERR_INVALID_ARGUMENT, "a per-call ceiling gain cannot feed the limiter: set AW_GAIN_NONE or AW_GAIN_FIXED first");
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    const bool same_shape = sp->lim.d && sp->lim.attack == attack_frames && sp->lim.hold == hold_frames;
    if (sp->lim.on && same_shape) { sp->lim.ceiling = ceiling; return AW_OK; }
    aw_status st = AW_OK;
    const int64_t longest = std::max(sp->reserved_frames, sp->host_reserved_frames);
    if (longest > 0 && (st = grow_buf(sp, &sp->lim.d_y, (size_t)sp->n_streams * (size_t)longest * 2)) != AW_OK) return st;
    if (!same_shape) {
        awr::Buf<unsigned char> d;          // the new records are made first, then the old ones dropped
        if ((st = stage_alloc(sp, &d, awst::Limiter{{(size_t)sp->n_streams}, attack_frames, hold_frames}.total, 0)) != AW_OK) return st;
        if (sp->lim.d) AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));
        sp->lim.d = std::move(d);
        sp->lim.attack = attack_frames; sp->lim.hold = hold_frames; sp->lim.hist.cur = 0;
    }
    if ((st = lim_reset(sp, !same_shape)) != AW_OK) return st;
    tp_filter_once(sp);
    sp->lim.ceiling = ceiling;
    sp->lim.on = true;
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_spatializer_get_limiter(aw_spatializer *sp, int32_t first_stream, int32_t n, aw_stream_limiter *out) try {
    std::unique_lock<std::mutex> lk;
    aw_status st = get_begin(sp, first_stream, n, out, [](const aw_spatializer *s) { return s->lim.d.get(); }, "no limiter: aw_spatializer_set_limiter has not been called", &lk);
    if (st != AW_OK || !lk) return st;
    const awst::Limiter L = lim_layout(sp);
    std::vector<unsigned long long> lim, nf;
    std::vector<uint32_t> mg;
    if ((st = get_field(L.limited, sp->lim.d.get(), first_stream, n, &lim)) != AW_OK || (st = get_field(L.nonfinite, sp->lim.d.get(), first_stream, n, &nf)) != AW_OK ||
        (st = get_field(L.min_gain, sp->lim.d.get(), first_stream, n, &mg)) != AW_OK) return st;
    for (int32_t i = 0; i < n; ++i) {
        if (first_stream + i == 0) {     // the single-stream path's share (a handle of one stream)
            mg[(size_t)i] = std::min(mg[(size_t)i], sp->lim.host.min_gain_bits);
            lim[(size_t)i] += sp->lim.host.limited_frames; nf[(size_t)i] += sp->lim.host.nonfinite;
        }
        aw_stream_limiter &o = out[i];
        o.min_gain = awl::bits_float(mg[(size_t)i]);
        o.reserved = 0;
        o.frames = sp->lim.frames;
        o.limited_frames = lim[(size_t)i];
        o.nonfinite = nf[(size_t)i];
    }
    return AW_OK;
} AW_NOEXCEPT_TAIL

// Checks first, then the allocation and the upload (here, never on the process path); the setting changes only when all of it worked.
aw_status aw_spatializer_set_gain(aw_spatializer *sp, aw_gain_mode mode, const float *gains_host, int32_t n, float ceiling) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (const aw_status args = awr::gain_args(mode, gains_host, n, sp->n_streams, ceiling)) return args;
    if ((mode == AW_GAIN_PEAK_CEILING || mode == AW_GAIN_TRUE_PEAK_CEILING) && sp->lim.on)
        return fail(AW_ERR_INVALID_ARGUMENT, "a per-call ceiling gain cannot feed the limiter: switch the limiter off first");
    if (mode == AW_GAIN_NONE) { sp->lv.gain_mode = AW_GAIN_NONE; return AW_OK; }
    // the per-stream records below are sized by the stream count: a handle without streams or context has nothing to gain
    if (!sp->ctx || sp->n_streams < 1) return fail(AW_ERR_INVALID_ARGUMENT, "the handle has no streams");
    AW_HIP_TRY(hipSetDevice(sp->ctx->device));
    std::lock_guard<std::mutex> lk(sp->ctx->launch_mu);
    aw_status st = lv_buffers(sp);
    if (st != AW_OK) return st;
    if (mode == AW_GAIN_TRUE_PEAK_CEILING && !tp_runs(sp) && (st = tp_buffers(sp)) != AW_OK) return st;      // the true-peak kernel starts here, behind silence
    if (mode == AW_GAIN_FIXED) {
        std::vector<float> g((size_t)sp->n_streams);
        for (int32_t s = 0; s < sp->n_streams; ++s) g[(size_t)s] = gains_host[n == 1 ? 0 : s];
        // ordered behind whatever the context's stream still reads the old gains for
        AW_HIP_TRY(hipMemcpyAsync(lv_layout(sp).gains.at(sp->lv.d.get()), g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice, sp->ctx->stream));
        AW_HIP_TRY(hipStreamSynchronize(sp->ctx->stream));
        sp->lv.gains.swap(g);
    } else {
        sp->lv.gain_ceiling = ceiling;
    }
    sp->lv.gain_mode = mode;
    return AW_OK;
} AW_NOEXCEPT_TAIL

// No HIP call and no allocation: the encode kernels take the dither as launch arguments.
aw_status aw_spatializer_set_dither(aw_spatializer *sp, aw_dither mode, uint64_t seed, uint64_t first_stream) try {
    if (!sp) return fail(AW_ERR_INVALID_ARGUMENT, "sp is NULL");
    if (mode != AW_DITHER_NONE && mode != AW_DITHER_TPDF && mode != AW_DITHER_TPDF_HP) return fail(AW_ERR_INVALID_ARGUMENT, "unknown dither mode");
    sp->dither = mode;
    sp->dither_seed = seed;
    sp->dither_first_stream = first_stream;
    return AW_OK;
} AW_NOEXCEPT_TAIL

/* ---- mono engine (ConvolutionEngine) ------------------------------------------------------- */
aw_status aw_engine_create(aw_context *ctx, const float *hrir_samples, int32_t count, int32_t block_size,
                           aw_engine **out) try {
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!ctx || !hrir_samples) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (count <= 0 || block_size <= 0) return fail(AW_ERR_CONVOLUTION_SETUP_FAILED, "empty HRIR or non-positive block size");
    awr::Owner<aw_engine> owner(new (std::nothrow) aw_engine(), aw_engine_destroy);
    aw_engine *e = owner.get();
    if (!e) return fail(AW_ERR_OUT_OF_MEMORY, "engine");
    e->ctx = ctx; e->block_size = block_size;
    aw_status st = aw_hrir_create(ctx, hrir_samples, 1, count, 0.0, &e->hrir);
    const int32_t zero = 0;
    if (st == AW_OK) st = aw_spatializer_create(ctx, e->hrir, 1, &zero, &zero, 1, block_size, &e->sp);
    // the engine processes exactly block_size frames per call: everything process needs is allocated here, like
    // ConvolutionEngine.init (ConvolutionEngine.swift:97-138) — process does not allocate
    if (st == AW_OK) st = aw_spatializer_reserve_host(e->sp, block_size);
    if (st != AW_OK) return st;
    e->tmp_out.assign((size_t)block_size * 2, 0.f);
    *out = owner.release();
    return AW_OK;
} AW_NOEXCEPT_TAIL

void aw_engine_destroy(aw_engine *e) {
    if (!e) return;
    aw_spatializer_destroy(e->sp);
    aw_hrir_destroy(e->hrir);
    delete e;
}

int32_t aw_engine_block_size(const aw_engine *e) { return e ? e->block_size : 0; }

aw_status aw_engine_process(aw_engine *e, const float *input, float *output) try {
    if (!e || !input || !output) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    aw_status st = aw_spatializer_process_host(e->sp, input, e->tmp_out.data(), e->block_size);
    if (st != AW_OK) return st;
    for (int i = 0; i < e->block_size; ++i) output[i] = e->tmp_out[2 * (size_t)i];
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_engine_process_n(aw_engine *e, const float *input, float *output, int32_t frame_count) try {
    if (!e) return fail(AW_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (frame_count != e->block_size)      // guard count == blockSize else { return }  ConvolutionEngine.swift:372
        return fail(AW_ERR_BLOCK_SIZE_MISMATCH, "frameCount != blockSize: block ignored");
    return aw_engine_process(e, input, output);
} AW_NOEXCEPT_TAIL

aw_status aw_engine_process_accumulate(aw_engine *e, const float *input, float *acc) try {
    if (!e || !input || !acc) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    aw_status st = aw_spatializer_process_host(e->sp, input, e->tmp_out.data(), e->block_size);
    if (st != AW_OK) return st;
    for (int i = 0; i < e->block_size; ++i) acc[i] += e->tmp_out[2 * (size_t)i];    // vDSP_vadd, ConvolutionEngine.swift:393
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_engine_reset(aw_engine *e) try {
    if (!e) return fail(AW_ERR_INVALID_ARGUMENT, "engine is NULL");
    return aw_spatializer_reset(e->sp);
} AW_NOEXCEPT_TAIL

/* ---- callback-size adapter (RealtimeAudioProcessor) ---------------------------------------- */
aw_status aw_realtime_create(aw_context *ctx, const aw_hrir *hrir, int32_t n_renderers, const int32_t *left_track,
                             const int32_t *right_track, int32_t block_size, int32_t max_frames, aw_realtime **out) try {
    if (!out) return fail(AW_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!ctx || !hrir) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (block_size <= 0 || max_frames <= 0)      // precondition(blockSize > 0), (maxFramesPerCallback > 0)  :35-36
        return fail(AW_ERR_INVALID_ARGUMENT, "blockSize and maxFramesPerCallback must be positive");
    if (n_renderers < 0 || (n_renderers > 0 && (!left_track || !right_track)))
        return fail(AW_ERR_INVALID_ARGUMENT, "bad renderer list");
    awr::Owner<aw_realtime> owner(new (std::nothrow) aw_realtime(), aw_realtime_destroy);
    aw_realtime *p = owner.get();
    if (!p) return fail(AW_ERR_OUT_OF_MEMORY, "realtime");
    p->ctx = ctx; p->block_size = block_size; p->max_frames = max_frames; p->n_renderers = n_renderers;
    p->fifo_capacity = max_frames + block_size;                         // :41
    p->pending.assign((size_t)block_size * 2, 0.f);
    p->fifo_left.assign((size_t)p->fifo_capacity, 0.f);
    p->fifo_right.assign((size_t)p->fifo_capacity, 0.f);
    // everything a callback can need is allocated here, like the reference's init (RealtimeAudioProcessor.swift:30-62: pending, block and
    // FIFO buffers): one callback completes at most (block_size - 1 + max_frames) / block_size blocks = fewer than fifo_capacity frames
    p->ready_in.reserve((size_t)p->fifo_capacity * 2);
    p->ready_out.reserve((size_t)p->fifo_capacity * 2);
    const int used = std::min(n_renderers, 2);                          // min(renderers.count, 2)  :145
    if (used > 0) {
        int32_t lt[2] = {-1, -1}, rt[2] = {-1, -1};
        for (int r = 0; r < used; ++r) { lt[r] = left_track[r]; rt[r] = right_track[r]; }
        aw_status st = aw_spatializer_create(ctx, hrir, 2, lt, rt, 1, block_size, &p->sp);
        // device side: kernel scratch and the host entry's staging for the longest device call a callback can make (process must not allocate)
        if (st == AW_OK) st = aw_spatializer_reserve_host(p->sp, p->fifo_capacity);
        if (st != AW_OK) return st;
    }
    *out = owner.release();
    return AW_OK;
} AW_NOEXCEPT_TAIL

/* Introspection for the "process must not allocate" contract test: 0 bytes of host buffer capacity held (pending, ready, FIFO),
 * 1 bytes of grow-only device buffers (aw_spatializer_info 6), 2 device allocations made so far on the context (aw_spatializer_info 13). */
int64_t aw_realtime_info(const aw_realtime *p, int32_t what) {
    if (!p) return -1;
    switch (what) {
        case 0: return (int64_t)((p->pending.capacity() + p->ready_in.capacity() + p->ready_out.capacity() + p->fifo_left.capacity() + p->fifo_right.capacity()) * sizeof(float));
        case 1: return p->sp ? aw_spatializer_info(p->sp, 6) : 0;
        case 2: return p->ctx->device_allocs;
        default: return -1;
    }
}

void aw_realtime_destroy(aw_realtime *p) {
    if (!p) return;
    aw_spatializer_destroy(p->sp);
    delete p;
}

aw_status aw_realtime_process(aw_realtime *p, const float *in_l, const float *in_r, float *out_l, float *out_r,
                              int32_t frame_count) try {
    if (!p) return fail(AW_ERR_INVALID_ARGUMENT, "processor is NULL");
    if (frame_count <= 0) return AW_OK;                                 // guard frameCount > 0 else { return }  :84
    if (!in_l || !out_l || !out_r) return fail(AW_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (frame_count > p->max_frames)                                    // precondition  :85
        return fail(AW_ERR_INVALID_ARGUMENT, "frameCount exceeds maxFramesPerCallback");
    const int B = p->block_size;
    p->ready_in.clear();
    int off = 0;
    while (off < frame_count) {                                         // :88-116
        const int copy = std::min(B - p->pending_count, frame_count - off);
        for (int i = 0; i < copy; ++i) {
            p->pending[2 * (size_t)(p->pending_count + i)] = in_l[off + i];
            p->pending[2 * (size_t)(p->pending_count + i) + 1] = (in_r ? in_r : in_l)[off + i];   // mono dup :95-107
        }
        p->pending_count += copy;
        off += copy;
        if (p->pending_count == B) {
            // processPendingBlock (:141-172) — blocks completed inside one callback are convolved
            // together in one device call below; the result is block-size independent.
            p->ready_in.insert(p->ready_in.end(), p->pending.begin(), p->pending.end());
            p->pending_count = 0;
        }
    }
    const int ready_frames = (int)(p->ready_in.size() / 2);
    if (ready_frames > 0) {
        p->ready_out.assign((size_t)ready_frames * 2, 0.f);             // memset blockLeft/blockRight :142-143
        if (p->sp) {
            aw_status st = aw_spatializer_process_host(p->sp, p->ready_in.data(), p->ready_out.data(), ready_frames);
            if (st != AW_OK) return st;
        }
        for (int i = 0; i < ready_frames; ++i) {                        // FIFO push :166-171
            const int w = (p->fifo_read_index + p->fifo_count) % p->fifo_capacity;
            p->fifo_left[(size_t)w] = p->ready_out[2 * (size_t)i];
            p->fifo_right[(size_t)w] = p->ready_out[2 * (size_t)i + 1];
            p->fifo_count += 1;
        }
    }
    for (int i = 0; i < frame_count; ++i) {                             // drain :174-190
        if (p->fifo_count > 0) {
            out_l[i] = p->fifo_left[(size_t)p->fifo_read_index];
            out_r[i] = p->fifo_right[(size_t)p->fifo_read_index];
            p->fifo_read_index = (p->fifo_read_index + 1) % p->fifo_capacity;
            p->fifo_count -= 1;
        } else {
            out_l[i] = 0.f;
            out_r[i] = 0.f;
        }
    }
    return AW_OK;
} AW_NOEXCEPT_TAIL

aw_status aw_realtime_reset(aw_realtime *p) try {                           // :121-139
    if (!p) return fail(AW_ERR_INVALID_ARGUMENT, "processor is NULL");
    if (p->sp) {
        aw_status st = aw_spatializer_reset(p->sp);
        if (st != AW_OK) return st;
    }
    std::fill(p->pending.begin(), p->pending.end(), 0.f);
    std::fill(p->fifo_left.begin(), p->fifo_left.end(), 0.f);
    std::fill(p->fifo_right.begin(), p->fifo_right.end(), 0.f);
    p->pending_count = 0; p->fifo_read_index = 0; p->fifo_count = 0;
    return AW_OK;
} AW_NOEXCEPT_TAIL

/* ---- synthetic input --------------------------------------------------------------------------- */
aw_status aw_synth_fill(aw_context *ctx, float *dst, int32_t n_streams, int64_t frames, int32_t n_channels,
                        uint64_t seed, uint64_t first_stream) try {
    if (!ctx || !dst) return fail(AW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_streams <= 0 || frames <= 0 || n_channels <= 0) return fail(AW_ERR_INVALID_ARGUMENT, "non-positive size");
    AW_HIP_TRY(hipSetDevice(ctx->device));
    AW_HIP_TRY(awk::launch_synth_fill(dst, n_streams, frames * n_channels, seed, first_stream, ctx->stream));
    return AW_OK;
} AW_NOEXCEPT_TAIL

}  // extern "C"

aw_status awr::context_create_divided(int32_t device, int32_t copy_divisor, aw_context **out) { return context_create_impl(device, nullptr, false, out, copy_divisor); }

aw_status awr::eq_map_args(const aw_eq_definition *const *definitions, int32_t n_definitions, const int32_t *stream_definition, int32_t n_streams,
                           int32_t lowest, bool check_without_definitions) {
    if (n_definitions < 0) return fail(AW_ERR_INVALID_ARGUMENT, "n_definitions must be >= 0");
    if (n_definitions > 0 && !definitions) return fail(AW_ERR_INVALID_ARGUMENT, "definitions is NULL");
    for (int32_t i = 0; i < n_definitions; ++i)
        if (!definitions[i]) return fail(AW_ERR_INVALID_ARGUMENT, "definition " + std::to_string(i) + " is NULL");
    for (int s = 0; stream_definition && (n_definitions > 0 || check_without_definitions) && s < n_streams; ++s)
        if (stream_definition[s] < lowest || stream_definition[s] >= n_definitions)
            return fail(AW_ERR_INVALID_ARGUMENT, "stream_definition[" + std::to_string(s) + "] = " + std::to_string(stream_definition[s]) + " is outside [" +
                                                     std::to_string(lowest) + ", n_definitions)");
    return AW_OK;
}

aw_status awr::gain_args(aw_gain_mode mode, const float *gains_host, int32_t n, int32_t n_streams, float ceiling) {
    if (mode != AW_GAIN_NONE && mode != AW_GAIN_FIXED && mode != AW_GAIN_PEAK_CEILING && mode != AW_GAIN_TRUE_PEAK_CEILING)
        return fail(AW_ERR_INVALID_ARGUMENT, "unknown gain mode");
    if (mode == AW_GAIN_FIXED) {
        if (!gains_host) return fail(AW_ERR_INVALID_ARGUMENT, "gains_host is NULL");
        if (n != 1 && n != n_streams) return fail(AW_ERR_INVALID_ARGUMENT, "n must be 1 or the stream count");
        for (int32_t i = 0; i < n; ++i)
            if (!std::isfinite(gains_host[i])) return fail(AW_ERR_INVALID_ARGUMENT, "gains must be finite");
    }
    if ((mode == AW_GAIN_PEAK_CEILING || mode == AW_GAIN_TRUE_PEAK_CEILING) && !(ceiling > 0.0f && ceiling <= 1.0f)) return fail(AW_ERR_INVALID_ARGUMENT, "ceiling must lie in (0, 1]");
    return AW_OK;
}
