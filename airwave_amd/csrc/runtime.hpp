// runtime.hpp — internal C++ objects behind the opaque C handles of include/airwave_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/airwave_hip.h"
#include "device/kernels.hpp"
#include "host/device_buf.hpp"
#include "host/eq.hpp"
#include "host/eq_fade_plan.hpp"
#include "host/stage_records.hpp"

namespace awr {

void set_error(const std::string &msg);
aw_status fail(aw_status code, const std::string &msg);
aw_status fail_eq_filter(int enabled_index, int kind, int source_line, const std::string &msg);      // AW_ERR_EQ_INVALID_FILTER + aw_last_eq_filter_error
aw_status hip_fail(hipError_t e, const char *what);
// awh::eq_prepare of a definition (NULL: unity) with its refusals as the statuses and messages aw_eq_state_create gives (eq_runtime.cpp)
aw_status eq_prepare_checked(const awh::EqDefinition *def, double sample_rate, awh::EqPrepared &prep);
bool context_literal_resampler(const aw_context *ctx);
// The argument checks of the per-stream setters, by stream count, so that the single handle (runtime.cpp) and the multi-device handle
// (multi_runtime.cpp, which validates a whole argument before it touches a shard) answer with one order and one wording.
// eq_map_args: lowest = the smallest map entry allowed (-1, or AW_EQ_KEEP); gain_args: mode, gains and ceiling of aw_spatializer_set_gain.
aw_status eq_map_args(const aw_eq_definition *const *definitions, int32_t n_definitions, const int32_t *stream_definition, int32_t n_streams,
                      int32_t lowest, bool check_without_definitions);
aw_status gain_args(aw_gain_mode mode, const float *gains_host, int32_t n, int32_t n_streams, float ceiling);
// aw_context_create for a handle that drives several contexts side by side (multi_runtime.cpp): the host entry's copy pools of this context
// get max(1, default / copy_divisor) threads each, so that D contexts do not start D times the threads.  Not part of the ABI.
aw_status context_create_divided(int32_t device, int32_t copy_divisor, aw_context **out);
// The C ABI promises "no exceptions": every entry point that can allocate host memory (containers, strings, threads) is a
// function-try-block whose handler returns caught() — std::bad_alloc / std::length_error become AW_ERR_OUT_OF_MEMORY, anything else
// AW_ERR_INVALID_ARGUMENT with the exception's text in aw_last_error_message().  Handles under construction are held by Owner<> until
// the entry hands them out, so an exception on the way leaks nothing.
aw_status caught() noexcept;
#define AW_NOEXCEPT_TAIL catch (...) { return ::awr::caught(); }

#define AW_HIP_TRY(expr)                                          \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return ::awr::hip_fail(_e, #expr);  \
    } while (0)

template <class T> using Owner = std::unique_ptr<T, void (*)(T *)>;

}  // namespace awr

struct aw_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    awr::Event t0, t1;
    awr::Buf<awk::cf> d_tw1, d_twa, d_twb;                          // twiddle rows (FFTSetupManager analogue)
    awr::Buf<float> d_zeros;                                        // page of zeros (frames past the end of a call)
    bool literal_resampler = false;                                 // aw_context_set_resampler: aw_preset_activate resamples HRIRs with the literal vgenp call
    awk::LaunchCfg cfg;                                             // device properties + tuning knobs, read once at creation
    // Scratch pool (round 5): the grow-only HBM scratch of the partitioned and long-window kernels belongs to the CONTEXT and is
    // shared by every spatializer created on it — their calls are ordered on the context's stream, so one buffer of the largest
    // need serves them all, and a second spatializer (a preset change: HRIRManager.activatePreset builds a new renderer network
    // while the old one still plays, HRIRManager.swift:347-446) pays no second multi-GB hipMalloc.  launch_mu keeps one call's
    // launch sequence contiguous on the stream when two owners drive two handles of one context from two threads.
    awr::Buf<awk::cf> d_pool;                                       // (capacity: complex elements)
    std::mutex launch_mu;
    std::atomic<long long> device_allocs{0};                        // hipMalloc / hipHostMalloc calls made on behalf of this context's handles (tests: a reserved process path makes none)
    std::atomic<long long> sync_copies{0};                          // blocking hipMemcpy calls likewise (table uploads)
    // host-entry pipeline (aw_spatializer_process_host on a multi-stream batch): H2D of chunk k+1 || kernels of chunk k || D2H of chunk k-1
    struct CopyPool;                                                // a few host threads that copy slices of one buffer at a time (runtime.cpp)
    CopyPool *copy_pool_out = nullptr;                              // a second, smaller pool for the output direction (copy OUT of chunk k-1 beside copy IN of chunk k+1)
    CopyPool *copy_pool = nullptr;                                  // made with the pipeline objects; pageable caller buffers are bounced through page-locked chunks by it
    int copy_divisor = 1;                                           // both pools get max(1, default / copy_divisor) threads (awr::context_create_divided; 1 through the ABI's entries)
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    awr::Event ev_h2d[2], ev_run[2], ev_d2h[2];
};

struct aw_eq_definition {
    awh::EqDefinition def;
};

struct aw_hrir {
    aw_context *ctx = nullptr;
    int n_tracks = 0, taps = 0;
    double sample_rate = 0.0;
    std::vector<float> tracks;   // [n_tracks][taps], host
};

struct aw_spatializer {
    aw_context *ctx = nullptr;
    int n_channels = 0, n_pairs = 0, n_streams = 0, taps = 0;
    int path = 0;             // 0 fused single-partition overlap-save, 1 partitioned
    bool fused2 = false;      // path 0 on 16384-frame windows (polyphase, two output spectra): device/tile_ols2.hpp
    int ola_h = 0;            // path 0 on 8192-frame windows: calls with enough blocks run the overlap-add tile with blocks of 512 ola_h frames (device/tile_ola.hpp); 0: never
    int last_ola_h = 0;       // ola_h of the last call if it ran that tile, else 0
    int hop = 0, hist_len = 0, partitions = 1;
    awr::Buf<awk::cf2> d_tab;           // [partitions][pairs][N]
    awr::Buf<float> d_hist[2];
    int hist_cur = 0;
    // scratch of the partitioned / long-window kernels: the context's pool (aw_context::d_pool), grow-only; reserved_pool = what
    // aw_spatializer_reserve() asked of it for this spatializer (elements)
    size_t reserved_pool = 0;
    size_t scratch_budget = 0;          // bytes per stream chunk (AW_SPEC_SCRATCH_MB at create; 0 = from free memory at first use)
    bool cmac_group = false;            // partitioned path: block-group CMAC kernel instead of the marched one (> 8 pairs; AW_PART_CMAC=group)
    bool fwd_one_pair = false;          // partitioned path: forward kernel with one channel pair per workgroup (default for more than 4 pairs; AW_PART_FWD=1|2 forces either form)
    bool herm_ok = true;                // partitioned path, odd channel count: store/read only the non-redundant half of the last pair's spectrum
    // long-window path (device/tile_lw.hpp): chosen per call (awp::lw_choose, host/path_policy.hpp) for long calls of a path-1 spatializer and, past a measured HRIR length,
    // of a path-0 one; tables per window length, built on first use (aw_spatializer_reserve builds those of the plan its max_frames implies)
    struct LwPlan { int R = 0; awr::Buf<awk::LwTab> d_tab; awr::Buf<awk::LwTab2> d_tab16; awr::Buf<awk::cf> d_tw2, d_coarse, d_fine, d_step, d_tw_r, d_tw1m; };      // (move-only)
    std::vector<LwPlan> lw_plans;
    int lw_mode = -1;                   // AW_LW at create: -1 automatic (cost model), 0 never, 32/64/128 force that R where it fits
    std::vector<float> lw_tracks;       // the HRIR and channel map, kept for the lazily built tables
    std::vector<int32_t> lw_left, lw_right;
    int lw_n_tracks = 0;
    awr::Buf<float> d_lw_tracks;        // device copies of the same for the prep kernels (device/prep_kernels.hip), made with the first table set
    awr::Buf<int32_t> d_lw_left, d_lw_right;
    awr::Buf<float> d_tail;             // 32 floats: the last frame of the last stream of a call + zeros (wide split kernel, tile_lw.hpp)
    int last_lw_R = 0;                  // R of the last call's (first group of) windows (0: the partitioned kernels ran)
    int last_lw_R2 = 0;                 // R of its remainder window when the call ran as two groups
    int64_t reserved_frames = 0;        // aw_spatializer_reserve(): buffers are sized for calls up to this many frames
    // host-entry staging (grow-only; a multi-stream batch is staged in two chunks of streams each way: aw_spatializer_process_host)
    awr::Buf<float> d_stage_in, d_stage_out;
    // one-stream, callback-sized calls (aw_spatializer_process_planar, aw_engine_*, aw_realtime_*): page-locked staging that the kernels read
    // and write DIRECTLY over PCIe — no copy engine, no (de)interleave kernels: the caller's samples are (de)interleaved by the CPU on the way
    awr::Buf<float, awr::Kind::pinned> h_pin_in, h_pin_out;
    // multi-stream host entry on PAGEABLE caller buffers: page-locked bounce chunks (two each way), filled / drained by the context's copy threads
    awr::Buf<unsigned char, awr::Kind::pinned> h_bounce_in, h_bounce_out;       // (both slots each)
    // integer PCM entries (aw_spatializer_process_pcm / _process_host_pcm): the host entry's device PCM slots (two chunks each way; the
    // float32 formats use d_stage_in / d_stage_out themselves) and the device counter of its clipped samples
    awr::Buf<unsigned char> d_pcm_in, d_pcm_out;
    awr::Buf<unsigned long long> d_clip;
    // dither of the s16 / s24 encode (aw_spatializer_set_dither) and the frame position that keys it: frames processed since create /
    // reset, advanced once per call by sp_begin_call (aw_spatializer_info 18)
    int dither = 0;                               // aw_dither
    uint64_t dither_seed = 0, dither_first_stream = 0;
    uint64_t position = 0;
    // The output stages of the four batch entries, in pipeline order.  Each has ONE device allocation `d`, made by its setter (never on the
    // process path) and laid out as host/stage_records.hpp states, and counts the frames it saw since the last reset (the same for every
    // stream); `host` is what the single-stream page-locked path did on the CPU instead (added to stream 0's record on read).
    struct Stage { awr::Buf<unsigned char> d; uint64_t frames = 0; };
    struct PingPong {                                 // two history slots: a call reads slot cur and writes the other
        int cur = 0; bool ran = false;                // ran: this call queued the stage's kernel, so its history slot is the next call's
        void end_call(bool queued = true) { if (ran && queued) cur ^= 1; ran = false; }
    };
    // aw_spatializer_set_equalizer / _set_equalizer_target: the one stage in front of the meters; rules: device/eq_stage.hpp.  d: the stage is on
    struct Equalizer : Stage {
        int n_presets = 0, kmax = 0; size_t table_doubles = 0;
        std::vector<unsigned char> image;             // what the setter uploads behind the state (map, headers, tables): kept while the copy may read it
        // target changes (aw_spatializer_set_equalizer_target).  The presets the stage holds, as prepared: the target setter rebuilds the
        // stage's one table from those still in use and the new ones.  The three maps are the host's copies of the device's, moved as the
        // clock moves: once per call, by batch_end.
        std::vector<awh::EqPrepared> prepared;
        std::vector<int32_t> map, to_map, pending_map;
        awr::Buf<unsigned char> fade;                 // awst::EqualizerFade, made by the first target; an install drops it
        awef::Clock clock;
        awef::Plan plan; bool planned = false;        // the running call's cuts (batch_begin); planned: batch_end moves the clock by them
    } eq;
    struct Levels : Stage {                           // aw_spatializer_set_metering / _set_gain (either makes d); rules: device/levels.hpp
        bool metering = false;
        int gain_mode = 0; float gain_ceiling = 1.0f; // aw_gain_mode
        std::vector<float> gains;                     // FIXED: one per stream
        awl::Record host{};
        // what the last batch call applied, for aw_stream_levels::gain
        int applied_mode = 0;
        float applied_ceiling = 1.0f, applied_host_gain = 1.0f;
        bool applied_on_host = false;                 // PEAK_CEILING: the single-stream path computed it (applied_host_gain), else the call-local peaks hold it
        std::vector<float> applied_gains;
    } lv;
    double sample_rate = 0.0;                         // the HRIR's
    // aw_spatializer_set_loudness; rules: device/loudness.hpp.  hop: frames per hop (rate / 10); cap: hops recorded per stream; frames fixes the hop index
    struct Loudness : Stage { bool on = false; int64_t hop = 0, cap = 0; } ld;
    struct TruePeak : Stage {                         // aw_spatializer_set_true_peak, AW_GAIN_TRUE_PEAK_CEILING (either makes d); rules: device/truepeak.hpp
        bool on = false; PingPong hist;
        uint32_t pinned_call_bits = 0;                // the single-stream page-locked path under AW_GAIN_TRUE_PEAK_CEILING: the call's true peak, read back
    } tp;
    float tp_filter[36] = {}; bool tp_filter_built = false;      // c[p][k] of the true-peak interpolator: built by whichever of the true-peak and limiter setters runs first
    struct Limiter : Stage {                          // aw_spatializer_set_limiter (d is made anew when attack or hold change the halo); rules: device/limiter.hpp
        bool on = false; PingPong hist;
        int attack = 0, hold = 0; float ceiling = 0.0f;
        awr::Buf<float> d_y;                          // float32 staging the convolution kernels write y into while the limiter is on (the kernel is
                                                      // out of place): one chunk of streams, grow-only like the other staging
        awlim::Record host;
        std::vector<float> host_hist;                 // the single-stream path's history while it is the newer one
        bool hist_on_host = false;
    } lim;
    int64_t host_chunk_streams = 0;               // streams per staged chunk of the last host call (0: the whole batch in one piece, serial)
    int64_t host_chunk_reserved = 0, host_reserved_frames = 0;   // aw_spatializer_reserve_host: the chunking its buffers were sized for, and up to which call length
    // what the last aw_spatializer_reserve spent where (microseconds): float64 table build on host threads, table upload (hipMalloc +
    // hipMemcpy), scratch pool growth (hipMalloc) — bench.py's config.activation
    int64_t reserve_tables_us = 0, reserve_upload_us = 0, reserve_scratch_us = 0;
    awr::Buf<unsigned long long> d_dbg;    // AW_STAMPS diagnostic builds only (capacity: words)
    long long dbg_nwg = 0;
    // profiling of the dominant kernel
    bool profiling = false;
    awr::Event k0, k1;
    double kernel_ms_sum = 0.0;
    int kernel_launches = 0;
    long long dominant_frames = 0;         // output frames produced by the timed (dominant) launch of the last call
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // recorded, not yet read
    // per-launch stage timing (profiling only): every kernel of the step, by name
    struct StageRec { const char *name; hipEvent_t e0, e1; };
    struct StageStat { const char *name; double ms_sum; int launches; };
    std::vector<StageRec> stage_pending;
    std::vector<StageStat> stage_stats;
    std::vector<hipEvent_t> event_pool;
};

struct aw_engine {
    aw_context *ctx = nullptr;
    aw_hrir *hrir = nullptr;
    aw_spatializer *sp = nullptr;
    int block_size = 0;
    std::vector<float> tmp_out;   // [block][2]
};

struct aw_realtime {
    aw_context *ctx = nullptr;
    aw_spatializer *sp = nullptr;     // 1 stream, 2 input channels (L, R) -> first min(n,2) renderers
    int block_size = 0, max_frames = 0, fifo_capacity = 0, n_renderers = 0;
    std::vector<float> pending;       // [block][2] interleaved L,R
    std::vector<float> ready_in;      // completed blocks of this callback, interleaved
    std::vector<float> ready_out;
    std::vector<float> fifo_left, fifo_right;
    int pending_count = 0, fifo_read_index = 0, fifo_count = 0;
};
