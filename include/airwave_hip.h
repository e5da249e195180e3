/*
 * airwave_hip.h — C ABI of the MI355X-native batch HRIR spatializer (libairwave_hip.so).
 *
 * This is the drop-in boundary for ONE path of sallliisa/Airwave: the per-virtual-speaker
 * partitioned FFT convolution + stereo downmix (ConvolutionEngine / VirtualSpeaker /
 * RealtimeAudioProcessor / HRIRManager.activatePreset).  Every entry point cites the reference
 * interface it replaces (paths relative to the reference repository root).  Host code in any
 * language binds these symbols (Swift module map + wrapper: swift/; ctypes: airwave_amd/;
 * C++ RAII mirror: include/airwave_hip.hpp).  See INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; opaque handles; every function returns aw_status (0 = ok);
 *    no exceptions or callbacks cross the boundary; aw_last_error_message() gives detail.
 *  - a handle is single-threaded for process/reset (like ConvolutionEngine: "not thread-safe,
 *    one owner"); independent handles are independent.
 *  - creation may block and allocate (the reference builds engines on a background queue,
 *    HRIRManager.swift:347); aw_spatializer_process on device buffers does not allocate once
 *    aw_spatializer_reserve has sized the handle (or it has seen a call of that size class:
 *    scratch is grow-only).  The scratch of the multi-kernel paths is a pool of the CONTEXT,
 *    shared by its spatializers; a handle is still single-owner, handles of one context may be
 *    driven from different threads (their launch sequences are serialised).
 *  - there is NO CPU fallback: without a HIP device every create returns AW_ERR_NO_DEVICE.
 */
#ifndef AIRWAVE_HIP_H
#define AIRWAVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AW_API __attribute__((visibility("default")))

/* ---- status codes ---------------------------------------------------------------------------- */
typedef int32_t aw_status;
enum {
    AW_OK = 0,
    AW_ERR_INVALID_ARGUMENT = 1,         /* Swift precondition failures (RealtimeAudioProcessor.swift:35-36,85) */
    AW_ERR_OUT_OF_MEMORY = 2,
    AW_ERR_HIP = 3,                      /* any HIP runtime error; message has hipGetErrorString */
    AW_ERR_NO_DEVICE = 4,                /* no HIP device / ordinal out of range */
    AW_ERR_INVALID_CHANNEL_MAPPING = 5,  /* HRIRError.invalidChannelMapping  HRIRManager.swift:375-379 */
    AW_ERR_CONVOLUTION_SETUP_FAILED = 6, /* HRIRError.convolutionSetupFailed HRIRManager.swift:406-409,420-422 */
    AW_ERR_INVALID_CHANNEL_COUNT = 7,    /* WAVError/HRIRError.invalidChannelCount WAVLoader.swift:40-42, HRIRManager.swift:223 */
    AW_ERR_WAV_FILE_READ = 8,            /* WAVError.fileReadError   WAVLoader.swift:31-33,59-61 */
    AW_ERR_WAV_EMPTY_FILE = 9,           /* WAVError.emptyFile       WAVLoader.swift:44-46 */
    AW_ERR_WAV_UNSUPPORTED_FORMAT = 10,  /* WAVError.unsupportedFormat WAVLoader.swift:89-91 */
    AW_ERR_BLOCK_SIZE_MISMATCH = 11,     /* ConvolutionEngine.process(input:output:frameCount:) guard, ConvolutionEngine.swift:372 */
    AW_ERR_EQ_PARSE = 12,                /* EqualizerParseError                     EqualizerAPOParser.swift:8-21 */
    AW_ERR_EQ_INVALID_SAMPLE_RATE = 13,  /* ParametricEqualizerPreparationError.invalidSampleRate  ParametricEqualizerProcessor.swift:100-101 */
    AW_ERR_EQ_NON_FINITE_PREAMP = 14,    /* .nonFinitePreamp  :102 */
    AW_ERR_EQ_TOO_MANY_FILTERS = 15,     /* .tooManyFilters   :103 (also the maxFramesPerCallback guard, :148-150) */
    AW_ERR_EQ_INVALID_FILTER = 16,       /* .invalidFilter(index:error:)  :104; BiquadCoefficientError  BiquadCoefficientBuilder.swift:11-16 */
    AW_ERR_EQ_NOT_FOLDABLE = 17          /* aw_eq_fold_hrir: the equalizer's impulse response does not decay to the tolerance within the allowed length */
};
AW_API const char *aw_status_string(aw_status s);
AW_API const char *aw_last_error_message(void); /* thread-local, valid until the next failing call */
/* The structured part of the calling thread's last AW_ERR_EQ_INVALID_FILTER — what EqualizerRuntimeEffect.map builds
 * EqualizerAudioEffectError.invalidFilter(line:reason:) from (EqualizerRuntimeEffect.swift:80-100): the index among the ENABLED filters
 * (ParametricEqualizerPreparationError.invalidFilter(index:error:), ParametricEqualizerProcessor.swift:188-202), the
 * BiquadCoefficientError kind (aw_biquad_make) and that filter's sourceLine (0 if the definition carried none).  Returns 1 and fills
 * the non-NULL outputs, or 0 when the thread's last failing call was something else. */
AW_API int32_t aw_last_eq_filter_error(int32_t *enabled_index, int32_t *error_kind, int32_t *source_line);

/* ---- context: device + stream + twiddle tables -------------------------------------------------
 * Replaces FFTSetupManager.shared.getSetup(log2n:) (FFTSetupManager.swift:41-60): the twiddle
 * table is built once per context and shared by every spatializer/engine created on it. */
typedef struct aw_context aw_context;
AW_API aw_status aw_context_create(int32_t device_ordinal, aw_context **out);
/* Same, but launches on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
AW_API aw_status aw_context_create_on_stream(int32_t device_ordinal, void *hip_stream, aw_context **out);
/* Stream order (tests/test_gpu_stream_order.py, tests/test_stream_order_contract.py).  Every kernel, memset and copy of the device-buffer
 * entries is queued on the context's stream — the caller's, or the one aw_context_stream returns, on which a caller may queue work of its
 * own — so a producer queued there before a call and a consumer queued there after it need no host synchronisation, on a non-blocking
 * side stream as on the legacy default stream.
 *  - these only enqueue and return while earlier work on the stream is still running: aw_spatializer_process and _process_pcm on a
 *    reserved handle (every kernel path and every output stage), aw_spatializer_reset, aw_eq_state_process, aw_eq_process, aw_synth_fill.
 *    Handles of one context, and contexts on different streams, may be interleaved from one host thread; work of one context never waits
 *    behind another context's stream.
 *  - these synchronise the context's stream before they return, because the host reads or hands over memory then: aw_memcpy_h2d /
 *    aw_memcpy_d2h, the record getters (aw_spatializer_get_levels read on a busy stream returns the records of the finished calls), the
 *    host entries aw_spatializer_process_host / _process_host_pcm (ordered behind what the stream already holds), and the first
 *    long-window call of a handle that was not reserved, which builds its tables.  aw_spatializer_destroy waits for the stream before it
 *    frees, so a handle may be destroyed with its calls still queued (the handle first, then its context).
 *  - a caller's stream is never destroyed by the library. */
AW_API void aw_context_destroy(aw_context *ctx);
AW_API aw_status aw_context_synchronize(aw_context *ctx);
AW_API void *aw_context_stream(aw_context *ctx);          /* the hipStream_t kernels are launched on */
/* HIP-event stopwatch on the context's stream (bench.py times the kernels with these). */
AW_API aw_status aw_context_timer_start(aw_context *ctx);
AW_API aw_status aw_context_timer_stop(aw_context *ctx, float *elapsed_ms); /* records, syncs, returns ms */

/* The HBM scratch of the multi-kernel paths (long HRIRs, long calls) is ONE grow-only pool per context, shared by the
 * spatializers created on it.  aw_spatializer_reserve grows it as needed; a host that knows its largest batch can size it at
 * start-up instead (one large hipMalloc, whose wall time varies from 0.2 ms to seconds on MI355X boxes).  The analogue of
 * allocating every engine buffer in ConvolutionEngine.init (ConvolutionEngine.swift:97-138), hoisted to the context. */
AW_API aw_status aw_context_reserve_scratch(aw_context *ctx, size_t bytes);
AW_API size_t aw_context_scratch_bytes(const aw_context *ctx);

/* Measured ceilings of the device (bench / diagnostics; blocks, allocates its own buffers, never on a process path).
 * aw_context_bandwidth_probe: a read-only, a write-only and a copy kernel over `bytes` (>= 64 MiB) of HBM each, best of
 * `repetitions`; GB/s, the copy's figure counting bytes read + bytes written.  SURVEY.md 8d asks for this next to the
 * vendor peak the roofline is priced on.  aw_context_pcie_probe: page-locked host memory to the device, back, and both at
 * once (GB/s; duplex = bytes both ways / time) — the yardstick for aw_spatializer_process_host. */
AW_API aw_status aw_context_bandwidth_probe(aw_context *ctx, size_t bytes, int32_t repetitions, double *read_gbs,
                                            double *write_gbs, double *copy_gbs);
AW_API aw_status aw_context_pcie_probe(aw_context *ctx, size_t bytes, int32_t repetitions, double *h2d_gbs, double *d2h_gbs,
                                       double *duplex_gbs);

/* Device memory helpers for hosts without their own HIP bindings (Swift, ctypes). */
AW_API aw_status aw_device_alloc(aw_context *ctx, size_t bytes, void **dptr);
AW_API aw_status aw_device_free(aw_context *ctx, void *dptr);
AW_API aw_status aw_memcpy_h2d(aw_context *ctx, void *dst_device, const void *src_host, size_t bytes);
AW_API aw_status aw_memcpy_d2h(aw_context *ctx, void *dst_host, const void *src_device, size_t bytes);
/* Page-locked host memory (hipHostMalloc): buffers from here cross PCIe by DMA, without the HIP runtime's staging copy, when
 * handed to the host entries below.  The analogue of the caller-owned render buffers of AudioPipeline.swift:3-11. */
AW_API aw_status aw_host_alloc_pinned(aw_context *ctx, size_t bytes, void **ptr);
AW_API aw_status aw_host_free_pinned(aw_context *ctx, void *ptr);

/* ---- HRIR set --------------------------------------------------------------------------------
 * The planar impulse responses a preset provides (WAVData.audioData, WAVLoader.swift:12-17):
 * tracks is [n_tracks][taps] float32 on the HOST. */
typedef struct aw_hrir aw_hrir;
AW_API aw_status aw_hrir_create(aw_context *ctx, const float *tracks, int32_t n_tracks, int32_t taps,
                                double sample_rate, aw_hrir **out);
AW_API void aw_hrir_destroy(aw_hrir *h);
AW_API int32_t aw_hrir_track_count(const aw_hrir *h);
AW_API int32_t aw_hrir_taps(const aw_hrir *h);
AW_API double aw_hrir_sample_rate(const aw_hrir *h);

/* ---- batch spatializer -----------------------------------------------------------------------
 * n_streams independent streams, each = the engine network HRIRManager.activatePreset builds
 * (one ConvolutionEngine per (input channel, ear), HRIRManager.swift:366-418) plus the downmix
 * of RealtimeAudioProcessor.processPendingBlock (RealtimeAudioProcessor.swift:141-164) without
 * its two-renderer cap:  out_L = sum_c x_c * h[left_track[c]],  out_R = sum_c x_c * h[right_track[c]].
 * A channel with left_track[c] < 0 or right_track[c] < 0 is skipped (HRIRManager.swift:370-372);
 * an index >= n_tracks is AW_ERR_INVALID_CHANNEL_MAPPING (:375-379); no mapped channel at all is
 * AW_ERR_CONVOLUTION_SETUP_FAILED (:420-422).  block_hint: 0 = automatic (results do not depend on it).
 * Any n_in_channels > 0 and any HRIR length are accepted.  Tested on the GPU: 1 - 18, 24 and 32 channels (up to 16 on every
 * kernel path; beyond 16 there is no overlap-add tile and no long-window kernel, AW_OLA / AW_LW are ignored there and every call
 * runs the run-time-loop kernels of the fused or the partitioned path), HRIRs of up to 98 305 taps on the partitioned path and
 * up to 131 072 on the long-window kernels (tests/test_gpu_wide_layouts.py, tests/test_gpu_long_hrir.py). */
typedef struct aw_spatializer aw_spatializer;
AW_API aw_status aw_spatializer_create(aw_context *ctx, const aw_hrir *hrir, int32_t n_in_channels,
                                       const int32_t *left_track, const int32_t *right_track,
                                       int32_t n_streams, int32_t block_hint, aw_spatializer **out);
AW_API void aw_spatializer_destroy(aw_spatializer *sp);
/* Offline/batch entry: DEVICE buffers.  in: [stream][frames][n_in_channels] interleaved float32,
 * out: [stream][frames][2].  Any frames >= 1; state (the convolution tail) carries over to the
 * next call exactly like consecutive ConvolutionEngine.process calls.  Asynchronous on the
 * context stream. */
AW_API aw_status aw_spatializer_process(aw_spatializer *sp, const float *in_device, float *out_device, int64_t frames);
/* Same with HOST buffers; synchronous.  A multi-stream batch crosses PCIe in chunks of streams, double buffered on three HIP
 * streams (H2D of chunk k+1 || kernels of chunk k || D2H of chunk k-1; streams are independent, so chunks are); page-locked
 * buffers (aw_host_alloc_pinned) move by DMA directly, pageable ones are bounced through page-locked chunks by host copy threads.  Small batches and
 * single streams (the plug-in shaped calls of aw_engine_* / aw_realtime_*) go in one piece.
 * The call holds the context's launch lock from entry to return (other handles of the context wait for its whole PCIe time); on an
 * error the contents of out_host are unspecified and the streams' state is that of a failed call: aw_spatializer_reset before reuse.
 * Without aw_spatializer_reserve_host the first call also creates the pipeline's streams, events and copy threads. */
AW_API aw_status aw_spatializer_process_host(aw_spatializer *sp, const float *in_host, float *out_host, int64_t frames);
/* aw_spatializer_reserve plus the device-side staging of the host entry for calls of up to max_frames frames (two chunks
 * each way): afterwards aw_spatializer_process_host does not allocate either.  (The scratch pool is sized as aw_spatializer_reserve
 * sizes it — for the whole batch — although the host entry only ever runs one staged chunk of streams at a time; AW_SPEC_SCRATCH_MB
 * bounds it for hosts that never use the device entry.) */
AW_API aw_status aw_spatializer_reserve_host(aw_spatializer *sp, int64_t max_frames);
/* ---- integer PCM sample formats ---------------------------------------------------------------
 * The batch entries in any pair of sample formats: an offline host that holds 16- or 24-bit PCM hands it over as it is, and half
 * the bytes cross PCIe.  Layouts are those of aw_spatializer_process: input [stream][frames][n_in_channels], output
 * [stream][frames][2], elements of the given format; mixed pairs (s16 in, f32 out, ...) are allowed.  F32 / F32 through these
 * entries is aw_spatializer_process / aw_spatializer_process_host, bit for bit.
 *  - decode is aw_wav_load's rule: s16 (float)s / 32768, s24 (float)((double)s / 8388608), s32 (float)((double)s / 2147483648).
 *    Each scale is a power of two, so every PCM input is an exact float32 input to the same kernels.
 *  - encode is the inverse scale, rounded to nearest with ties to even, then saturated to the integer range (s32 computed in
 *    double); NaN encodes to 0.  A sample is clipped when the rounded value lies outside the integer range, or when it is NaN
 *    or +-inf.  No dither by default; aw_spatializer_set_dither (below) adds TPDF dither to s16 and s24 output.
 *  - a NULL handle or buffer, or an unknown format, returns AW_ERR_INVALID_ARGUMENT before any HIP call.  On a failed host call
 *    the output contents are unspecified, as for aw_spatializer_process_host. */
typedef int32_t aw_sample_format;
enum {
    AW_SAMPLE_F32 = 0,   /* float32 */
    AW_SAMPLE_S16 = 1,   /* int16 */
    AW_SAMPLE_S24 = 2,   /* packed 3-byte little-endian two's complement, as in WAV */
    AW_SAMPLE_S32 = 3    /* int32 */
};
AW_API int32_t aw_sample_format_bytes(aw_sample_format f);   /* 4, 2, 3, 4; 0 for an unknown format */
/* DEVICE buffers (any byte alignment), asynchronous on the context stream.  The call's streams go through the host entry's
 * float32 staging in chunks of streams (AW_HOST_CHUNK_MB of input bytes), so memory is bounded by a chunk, not the batch.
 * clipped_device: NULL, or a device uint64 that the call atomically adds its clipped-sample count to. */
AW_API aw_status aw_spatializer_process_pcm(aw_spatializer *sp, const void *in_device, aw_sample_format in_format,
                                            void *out_device, aw_sample_format out_format, int64_t frames, uint64_t *clipped_device);
/* HOST buffers, synchronous: the chunked PCIe pipeline of aw_spatializer_process_host, chunked by PCM input bytes; each chunk is
 * decoded and encoded on the device.  clipped: NULL, or receives the call's clipped-sample count. */
AW_API aw_status aw_spatializer_process_host_pcm(aw_spatializer *sp, const void *in_host, aw_sample_format in_format,
                                                 void *out_host, aw_sample_format out_format, int64_t frames, uint64_t *clipped);
/* aw_spatializer_reserve_host for these formats: afterwards neither PCM entry allocates for calls of up to max_frames frames. */
AW_API aw_status aw_spatializer_reserve_pcm(aw_spatializer *sp, int64_t max_frames, aw_sample_format in_format,
                                            aw_sample_format out_format);
/* Dither of the integer encode.  Applies to every later s16 / s24 encode of this handle's PCM entries (device, host, and the
 * single-stream path of the host entry).  s32 and f32 output are never dithered: float32's 24-bit mantissa is coarser than an
 * s32 LSB for nearly every sample, so s32 stays the rounding above.  AW_DITHER_NONE, the default, is that rounding byte for byte.
 *  - position p: frames processed by this handle since it was created or last passed to aw_spatializer_reset.  Every process entry
 *    advances it (float, PCM, host, device, planar; aw_spatializer_info 18); after a failed call it is as unspecified as the state.
 *    The noise of a sample depends only on (seed, global stream, p, ear), so splitting a call in two, or chunking a batch by streams,
 *    changes no output bit.
 *  - first_stream: the global index of this handle's stream 0, as in aw_synth_fill: a batch sharded over several handles gets the
 *    noise of one handle holding every stream.
 *  - with g = first_stream + s, K = ((seed ^ 0xD1B54A32D192ED03) + g) * 0x9E3779B97F4A7C15 (mod 2^64) and splitmix64 as in
 *    aw_synth_fill, the dither d in LSB of ear e (0 left, 1 right) of frame p is
 *      AW_DITHER_TPDF:    h = splitmix64(K + 2p + e), d = (float)((int32_t)(h >> 40) - (int32_t)((h >> 16) & 0xFFFFFF)) * 2^-24
 *      AW_DITHER_TPDF_HP: r(p) = ((splitmix64(K + p) >> (e ? 16 : 40)) & 0xFFFFFF) * 2^-24, d = r(p) - r(p - 1)  (p - 1 mod 2^64):
 *                         high-pass TPDF, stateless (r(p - 1) is recomputed from the counter)
 *    and the sample encodes as s16 rintf(x * 32768.0f + d), s24 rintf(x * 8388608.0f + d), saturated; the NaN and clip rules are
 *    those above (a sample that the dither pushes past full scale counts as clipped).  d lies in (-1, 1): triangular, 1/6 LSB^2.
 *  - a NULL handle or an unknown mode returns AW_ERR_INVALID_ARGUMENT before any HIP call.  Allocates nothing.  Do not call it while
 *    a process call on the same handle is running. */
typedef int32_t aw_dither;
enum {
    AW_DITHER_NONE = 0,      /* round to nearest, ties to even (the default) */
    AW_DITHER_TPDF = 1,      /* triangular (two uniforms), white */
    AW_DITHER_TPDF_HP = 2    /* triangular, high-pass (difference of consecutive uniforms) */
};
AW_API aw_status aw_spatializer_set_dither(aw_spatializer *sp, aw_dither mode, uint64_t seed, uint64_t first_stream);
/* Per-stream output levels and gain of the four batch entries: aw_spatializer_process, _process_pcm, _process_host and
 * _process_host_pcm.  An output ear is the sum of up to 14 convolutions, so output beyond full scale is the normal case; the meter
 * tells a host which of its streams clipped and by how much, the gain prevents it, and neither moves float32 output over PCIe.  The
 * planar entry and the engine / realtime adapters are neither metered nor gained.  With the meter off and the gain AW_GAIN_NONE
 * (the defaults) every entry launches the kernels and writes the bytes it always has.
 *  - the meter sees every float32 output sample y BEFORE the gain.  A y that is NaN or +-inf counts in nonfinite and in nothing else;
 *    otherwise peak = max(peak, |y|) and energy += (double)y * (double)y, per ear.  The product is exact in double; the order of the
 *    additions is unspecified, so energy may differ between runs by summation order (at most N * 2^-53 relative over N samples) while
 *    every other field is exact.  clipped counts what the integer encodes of this stream clipped, after gain and dither.
 *  - the gain multiplies once in float32: the gained sample is (float)(y * g), and the encode rules above (dither included) see that
 *    value; float32 output is that value.
 *  - AW_GAIN_PEAK_CEILING gives every stream, in every call, g = p > c ? c / p : 1, where p is the larger of the stream's two ear peaks
 *    over THIS CALL's frames (non-finite samples excluded) and c / p is the correctly rounded float32 quotient.  It is per call: a host
 *    that splits a file over calls in time should meter first (pass one), then set AW_GAIN_FIXED gains (pass two), or every call gets
 *    a gain of its own.  A ceiling of exactly 1 can still clip by one LSB, through the rounding of the quotient or through dither.
 *  - levels accumulate over every later batch call until aw_spatializer_reset_levels or aw_spatializer_reset.  Chunking a batch by
 *    streams (AW_HOST_CHUNK_MB), sharding it over handles, pinned or pageable, aligned or unaligned buffers change no output bit and
 *    no field but energy's summation order; splitting calls in time changes none either under AW_GAIN_NONE and AW_GAIN_FIXED.
 *  - peak and energy are raw material.  Integrated loudness in LUFS (K-weighting and gating, ITU-R BS.1770) is provided:
 *    aw_spatializer_set_loudness below; so is the true peak (4x oversampling): aw_spatializer_set_true_peak, and the gain that holds a
 *    true-peak ceiling, AW_GAIN_TRUE_PEAK_CEILING.  A look-ahead true-peak limiter is provided too: aw_spatializer_set_limiter
 *    below; compressors and multiband dynamics are a host's business and are not provided. */
typedef struct aw_stream_levels {
    float    peak[2];      /* max |y| per ear (left, right) over finite samples, before gain */
    float    gain;         /* the gain the last call applied to this stream (1 if none) */
    uint32_t reserved;     /* 0 */
    double   energy[2];    /* sum of y^2 per ear, before gain */
    uint64_t frames;       /* frames metered */
    uint64_t clipped;      /* samples this stream's integer encodes clipped (after gain and dither) */
    uint64_t nonfinite;    /* NaN / inf samples, both ears */
} aw_stream_levels;        /* 56 bytes */
typedef int32_t aw_gain_mode;
enum {
    AW_GAIN_NONE = 0,          /* no gain (the default) */
    AW_GAIN_FIXED = 1,         /* one gain per stream, given by the host */
    AW_GAIN_PEAK_CEILING = 2,  /* per stream and call: scale down to the ceiling where the call's peak exceeds it */
    AW_GAIN_TRUE_PEAK_CEILING = 3   /* the same over the call's TRUE peak: g = tp > c ? c / tp : 1 (aw_stream_true_peak, below) */
};
/* on != 0: allocates the per-stream records at once (a later aw_spatializer_reserve / _reserve_pcm still means "no allocation on the
 * process path") and meters every later batch call; 0: stops metering, the records stay readable.  Do not call these four setters while
 * a process call on the same handle is running. */
AW_API aw_status aw_spatializer_set_metering(aw_spatializer *sp, int32_t on);
/* Synchronises the context's stream and copies the records of streams [first_stream, first_stream + n) to out_host.  A range outside the
 * handle's streams returns AW_ERR_INVALID_ARGUMENT, as does a handle on which neither set_metering nor set_gain was ever called. */
AW_API aw_status aw_spatializer_get_levels(aw_spatializer *sp, int32_t first_stream, int32_t n, aw_stream_levels *out_host);
/* Zeroes every record (asynchronous on the context's stream); the meter and gain settings stay. */
AW_API aw_status aw_spatializer_reset_levels(aw_spatializer *sp);
/* AW_GAIN_NONE: gains_host, n and ceiling are ignored.  AW_GAIN_FIXED: n finite gains, n == 1 (every stream) or n == the stream count,
 * uploaded by this call (never on the process path); ceiling is ignored.  AW_GAIN_PEAK_CEILING and AW_GAIN_TRUE_PEAK_CEILING:
 * 0 < ceiling <= 1; gains_host and n are ignored.  A NULL handle, an unknown mode, a bad n, a NaN / inf gain, a bad ceiling or (for a mode
 * other than AW_GAIN_NONE) a handle without streams returns AW_ERR_INVALID_ARGUMENT before any HIP call, and the previous setting stays. */
AW_API aw_status aw_spatializer_set_gain(aw_spatializer *sp, aw_gain_mode mode, const float *gains_host, int32_t n, float ceiling);
/* Per-stream integrated loudness (ITU-R BS.1770-4) of the four batch entries, measured on the device from the float32 output y BEFORE
 * the gain — the level meter's tap — so that a host can bring every stream to a target such as -16 or -23 LUFS without moving float32
 * output over PCIe: pass one measures, aw_loudness_gain gives the AW_GAIN_FIXED gains, pass two writes the file
 * (examples/offline_batch_loudness.c).  Off by default; while it is off every entry launches the kernels and writes the bytes it always
 * has.  The planar entry and the engine / realtime adapters are not measured.
 *  - K-weighting: per ear, the shelf and the high-pass biquad in Float64, their coefficients derived for the HRIR's sample rate
 *    (aw_hrir_sample_rate) from the analog prototypes behind the standard's 48 kHz table (shelf f0 = 1681.974450955533 Hz,
 *    G = 3.999843853973347 dB, Q = 0.7071752369554196, band gain exponent 0.4996667741545416; high-pass f0 = 38.13547087602444 Hz,
 *    Q = 0.5003270373238773, numerator 1, -2, 1; bilinear transform with K = tan(pi f0 / fs)).  At 48 kHz these are the table values.
 *    A NaN or +-inf y enters the filters as 0 and counts in nonfinite.
 *  - hop energies: a hop is rate / 10 frames (100 ms); E[s][h] = the sum of (k_L^2 + k_R^2) over the frames of hop h of stream s, k the
 *    K-weighted output, both ears with channel weight 1.  The device keeps [stream][ceil(10 max_seconds)] doubles; frames past that
 *    capacity are not measured and are reported in frames_dropped.  aw_spatializer_get_loudness_hops returns them raw: momentary and
 *    short-term loudness and LRA are sums over them that a host can form.
 *  - gating, on the host at read-out, over complete hops only: block j covers hops j .. j+3 (400 ms, 75 % overlap),
 *    z_j = (E[j] + .. + E[j+3]) / (4 hop), l_j = -0.691 + 10 log10 z_j; the absolute gate keeps l_j > -70; the relative threshold is
 *    -0.691 + 10 log10(mean of z over those blocks) - 10; integrated_lufs is -0.691 + 10 log10(mean of z over the blocks above both).
 *    With no such block it is -INFINITY (and so is the threshold with no block above the absolute gate).
 *  - chunking a batch by streams (AW_HOST_CHUNK_MB), pinned or pageable buffers and sharding over handles change no bit of any hop
 *    energy; splitting calls in time changes them by Float64 summation order only, and a given split gives the same bits every time.
 *  - aw_spatializer_reset and aw_spatializer_reset_levels zero the hop energies, the filter state and the frame count. */
typedef struct aw_stream_loudness {
    double   integrated_lufs;           /* gated loudness, LUFS; -INFINITY when no block passes the gates */
    double   relative_threshold_lufs;   /* the relative gate, LUFS */
    uint32_t blocks;                    /* complete 400 ms blocks */
    uint32_t blocks_above_absolute;     /* ... above -70 LUFS */
    uint32_t blocks_gated;              /* ... above both gates: what integrated_lufs averages */
    uint32_t reserved;                  /* 0 */
    uint64_t frames;                    /* frames of the measured calls since the last reset */
    uint64_t frames_dropped;            /* of those, frames past the capacity: not measured */
    uint64_t nonfinite;                 /* NaN / inf samples, both ears, that entered the filters as 0 */
} aw_stream_loudness;                   /* 56 bytes */
/* on != 0: allocates the filter state and the hop energies of max_seconds per stream at once (never on the process path; a capacity
 * other than the one held makes new, empty records) and measures every later batch call; 0: stops measuring, the records stay readable
 * and max_seconds is ignored.  A NULL handle, an HRIR sample rate that is not a finite positive multiple of 10 Hz, or a max_seconds that
 * is <= 0 or not finite returns AW_ERR_INVALID_ARGUMENT before any HIP call.  Do not call it while a process call on the same handle is
 * running. */
AW_API aw_status aw_spatializer_set_loudness(aw_spatializer *sp, int32_t on, double max_seconds);
/* Synchronises the context's stream, copies the hop energies of streams [first_stream, first_stream + n) and gates them on the host. */
AW_API aw_status aw_spatializer_get_loudness(aw_spatializer *sp, int32_t first_stream, int32_t n, aw_stream_loudness *out_host);
/* The raw hop energies [first_hop, first_hop + n) of one stream (the hop in progress included); the range must lie in the capacity. */
AW_API aw_status aw_spatializer_get_loudness_hops(aw_spatializer *sp, int32_t stream, int64_t first_hop, int64_t n, double *out_host);
/* *gain = 10^((target_lufs - lufs) / 20) as float32.  A NULL gain, a non-finite loudness (a silent stream measures -INFINITY) or target,
 * or a gain that is no finite float32 returns AW_ERR_INVALID_ARGUMENT and leaves *gain alone. */
AW_API aw_status aw_loudness_gain(double lufs, double target_lufs, float *gain);
/* Per-stream true peak (ITU-R BS.1770-4 Annex 2; dBTP = 20 log10 of it) of the four batch entries, measured on the device from the float32
 * output y BEFORE the gain — the level meter's tap — the figure every loudness delivery specification sets beside its LUFS target
 * (usually -1 dBTP).  The sample peak of aw_stream_levels under-reads it by up to 3 dB: a sine at a quarter of the sample rate, sampled at
 * 45 degrees, reads -3.01 dB.  examples/offline_batch_true_peak.c brings every stream to -16 LUFS and -1 dBTP.  Off by default; while it is
 * off and the gain is not AW_GAIN_TRUE_PEAK_CEILING every entry launches the kernels and writes the bytes it always has.  The planar
 * entry and the engine / realtime adapters are not measured.
 *  - the interpolator: 4x oversampling at every sample rate by a 49-tap Hann-windowed sinc,
 *    h[j] = sinc((j - 24) / 4) * (0.5 - 0.5 cos(2 pi j / 48)), j = 0 .. 48, formed in double and rounded once to float32 (the libebur128
 *    construction; BS.1770's own table is an example — EBU Tech 3341's +0.2 / -0.4 dB is the measure).  Phase 0 is the identity; the
 *    phases p = 1, 2, 3 have twelve taps c[p][k] = h[p + 4k], which aw_true_peak_filter returns.
 *  - per ear and frame n, with v[i] = y[i] where finite, else 0 (counted in nonfinite), and v[i] before the first measured frame 0:
 *    t_p[n] = fmaf(c[p][11], v[n-11], .. fmaf(c[p][1], v[n-1], c[p][0] * v[n]) ..) in float32, and the true peak is the largest of
 *    |v[n]|, |t_1[n]|, |t_2[n]|, |t_3[n]| over the frames: never below aw_stream_levels.peak.  The filter's six frames of lookahead are
 *    not flushed: the last frames of a call contribute their windows when the next call brings later frames.
 *  - every field is a pure function of the stream's samples since the last reset: chunking a batch by streams (AW_HOST_CHUNK_MB), sample
 *    formats, pinned or pageable buffers, sharding over handles AND splitting calls in time change no bit.
 *  - AW_GAIN_TRUE_PEAK_CEILING (aw_spatializer_set_gain, 0 < ceiling <= 1) gives every stream, in every call, g = tp > c ? c / tp : 1
 *    with tp the stream's call_true_peak, and runs the measurement kernel in every call whether or not set_true_peak is on.  Like
 *    AW_GAIN_PEAK_CEILING it is per call: a host that splits a file over calls in time should measure first (pass one), then set
 *    AW_GAIN_FIXED gains of c / true_peak (pass two).  The first 11 windows of a call look back at the UNGAINED frames of the call
 *    before.  Dither and the rounding of the integer encode come after the gain and can exceed the ceiling by the order of one LSB.
 *  - aw_spatializer_reset and aw_spatializer_reset_levels zero the peaks, the counts and the carried frames. */
typedef struct aw_stream_true_peak {
    float    true_peak[2];   /* per ear, linear full scale, since the last reset; >= aw_stream_levels.peak */
    float    call_true_peak; /* larger ear over the last measured call */
    uint32_t reserved;       /* 0 */
    uint64_t frames;         /* frames measured */
    uint64_t nonfinite;      /* NaN / inf samples that entered as 0 */
} aw_stream_true_peak;       /* 32 bytes */
/* on != 0: allocates the per-stream records at once (never on the process path) and measures every later batch call; switching it on
 * from off zeroes the carried frames — frames of unmeasured calls are not predecessors — while the peaks stay until a reset.  0: stops
 * measuring, the records stay readable.  A NULL handle or a handle without streams returns AW_ERR_INVALID_ARGUMENT before any HIP call.  Do not call it while a
 * process call on the same handle is running. */
AW_API aw_status aw_spatializer_set_true_peak(aw_spatializer *sp, int32_t on);
/* Synchronises the context's stream and copies the records of streams [first_stream, first_stream + n) to out_host.  A range outside the
 * handle's streams returns AW_ERR_INVALID_ARGUMENT, as does a handle on which neither set_true_peak nor AW_GAIN_TRUE_PEAK_CEILING was
 * ever used. */
AW_API aw_status aw_spatializer_get_true_peak(aw_spatializer *sp, int32_t first_stream, int32_t n, aw_stream_true_peak *out_host);
/* The coefficients the library uses: out36[(p - 1) * 12 + k] = c[p][k], p = 1 .. 3. */
AW_API aw_status aw_true_peak_filter(float out36[36]);
/* Look-ahead true-peak limiter on the output of the four batch entries, on the device: a stream can be brought to its loudness target
 * (AW_GAIN_FIXED) AND held under a true-peak ceiling without moving float32 output over PCIe (examples/offline_batch_limiter.c).  Off by
 * default; while it is off every entry launches the kernels and writes the bytes it always has.  The planar entry and the engine /
 * realtime adapters are not limited.  Per stream, stereo-linked, with n the frame index since the last reset, c the ceiling,
 * L = attack_frames (attack = release), H = hold_frames, g_s the stream's AW_GAIN_FIXED gain (1 under AW_GAIN_NONE), W = L + 12 + H and
 * D = L + 11:
 *  - u[n][e] = (float)(y[n][e] * g_s) — the gain's one float32 product, made inside the limiter: the scale / encode kernels then run
 *    without gain, and aw_stream_levels.gain stays the fixed gain.  The meter, the loudness and the true peak keep tapping y.
 *  - p[n]: the larger ear of the true-peak detector above over v = u where finite, else 0 (counted in nonfinite); the same
 *    coefficients and fmaf order as aw_stream_true_peak.
 *  - r[n] = p[n] > c ? c / p[n] correctly rounded : 1 (1 before the first frame); q[n] = floor(r[n] * 2^30) as uint32.
 *  - m[n] = min(q[n] .. q[n - (W - 1)]); S[n] = m[n] + .. + m[n - (L - 1)] in uint64 (exact in any order);
 *    g[n] = (float)((double)S[n] / ((double)L * 2^30)).
 *  - z[n][e] = (float)(u[n - D][e] * g[n]), u = 0 before the stream's first frame.  z goes where y went: float32 output, or the
 *    integer encode with its dither; clipped counts what the encode of z clipped.  A non-finite y comes out non-finite, D frames later.
 *  - g[n] <= r[k] for every detector frame k in [n - D - H, n - D + 11]: no sample of z exceeds c by more than the rounding of c / p
 *    and of the product, and the gain is flat across the twelve frames of an isolated peak's window, whose true peak lands at c up to
 *    float32 rounding.  Dense material can overshoot c slightly between such windows while the gain moves: measured on noise at 2.5
 *    times full scale, 1.4e-3 of c at attack 16 / hold 0, 4e-5 at 64 / 128, 7e-6 and less from 256 / 256 on (DESIGN.md has the table).
 *  - latency: D frames (aw_spatializer_info 24).  The last D frames of a file come out when the host feeds D more frames of zeros.
 *  - every bit of z and every field is a pure function of the stream's samples since the last reset: chunking a batch by streams
 *    (AW_HOST_CHUNK_MB), sample formats, pinned or pageable buffers, sharding over handles AND splitting calls in time change none.
 *    This is why the per-call gains AW_GAIN_PEAK_CEILING and AW_GAIN_TRUE_PEAK_CEILING cannot be combined with it.
 *  - aw_spatializer_reset and aw_spatializer_reset_levels zero the records and the carried frames. */
typedef struct aw_stream_limiter {
    float    min_gain;        /* lowest g applied since the last reset (1 if never limited) */
    uint32_t reserved;        /* 0 */
    uint64_t frames;          /* frames that went through the limiter */
    uint64_t limited_frames;  /* of those, output frames with g < 1 */
    uint64_t nonfinite;       /* NaN / inf samples that entered the detector as 0 */
} aw_stream_limiter;          /* 32 bytes */
/* on != 0: 0 < ceiling <= 1, 16 <= attack_frames <= 512, 0 <= hold_frames <= 1024.  Allocates the records, the carried frames (the last
 * W + L + 9 frames of u per stream, in two slots) and the float32 staging the convolution kernels write into while the limiter is on
 * (sized for what aw_spatializer_reserve / _reserve_pcm / _reserve_host have reserved so far; a reserve made afterwards sizes it too), so
 * that a reserved process path still does not allocate.  Switching it on from off, or changing attack or hold, starts from empty
 * history.  0: switches it off; the other arguments are ignored and the records stay readable.  A NULL handle, a handle without streams,
 * a ceiling outside (0, 1] or not finite, attack_frames or hold_frames out of range, or a gain mode of AW_GAIN_PEAK_CEILING /
 * AW_GAIN_TRUE_PEAK_CEILING returns AW_ERR_INVALID_ARGUMENT before any HIP call and leaves the previous setting; while the limiter is
 * on, aw_spatializer_set_gain refuses those two modes likewise.  Do not call it while a process call on the same handle is running. */
AW_API aw_status aw_spatializer_set_limiter(aw_spatializer *sp, int32_t on, float ceiling, int32_t attack_frames, int32_t hold_frames);
/* Synchronises the context's stream and copies the records of streams [first_stream, first_stream + n) to out_host.  A range outside the
 * handle's streams returns AW_ERR_INVALID_ARGUMENT, as does a handle on which set_limiter was never switched on. */
AW_API aw_status aw_spatializer_get_limiter(aw_spatializer *sp, int32_t first_stream, int32_t n, aw_stream_limiter *out_host);
/* StereoAudioProcessing.process shape (AudioPipeline.swift:3-11) for a 1-stream, 2-channel
 * spatializer: planar HOST buffers, input_right may be NULL (mono duplication). Zero latency. */
AW_API aw_status aw_spatializer_process_planar(aw_spatializer *sp, const float *input_left, const float *input_right,
                                               float *output_left, float *output_right, int32_t frame_count);
/* Sizes every internal device buffer for calls of up to max_frames frames, so that the process entries never
 * allocate afterwards (the reference allocates all engine state in ConvolutionEngine.init, ConvolutionEngine.swift:97-138,
 * and nothing in process; creation may block, process must not).  Optional: without it buffers grow on first use. */
AW_API aw_status aw_spatializer_reserve(aw_spatializer *sp, int64_t max_frames);
/* ConvolutionEngine.reset() for every engine of every stream (ConvolutionEngine.swift:397-407). */
AW_API aw_status aw_spatializer_reset(aw_spatializer *sp);
AW_API int32_t aw_spatializer_stream_count(const aw_spatializer *sp);
AW_API int32_t aw_spatializer_channel_count(const aw_spatializer *sp);
/* Introspection for benches/tests: 0 fft length, 1 hop, 2 partitions, 3 path (0 fused, 1 partitioned),
 * 4 history frames, 5 output frames produced by the launch that aw_spatializer_kernel_time() times
 * (the interior-tile launch of the last call; the few boundary tiles are a second, untimed launch),
 * 6 bytes of grow-only internal device buffers currently allocated (sized by aw_spatializer_reserve or by the largest call so far),
 * 7 rows R of the last call's windows when it ran on the long-window kernels (windows of R x 4096 frames; 0: it ran on the
 *   fused / partitioned kernels that 0-3 describe).  The kernel set is chosen per call; results do not depend on it.
 * 8 rows of the remainder window of a call that ran as two groups of windows, 9 long-window table sets built so far,
 * 10 / 11 / 12 microseconds the last aw_spatializer_reserve spent on the float64 table build (host threads) / the table upload /
 *   growing the context's scratch pool, 13 device or page-locked allocations and 14 blocking table uploads made so far on behalf
 *   of the context's handles (a reserved process path makes neither), 15 streams per staged chunk of the last host-entry call,
 * 18 frames processed since create / the last aw_spatializer_reset (the dither's frame position, aw_spatializer_set_dither),
 * 19 the level meter is on (aw_spatializer_set_metering), 20 the aw_gain_mode of the batch entries (aw_spatializer_set_gain),
 * 21 the loudness measurement is on (aw_spatializer_set_loudness), 22 the true-peak measurement is on (aw_spatializer_set_true_peak),
 * 23 the limiter is on (aw_spatializer_set_limiter), 24 its latency D in frames (0 while it is off),
 * 25 presets the equalizer stage holds (aw_spatializer_set_equalizer, aw_spatializer_set_equalizer_target; 0 and no fade: the stage is off),
 * 26 the largest enabled-filter count among them, 27 frames left of the running fade to a new target (0: none), 28 a target is published
 * and has not begun (1 / 0). */
AW_API int64_t aw_spatializer_info(const aw_spatializer *sp, int32_t what);
/* Average device time of the dominant kernel over the launches since the last call (HIP events
 * on the context stream); used for bench.py's roofline object.  Returns launches counted. */
AW_API aw_status aw_spatializer_set_profiling(aw_spatializer *sp, int32_t enabled);
AW_API int32_t aw_spatializer_kernel_time(aw_spatializer *sp, double *avg_ms, const char **kernel_name);
/* While profiling is on every kernel launch of the partitioned path (and the history carry of every path) is bracketed by
 * HIP events of its own; this iterates the per-kernel sums since profiling was switched on: index 0, 1, ... until it
 * returns 0.  total_ms / launches are over all calls; names are static strings. */
AW_API int32_t aw_spatializer_stage_time(aw_spatializer *sp, int32_t index, const char **name, double *total_ms, int32_t *launches);

/* Diagnostic builds only (library compiled with -DAW_STAMPS=1, see tools/archive/stamps.py): copies the
 * per-workgroup phase time stamps of the last fused-kernel launch to host_out as
 * [workgroup][16] uint64 shader-clock values.  The shipped library returns AW_ERR_INVALID_ARGUMENT. */
AW_API aw_status aw_spatializer_debug_stamps(aw_spatializer *sp, uint64_t *host_out, int64_t capacity_words,
                                             int64_t *n_workgroups);

/* ---- mono engine: ConvolutionEngine (ConvolutionEngine.swift:14-408) ---------------------------
 * init?(hrirSamples:blockSize:) :68 / process(input:output:) :232 / processAndAccumulate :388 /
 * reset() :397.  HOST buffers of exactly block_size frames. */
typedef struct aw_engine aw_engine;
AW_API aw_status aw_engine_create(aw_context *ctx, const float *hrir_samples, int32_t count, int32_t block_size,
                                  aw_engine **out);
AW_API void aw_engine_destroy(aw_engine *e);
AW_API aw_status aw_engine_process(aw_engine *e, const float *input, float *output);
/* frame_count != block_size returns AW_ERR_BLOCK_SIZE_MISMATCH and leaves output untouched
 * (the Swift array wrapper silently returns, ConvolutionEngine.swift:370-373). */
AW_API aw_status aw_engine_process_n(aw_engine *e, const float *input, float *output, int32_t frame_count);
AW_API aw_status aw_engine_process_accumulate(aw_engine *e, const float *input, float *output_accumulator);
AW_API aw_status aw_engine_reset(aw_engine *e);
AW_API int32_t aw_engine_block_size(const aw_engine *e);

/* ---- callback-size adapter: RealtimeAudioProcessor (RealtimeAudioProcessor.swift:11-191) --------
 * Renderer r convolves with hrir tracks (left_track[r], right_track[r]); like the reference only
 * the first min(n_renderers, 2) renderers run, fed from the left / right input (:145-147).
 * Pending-buffer + FIFO semantics, latency block_size - callback frames, silence on underflow. */
typedef struct aw_realtime aw_realtime;
AW_API aw_status aw_realtime_create(aw_context *ctx, const aw_hrir *hrir, int32_t n_renderers,
                                    const int32_t *left_track, const int32_t *right_track, int32_t block_size,
                                    int32_t max_frames_per_callback, aw_realtime **out);
AW_API void aw_realtime_destroy(aw_realtime *p);
AW_API aw_status aw_realtime_process(aw_realtime *p, const float *input_left, const float *input_right,
                                     float *left_output, float *right_output, int32_t frame_count);
AW_API aw_status aw_realtime_reset(aw_realtime *p);
/* Everything a callback needs is allocated by aw_realtime_create (RealtimeAudioProcessor.init, :30-62); this lets a host or a
 * test check it: 0 bytes of host buffer capacity held, 1 bytes of grow-only device buffers, 2 device allocations made so far
 * on the context.  None of them moves across aw_realtime_process calls. */
AW_API int64_t aw_realtime_info(const aw_realtime *p, int32_t what);

/* ---- host-side data model (no GPU needed) ----------------------------------------------------- */
/* WAVLoader.load (WAVLoader.swift:26-99): any RIFF/WAVE -> planar float32. */
typedef struct aw_wav aw_wav;
AW_API aw_status aw_wav_load(const char *path, aw_wav **out);
AW_API void aw_wav_destroy(aw_wav *w);
AW_API double aw_wav_sample_rate(const aw_wav *w);
AW_API int32_t aw_wav_channel_count(const aw_wav *w);
AW_API int32_t aw_wav_frame_count(const aw_wav *w);
AW_API const float *aw_wav_channel(const aw_wav *w, int32_t channel);   /* frame_count floats */
AW_API const float *aw_wav_planar(const aw_wav *w);                     /* [channels][frames] */

/* InputLayout (VirtualSpeaker.swift:59-100).  Speakers are identified by their case name
 * ("FL", "FR", "FC", "LFE", "BL", "BR", "SL", "SR", "TFL", ... ) or, for .custom, the custom name. */
typedef struct aw_layout aw_layout;
AW_API aw_status aw_layout_detect(int32_t channel_count, aw_layout **out);      /* InputLayout.detect :88-99 */
AW_API aw_status aw_layout_create(const char *const *speaker_names, int32_t count, const char *name, aw_layout **out);
AW_API void aw_layout_destroy(aw_layout *l);
AW_API int32_t aw_layout_count(const aw_layout *l);
AW_API const char *aw_layout_speaker(const aw_layout *l, int32_t index);
AW_API const char *aw_layout_name(const aw_layout *l);

/* HRIRChannelMap (VirtualSpeaker.swift:103-347): speaker -> (left-ear track, right-ear track). */
typedef struct aw_channel_map aw_channel_map;
AW_API aw_status aw_map_hesuvi14(const aw_layout *speakers, aw_channel_map **out);          /* :270-297 */
AW_API aw_status aw_map_hesuvi7(const aw_layout *speakers, aw_channel_map **out);           /* :224-250 */
AW_API aw_status aw_map_interleaved_pairs(const aw_layout *speakers, aw_channel_map **out); /* :126-159 */
AW_API aw_status aw_map_split_blocks(const aw_layout *speakers, aw_channel_map **out);      /* :200-209 */
AW_API aw_status aw_map_parse_text(const char *text, aw_channel_map **out);                 /* parseHeSuViFormat :301-346 */
AW_API void aw_map_destroy(aw_channel_map *m);
AW_API int32_t aw_map_count(const aw_channel_map *m);
/* getIndices(for:) :115-117 — returns 1 and fills the indices when the speaker is mapped, else 0. */
AW_API int32_t aw_map_get(const aw_channel_map *m, const char *speaker, int32_t *left_ear, int32_t *right_ear);
/* The per-speaker loop of activatePreset (HRIRManager.swift:366-379,420-422): fills
 * left_track/right_track[layout count] with -1 for unmapped speakers. */
AW_API aw_status aw_map_resolve(const aw_channel_map *m, const aw_layout *layout, int32_t n_tracks,
                                int32_t *left_track, int32_t *right_track);

/* Resampler.resampleHighQuality (Resampler.swift:31-68), the INTENDED linear interpolation
 * out[i] = lerp(input, i * fromRate / toRate); see DESIGN.md for the vDSP_vgenp divergence. */
AW_API int32_t aw_resample_output_count(int32_t count, double from_rate, double to_rate);
AW_API aw_status aw_resample(const float *input, int32_t count, double from_rate, double to_rate, float *output,
                             int32_t output_capacity, int32_t *output_count);
/* The LITERAL call the reference makes (Resampler.swift:56-65): vDSP_vramp(0, stride) into a control vector, then
 * vDSP_vgenp(A = input, B = control, C = output, N = outputCount, M = input.count), as Apple documents vgenp: the knots
 * (B[m], A[m]) define a piecewise-linear function that is evaluated at the INTEGERS n = 0..N-1 (C[n] = A[0] for n <= B[0],
 * A[M-1] past the last knot).  With B[m] = m * stride that is lerp(input, n / stride) — the inverse of the intended ratio:
 * 48 -> 96 kHz yields input[2n] then holds the last sample, 48 -> 44.1 kHz stretches the response instead of compressing it.
 * Same output length as aw_resample.  Optional; nothing selects it unless asked (aw_context_set_resampler). */
AW_API aw_status aw_resample_vgenp(const float *input, int32_t count, double from_rate, double to_rate, float *output,
                                   int32_t output_capacity, int32_t *output_count);
/* Which of the two aw_preset_activate uses when it resamples an HRIR: 0 = intended interpolation (default), 1 = literal vgenp. */
AW_API aw_status aw_context_set_resampler(aw_context *ctx, int32_t literal_vgenp);

/* HRIRManager.activatePreset body (HRIRManager.swift:347-446): load WAV -> choose map (7 tracks:
 * hesuvi7, else hesuvi14; or `custom_map`) -> resolve -> resample HRIR to target rate when it
 * differs by > 0.01 Hz -> build the spatializer.  *hrir_out (optional) receives the HRIR handle
 * the spatializer was built from (caller destroys both). */
AW_API aw_status aw_preset_activate(aw_context *ctx, const char *wav_path, double target_sample_rate,
                                    const aw_layout *input_layout, const aw_channel_map *custom_map,
                                    int32_t n_streams, aw_spatializer **spatializer_out, aw_hrir **hrir_out);

/* Seeded synthetic input on the device: U(-0.5,0.5) counter RNG,
 * value(stream, i) as oracle/airwave_oracle.h:orc_synth_value.  dst: [n_streams][frames][n_channels]. */
AW_API aw_status aw_synth_fill(aw_context *ctx, float *dst_device, int32_t n_streams, int64_t frames,
                               int32_t n_channels, uint64_t seed, uint64_t first_stream);

/* ==== Parametric EQ (the effect that follows the spatializer) ======================
 * Mirrors BiquadCoefficientBuilder, EqualizerAPOParser, ParametricEqualizerState and
 * ParametricEqualizerProcessor for a batch of independent stereo streams held in HBM
 * ([stream][frames][2] interleaved L,R float32 — the spatializer's output layout).  Arithmetic is
 * Float64 like the reference's; the time axis is evaluated chunk-parallel (device/eq_cascade.hpp), so
 * results agree with the sequential recurrence to Float64 rounding (<= 1 ulp of the Float32 output). */

/* BiquadCoefficientBuilder.make  BiquadCoefficientBuilder.swift:29-107.  type: 0 peaking, 1 lowShelf,
 * 2 highShelf.  coefficients_out = {b0, b1, b2, a1, a2}.  On AW_ERR_EQ_INVALID_FILTER *error_kind is the
 * BiquadCoefficientError: 1 invalidSampleRate, 2 invalidFrequency, 3 invalidQ, 4 nonFiniteInput,
 * 5 nonFiniteCoefficients (error_kind may be NULL). */
AW_API aw_status aw_biquad_make(int32_t type, double gain_db, double frequency_hz, double q, double sample_rate,
                                double coefficients_out[5], int32_t *error_kind);

/* EqualizerDefinition / EqualizerFilter  EqualizerPreset.swift:9-27 (host object). */
typedef struct aw_eq_definition aw_eq_definition;
AW_API aw_status aw_eq_definition_create(double preamp_db, aw_eq_definition **out);
AW_API aw_status aw_eq_definition_add_filter(aw_eq_definition *d, int32_t is_enabled, int32_t type, double frequency_hz,
                                             double gain_db, double q);
/* EqualizerFilter.sourceLine / sourceNumber of filter `index` (defaults: index + 1, none = -1). */
AW_API aw_status aw_eq_definition_set_source(aw_eq_definition *d, int32_t index, int32_t source_line, int64_t source_number);
AW_API void aw_eq_definition_destroy(aw_eq_definition *d);
AW_API double aw_eq_definition_preamp_db(const aw_eq_definition *d);
AW_API int32_t aw_eq_definition_filter_count(const aw_eq_definition *d);
/* source_number_out: -1 when the directive carried no number (nil).  Any out pointer may be NULL. */
AW_API aw_status aw_eq_definition_filter(const aw_eq_definition *d, int32_t index, int32_t *source_line, int64_t *source_number,
                                         int32_t *is_enabled, int32_t *type, double *frequency_hz, double *gain_db, double *q);
/* EqualizerAPOParser.parse(data:filename:)  EqualizerAPOParser.swift:36-151.  On AW_ERR_EQ_PARSE the
 * issues are written to issues_out as "line N: reason" / "reason" joined by "; " (the text of
 * EqualizerParseError.errorDescription without the filename prefix), truncated to issues_capacity. */
AW_API aw_status aw_eq_parse(const void *data, size_t size, aw_eq_definition **out, char *issues_out, size_t issues_capacity);

/* ParametricEqualizerState  ParametricEqualizerProcessor.swift:16-98, prepared by
 * ParametricEqualizerProcessor.prepare(definition:sampleRate:) :168-212, for n_streams streams.
 * definition may be NULL (unity).  On AW_ERR_EQ_INVALID_FILTER aw_last_error_message() names the filter. */
typedef struct aw_eq_state aw_eq_state;
AW_API aw_status aw_eq_state_create(aw_context *ctx, const aw_eq_definition *definition, double sample_rate,
                                    int32_t n_streams, aw_eq_state **out);
AW_API void aw_eq_state_destroy(aw_eq_state *s);
AW_API aw_status aw_eq_state_reset(aw_eq_state *s);                                     /* reset() :49-56 */
/* process(...) :58-91 on device buffers, in place allowed; asynchronous on the context stream. */
AW_API aw_status aw_eq_state_process(aw_eq_state *s, const float *in_device, float *out_device, int64_t frames);
AW_API int32_t aw_eq_state_filter_count(const aw_eq_state *s);
AW_API double aw_eq_state_preamp_linear(const aw_eq_state *s);

/* The equalizer FOLDED INTO THE HRIR (batch hosts; round 6).  In the reference's graph the equalizer follows the spatializer
 * (AudioEffectGraph.swift:195-211: spatial effect, then equalizer) and, between two setTarget calls, is a linear time-invariant filter
 * (preamp x biquad cascade, ParametricEqualizerProcessor.swift:58-91), so EQ(x * h) = x * (h * g) with g its impulse response.  This
 * entry convolves every HRIR track with g once, on the host, in Float64 with the reference's own recurrence; a spatializer created
 * from the folded tracks then applies both effects in its one pass over the audio — instead of ParametricEqualizerState.process
 * re-reading and re-writing every stereo frame with ten sequential Float64 sections.  g is cut after response_taps = the smallest L
 * with sum_{n >= L} |g[n]| <= tail_tolerance x max |g|; the result differs from EQ-after-spatializer by at most *tail_bound x the
 * spatializer output's peak (tail_bound <= tail_tolerance; 1e-7 is two orders below the 1e-5 parity tolerance).
 *   tracks: [n_tracks][taps] at sample_rate (resampled like HRIRManager.swift:389-403 does, if the device rate differs)
 *   out_tracks: NULL = only *out_taps is computed (= taps + response_taps - 1); else [n_tracks][*out_taps]
 * AW_ERR_EQ_NOT_FOLDABLE: the response does not decay to the tolerance within max_taps - taps + 1 frames (a narrow band at a few Hz):
 * the host keeps the cascade (aw_eq_state_process / aw_eq_process after the spatializer).  Validation and its errors as
 * aw_eq_state_create.  definition NULL = unity (the tracks come back unchanged).  Host only: no device work. */
AW_API aw_status aw_eq_fold_hrir(const aw_eq_definition *definition_or_null, double sample_rate, const float *tracks, int32_t n_tracks,
                                 int32_t taps, double tail_tolerance, int32_t max_taps, float *out_tracks, int32_t *out_taps,
                                 int32_t *response_taps, double *tail_bound);

/* Equalizer of the batch entries (the reference's graph order: spatializer, then equalizer — AudioEffectGraph.swift:195-211;
 * one preset per output device — DeviceProfileManager).  definitions[0 .. n_definitions): the presets; stream_definition[s], s < stream count:
 * the preset of stream s, -1 = this stream is not equalized; NULL = every stream takes preset 0.  n_definitions == 0 switches the stage off.
 * Runs at the spatializer's sample rate (the HRIR's).
 *  - arithmetic: both ears of an equalized stream's convolution output go through ParametricEqualizerState.process of its preset
 *    (:58-91: preamp, the enabled biquads in Float64, one rounding to float32, the subnormal flush), bit for bit what aw_eq_state_process
 *    over the same calls gives; the Float64 state is carried from call to call.  A stream mapped to -1 keeps its samples.
 *  - position: in the four batch entries (aw_spatializer_process, _process_pcm, _process_host, _process_host_pcm), between the convolution
 *    and the first meter, in place — loudness, true peak, levels, every gain mode, the limiter, the dither and the encode see the equalized
 *    signal.  aw_spatializer_process_planar does not run it: the plug-in path has aw_eq, with its crossfades.
 *  - with the stage off a call queues what it queued before this entry existed, and every output bit is the same.
 *  - chunking a batch by streams (AW_HOST_CHUNK_MB), sample formats, pinned or pageable buffers and sharding over handles change no bit;
 *    splitting calls in time moves the kernel's chunk boundaries and changes the last bit of some samples (reassociation in Float64).
 *  - state: aw_spatializer_reset zeroes the filter state; every call that installs presets does too.  An install never crossfades: a
 *    setting that changes while audio plays is published with aw_spatializer_set_equalizer_target (next entry), which fades to it over
 *    20 ms as the reference does; the plug-in path keeps aw_eq for that (aw_eq_set_target, below).
 *  - the definitions are read during the call and not kept.  The call makes the stage's one device allocation (state, map, tables); no
 *    batch entry allocates for it afterwards, and it needs no staging.  Do not call it while a process call on the same handle is running.
 * Errors: a preset that cannot be prepared returns what aw_eq_state_create returns for it (AW_ERR_EQ_*; aw_last_eq_filter_error for a bad
 * filter) and aw_last_error_message() also names the definition's index.  A NULL handle, n_definitions < 0, NULL definitions with
 * n_definitions > 0, a NULL entry, or a map entry outside [-1, n_definitions) returns AW_ERR_INVALID_ARGUMENT.  A call that fails leaves
 * the previous stage as it was. */
AW_API aw_status aw_spatializer_set_equalizer(aw_spatializer *sp, const aw_eq_definition *const *definitions, int32_t n_definitions,
                                              const int32_t *stream_definition);

/* A target change of the batch entries' equalizer (ParametricEqualizerProcessor.setTarget, :226-228, :253-374): publishes a target that
 * the stage fades to over T = max(1, round(0.020 * sample rate)) frames, half away from zero, at the spatializer's rate.  Not an install:
 * aw_spatializer_set_equalizer keeps its meaning (install, zero the state, no fade) and also ends a running fade and a published target.
 * stream_definition[s]: p in [0, n_definitions) — stream s fades to a freshly zeroed state of definitions[p], also when that definition is
 * the one it already runs (the reference fades between two state objects); -1 — it fades to unity and then keeps its samples; AW_EQ_KEEP —
 * it is not part of the change: its preset and its Float64 state go on untouched.  NULL: every stream takes definition 0.  n_definitions
 * == 0 is allowed when every entry is -1 or AW_EQ_KEEP.  A handle whose stage is off counts as every stream at -1 and the call switches
 * the stage on (the reference's processor starts at unity).
 *  - one fade clock per handle.  A published target begins at the first frame of the next batch call or, while a fade runs, at the frame
 *    where that fade ends, also in the middle of a call.  Until it begins a newer publication is merged into it stream by stream: an entry
 *    that is not AW_EQ_KEEP replaces the older one.  When a fade ends the fading streams' new preset and state become their active ones.
 *    There is no retirement box: the stage behaves as aw_eq does when its host drains after every call.
 *  - arithmetic, per ear of a fading stream, frame i of the fade counted from 1: old = the active preset's ParametricEqualizerState.process
 *    going on from its state (the sample itself at -1), new = the target's from a zero state (the sample itself for -1), both rounded to
 *    float32; out = Float(Double(old) * (1 - g) + Double(new) * g), g = Double(i) / Double(T) (:296-304), computed as aw_eq's blend is:
 *    the new side's product rounded to Float64, the old side's fused into the sum, fma(Double(old), 1 - g, Double(new) * g).
 *  - a call is cut at every frame where the clock begins or ends a fade, and every stream, fading or not, is processed as those pieces in
 *    order, each as aw_eq_state_process splits a call.  A group of streams with one target history therefore equals aw_eq over the
 *    stage-off output bit for bit, and a stream at AW_EQ_KEEP a handle given the pieces as calls.  Chunking by streams, sample formats,
 *    pinned or pageable buffers and sharding over handles that receive the same publications change no bit; the clock moves once per call.
 *  - with no fade running and none published a call queues what it queued before this entry existed.
 *  - aw_spatializer_reset zeroes every filter state (active, faded from, faded to) and leaves the setting, the clock and a published
 *    target where they are (applyPendingReset, :341-352).
 *  - the call may allocate, upload and synchronise; no batch entry allocates, frees or synchronises for the stage: the fade, its begin and
 *    its end are queued on the context's stream.  Do not call it while a process call on the same handle is running.
 * Errors: as aw_spatializer_set_equalizer, with AW_EQ_KEEP allowed in the map; NULL stream_definition with n_definitions == 0 is
 * AW_ERR_INVALID_ARGUMENT too.  A call that fails leaves the stage, the clock and a published target as they were.
 * aw_spatializer_info: 27 the frames left of the running fade, 28 whether a target is published and has not begun. */
#define AW_EQ_KEEP (-2)
AW_API aw_status aw_spatializer_set_equalizer_target(aw_spatializer *sp, const aw_eq_definition *const *definitions, int32_t n_definitions,
                                                     const int32_t *stream_definition);

/* ParametricEqualizerProcessor  :116-408: starts at unity; aw_eq_set_target prepares and publishes a
 * target that the next process call crossfades to over max(1, round(0.020 * sample_rate)) frames
 * (:155); newest target wins while a fade runs (:311-333); a finished fade parks the old state in a
 * one-slot retirement box that aw_eq_drain_retired empties, and a full box holds the next fade back
 * (:373-406).  Threads, as in the reference: aw_eq_set_target / aw_eq_reset / aw_eq_drain_retired may be called
 * from a control thread while ONE other thread is inside aw_eq_process*, which only tries the publication, reset and
 * retirement locks (:322,:342,:380,:393) and, when one is contended, keeps its prior target / applies the reset on a
 * later call / defers the retirement.  max_frames_per_callback: 0 = unlimited (batch); otherwise the reference's guard
 * 1..4096 (:148-150, AW_ERR_EQ_TOO_MANY_FILTERS as there) and process() rejects longer calls. */
typedef struct aw_eq aw_eq;
AW_API aw_status aw_eq_create(aw_context *ctx, double sample_rate, int32_t n_streams, int32_t max_frames_per_callback,
                              aw_eq **out);
AW_API void aw_eq_destroy(aw_eq *eq);
AW_API aw_status aw_eq_set_target(aw_eq *eq, const aw_eq_definition *definition_or_null);   /* setTarget :226-228 */
AW_API aw_status aw_eq_reset(aw_eq *eq);                                                     /* reset()   :230-234 */
AW_API aw_status aw_eq_drain_retired(aw_eq *eq);                                             /* drainRetiredStates :237-241 */
AW_API aw_status aw_eq_process(aw_eq *eq, const float *in_device, float *out_device, int64_t frames);
/* The StereoAudioProcessing surface (AudioPipeline.swift:3-11): HOST planar buffers, one stream,
 * in_right may be NULL (left is duplicated, :68); synchronous. */
AW_API aw_status aw_eq_process_planar(aw_eq *eq, const float *in_left, const float *in_right, float *out_left,
                                      float *out_right, int32_t frames);
/* withPublicationLockForTesting :229-233: hold != 0 takes the publication lock, 0 releases it (same thread). */
AW_API aw_status aw_eq_debug_hold_publication_lock(aw_eq *eq, int32_t hold);
AW_API int32_t aw_eq_transition_length(const aw_eq *eq);
AW_API int32_t aw_eq_is_transitioning(const aw_eq *eq);

/* ---- batch sample-rate converter ---------------------------------------------------------------
 * Audio-rate conversion has no counterpart in the reference.  What the reference resamples is an HRIR at activation, by two-point linear
 * interpolation (Resampler.swift:31-68; aw_resample above), which is right for an impulse response and images and aliases at about
 * -30 dB on audio: audio does not take that path.  aw_rateconv is a polyphase Kaiser-windowed sinc (48 zero crossings a side, beta 10,
 * stopband from the lower Nyquist on; rules and constants: airwave_amd/csrc/device/rateconv.hpp), a stand-alone handle beside aw_eq: it
 * changes the frame count, which the in-place stages of the batch entries cannot, and it takes any channel count 1..16, so it can sit in
 * front of a spatializer or behind one.
 *  - rates are positive integers in Hz (passed as doubles that must be integral).  With g = gcd(in, out), L = out / g and M = in / g,
 *    equal rates and an L or M above 640 are refused; 640 covers every pair among 44100, 48000, 88200, 96000, 176400 and 192000.  Every
 *    refusal is AW_ERR_INVALID_ARGUMENT with a message; no ratio is approximated.
 *  - output n of a stream sits exactly at input time n M / L (time aligned) and is written once input frame floor(n M / L) + latency has
 *    arrived: after N input frames in total a stream has produced max(0, ceil((N - latency) L / M)) frames.
 *  - every output is a pure function of the stream's input since the last reset: splitting calls in time, sharding streams over handles
 *    and buffer alignment change no bit.  Inputs are not sanitised: a NaN reaches the outputs whose windows hold it.
 * aw_rateconv_plan / _filter are pure host and need no context: what a pair of rates means, and the float32 table c[L][taps].
 * aw_rateconv_create makes every device allocation (the table, two history slots [streams][taps - 1][channels], the counts); no later
 * call allocates.  aw_rateconv_process reads [streams][in_frames][channels] float32 and writes [streams][*out_frames][channels], dense in
 * the count it produced, which is what aw_rateconv_output_frames(rc, in_frames) said; it is asynchronous on the context's stream.  A
 * call may produce 0 frames (fewer than latency + 1 input frames so far): it then only moves the history.  out_capacity_frames below
 * the count returns AW_ERR_INVALID_ARGUMENT and leaves the handle untouched.  in and out must not overlap, and need 4-byte alignment
 * only.  aw_rateconv_flush is exactly a process call of `latency` zero frames followed by aw_rateconv_reset: after it a stream fed N
 * frames has produced ceil(N L / M) in total.  One owner thread per handle, as for aw_eq; destroy waits for the stream. */
typedef struct aw_rateconv aw_rateconv;
AW_API aw_status aw_rateconv_plan(double in_rate, double out_rate, int32_t *L, int32_t *M, int32_t *taps, int32_t *latency /* D, input frames */);
AW_API aw_status aw_rateconv_filter(double in_rate, double out_rate, float *c /* [L][taps] */, int64_t capacity_floats);
AW_API aw_status aw_rateconv_create(aw_context *ctx, double in_rate, double out_rate, int32_t n_streams, int32_t n_channels, aw_rateconv **out);
AW_API void aw_rateconv_destroy(aw_rateconv *rc);
/* what: 0 L, 1 M, 2 taps, 3 latency, 4 tile (output frames per workgroup), 5 frames consumed, 6 frames produced, 7 the aw_dither mode,
 * 8 the aw_gain_mode, 9 metering on (7 - 9: the settings of the aw_pcm_rateconv_* entries below), 10 true-peak measuring on, 11 output
 * frames per workgroup of the measuring form, 0 where it has none (10 - 11: the aw_tp_rateconv_* entries below); -1 otherwise */
AW_API int64_t aw_rateconv_info(const aw_rateconv *rc, int32_t what);
AW_API int64_t aw_rateconv_output_frames(const aw_rateconv *rc, int64_t in_frames);  /* what the next process call of in_frames writes */
AW_API aw_status aw_rateconv_process(aw_rateconv *rc, const float *in_device, int64_t in_frames, float *out_device,
                                     int64_t out_capacity_frames, int64_t *out_frames);
AW_API aw_status aw_rateconv_flush(aw_rateconv *rc, float *out_device, int64_t out_capacity_frames, int64_t *out_frames);
AW_API aw_status aw_rateconv_reset(aw_rateconv *rc);
/* Integer PCM in and out of the converter, with dither, gain and levels: the same handle through the entries below, so that a converter
 * behind a spatializer writes the file a host delivers (s16 / s24 / s32, dithered, gained, metered, with a clip count) and one in front of
 * a spatializer reads the 16- or 24-bit PCM a host holds.  Decode and encode are fused into the converter's kernel: there is no float32
 * staging and no allocation on a process path.  aw_rateconv_process, _flush and _reset keep their behaviour exactly and ignore dither,
 * gain and metering; both families may be mixed on one handle from call to call, and so may the formats (the carried history is float32).
 * For stream s of the handle (global stream first_stream + s) and channel ch:
 *  - decode: x is the input; F32 as it is, s16 / s24 / s32 by the rules of "integer PCM sample formats" above (exact: the scales are
 *    powers of two).
 *  - convert: y is what the rule of aw_rateconv_process makes of x.  F32 in, F32 out, no gain and no dither gives its bits.
 *  - gain: u = (float)(y * g_s) under AW_GAIN_FIXED, u = y under AW_GAIN_NONE.
 *  - encode: F32 output is u; s32 is the s32 rule above, never dithered; s16 / s24 are rintf(u * 32768.0f + d) / rintf(u * 8388608.0f + d),
 *    saturated, with the NaN and clip rules above and d the dither of aw_spatializer_set_dither's formulas at position p = n, ear
 *    e = ch & 1 and key K_j, j = ch >> 1:
 *      n   = the stream's absolute output frame index since the last reset or flush (aw_rateconv_info 6 plus the frame's index in the call)
 *      K_j = ((seed ^ 0xD1B54A32D192ED03) + first_stream + s) * 0x9E3779B97F4A7C15 + j * 0xA0761D6478BD642F   (mod 2^64).
 *    For a stereo converter K_0 is the spatializer's key: the noise of frame n is bit for bit what aw_spatializer_set_dither with the same
 *    seed and first stream gives at position n.  Further channel pairs get keys of their own (the spatializer's 2p + e counter would
 *    collide from the third channel on).
 *  - records (aw_rateconv_levels), per stream, while metering is on: peak = max |y| over finite samples of all channels, BEFORE the gain;
 *    nonfinite counts NaN / +-inf y; frames counts output frames written; clipped counts the samples the integer encode clipped, after
 *    gain and dither.  Every field is a max or an integer sum, so every field is exact.  Reset and flush restart n at 0 and leave the
 *    records alone: they live until aw_pcm_rateconv_reset_levels, so a host reads them after the flush.
 *  - clipped_device: NULL, or a device uint64 that the call atomically adds its clipped count to, as in aw_spatializer_process_pcm; it
 *    works with metering off.
 *  - flush feeds `latency` frames of zeros whatever the input format was, writes in out_format, then resets as aw_rateconv_flush does.
 *  - splitting calls in time, sharding streams over handles (with first_stream), the byte alignment of either buffer and the kernel's
 *    tiling change no output byte and no record field.  Buffers may have ANY byte alignment, F32 included (F32 keeps its 4-byte rule
 *    only through aw_rateconv_process / _flush).
 *  - loudness, true peak and the limiter of a spatializer in front of the converter measure the signal BEFORE conversion; the converter's
 *    own peak is the SAMPLE peak after it.  A true-peak meter or limiter after the converter is not provided here.
 *    (The meter and a ceiling pass are the aw_tp_rateconv_* entries: "True peak of the converted output" below.)
 * An unknown format, a NULL handle, a NULL input with in_frames > 0 or a capacity below the count returns AW_ERR_INVALID_ARGUMENT before
 * any HIP call, leaves the handle untouched and does not write *out_frames.  Process, flush and reset_levels only enqueue on the context's
 * stream; get_levels copies on that stream and then synchronises it. */
typedef struct aw_rateconv_levels {
    float    peak;         /* max |y| over finite samples of every channel, before gain */
    uint32_t reserved;     /* 0 */
    uint64_t frames;       /* output frames written */
    uint64_t clipped;      /* samples the integer encodes clipped (after gain and dither) */
    uint64_t nonfinite;    /* NaN / inf samples y */
} aw_rateconv_levels;      /* 32 bytes */
AW_API aw_status aw_pcm_rateconv_process(aw_rateconv *rc, const void *in_device, aw_sample_format in_format, int64_t in_frames,
                                         void *out_device, aw_sample_format out_format, int64_t out_capacity_frames, int64_t *out_frames,
                                         uint64_t *clipped_device);
AW_API aw_status aw_pcm_rateconv_flush(aw_rateconv *rc, void *out_device, aw_sample_format out_format, int64_t out_capacity_frames,
                                       int64_t *out_frames, uint64_t *clipped_device);
/* Applies to every later s16 / s24 encode of the aw_pcm_rateconv_* entries.  An unknown mode is refused.  Allocates nothing. */
AW_API aw_status aw_pcm_rateconv_set_dither(aw_rateconv *rc, aw_dither mode, uint64_t seed, uint64_t first_stream);
/* AW_GAIN_NONE: gains_host and n are ignored.  AW_GAIN_FIXED: n finite gains, n == 1 (every stream) or n == the stream count, uploaded by
 * this call (one allocation; it waits for the context's stream first).  AW_GAIN_PEAK_CEILING and AW_GAIN_TRUE_PEAK_CEILING are refused
 * with AW_ERR_INVALID_ARGUMENT: they are per-call functions of a peak, which the one-pass kernel does not have.  A refusal leaves the
 * previous setting. */
AW_API aw_status aw_pcm_rateconv_set_gain(aw_rateconv *rc, aw_gain_mode mode, const float *gains_host, int32_t n);
/* on != 0: allocates the records at the first such call (one allocation, never on a process path) and meters every later
 * aw_pcm_rateconv_* call; 0: stops metering, the records stay readable. */
AW_API aw_status aw_pcm_rateconv_set_metering(aw_rateconv *rc, int32_t on);
/* Copies the records of streams [first_stream, first_stream + n) to out_host on the context's stream, then synchronises it.  A range
 * outside the handle's streams, or a handle on which set_metering(on) was never called, returns AW_ERR_INVALID_ARGUMENT. */
AW_API aw_status aw_pcm_rateconv_get_levels(aw_rateconv *rc, int32_t first_stream, int32_t n, aw_rateconv_levels *out_host);
/* Zeroes every record (asynchronous on the context's stream); the settings stay. */
AW_API aw_status aw_pcm_rateconv_reset_levels(aw_rateconv *rc);
/* True peak of the converted output, and a ceiling pass.  Resampling moves inter-sample peaks, so a true peak measured in front of the
 * converter does not hold behind it.  While measuring is on, the aw_pcm_rateconv_* entries apply the spatializer's true-peak rule
 * ("per-stream true peak" above: aw_true_peak_filter, 49-tap Hann-windowed sinc, phases 1 .. 3, fixed fmaf chains, integer max) to their
 * own output inside the converter's kernel, with no float32 staging.  For stream s, channel ch and the stream's absolute output index n
 * since the last reset or flush:
 *  - y[n] is the converter's float32 output BEFORE gain, dither and encode; v[n] = y[n] where it is finite, else 0; v[n] = 0 for n < 0.
 *  - frame n of channel ch contributes max(|v[n]|, |t_1[n]|, |t_2[n]|, |t_3[n]|), t_p[n] the fmaf chain of aw_true_peak_filter's phase p
 *    over v[n], v[n-1], .., v[n-11] of that channel, kept as the bit pattern of the absolute value.
 *  - the record: true_peak = the maximum over channels and frames of the contributions, sample_peak = max |v| over the same frames,
 *    frames = the output frames measured.  Maxima of bit patterns and an integer sum: every field is exact.
 *  - flush and reset zero the carried v (the stream's last 11 cleaned output frames) and restart n; the records live until
 *    aw_tp_rateconv_reset_records.  The six-frame look-ahead of the centred filter is not flushed, as in the spatializer.
 *  - splitting calls in time, sharding streams over handles, buffer alignment, sample formats and the kernel's tiling change no bit of
 *    any field.  Output bytes, aw_rateconv_levels and clip counts are exactly those with measuring off.
 *  - aw_rateconv_process / _flush / _reset keep their behaviour and do not measure: a float32-family process call between measured calls
 *    is NOT seen by the meter, which goes on as if those frames had not been produced.  _reset and both flushes zero the carried v.
 * aw_tp_rateconv_measure / _measure_flush are aw_pcm_rateconv_process / _flush without an output buffer: the counts and the input history
 * move exactly as there, *out_frames is the count the call would have written, and only the true-peak records change: no byte of
 * output, no levels record and no clip count.  measure_flush ends with the reset, so a second pass over the same input starts clean.
 * The ceiling is host arithmetic over the records of such a first pass:
 *      g_s = true_peak_s > c ? c / true_peak_s : 1      (float32)
 *      aw_pcm_rateconv_set_gain(rc, AW_GAIN_FIXED, g, n_streams), then the second pass through aw_pcm_rateconv_process / _flush.
 * Outputs are a pure function of the input, so the second pass produces the y the first measured, and g y holds c up to the roundings
 * of the product and of a second reading.  AW_GAIN_PEAK_CEILING and AW_GAIN_TRUE_PEAK_CEILING stay refused by aw_pcm_rateconv_set_gain.
 * A NULL handle, an unknown format, a NULL input with in_frames > 0, a negative in_frames or a range outside the handle returns
 * AW_ERR_INVALID_ARGUMENT before any HIP call and writes nothing. */
typedef struct aw_rateconv_true_peak {
    float    true_peak;    /* max over channels and frames of the contributions, linear full scale */
    float    sample_peak;  /* max |v| over the same frames (equals aw_rateconv_levels.peak when both meters saw the same calls) */
    uint64_t frames;       /* output frames measured */
} aw_rateconv_true_peak;   /* 16 bytes */
/* on != 0: makes the one device allocation the feature needs at the first such call (the records and two slots of carried v
 * [streams][11][channels]; never on a process path) and measures every later aw_pcm_rateconv_* call; switching it on again after 0
 * starts from v = 0.  The measuring form computes 11 output frames beside its tile; for the few handles whose tile (aw_rateconv_info 4)
 * leaves none, on != 0 returns AW_ERR_INVALID_ARGUMENT and leaves the setting.  0: stops measuring, the records stay readable. */
AW_API aw_status aw_tp_rateconv_set(aw_rateconv *rc, int32_t on);
/* Copies the records of streams [first_stream, first_stream + n) to out_host on the context's stream, then synchronises it.  A range
 * outside the handle's streams, or a handle that was never switched on, returns AW_ERR_INVALID_ARGUMENT. */
AW_API aw_status aw_tp_rateconv_get(aw_rateconv *rc, int32_t first_stream, int32_t n, aw_rateconv_true_peak *out_host);
/* Zeroes every record (asynchronous on the context's stream); the setting and the carried v stay. */
AW_API aw_status aw_tp_rateconv_reset_records(aw_rateconv *rc);
/* Both require measuring to be on (AW_ERR_INVALID_ARGUMENT otherwise, the counts untouched) and only enqueue on the context's stream. */
AW_API aw_status aw_tp_rateconv_measure(aw_rateconv *rc, const void *in_device, aw_sample_format in_format, int64_t in_frames,
                                        int64_t *out_frames);
AW_API aw_status aw_tp_rateconv_measure_flush(aw_rateconv *rc, int64_t *out_frames);

/* ---- multi-device batch spatializer ------------------------------------------------------------
 * One handle, N devices: a single-process host in C or Swift spreads a batch over the GPUs of a box without RCCL, a second process or
 * threads of its own.  No counterpart in the reference, which renders one stream on one CPU.  There is no new arithmetic here: a shard is
 * an aw_context + aw_hrir + aw_spatializer of the library, driven through the single-handle entries above.
 *
 * Devices.  aw_device_count returns the number of visible HIP devices, 0 when there is none or no driver; it never fails.
 * aw_device_info fills the struct below (the struct tag and the function share a name, so C code writes `struct aw_device_info`); an
 * ordinal out of range returns AW_ERR_NO_DEVICE, as aw_context_create does.  The calling thread's current device is left as it was.
 * Asking for the free memory initialises the HIP runtime on that device, as creating a context there would: on a shared box ask only
 * about the devices you mean to use. */
struct aw_device_info {
    char     name[256];        /* marketing name, NUL-terminated */
    char     arch[64];         /* architecture name as the runtime reports it, e.g. "gfx950:sramecc+:xnack-" */
    int32_t  compute_units;
    int32_t  reserved;         /* 0 */
    uint64_t total_bytes;      /* device memory */
    uint64_t free_bytes;       /* ... of which free at the time of the call */
};                             /* 344 bytes */
AW_API int32_t aw_device_count(void);
AW_API aw_status aw_device_info(int32_t ordinal, struct aw_device_info *out);
/* The shard rule (airwave_amd/csrc/host/shard_plan.hpp; airwave_amd/sharding.py's shard_streams): with D = n_devices, q = n_streams / D and
 * r = n_streams % D, shard i owns the contiguous streams [i q + min(i, r), + q + (i < r ? 1 : 0)): stream order is kept and the first r
 * shards are one stream longer.  Shard i lives on device_ordinals[i]; an ordinal may repeat, which puts several contexts on one device
 * (how a one-GPU box runs this code).  D > n_streams leaves the last shards empty: an empty shard owns nothing and starts no thread.
 *
 * What equals what.  Output bytes, the clipped total and every record of the multi handle equal, bit for bit, those of separately created
 * single handles, one per non-empty shard — aw_spatializer_create with the shard's stream count on a context of its own on that ordinal —
 * given the same slices of the buffers, the same sequence of calls and the same settings, aw_spatializer_set_dither with first_stream +
 * the shard's first stream.  The one exception is aw_stream_levels.energy, which no two runs of any handle reproduce bit for bit: its float64
 * additions come in an unspecified order ("per-stream output levels" above), so it agrees within that section's bound, N * 2^-53 relative
 * over N samples.  Against ONE handle of n_streams streams only the library's tolerance holds (1e-5 of peak against the float64
 * oracle): the kernels of a call are chosen from the handle's stream count and the call's length (aw_spatializer_info 0-3 and 7), so a
 * shard of 512 streams may run other kernels than a handle of 1024.  Where those figures agree between the big handle and every shard,
 * the "sharding over handles changes no bit" statements of the sections above apply.
 *
 * Threads.  aw_multi_create starts one persistent thread per non-empty shard; they sleep between calls.  aw_multi_reserve_pcm and
 * aw_multi_process_host_pcm run on them, one shard each, side by side, and return when every shard has finished: no work of a call
 * outlives it.  Every other entry runs on the caller's thread, shard after shard.  The handle is single-owner like every handle: one call
 * at a time.  The contexts' copy threads (pageable buffers) are divided among the shards: each context gets max(1, default / non-empty
 * shards) of them.  After aw_multi_reserve_pcm a process call of up to max_frames frames in those formats allocates nothing, on the host
 * or on any device, and starts no thread.
 *
 * Failures.  A failing shard's status is returned — of several, the lowest shard index — and aw_last_error_message() of the CALLING
 * thread carries that shard's message prefixed with "shard i (device o): ".  A failed aw_multi_create has destroyed what it built.  After
 * a failed process call the output contents and the streams' state are unspecified, as for one handle: aw_multi_reset before reuse.  A
 * setter validates its whole argument before it touches a shard, so a call refused for its arguments (AW_ERR_INVALID_ARGUMENT) has
 * changed none; a HIP failure half-way through a setter leaves the shards before it changed: set again or destroy.
 *
 * aw_multi_create: n_devices 1 .. 64; tracks [n_tracks][taps] on the host as for aw_hrir_create; the channel map, n_streams (>= 1) and
 * block_hint as for aw_spatializer_create, whose statuses an unusable HRIR or map gets.  Every argument error is answered before any HIP
 * call. */
typedef struct aw_multi aw_multi;
AW_API aw_status aw_multi_create(const int32_t *device_ordinals, int32_t n_devices, const float *tracks, int32_t n_tracks, int32_t taps,
                                 double sample_rate, int32_t n_in_channels, const int32_t *left_track, const int32_t *right_track,
                                 int32_t n_streams, int32_t block_hint, aw_multi **out);
AW_API void aw_multi_destroy(aw_multi *m);
AW_API int32_t aw_multi_shard_count(const aw_multi *m);     /* n_devices, empty shards included */
AW_API int32_t aw_multi_stream_count(const aw_multi *m);
AW_API int32_t aw_multi_channel_count(const aw_multi *m);
/* Shard `shard`: its device ordinal, first stream and stream count (0: empty).  Any output may be NULL. */
AW_API aw_status aw_multi_shard(const aw_multi *m, int32_t shard, int32_t *device_ordinal, int32_t *first_stream, int32_t *count);
/* BORROWED handles of a shard, NULL for an empty shard or an index out of range: for aw_spatializer_info, profiling and the probes.  Do
 * not process, configure, reset or destroy through them: the multi handle owns them and keeps its shards in step. */
AW_API aw_spatializer *aw_multi_spatializer(const aw_multi *m, int32_t shard);
AW_API aw_context *aw_multi_context(const aw_multi *m, int32_t shard);
/* aw_spatializer_reserve_pcm of every shard, on the workers. */
AW_API aw_status aw_multi_reserve_pcm(aw_multi *m, int64_t max_frames, aw_sample_format in_format, aw_sample_format out_format);
/* HOST buffers laid out as ONE handle of n_streams streams takes them: in [stream][frames][n_in_channels], out [stream][frames][2],
 * elements of the given formats.  Shard i runs aw_spatializer_process_host_pcm on its slice (F32 / F32: aw_spatializer_process_host) on
 * its own worker.  clipped: NULL, or receives the sum over the shards.  Synchronous. */
AW_API aw_status aw_multi_process_host_pcm(aw_multi *m, const void *in_host, aw_sample_format in_format, void *out_host,
                                           aw_sample_format out_format, int64_t frames, uint64_t *clipped);
AW_API aw_status aw_multi_reset(aw_multi *m);               /* aw_spatializer_reset of every shard */
/* Page-locked host memory that EVERY device of the handle can DMA (hipHostMalloc, portable): with buffers from here each shard's slice
 * takes the DMA path of the host entry, not the bounce path.  Free it before the handle is destroyed. */
AW_API aw_status aw_multi_alloc_pinned(aw_multi *m, size_t bytes, void **ptr);
AW_API aw_status aw_multi_free_pinned(aw_multi *m, void *ptr);
/* The settings of the single handle, each shard given its slice.  Arguments, defaults and errors are those of the aw_spatializer_* entry
 * of the same name; per-stream arrays (gains_host with n == n_streams, stream_definition) hold one entry per stream of the multi handle.
 *  - set_dither: shard i gets first_stream + its first stream, so the handle's noise is that of one handle holding every stream, and the
 *    multi handle can itself be a shard of a larger job.
 *  - set_equalizer / set_equalizer_target: the definitions go to every shard, stream_definition is sliced (AW_EQ_KEEP where the single
 *    entry allows it), NULL stays NULL. */
AW_API aw_status aw_multi_set_dither(aw_multi *m, aw_dither mode, uint64_t seed, uint64_t first_stream);
AW_API aw_status aw_multi_set_metering(aw_multi *m, int32_t on);
AW_API aw_status aw_multi_reset_levels(aw_multi *m);
AW_API aw_status aw_multi_set_gain(aw_multi *m, aw_gain_mode mode, const float *gains_host, int32_t n, float ceiling);
AW_API aw_status aw_multi_set_loudness(aw_multi *m, int32_t on, double max_seconds);
AW_API aw_status aw_multi_set_true_peak(aw_multi *m, int32_t on);
AW_API aw_status aw_multi_set_limiter(aw_multi *m, int32_t on, float ceiling, int32_t attack_frames, int32_t hold_frames);
AW_API aw_status aw_multi_set_equalizer(aw_multi *m, const aw_eq_definition *const *definitions, int32_t n_definitions,
                                        const int32_t *stream_definition);
AW_API aw_status aw_multi_set_equalizer_target(aw_multi *m, const aw_eq_definition *const *definitions, int32_t n_definitions,
                                               const int32_t *stream_definition);
/* The records of the GLOBAL streams [first_stream, first_stream + n), gathered across shard boundaries; each shard's part is what the
 * aw_spatializer_get_* entry of the same name returns (and synchronises that shard's stream).  get_loudness_hops goes to the shard that
 * owns the stream. */
AW_API aw_status aw_multi_get_levels(aw_multi *m, int32_t first_stream, int32_t n, aw_stream_levels *out_host);
AW_API aw_status aw_multi_get_loudness(aw_multi *m, int32_t first_stream, int32_t n, aw_stream_loudness *out_host);
AW_API aw_status aw_multi_get_loudness_hops(aw_multi *m, int32_t stream, int64_t first_hop, int64_t n, double *out_host);
AW_API aw_status aw_multi_get_true_peak(aw_multi *m, int32_t first_stream, int32_t n, aw_stream_true_peak *out_host);
AW_API aw_status aw_multi_get_limiter(aw_multi *m, int32_t first_stream, int32_t n, aw_stream_limiter *out_host);

AW_API const char *aw_version(void);

#ifdef __cplusplus
}
#endif
#endif
