// airwave_hip.hpp — header-only C++ mirror of the reference's Swift types over the C ABI
// (include/airwave_hip.h).  Same names and call shapes as ConvolutionEngine.swift /
// RealtimeAudioProcessor.swift / HRIRManager.swift so that C++ hosts (and the ABI replay harness in
// tests/harness/) read like the reference.  Errors surface as aw::Error (status + message);
// the failable initialiser `init?` becomes `ConvolutionEngine::make` returning nullptr.
#pragma once
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "airwave_hip.h"

namespace aw {

struct Error : std::runtime_error {
    aw_status status;
    Error(aw_status s, const std::string &m) : std::runtime_error(std::string(aw_status_string(s)) + ": " + m), status(s) {}
};
inline void check(aw_status s) {
    if (s != AW_OK) throw Error(s, aw_last_error_message());
}

class Context {
  public:
    explicit Context(int device = 0) { check(aw_context_create(device, &h_)); }
    Context(int device, void *hip_stream) { check(aw_context_create_on_stream(device, hip_stream, &h_)); }
    ~Context() { aw_context_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    aw_context *get() const { return h_; }
    void synchronize() { check(aw_context_synchronize(h_)); }
    void reserveScratch(size_t bytes) { check(aw_context_reserve_scratch(h_, bytes)); }      // the pool its spatializers share, sized at start-up
    size_t scratchBytes() const { return aw_context_scratch_bytes(h_); }
  private:
    aw_context *h_ = nullptr;
};

// ConvolutionEngine.swift:14-408
class ConvolutionEngine {
  public:
    // init?(hrirSamples:blockSize:)  :68 — nullptr instead of nil
    static std::unique_ptr<ConvolutionEngine> make(Context &ctx, const std::vector<float> &hrirSamples, int blockSize = 512) {
        aw_engine *e = nullptr;
        if (aw_engine_create(ctx.get(), hrirSamples.data(), (int32_t)hrirSamples.size(), blockSize, &e) != AW_OK) return nullptr;
        return std::unique_ptr<ConvolutionEngine>(new ConvolutionEngine(e));
    }
    ~ConvolutionEngine() { aw_engine_destroy(h_); }
    void process(const float *input, float *output) { check(aw_engine_process(h_, input, output)); }                  // :232
    // process(input:output:frameCount:) :370 — silently ignores a wrong count, like the reference
    void process(const std::vector<float> &input, std::vector<float> &output, int frameCount = -1) {
        const int count = frameCount < 0 ? blockSize() : frameCount;
        const aw_status s = aw_engine_process_n(h_, input.data(), output.data(), count);
        if (s != AW_OK && s != AW_ERR_BLOCK_SIZE_MISMATCH) check(s);
    }
    void processAndAccumulate(const float *input, float *outputAccumulator) {                                      // :388
        check(aw_engine_process_accumulate(h_, input, outputAccumulator));
    }
    void reset() { check(aw_engine_reset(h_)); }                                                                   // :397
    int blockSize() const { return aw_engine_block_size(h_); }
  private:
    explicit ConvolutionEngine(aw_engine *e) : h_(e) {}
    aw_engine *h_;
};

class HRIR {
  public:
    HRIR(Context &ctx, const float *tracks, int nTracks, int taps, double sampleRate) {
        check(aw_hrir_create(ctx.get(), tracks, nTracks, taps, sampleRate, &h_));
    }
    ~HRIR() { aw_hrir_destroy(h_); }
    HRIR(const HRIR &) = delete;
    aw_hrir *get() const { return h_; }
  private:
    aw_hrir *h_ = nullptr;
};

// The batch engine network (HRIRManager.RendererState + processPendingBlock, generalised to N speakers)
class Spatializer {
  public:
    Spatializer(Context &ctx, const HRIR &hrir, const std::vector<int32_t> &leftTrack, const std::vector<int32_t> &rightTrack,
                int nStreams = 1) {
        check(aw_spatializer_create(ctx.get(), hrir.get(), (int32_t)leftTrack.size(), leftTrack.data(), rightTrack.data(),
                                    nStreams, 0, &h_));
    }
    explicit Spatializer(aw_spatializer *adopt) : h_(adopt) {}
    ~Spatializer() { aw_spatializer_destroy(h_); }
    Spatializer(const Spatializer &) = delete;
    void processDevice(const float *in, float *out, int64_t frames) { check(aw_spatializer_process(h_, in, out, frames)); }
    void processHost(const float *in, float *out, int64_t frames) { check(aw_spatializer_process_host(h_, in, out, frames)); }
    // StereoAudioProcessing.process  AudioPipeline.swift:3-11
    void process(const float *inputLeft, const float *inputRight, float *outputLeft, float *outputRight, int frameCount) {
        check(aw_spatializer_process_planar(h_, inputLeft, inputRight, outputLeft, outputRight, frameCount));
    }
    void reserve(int64_t maxFrames) { check(aw_spatializer_reserve(h_, maxFrames)); }
    void reserveHost(int64_t maxFrames) { check(aw_spatializer_reserve_host(h_, maxFrames)); }     // + the host entry's device-side staging
    // integer PCM (aw_sample_format): device / host entries in any pair of formats; the host entry returns the clipped-sample count
    void processPcmDevice(const void *in, aw_sample_format inFormat, void *out, aw_sample_format outFormat, int64_t frames,
                          uint64_t *clippedDevice = nullptr) {
        check(aw_spatializer_process_pcm(h_, in, inFormat, out, outFormat, frames, clippedDevice));
    }
    uint64_t processPcmHost(const void *in, aw_sample_format inFormat, void *out, aw_sample_format outFormat, int64_t frames) {
        uint64_t clipped = 0;
        check(aw_spatializer_process_host_pcm(h_, in, inFormat, out, outFormat, frames, &clipped));
        return clipped;
    }
    void reservePcm(int64_t maxFrames, aw_sample_format inFormat, aw_sample_format outFormat) {
        check(aw_spatializer_reserve_pcm(h_, maxFrames, inFormat, outFormat));
    }
    // TPDF dither of later s16 / s24 encodes (aw_dither); firstStream: the global index of this handle's stream 0
    void setDither(aw_dither mode, uint64_t seed = 0, uint64_t firstStream = 0) { check(aw_spatializer_set_dither(h_, mode, seed, firstStream)); }
    // per-stream levels and gain of the batch entries (aw_stream_levels, aw_gain_mode)
    void setMetering(bool on) { check(aw_spatializer_set_metering(h_, on ? 1 : 0)); }
    std::vector<aw_stream_levels> levels() {
        std::vector<aw_stream_levels> out((size_t)aw_spatializer_stream_count(h_));
        check(aw_spatializer_get_levels(h_, 0, (int32_t)out.size(), out.data()));
        return out;
    }
    void resetLevels() { check(aw_spatializer_reset_levels(h_)); }
    void setGainNone() { check(aw_spatializer_set_gain(h_, AW_GAIN_NONE, nullptr, 0, 0.0f)); }
    void setGainFixed(const std::vector<float> &gains) { check(aw_spatializer_set_gain(h_, AW_GAIN_FIXED, gains.data(), (int32_t)gains.size(), 0.0f)); }
    void setGainPeakCeiling(float ceiling) { check(aw_spatializer_set_gain(h_, AW_GAIN_PEAK_CEILING, nullptr, 0, ceiling)); }
    // per-stream BS.1770 integrated loudness of the batch entries (aw_stream_loudness)
    void setLoudness(bool on, double maxSeconds = 0.0) { check(aw_spatializer_set_loudness(h_, on ? 1 : 0, maxSeconds)); }
    std::vector<aw_stream_loudness> loudness() {
        std::vector<aw_stream_loudness> out((size_t)aw_spatializer_stream_count(h_));
        check(aw_spatializer_get_loudness(h_, 0, (int32_t)out.size(), out.data()));
        return out;
    }
    std::vector<double> loudnessHops(int32_t stream, int64_t firstHop, int64_t count) {
        std::vector<double> out((size_t)count);
        check(aw_spatializer_get_loudness_hops(h_, stream, firstHop, count, out.data()));
        return out;
    }
    static float loudnessGain(double lufs, double targetLufs) { float g = 1.0f; check(aw_loudness_gain(lufs, targetLufs, &g)); return g; }
    // per-stream true peak of the batch entries (aw_stream_true_peak); the gain that holds a true-peak ceiling
    void setTruePeak(bool on) { check(aw_spatializer_set_true_peak(h_, on ? 1 : 0)); }
    std::vector<aw_stream_true_peak> truePeak() {
        std::vector<aw_stream_true_peak> out((size_t)aw_spatializer_stream_count(h_));
        check(aw_spatializer_get_true_peak(h_, 0, (int32_t)out.size(), out.data()));
        return out;
    }
    void setGainTruePeakCeiling(float ceiling) { check(aw_spatializer_set_gain(h_, AW_GAIN_TRUE_PEAK_CEILING, nullptr, 0, ceiling)); }
    // look-ahead true-peak limiter of the batch entries (aw_stream_limiter); latency: info(24) frames
    void setLimiter(bool on, float ceiling = 1.0f, int32_t attackFrames = 64, int32_t holdFrames = 128) {
        check(aw_spatializer_set_limiter(h_, on ? 1 : 0, ceiling, attackFrames, holdFrames));
    }
    std::vector<aw_stream_limiter> limiter() {
        std::vector<aw_stream_limiter> out((size_t)aw_spatializer_stream_count(h_));
        check(aw_spatializer_get_limiter(h_, 0, (int32_t)out.size(), out.data()));
        return out;
    }
    // equalizer stage of the batch entries, one preset per stream (EqualizerDefinition::get(), below); streamDefinition empty: every stream
    // takes preset 0, else one entry per stream (-1: not equalized); no definitions: the stage is off
    void setEqualizer(const std::vector<const aw_eq_definition *> &definitions, const std::vector<int32_t> &streamDefinition = {}) {
        if (!streamDefinition.empty() && streamDefinition.size() != (size_t)aw_spatializer_stream_count(h_)) throw Error(AW_ERR_INVALID_ARGUMENT, "streamDefinition needs one entry per stream");
        check(aw_spatializer_set_equalizer(h_, definitions.data(), (int32_t)definitions.size(), streamDefinition.empty() ? nullptr : streamDefinition.data()));
    }
    // a target the stage fades to over 20 ms from the next batch call on; entries as setEqualizer's, AW_EQ_KEEP: the stream is not part of the change
    void setEqualizerTarget(const std::vector<const aw_eq_definition *> &definitions, const std::vector<int32_t> &streamDefinition = {}) {
        if (!streamDefinition.empty() && streamDefinition.size() != (size_t)aw_spatializer_stream_count(h_)) throw Error(AW_ERR_INVALID_ARGUMENT, "streamDefinition needs one entry per stream");
        check(aw_spatializer_set_equalizer_target(h_, definitions.data(), (int32_t)definitions.size(), streamDefinition.empty() ? nullptr : streamDefinition.data()));
    }
    int64_t info(int32_t what) const { return aw_spatializer_info(h_, what); }
    void reset() { check(aw_spatializer_reset(h_)); }
    aw_spatializer *get() const { return h_; }
  private:
    aw_spatializer *h_ = nullptr;
};

// aw_device_count / aw_device_info
inline int deviceCount() { return aw_device_count(); }
inline struct aw_device_info deviceInfo(int ordinal) {          // (the C function of the same name hides the plain struct name)
    struct aw_device_info d;
    check(::aw_device_info(ordinal, &d));
    return d;
}

// aw_multi: the batch spatializer over several devices behind one handle (one ordinal per shard; an ordinal may repeat).  Host buffers laid
// out as one Spatializer of nStreams streams takes them; bit-exact against separately driven Spatializers of the shards' stream counts.
class MultiSpatializer {
  public:
    struct Shard { int32_t ordinal, firstStream, count; };
    MultiSpatializer(const std::vector<int32_t> &devices, const float *tracks, int nTracks, int taps, double sampleRate,
                     const std::vector<int32_t> &leftTrack, const std::vector<int32_t> &rightTrack, int nStreams) {
        check(aw_multi_create(devices.data(), (int32_t)devices.size(), tracks, nTracks, taps, sampleRate, (int32_t)leftTrack.size(), leftTrack.data(),
                              rightTrack.data(), nStreams, 0, &h_));
    }
    ~MultiSpatializer() { aw_multi_destroy(h_); }
    MultiSpatializer(const MultiSpatializer &) = delete;
    MultiSpatializer &operator=(const MultiSpatializer &) = delete;
    int streamCount() const { return aw_multi_stream_count(h_); }
    int channelCount() const { return aw_multi_channel_count(h_); }
    std::vector<Shard> shards() const {
        std::vector<Shard> out((size_t)aw_multi_shard_count(h_));
        for (size_t i = 0; i < out.size(); ++i) check(aw_multi_shard(h_, (int32_t)i, &out[i].ordinal, &out[i].firstStream, &out[i].count));
        return out;
    }
    int64_t shardInfo(int32_t shard, int32_t what) const { return aw_spatializer_info(aw_multi_spatializer(h_, shard), what); }   // (borrowed handle)
    void reservePcm(int64_t maxFrames, aw_sample_format inFormat, aw_sample_format outFormat) { check(aw_multi_reserve_pcm(h_, maxFrames, inFormat, outFormat)); }
    uint64_t processPcmHost(const void *in, aw_sample_format inFormat, void *out, aw_sample_format outFormat, int64_t frames) {
        uint64_t clipped = 0;
        check(aw_multi_process_host_pcm(h_, in, inFormat, out, outFormat, frames, &clipped));
        return clipped;
    }
    void processHost(const float *in, float *out, int64_t frames) { check(aw_multi_process_host_pcm(h_, in, AW_SAMPLE_F32, out, AW_SAMPLE_F32, frames, nullptr)); }
    void reset() { check(aw_multi_reset(h_)); }
    // page-locked host memory every device of the handle can DMA; free it before the handle goes
    void *allocPinned(size_t bytes) { void *p = nullptr; check(aw_multi_alloc_pinned(h_, bytes, &p)); return p; }
    void freePinned(void *p) { check(aw_multi_free_pinned(h_, p)); }
    void setDither(aw_dither mode, uint64_t seed = 0, uint64_t firstStream = 0) { check(aw_multi_set_dither(h_, mode, seed, firstStream)); }
    void setMetering(bool on) { check(aw_multi_set_metering(h_, on ? 1 : 0)); }
    void resetLevels() { check(aw_multi_reset_levels(h_)); }
    void setGainNone() { check(aw_multi_set_gain(h_, AW_GAIN_NONE, nullptr, 0, 0.0f)); }
    void setGainFixed(const std::vector<float> &gains) { check(aw_multi_set_gain(h_, AW_GAIN_FIXED, gains.data(), (int32_t)gains.size(), 0.0f)); }
    void setGainPeakCeiling(float ceiling) { check(aw_multi_set_gain(h_, AW_GAIN_PEAK_CEILING, nullptr, 0, ceiling)); }
    void setGainTruePeakCeiling(float ceiling) { check(aw_multi_set_gain(h_, AW_GAIN_TRUE_PEAK_CEILING, nullptr, 0, ceiling)); }
    void setLoudness(bool on, double maxSeconds = 0.0) { check(aw_multi_set_loudness(h_, on ? 1 : 0, maxSeconds)); }
    void setTruePeak(bool on) { check(aw_multi_set_true_peak(h_, on ? 1 : 0)); }
    void setLimiter(bool on, float ceiling = 1.0f, int32_t attackFrames = 64, int32_t holdFrames = 128) {
        check(aw_multi_set_limiter(h_, on ? 1 : 0, ceiling, attackFrames, holdFrames));
    }
    // streamDefinition: empty (every stream takes preset 0) or one entry per stream of the multi handle
    void setEqualizer(const std::vector<const aw_eq_definition *> &definitions, const std::vector<int32_t> &streamDefinition = {}) {
        if (!streamDefinition.empty() && streamDefinition.size() != (size_t)streamCount()) throw Error(AW_ERR_INVALID_ARGUMENT, "streamDefinition needs one entry per stream");
        check(aw_multi_set_equalizer(h_, definitions.data(), (int32_t)definitions.size(), streamDefinition.empty() ? nullptr : streamDefinition.data()));
    }
    void setEqualizerTarget(const std::vector<const aw_eq_definition *> &definitions, const std::vector<int32_t> &streamDefinition = {}) {
        if (!streamDefinition.empty() && streamDefinition.size() != (size_t)streamCount()) throw Error(AW_ERR_INVALID_ARGUMENT, "streamDefinition needs one entry per stream");
        check(aw_multi_set_equalizer_target(h_, definitions.data(), (int32_t)definitions.size(), streamDefinition.empty() ? nullptr : streamDefinition.data()));
    }
    // records of the global streams [firstStream, firstStream + n), gathered across the shards
    std::vector<aw_stream_levels> levels(int32_t firstStream, int32_t n) { return records<aw_stream_levels>(firstStream, n, aw_multi_get_levels); }
    std::vector<aw_stream_loudness> loudness(int32_t firstStream, int32_t n) { return records<aw_stream_loudness>(firstStream, n, aw_multi_get_loudness); }
    std::vector<aw_stream_true_peak> truePeak(int32_t firstStream, int32_t n) { return records<aw_stream_true_peak>(firstStream, n, aw_multi_get_true_peak); }
    std::vector<aw_stream_limiter> limiter(int32_t firstStream, int32_t n) { return records<aw_stream_limiter>(firstStream, n, aw_multi_get_limiter); }
    std::vector<double> loudnessHops(int32_t stream, int64_t firstHop, int64_t count) {
        std::vector<double> out((size_t)count);
        check(aw_multi_get_loudness_hops(h_, stream, firstHop, count, out.data()));
        return out;
    }
    aw_multi *get() const { return h_; }
  private:
    template <class R> std::vector<R> records(int32_t firstStream, int32_t n, aw_status (*get)(aw_multi *, int32_t, int32_t, R *)) {
        std::vector<R> out((size_t)(n > 0 ? n : 0));
        check(get(h_, firstStream, n, out.data()));
        return out;
    }
    aw_multi *h_ = nullptr;
};

// RealtimeAudioProcessor.swift:11-191
class RealtimeAudioProcessor {
  public:
    RealtimeAudioProcessor(Context &ctx, const HRIR &hrir, const std::vector<int32_t> &leftTrack,
                           const std::vector<int32_t> &rightTrack, int blockSize = 512, int maxFramesPerCallback = 4096) {
        check(aw_realtime_create(ctx.get(), hrir.get(), (int32_t)leftTrack.size(), leftTrack.data(), rightTrack.data(), blockSize,
                                 maxFramesPerCallback, &h_));
    }
    ~RealtimeAudioProcessor() { aw_realtime_destroy(h_); }
    void process(const float *inputLeft, const float *inputRight, float *leftOutput, float *rightOutput, int frameCount) {   // :77
        check(aw_realtime_process(h_, inputLeft, inputRight, leftOutput, rightOutput, frameCount));
    }
    void reset() { check(aw_realtime_reset(h_)); }                                                                            // :121
    int64_t info(int32_t what) const { return aw_realtime_info(h_, what); }          // 0 host bytes, 1 device bytes, 2 device allocations: constant across process()
  private:
    aw_realtime *h_ = nullptr;
};

// ---- parametric EQ (EqualizerPreset.swift, EqualizerAPOParser.swift, ParametricEqualizerProcessor.swift) ----
enum class EqualizerFilterType : int32_t { peaking = 0, lowShelf = 1, highShelf = 2 };

class EqualizerDefinition {
  public:
    explicit EqualizerDefinition(double preampDB = 0.0) { check(aw_eq_definition_create(preampDB, &h_)); }
    // EqualizerAPOParser.parse(data:filename:) — throws aw::Error(AW_ERR_EQ_PARSE, "line N: reason; ...")
    static EqualizerDefinition parse(const void *data, size_t size) {
        aw_eq_definition *d = nullptr;
        char issues[4096];
        const aw_status s = aw_eq_parse(data, size, &d, issues, sizeof(issues));
        if (s != AW_OK) throw Error(s, issues);
        return EqualizerDefinition(d);
    }
    EqualizerDefinition(EqualizerDefinition &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    EqualizerDefinition(const EqualizerDefinition &) = delete;
    ~EqualizerDefinition() { aw_eq_definition_destroy(h_); }
    EqualizerDefinition &addFilter(EqualizerFilterType type, double frequencyHz, double gainDB, double q, bool isEnabled = true) {
        check(aw_eq_definition_add_filter(h_, isEnabled ? 1 : 0, (int32_t)type, frequencyHz, gainDB, q));
        return *this;
    }
    double preampDB() const { return aw_eq_definition_preamp_db(h_); }
    int filterCount() const { return aw_eq_definition_filter_count(h_); }
    const aw_eq_definition *get() const { return h_; }
    // aw_eq_fold_hrir: this equalizer folded into HRIR tracks ([nTracks][taps] planar at sampleRate) — EQ(x * h) = x * (h * g), the spatial
    // effect and the equalizer that follows it (AudioEffectGraph.swift:195-211) in one pass.  Returns [nTracks][outTaps]; throws
    // aw::Error(AW_ERR_EQ_NOT_FOLDABLE) when the response does not decay within maxTaps - taps + 1 frames (run the cascade then).
    struct Folded { std::vector<float> tracks; int taps; int responseTaps; double tailBound; };
    Folded foldInto(const float *tracks, int nTracks, int taps, double sampleRate, double tailTolerance = 1e-7, int maxTaps = 65536) const {
        Folded f{};
        int32_t outTaps = 0, response = 0;
        check(aw_eq_fold_hrir(h_, sampleRate, tracks, nTracks, taps, tailTolerance, maxTaps, nullptr, &outTaps, &response, &f.tailBound));
        f.tracks.resize((size_t)nTracks * (size_t)outTaps);
        check(aw_eq_fold_hrir(h_, sampleRate, tracks, nTracks, taps, tailTolerance, maxTaps, f.tracks.data(), &outTaps, &response, &f.tailBound));
        f.taps = outTaps; f.responseTaps = response;
        return f;
    }
  private:
    explicit EqualizerDefinition(aw_eq_definition *d) : h_(d) {}
    aw_eq_definition *h_ = nullptr;
};

// ParametricEqualizerProcessor :116-408 (one stream, planar host buffers: the StereoAudioProcessing surface)
class ParametricEqualizerProcessor {
  public:
    ParametricEqualizerProcessor(Context &ctx, double sampleRate, int maxFramesPerCallback = 4096) {
        check(aw_eq_create(ctx.get(), sampleRate, 1, maxFramesPerCallback, &h_));
    }
    ~ParametricEqualizerProcessor() { aw_eq_destroy(h_); }
    ParametricEqualizerProcessor(const ParametricEqualizerProcessor &) = delete;
    void setTarget(const EqualizerDefinition *definition) { check(aw_eq_set_target(h_, definition ? definition->get() : nullptr)); }   // :226
    void reset() { check(aw_eq_reset(h_)); }                                                                                          // :230
    template <class F> void withPublicationLockForTesting(F body) {                                                                   // :229-233
        check(aw_eq_debug_hold_publication_lock(h_, 1));
        body();
        check(aw_eq_debug_hold_publication_lock(h_, 0));
    }
    void drainRetiredStates() { check(aw_eq_drain_retired(h_)); }                                                                     // :237
    void process(const float *inputLeft, const float *inputRight, float *leftOutput, float *rightOutput, int frameCount) {          // :253
        check(aw_eq_process_planar(h_, inputLeft, inputRight, leftOutput, rightOutput, frameCount));
    }
    int transitionLength() const { return aw_eq_transition_length(h_); }
  private:
    aw_eq *h_ = nullptr;
};

// aw_rateconv: the batch sample-rate converter (no counterpart in the reference, whose Resampler.swift:31-68 interpolates an HRIR, not audio)
struct RateConversionPlan { int32_t L = 0, M = 0, taps = 0, latency = 0; };
inline RateConversionPlan rateConversionPlan(double inRate, double outRate) {
    RateConversionPlan p;
    check(aw_rateconv_plan(inRate, outRate, &p.L, &p.M, &p.taps, &p.latency));
    return p;
}
inline std::vector<float> rateConversionFilter(double inRate, double outRate) {          // c[L][taps]
    const RateConversionPlan p = rateConversionPlan(inRate, outRate);
    std::vector<float> c((size_t)p.L * (size_t)p.taps);
    check(aw_rateconv_filter(inRate, outRate, c.data(), (int64_t)c.size()));
    return c;
}
class RateConverter {
  public:
    RateConverter(Context &ctx, double inRate, double outRate, int nStreams, int nChannels) {
        check(aw_rateconv_create(ctx.get(), inRate, outRate, nStreams, nChannels, &h_));
    }
    ~RateConverter() { aw_rateconv_destroy(h_); }
    RateConverter(const RateConverter &) = delete;
    int64_t info(int32_t what) const { return aw_rateconv_info(h_, what); }
    int64_t outputFrames(int64_t inFrames) const { return aw_rateconv_output_frames(h_, inFrames); }
    // device buffers; returns the frames written
    int64_t process(const float *inDevice, int64_t inFrames, float *outDevice, int64_t outCapacityFrames) {
        int64_t n = 0;
        check(aw_rateconv_process(h_, inDevice, inFrames, outDevice, outCapacityFrames, &n));
        return n;
    }
    int64_t flush(float *outDevice, int64_t outCapacityFrames) {
        int64_t n = 0;
        check(aw_rateconv_flush(h_, outDevice, outCapacityFrames, &n));
        return n;
    }
    void reset() { check(aw_rateconv_reset(h_)); }
    // integer PCM in and out (aw_pcm_rateconv_*): device buffers of any byte alignment; clippedDevice: nullptr, or a device uint64 the
    // call adds its clipped-sample count to
    int64_t processPcm(const void *inDevice, aw_sample_format inFormat, int64_t inFrames, void *outDevice, aw_sample_format outFormat,
                       int64_t outCapacityFrames, uint64_t *clippedDevice = nullptr) {
        int64_t n = 0;
        check(aw_pcm_rateconv_process(h_, inDevice, inFormat, inFrames, outDevice, outFormat, outCapacityFrames, &n, clippedDevice));
        return n;
    }
    int64_t flushPcm(void *outDevice, aw_sample_format outFormat, int64_t outCapacityFrames, uint64_t *clippedDevice = nullptr) {
        int64_t n = 0;
        check(aw_pcm_rateconv_flush(h_, outDevice, outFormat, outCapacityFrames, &n, clippedDevice));
        return n;
    }
    void setDither(aw_dither mode, uint64_t seed = 0, uint64_t firstStream = 0) { check(aw_pcm_rateconv_set_dither(h_, mode, seed, firstStream)); }
    void setGainNone() { check(aw_pcm_rateconv_set_gain(h_, AW_GAIN_NONE, nullptr, 0)); }
    void setGainFixed(const std::vector<float> &gains) { check(aw_pcm_rateconv_set_gain(h_, AW_GAIN_FIXED, gains.data(), (int32_t)gains.size())); }
    void setMetering(bool on) { check(aw_pcm_rateconv_set_metering(h_, on ? 1 : 0)); }
    std::vector<aw_rateconv_levels> levels(int32_t firstStream, int32_t n) {
        std::vector<aw_rateconv_levels> out((size_t)(n > 0 ? n : 0));
        check(aw_pcm_rateconv_get_levels(h_, firstStream, n, out.data()));
        return out;
    }
    void resetLevels() { check(aw_pcm_rateconv_reset_levels(h_)); }
    // true peak of the converted output and the ceiling pass (aw_tp_rateconv_*)
    void setTruePeak(bool on) { check(aw_tp_rateconv_set(h_, on ? 1 : 0)); }
    std::vector<aw_rateconv_true_peak> truePeak(int32_t firstStream, int32_t n) {
        std::vector<aw_rateconv_true_peak> out((size_t)(n > 0 ? n : 0));
        check(aw_tp_rateconv_get(h_, firstStream, n, out.data()));
        return out;
    }
    void resetTruePeak() { check(aw_tp_rateconv_reset_records(h_)); }
    int64_t measure(const void *inDevice, aw_sample_format inFormat, int64_t inFrames) {
        int64_t n = 0;
        check(aw_tp_rateconv_measure(h_, inDevice, inFormat, inFrames, &n));
        return n;
    }
    int64_t measureFlush() {
        int64_t n = 0;
        check(aw_tp_rateconv_measure_flush(h_, &n));
        return n;
    }
    // g = tp > c ? c / tp : 1 in float32 over what the records hold, for setGainFixed before the second pass
    std::vector<float> ceilingGains(float ceiling, int32_t nStreams) {
        std::vector<float> g;
        for (const aw_rateconv_true_peak &r : truePeak(0, nStreams)) g.push_back(r.true_peak > ceiling ? ceiling / r.true_peak : 1.0f);
        return g;
    }
  private:
    aw_rateconv *h_ = nullptr;
};

}  // namespace aw
