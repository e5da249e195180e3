//  BatchSpatializer.swift
//  Offline/batch entry that the macOS product does not have: N independent streams of interleaved
//  multichannel PCM resident on the GPU -> interleaved stereo, one call.

import Foundation
import CAirwaveHIP

public final class BatchSpatializer {
    private let handle: OpaquePointer
    public let streams: Int
    public let channels: Int

    /// The equalizer of the batch, if one was folded into the HRIR: samples of its impulse response that were kept and the bound on what
    /// the cut can change relative to the spatializer output's peak (aw_eq_fold_hrir).  nil: no equalizer, or not folded.
    public private(set) var foldedEqualizer: (responseTaps: Int, tailBound: Double)?

    /// tracks: planar HRIR ([track][tap]); leftTrack/rightTrack per input channel, -1 = speaker without a mapping
    /// (skipped like HRIRManager.swift:370-372).  Throws the reference's error categories as NSError codes.
    /// equalizer: the definition AudioEffectGraph would run AFTER the spatial effect (AudioEffectGraph.swift:195-211).  A batch host knows
    /// it up front, so it is folded into the HRIR here — EQ(x * h) = x * (h * g), one pass over the audio instead of two — when its impulse
    /// response decays within `equalizerMaxTaps`; otherwise (AW_ERR_EQ_NOT_FOLDABLE) the initialiser throws and the host runs
    /// `HIPEqualizerEffect` / aw_eq_process on the output as the reference's graph does.
    public init(context: HIPContext, tracks: [[Float]], sampleRate: Double, leftTrack: [Int32], rightTrack: [Int32], streams: Int,
                equalizer: HIPEqualizerDefinition? = nil, equalizerTailTolerance: Double = 1e-7, equalizerMaxTaps: Int32 = 65536) throws {
        precondition(leftTrack.count == rightTrack.count)
        var taps = tracks.first?.count ?? 0
        var flat = tracks.flatMap { $0 }
        if let definition = equalizer {
            guard let def = HIPEqualizerEffect.makeDefinitionHandle(definition) else { throw BatchSpatializer.error(AW_ERR_OUT_OF_MEMORY) }
            defer { aw_eq_definition_destroy(def) }
            var outTaps: Int32 = 0, response: Int32 = 0, bound = 0.0
            var st = flat.withUnsafeBufferPointer {
                aw_eq_fold_hrir(def, sampleRate, $0.baseAddress, Int32(tracks.count), Int32(taps), equalizerTailTolerance, equalizerMaxTaps, nil, &outTaps, &response, &bound)
            }
            guard st == AW_OK else { throw BatchSpatializer.error(st) }
            var folded = [Float](repeating: 0, count: tracks.count * Int(outTaps))
            st = flat.withUnsafeBufferPointer { src in
                folded.withUnsafeMutableBufferPointer { dst in
                    aw_eq_fold_hrir(def, sampleRate, src.baseAddress, Int32(tracks.count), Int32(taps), equalizerTailTolerance, equalizerMaxTaps, dst.baseAddress, &outTaps, &response, &bound)
                }
            }
            guard st == AW_OK else { throw BatchSpatializer.error(st) }
            flat = folded
            taps = Int(outTaps)
            foldedEqualizer = (Int(response), bound)
        }
        var hrir: OpaquePointer?
        var st = flat.withUnsafeBufferPointer { aw_hrir_create(context.handle, $0.baseAddress, Int32(tracks.count), Int32(taps), sampleRate, &hrir) }
        guard st == AW_OK, let h = hrir else { throw BatchSpatializer.error(st) }
        defer { aw_hrir_destroy(h) }
        var sp: OpaquePointer?
        st = aw_spatializer_create(context.handle, h, Int32(leftTrack.count), leftTrack, rightTrack, Int32(streams), 0, &sp)
        guard st == AW_OK, let s = sp else { throw BatchSpatializer.error(st) }
        handle = s
        self.streams = streams
        self.channels = leftTrack.count
    }
    deinit { aw_spatializer_destroy(handle) }

    /// Device pointers: input [stream][frame][channel], output [stream][frame][2].  Asynchronous on the context stream.
    public func process(deviceInput: UnsafePointer<Float>, deviceOutput: UnsafeMutablePointer<Float>, frames: Int64) throws {
        let st = aw_spatializer_process(handle, deviceInput, deviceOutput, frames)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// Sizes every internal device buffer for calls of up to `maxFrames` frames; `process` never allocates afterwards.
    public func reserve(maxFrames: Int64) throws {
        let st = aw_spatializer_reserve(handle, maxFrames)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// Host buffers: the batch crosses PCIe in chunks of streams, H2D of the next chunk and D2H of the previous one under the
    /// kernels of the current one.  Page-locked buffers (`aw_host_alloc_pinned`) move by DMA directly.  Synchronous.
    public func process(hostInput: UnsafePointer<Float>, hostOutput: UnsafeMutablePointer<Float>, frames: Int64) throws {
        let st = aw_spatializer_process_host(handle, hostInput, hostOutput, frames)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// Host buffers of 16-bit PCM (`aw_spatializer_process_host_pcm`, s16 in / s16 out): the same chunked pipeline at half the
    /// bytes; decoded and encoded on the device (round half to even, saturated).  Returns the call's clipped-sample count.
    @discardableResult
    public func process(hostInput: UnsafePointer<Int16>, hostOutput: UnsafeMutablePointer<Int16>, frames: Int64) throws -> UInt64 {
        var clipped: UInt64 = 0
        let st = aw_spatializer_process_host_pcm(handle, hostInput, aw_sample_format(AW_SAMPLE_S16), hostOutput,
                                                 aw_sample_format(AW_SAMPLE_S16), frames, &clipped)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
        return clipped
    }

    /// TPDF dither of every later s16 / s24 encode (`aw_spatializer_set_dither`; `AW_DITHER_NONE`, the default, rounds as above).
    /// `firstStream`: the global index of this batch's stream 0, so that a batch split over several spatializers gets one batch's noise.
    /// Not while a `process` call on this spatializer is running.
    public func setDither(_ mode: Int32, seed: UInt64 = 0, firstStream: UInt64 = 0) throws {
        let st = aw_spatializer_set_dither(handle, aw_dither(mode), seed, firstStream)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// Per-stream level meter of every later batch call (`aw_spatializer_set_metering`); switching it on allocates the records here.
    public func setMetering(_ on: Bool) throws {
        let st = aw_spatializer_set_metering(handle, on ? 1 : 0)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// The records of every stream (`aw_spatializer_get_levels`): peak and energy per ear before gain, the gain the last call applied,
    /// frames metered, clipped and non-finite samples.  Synchronises the context's stream.
    public func levels() throws -> [aw_stream_levels] {
        let n = aw_spatializer_stream_count(handle)
        var out = [aw_stream_levels](repeating: aw_stream_levels(), count: Int(n))
        let st = out.withUnsafeMutableBufferPointer { aw_spatializer_get_levels(handle, 0, n, $0.baseAddress) }
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
        return out
    }

    public func resetLevels() throws {
        let st = aw_spatializer_reset_levels(handle)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// Output gain of the batch entries (`aw_spatializer_set_gain`): `AW_GAIN_NONE`; `AW_GAIN_FIXED` with one gain or one per stream;
    /// `AW_GAIN_PEAK_CEILING` with 0 < ceiling <= 1, per stream and per call.
    public func setGain(_ mode: Int32, gains: [Float] = [], ceiling: Float = 0) throws {
        let st = gains.withUnsafeBufferPointer { aw_spatializer_set_gain(handle, aw_gain_mode(mode), $0.baseAddress, Int32(gains.count), ceiling) }
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// BS.1770 integrated loudness of every later batch call (`aw_spatializer_set_loudness`), measured per stream before the gain;
    /// switching it on allocates the hop energies of `maxSeconds` per stream here, not on the process path.
    public func setLoudness(_ on: Bool, maxSeconds: Double = 0) throws {
        let st = aw_spatializer_set_loudness(handle, on ? 1 : 0, maxSeconds)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// The gated loudness of every stream (`aw_spatializer_get_loudness`): integrated LUFS, the relative threshold, block counts, frames
    /// measured and dropped, non-finite samples.  Synchronises the context's stream.
    public func loudness() throws -> [aw_stream_loudness] {
        let n = aw_spatializer_stream_count(handle)
        var out = [aw_stream_loudness](repeating: aw_stream_loudness(), count: Int(n))
        let st = out.withUnsafeMutableBufferPointer { aw_spatializer_get_loudness(handle, 0, n, $0.baseAddress) }
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
        return out
    }

    /// The raw 100 ms hop energies of one stream (`aw_spatializer_get_loudness_hops`): material for momentary / short-term loudness.
    public func loudnessHops(stream: Int32, firstHop: Int64, count: Int64) throws -> [Double] {
        var out = [Double](repeating: 0, count: Int(count))
        let st = out.withUnsafeMutableBufferPointer { aw_spatializer_get_loudness_hops(handle, stream, firstHop, count, $0.baseAddress) }
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
        return out
    }

    /// The gain that brings a measured loudness to a target (`aw_loudness_gain`); nil for a silent stream (-infinity LUFS).
    public static func loudnessGain(lufs: Double, target: Double) -> Float? {
        var g: Float = 1
        return aw_loudness_gain(lufs, target, &g) == AW_OK ? g : nil
    }

    /// Look-ahead true-peak limiter on the output of every later batch call (`aw_spatializer_set_limiter`), behind the `AW_GAIN_FIXED`
    /// gain: 0 < ceiling <= 1, 16 <= attackFrames <= 512, 0 <= holdFrames <= 1024.  The output is `limiterLatency` frames late; feed that
    /// many frames of zeros to flush a file.  Switching it on allocates here, not on the process path.
    public func setLimiter(_ on: Bool, ceiling: Float = 1, attackFrames: Int32 = 64, holdFrames: Int32 = 128) throws {
        let st = aw_spatializer_set_limiter(handle, on ? 1 : 0, ceiling, attackFrames, holdFrames)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// The limiter's latency in frames (`aw_spatializer_info` 24); 0 while it is off.
    public var limiterLatency: Int64 { aw_spatializer_info(handle, 24) }

    /// The limiter's records of every stream (`aw_spatializer_get_limiter`): the lowest gain applied, frames, limited frames and
    /// non-finite samples.  Synchronises the context's stream.
    public func limiter() throws -> [aw_stream_limiter] {
        let n = aw_spatializer_stream_count(handle)
        var out = [aw_stream_limiter](repeating: aw_stream_limiter(), count: Int(n))
        let st = out.withUnsafeMutableBufferPointer { aw_spatializer_get_limiter(handle, 0, n, $0.baseAddress) }
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
        return out
    }

    /// A target the equalizer stage of the batch entries fades to over 20 ms, from the next batch call on
    /// (`aw_spatializer_set_equalizer_target`).  `streamDefinition`: per stream an index into `definitions`, -1 (fade to unity) or
    /// `BatchSpatializer.equalizerKeep` (the stream is not part of the change); empty: every stream takes definition 0.  A stage that is
    /// off counts as every stream at unity.  Allocates and uploads here, not on the process path.
    public static let equalizerKeep: Int32 = -2        // AW_EQ_KEEP
    public func setEqualizerTarget(definitions: [HIPEqualizerDefinition], streamDefinition: [Int32] = []) throws {
        precondition(streamDefinition.isEmpty || streamDefinition.count == Int(aw_spatializer_stream_count(handle)))
        var handles: [OpaquePointer?] = []
        defer { for h in handles { aw_eq_definition_destroy(h) } }
        for d in definitions {
            guard let h = HIPEqualizerEffect.makeDefinitionHandle(d) else { throw BatchSpatializer.error(AW_ERR_OUT_OF_MEMORY) }
            handles.append(h)
        }
        let st = handles.withUnsafeBufferPointer { defs in
            streamDefinition.withUnsafeBufferPointer { map in
                aw_spatializer_set_equalizer_target(handle, defs.baseAddress, Int32(defs.count), streamDefinition.isEmpty ? nil : map.baseAddress)
            }
        }
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    /// Frames left of the running fade (`aw_spatializer_info` 27) and whether a target is published and has not begun (28).
    public var equalizerFadeFramesLeft: Int64 { aw_spatializer_info(handle, 27) }
    public var equalizerTargetPending: Bool { aw_spatializer_info(handle, 28) == 1 }

    /// `reserve` plus the host entry's device-side staging: `process(hostInput:…)` never allocates afterwards either.
    public func reserveHost(maxFrames: Int64) throws {
        let st = aw_spatializer_reserve_host(handle, maxFrames)
        guard st == AW_OK else { throw BatchSpatializer.error(st) }
    }

    public func reset() { _ = aw_spatializer_reset(handle) }

    static func error(_ st: aw_status) -> NSError {
        NSError(domain: "AirwaveHIP", code: Int(st), userInfo: [NSLocalizedDescriptionKey: String(cString: aw_last_error_message())])
    }
}
