// TEST-ONLY, compile only (tests/test_multi_host.py, plain g++): the C++ mirror of the multi-device handle in include/airwave_hip.hpp is
// instantiated with every member a host would call, so a signature that drifts from include/airwave_hip.h fails to compile.
#include "../../include/airwave_hip.hpp"

int main() {
    std::vector<float> tracks(2 * 8, 1.0f);
    aw::MultiSpatializer m({0, 0}, tracks.data(), 2, 8, 48000.0, {0, 1}, {1, 0}, 5);
    const std::vector<aw::MultiSpatializer::Shard> shards = m.shards();
    const int64_t fft = m.shardInfo(0, 0);
    m.reservePcm(1000, AW_SAMPLE_S16, AW_SAMPLE_S16);
    int16_t *in = static_cast<int16_t *>(m.allocPinned(5 * 1000 * 2 * sizeof(int16_t)));
    int16_t *out = static_cast<int16_t *>(m.allocPinned(5 * 1000 * 2 * sizeof(int16_t)));
    m.setDither(AW_DITHER_TPDF, 1, 0);
    m.setMetering(true);
    m.setGainFixed(std::vector<float>(5, 0.5f));
    m.setGainNone();
    m.setGainPeakCeiling(0.9f);
    m.setGainTruePeakCeiling(0.9f);
    m.setLoudness(true, 10.0);
    m.setTruePeak(true);
    m.setLimiter(true);
    aw::EqualizerDefinition def(0.0);
    m.setEqualizer({def.get()}, {0, 0, -1, 0, 0});
    m.setEqualizerTarget({def.get()}, {0, AW_EQ_KEEP, -1, 0, 0});
    const uint64_t clipped = m.processPcmHost(in, AW_SAMPLE_S16, out, AW_SAMPLE_S16, 1000);
    std::vector<float> fin(5 * 100 * 2), fout(5 * 100 * 2);
    m.processHost(fin.data(), fout.data(), 100);
    const size_t records = m.levels(0, 5).size() + m.loudness(1, 3).size() + m.truePeak(0, 5).size() + m.limiter(2, 2).size() + m.loudnessHops(3, 0, 2).size();
    m.resetLevels();
    m.reset();
    m.freePinned(in);
    m.freePinned(out);
    const struct aw_device_info d = aw::deviceInfo(0);
    return (int)(shards.size() + (size_t)fft + clipped + records + (size_t)d.compute_units + (size_t)aw::deviceCount() + (size_t)m.streamCount() + (size_t)m.channelCount()) & 0;
}
