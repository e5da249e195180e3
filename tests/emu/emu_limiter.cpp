// emu_limiter.cpp — TEST-ONLY: the limiter kernel (airwave_amd/csrc/device/limiter_tile.hpp, the code hipcc compiles) on the CPU: one
// emulated workgroup of kLimThreads std::threads per tile and stream, the grid launch_limiter makes; workgroup barriers are a
// std::barrier, the wave operations go through a mailbox, the atomics are std::atomic_ref.  Beside it the header's sequential rule, its
// detector, and the true-peak rule for measuring an output.
#include <atomic>
#include <barrier>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "../../airwave_amd/csrc/device/limiter_tile.hpp"

namespace {

struct LimShared {
    std::barrier<> wg;
    std::vector<std::unique_ptr<std::barrier<>>> wave;
    std::vector<unsigned char> lds;
    std::vector<unsigned long long> box;
    LimShared() : wg(awk::kLimThreads), lds((size_t)awk::kLimLdsBytes + 16, 0xC3), box((size_t)awk::kLimThreads) {
        for (int w = 0; w < awk::kLimThreads / 64; ++w) wave.emplace_back(new std::barrier<>(64));
    }
    unsigned char *base() { return lds.data() + ((16 - (reinterpret_cast<uintptr_t>(lds.data()) & 15u)) & 15u); }
};

struct LimEmuCtx {
    int tid_;
    LimShared *sh;
    int tid() const { return tid_; }
    unsigned char *lds() const { return sh->base(); }
    void barrier() const { sh->wg.arrive_and_wait(); }
    void in_lds(const void *l, size_t n) const {
        const unsigned char *b = static_cast<const unsigned char *>(l);
        if (b < sh->base() || b + n > sh->base() + awk::kLimLdsBytes) std::abort();
    }
    void ld16(const float *g, float (&x)[4]) const { if (reinterpret_cast<uintptr_t>(g) & 15u) std::abort(); std::memcpy(x, g, 16); }
    void st16(float *g, const float (&x)[4]) const { if (reinterpret_cast<uintptr_t>(g) & 15u) std::abort(); std::memcpy(g, x, 16); }
    void ld_lds16(const float *l, float *x) const { in_lds(l, 16); if (reinterpret_cast<uintptr_t>(l) & 15u) std::abort(); std::memcpy(x, l, 16); }
    void ld_lds8(const float *l, float *x) const { in_lds(l, 8); if (reinterpret_cast<uintptr_t>(l) & 7u) std::abort(); std::memcpy(x, l, 8); }
    template <class F> unsigned long long wave_reduce(unsigned long long v, int lanes, F f) const {
        sh->box[(size_t)tid_] = v;
        sh->wave[tid_ >> 6]->arrive_and_wait();
        unsigned long long r = lanes ? sh->box[(size_t)(tid_ & ~63)] : 0ull;
        for (int l = 1; l < lanes; ++l) r = f(r, sh->box[(size_t)(tid_ & ~63) + l]);
        sh->wave[tid_ >> 6]->arrive_and_wait();
        return r;
    }
    uint32_t wave_min(uint32_t v) const { return (uint32_t)wave_reduce(v, 64, [](unsigned long long a, unsigned long long b) { return a < b ? a : b; }); }
    unsigned wave_sum(unsigned v) const { return (unsigned)wave_reduce(v, 64, [](unsigned long long a, unsigned long long b) { return a + b; }); }
    unsigned long long wave_exclusive_sum(unsigned long long v) const {
        return wave_reduce(v, tid_ & 63, [](unsigned long long a, unsigned long long b) { return a + b; });
    }
    void atomic_min(uint32_t *a, uint32_t v) const {
        std::atomic_ref<uint32_t> r(*a);
        uint32_t old = r.load();
        while (old > v && !r.compare_exchange_weak(old, v)) {}
    }
    void atomic_add(unsigned long long *a, unsigned long long v) const { std::atomic_ref<unsigned long long>(*a).fetch_add(v); }
};

}  // namespace

extern "C" {

int emu_limiter_tile() { return awk::kLimTile; }
int emu_limiter_halo(int L, int H) { return awlim::halo(L, H); }
int emu_limiter_delay(int L) { return awlim::delay(L); }
void emu_limiter_filter(float *c) { float f[awtp::kCoefficients]; awtp::filter(f); std::memcpy(c, f, sizeof(f)); }

// in / out: [n_streams][frames][2] at any float (the test shifts them to try every alignment); gain: [n_streams] or NULL;
// hist_in / hist_out: [n_streams][halo][2]; min_gain, limited, nonfinite: [n_streams]
void emu_limiter(const float *in, float *out, int n_streams, long long frames, const float *gain, int L, int H, float ceiling,
                 const float *hist_in, float *hist_out, uint32_t *min_gain, unsigned long long *limited, unsigned long long *nonfinite) {
    awk::LimiterParams p{};
    p.in = in; p.out = out; p.frames = frames; p.n_streams = n_streams; p.gain = gain;
    p.hist_in = hist_in; p.hist_out = hist_out; p.min_gain = min_gain; p.limited = limited; p.nonfinite = nonfinite;
    p.L = L; p.H = H; p.ceiling = ceiling;
    float c[awtp::kCoefficients];
    awtp::filter(c);
    std::memcpy(p.c, c, sizeof(c));
    const long long tiles = (frames + awk::kLimTile - 1) / awk::kLimTile;
    LimShared sh;
    for (int s = 0; s < n_streams; ++s)
        for (long long tile = 0; tile < tiles; ++tile) {
            std::vector<std::thread> th;
            th.reserve(awk::kLimThreads);
            for (int t = 0; t < awk::kLimThreads; ++t)
                th.emplace_back([&, t]() {
                    LimEmuCtx ctx{t, &sh};
                    awk::limiter_tile<LimEmuCtx>(ctx, p, s, tile);
                });
            for (auto &x : th) x.join();
        }
}

// the header's rule over the same buffers, stream by stream (hist carried in place); g_out [n_streams][frames] and p_out likewise, or NULL
void emu_limiter_sequential(const float *in, float *out, int n_streams, long long frames, const float *gain, int L, int H, float ceiling,
                            float *hist, uint32_t *min_gain, unsigned long long *limited, unsigned long long *nonfinite, float *g_out,
                            uint32_t *p_out) {
    float c[awtp::kCoefficients];
    awtp::filter(c);
    const size_t hl = 2 * (size_t)awlim::halo(L, H);
    for (int s = 0; s < n_streams; ++s) {
        awlim::Record r;
        r.min_gain_bits = min_gain[s]; r.limited_frames = limited[s]; r.nonfinite = nonfinite[s];
        awlim::sequential(c, L, H, ceiling, gain ? gain[s] : 1.0f, in + (size_t)s * frames * 2, frames, hist + (size_t)s * hl,
                          out + (size_t)s * frames * 2, r, g_out ? g_out + (size_t)s * frames : nullptr, p_out ? p_out + (size_t)s * frames : nullptr);
        min_gain[s] = r.min_gain_bits; limited[s] = r.limited_frames; nonfinite[s] = r.nonfinite;
    }
}

// awtp::sequential over one stream from silence: the bits of the larger ear's true peak
uint32_t emu_limiter_true_peak(const float *y, long long frames) {
    float c[awtp::kCoefficients], hist[2 * awtp::kHistory] = {};
    awtp::filter(c);
    awtp::Record r{};
    awtp::sequential(c, y, frames, hist, r);
    return r.tp_bits[0] > r.tp_bits[1] ? r.tp_bits[0] : r.tp_bits[1];
}

}
