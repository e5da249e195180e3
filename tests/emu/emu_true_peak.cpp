// emu_true_peak.cpp — TEST-ONLY: the true-peak kernel (airwave_amd/csrc/device/truepeak_tile.hpp, the code hipcc compiles) on the CPU: one
// emulated workgroup of kTpThreads std::threads per tile and stream, the grid launch_truepeak makes; workgroup barriers are a
// std::barrier, the wave reductions go through a mailbox, the atomics are std::atomic_ref.  Beside it the header's sequential rule.
#include <atomic>
#include <barrier>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "../../airwave_amd/csrc/device/truepeak_tile.hpp"

namespace {

struct TpShared {
    std::barrier<> wg;
    std::vector<std::unique_ptr<std::barrier<>>> wave;
    std::vector<float> lds;
    std::vector<uint32_t> box;
    TpShared() : wg(awk::kTpThreads), lds((size_t)awk::kTpLdsFloats, -7.0f), box((size_t)awk::kTpThreads) {
        for (int w = 0; w < awk::kTpThreads / 64; ++w) wave.emplace_back(new std::barrier<>(64));
    }
};

struct TpEmuCtx {
    int tid_;
    TpShared *sh;
    int tid() const { return tid_; }
    float *lds() const { return sh->lds.data(); }
    void barrier() const { sh->wg.arrive_and_wait(); }
    void ld16(const float *g, float (&x)[4]) const { if (reinterpret_cast<uintptr_t>(g) & 15u) std::abort(); std::memcpy(x, g, 16); }
    void st16(float *l, const float (&x)[4]) const { if ((l - sh->lds.data()) & 3) std::abort(); std::memcpy(l, x, 16); }
    void ld_lds16(const float *l, float *x) const { if ((l - sh->lds.data()) & 3) std::abort(); std::memcpy(x, l, 16); }
    void ld_lds8(const float *l, float *x) const { if ((l - sh->lds.data()) & 1) std::abort(); std::memcpy(x, l, 8); }
    template <class F> uint32_t wave_reduce(uint32_t v, F f) const {
        sh->box[(size_t)tid_] = v;
        sh->wave[tid_ >> 6]->arrive_and_wait();
        uint32_t r = sh->box[(size_t)(tid_ & ~63)];
        for (int l = 1; l < 64; ++l) r = f(r, sh->box[(size_t)(tid_ & ~63) + l]);
        sh->wave[tid_ >> 6]->arrive_and_wait();
        return r;
    }
    uint32_t wave_max(uint32_t v) const { return wave_reduce(v, [](uint32_t a, uint32_t b) { return a > b ? a : b; }); }
    unsigned wave_sum(unsigned v) const { return wave_reduce(v, [](uint32_t a, uint32_t b) { return a + b; }); }
    void atomic_max(uint32_t *a, uint32_t v) const {
        std::atomic_ref<uint32_t> r(*a);
        uint32_t old = r.load();
        while (old < v && !r.compare_exchange_weak(old, v)) {}
    }
    void atomic_add(unsigned long long *a, unsigned long long v) const { std::atomic_ref<unsigned long long>(*a).fetch_add(v); }
};

}  // namespace

extern "C" {

int emu_true_peak_tile() { return awk::kTpTile; }

void emu_true_peak_filter(float *c) { float f[awtp::kCoefficients]; awtp::filter(f); std::memcpy(c, f, sizeof(f)); }

// in: [n_streams][frames][2] at any float (the test shifts it to try every alignment); hist_in / hist_out: [n_streams][11][2];
// tp_bits: [n_streams][2] or NULL; nonfinite: [n_streams]; call_tp: [n_streams]
void emu_true_peak(const float *in, int n_streams, long long frames, const float *hist_in, float *hist_out, uint32_t *tp_bits,
                   unsigned long long *nonfinite, uint32_t *call_tp) {
    awk::TruePeakParams p{};
    p.in = in; p.frames = frames; p.n_streams = n_streams;
    p.hist_in = hist_in; p.hist_out = hist_out; p.tp_bits = tp_bits; p.nonfinite = nonfinite; p.call_tp = call_tp;
    float c[awtp::kCoefficients];
    awtp::filter(c);
    std::memcpy(p.c, c, sizeof(c));
    const long long tiles = (frames + awk::kTpTile - 1) / awk::kTpTile;
    TpShared sh;
    for (int s = 0; s < n_streams; ++s)
        for (long long tile = 0; tile < tiles; ++tile) {
            std::vector<std::thread> th;
            th.reserve(awk::kTpThreads);
            for (int t = 0; t < awk::kTpThreads; ++t)
                th.emplace_back([&, t]() {
                    TpEmuCtx ctx{t, &sh};
                    awk::truepeak_tile<TpEmuCtx>(ctx, p, s, tile);
                });
            for (auto &x : th) x.join();
        }
}

// the header's rule over the same buffers, stream by stream (hist carried in place)
void emu_true_peak_sequential(const float *in, int n_streams, long long frames, float *hist, uint32_t *tp_bits, unsigned long long *nonfinite,
                              uint32_t *call_tp) {
    float c[awtp::kCoefficients];
    awtp::filter(c);
    for (int s = 0; s < n_streams; ++s) {
        awtp::Record r{{tp_bits[2 * s], tp_bits[2 * s + 1]}, call_tp[s], nonfinite[s]};
        awtp::sequential(c, in + (size_t)s * frames * 2, frames, hist + (size_t)s * 22, r);
        tp_bits[2 * s] = r.tp_bits[0]; tp_bits[2 * s + 1] = r.tp_bits[1]; call_tp[s] = r.call_tp_bits; nonfinite[s] = r.nonfinite;
    }
}

}
