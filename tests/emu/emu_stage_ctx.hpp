#pragma once
// emu_stage_ctx.hpp — TEST-ONLY: the CPU execution context of the output-stage tile kernels, the counterpart of
// airwave_amd/csrc/device/stage_gpu_ctx.hpp (emu_true_peak.cpp: StageEmuCtx<float>, emu_limiter.cpp: StageEmuCtx<unsigned char>).
// One emulated workgroup is a set of CPU threads (emu_workgroup.hpp): workgroup barriers are a std::barrier, the wave operations go
// through a 64-bit mailbox per thread, the atomics are std::atomic_ref.  The LDS image is aligned to 16 bytes, sized by the caller and
// poisoned; a vector access aborts where the hardware would misbehave silently: an LDS read outside the image or off its alignment, a
// 16-byte global access off a 16-byte boundary.
#include <atomic>
#include <barrier>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "emu_workgroup.hpp"

namespace {

struct StageEmuShared {
    std::barrier<> wg;
    std::vector<std::unique_ptr<std::barrier<>>> wave;
    size_t lds_bytes;
    std::vector<unsigned char> image;
    std::vector<unsigned long long> box;
    StageEmuShared(int threads, size_t lds_bytes_) : wg(threads), lds_bytes(lds_bytes_), image(lds_bytes_ + 16, 0xC3), box((size_t)threads) {
        for (int w = 0; w < threads / 64; ++w) wave.emplace_back(new std::barrier<>(64));
    }
    unsigned char *lds() { return image.data() + ((16 - (reinterpret_cast<uintptr_t>(image.data()) & 15u)) & 15u); }
};

template <class T> struct StageEmuCtx {
    int tid_;
    StageEmuShared *sh;
    int tid() const { return tid_; }
    T *lds() const { return reinterpret_cast<T *>(sh->lds()); }
    void barrier() const { sh->wg.arrive_and_wait(); }
    static void aligned(const void *p, unsigned n) { if (reinterpret_cast<uintptr_t>(p) & (n - 1u)) std::abort(); }
    void in_lds(const void *l, size_t n) const {
        const unsigned char *b = static_cast<const unsigned char *>(l);
        if (b < sh->lds() || b + n > sh->lds() + sh->lds_bytes) std::abort();
    }
    void ld16(const float *g, float (&x)[4]) const { aligned(g, 16); std::memcpy(x, g, 16); }
    void st16(float *p, const float (&x)[4]) const { aligned(p, 16); std::memcpy(p, x, 16); }
    void ld_lds16(const float *l, float *x) const { in_lds(l, 16); aligned(l, 16); std::memcpy(x, l, 16); }
    void ld_lds8(const float *l, float *x) const { in_lds(l, 8); aligned(l, 8); std::memcpy(x, l, 8); }
    // f over the values of the first `lanes` lanes of this thread's wave (0 for none)
    template <class F> unsigned long long wave_reduce(unsigned long long v, int lanes, F f) const {
        sh->box[(size_t)tid_] = v;
        sh->wave[tid_ >> 6]->arrive_and_wait();
        unsigned long long r = lanes ? sh->box[(size_t)(tid_ & ~63)] : 0ull;
        for (int l = 1; l < lanes; ++l) r = f(r, sh->box[(size_t)(tid_ & ~63) + l]);
        sh->wave[tid_ >> 6]->arrive_and_wait();
        return r;
    }
    uint32_t wave_min(uint32_t v) const { return (uint32_t)wave_reduce(v, 64, [](unsigned long long a, unsigned long long b) { return a < b ? a : b; }); }
    uint32_t wave_max(uint32_t v) const { return (uint32_t)wave_reduce(v, 64, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; }); }
    unsigned wave_sum(unsigned v) const { return (unsigned)wave_reduce(v, 64, [](unsigned long long a, unsigned long long b) { return a + b; }); }
    unsigned long long wave_exclusive_sum(unsigned long long v) const {
        return wave_reduce(v, tid_ & 63, [](unsigned long long a, unsigned long long b) { return a + b; });
    }
    void atomic_min(uint32_t *a, uint32_t v) const {
        std::atomic_ref<uint32_t> r(*a);
        uint32_t old = r.load();
        while (old > v && !r.compare_exchange_weak(old, v)) {}
    }
    void atomic_max(uint32_t *a, uint32_t v) const {
        std::atomic_ref<uint32_t> r(*a);
        uint32_t old = r.load();
        while (old < v && !r.compare_exchange_weak(old, v)) {}
    }
    void atomic_add(unsigned long long *a, unsigned long long v) const { std::atomic_ref<unsigned long long>(*a).fetch_add(v); }
};

}  // namespace
