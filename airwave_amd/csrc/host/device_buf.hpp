// device_buf.hpp — the owners of what the HIP runtime hands out by raw handle: Buf<T, Kind> (device or page-locked host memory) and Event.
// Every allocation the library keeps for itself lives in one of them: the destructor of whatever holds it frees it, and an early return
// cannot leak it.  Only aw_device_alloc / aw_host_alloc_pinned, which give the pointer to the caller, name the allocation calls themselves;
// a further unit that hands page-locked memory to its caller (aw_multi_alloc_pinned) goes through host_alloc_raw / host_free_raw below.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <utility>

namespace awr {

enum class Kind { device, pinned };
using Counter = std::atomic<long long>;          // aw_context::device_allocs / sync_copies; a `Counter *` below may be null (not counted)

// Move-only.  Every call that can fail returns the hipError_t of the HIP call that failed and leaves the buffer empty (capacity 0).
template <class T, Kind K = Kind::device> class Buf {
    T *p_ = nullptr;
    size_t cap_ = 0;          // elements
  public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf &operator=(Buf &&o) noexcept {          // takes the right side, THEN frees what the left held ("make the new one, then drop the old")
        if (this != &o) {
            Buf old(std::move(*this));
            p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~Buf() { (void)reset(); }
    T *get() const { return p_; }          // for kernel-launch structs
    explicit operator bool() const { return p_ != nullptr; }
    size_t capacity() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }
    hipError_t reset() {
        T *p = std::exchange(p_, nullptr);
        cap_ = 0;
        return !p ? hipSuccess : K == Kind::pinned ? hipHostFree(p) : hipFree(p);
    }
    // exactly n elements (what the buffer held is freed first); *allocs counts the allocation once it has succeeded
    hipError_t alloc(size_t n, Counter *allocs) {
        hipError_t e = reset();
        void *p = nullptr;
        if (e == hipSuccess) e = K == Kind::pinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p); cap_ = n;
        if (allocs) *allocs += 1;
        return hipSuccess;
    }
    // the grow-only buffers: nothing happens while the capacity suffices; else free, then allocate (the peak is one buffer, never two)
    hipError_t grow(size_t need, Counter *allocs) { return cap_ >= need ? hipSuccess : alloc(need, allocs); }
    // alloc + a blocking copy of n elements of host memory (*copies counts it); a buffer that was never written does not stay behind
    hipError_t upload(const T *src, size_t n, Counter *allocs, Counter *copies) {
        hipError_t e = alloc(n, allocs);
        if (e != hipSuccess) return e;
        if (copies) *copies += 1;
        e = hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)reset();
        return e;
    }
};

// Page-locked host memory that leaves the library (the caller owns it and gives it back): the allocation flags are the caller's business.
inline hipError_t host_alloc_raw(void **p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
inline hipError_t host_free_raw(void *p) { return hipHostFree(p); }

// The single named events.  Pooled and pending events circulate as raw handles and are not these.
class Event {
    hipEvent_t e_ = nullptr;
  public:
    Event() = default;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
    hipError_t create() { return hipEventCreate(&e_); }          // (into an empty owner)
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e_, flags); }
};

}  // namespace awr
