// Test-only stand-in for <hip/hip_runtime.h>: what airwave_amd/csrc/host/device_buf.hpp uses and no more, over malloc / free, so that the
// real header's types run under the host sanitizers (tests/harness/device_buf_check.cpp).  It keeps a count of live blocks per kind and of
// live events, logs one letter per call, and can fail the k-th allocation or the next copy.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
constexpr unsigned hipHostMallocDefault = 0, hipEventDisableTiming = 2;
typedef struct hip_stub_event *hipEvent_t;

namespace hip_stub {
inline int live[2], events, wrong_kind;          // live[0]: device blocks, live[1]: page-locked ones; wrong_kind: frees through the other pair of calls
inline int fail_at;                              // k > 0: the k-th allocation from now fails with hipErrorOutOfMemory
inline bool fail_copy;                           // the next hipMemcpy fails
inline std::string log;                          // m f: hipMalloc / hipFree, M F: the page-locked pair, c: hipMemcpy, e E: event made / destroyed
inline void (*on_free)(void *) = nullptr;        // called with the block before it goes
inline hipError_t alloc(void **p, size_t bytes, int kind) {
    log += "mM"[kind];
    *p = nullptr;
    if (fail_at > 0 && --fail_at == 0) return hipErrorOutOfMemory;
    char *b = static_cast<char *>(std::malloc(bytes + 16));          // 16 bytes in front say which pair of calls made the block
    b[0] = (char)kind;
    *p = b + 16;
    ++live[kind];
    return hipSuccess;
}
inline hipError_t release(void *p, int kind) {
    log += "fF"[kind];
    if (on_free) on_free(p);
    char *b = static_cast<char *>(p) - 16;
    if (b[0] != kind) ++wrong_kind;
    --live[(int)b[0]];
    std::free(b);
    return hipSuccess;
}
}  // namespace hip_stub

inline hipError_t hipMalloc(void **p, size_t bytes) { return hip_stub::alloc(p, bytes, 0); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return hip_stub::alloc(p, bytes, 1); }
inline hipError_t hipFree(void *p) { return hip_stub::release(p, 0); }
inline hipError_t hipHostFree(void *p) { return hip_stub::release(p, 1); }
inline hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) {
    hip_stub::log += 'c';
    if (hip_stub::fail_copy) { hip_stub::fail_copy = false; return hipErrorUnknown; }
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    hip_stub::log += 'e';
    *e = static_cast<hipEvent_t>(std::malloc(1));
    ++hip_stub::events;
    return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
inline hipError_t hipEventDestroy(hipEvent_t e) {
    hip_stub::log += 'E';
    --hip_stub::events;
    std::free(e);
    return hipSuccess;
}
