// loudness_kernels.hip — gfx950 kernels of the per-stream integrated loudness (device code in loudness_scan.hpp).
#include "loudness_kernels.hpp"
#include "scan_gpu_ctx.hpp"

namespace awk {

// The tables come in as `const __restrict__` kernel arguments: with a wave-uniform index hipcc reads them with scalar loads.
__global__ void __launch_bounds__(kEqThreads, 2) aw_loudness_kernel(LoudnessParams p, const double *__restrict__ tab, const double *__restrict__ plane) {
    extern __shared__ __align__(16) unsigned char ld_lds[];
    ScanGpuCtx ctx{reinterpret_cast<cf *>(ld_lds)};
    p.tab = tab;
    p.plane = plane;
    loudness_stream<ScanGpuCtx>(ctx, p, (long long)blockIdx.x);
}

__global__ void aw_loudness_sequential_kernel(LoudnessParams p, int n_streams) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_streams) loudness_sequential(p, i);
}

hipError_t prepare_loudness_kernels() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_loudness_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdLdsBytes);
}

hipError_t launch_loudness(const LoudnessParams &p, int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || p.frames <= 0) return hipSuccess;
    const long long body = p.hop >= kEqChunk ? p.frames - p.frames % kEqChunk : 0;
    if (body > 0) {
        LoudnessParams q = p;
        q.frames = body;
        hipLaunchKernelGGL(aw_loudness_kernel, dim3((unsigned)n_streams), dim3(kEqThreads), kLdLdsBytes, stream, q, q.tab, q.plane);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (p.frames > body) {
        LoudnessParams q = p;
        q.in = p.in + body * 2; q.frames = p.frames - body; q.frame0 = p.frame0 + body;
        hipLaunchKernelGGL(aw_loudness_sequential_kernel, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, stream, q, n_streams);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace awk
