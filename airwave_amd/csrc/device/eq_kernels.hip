// eq_kernels.hip — gfx950 kernels of the parametric EQ row (device code in eq_cascade.hpp).
#include "eq_kernels.hpp"
#include "scan_gpu_ctx.hpp"

#include <cstdlib>

#ifndef AW_EQ_WAVES
#define AW_EQ_WAVES 2
#endif
namespace awk {

// The tables come in as `const __restrict__` kernel arguments (not inside the struct): with a wave-uniform
// index that is what lets hipcc read them with scalar loads.  in/out may alias (in place) and are not restrict.
// E = 2: one workgroup per stream, two waves per SIMD.  E = 1: one per (stream, ear), three waves per SIMD (<= 168 VGPRs,
// 38 KB of LDS); workgroups b and b + 8 — the same XCD under the round-robin dispatch — take the two ears of one stream,
// so the frames both of them load cross the fabric once.
template <int E>
__global__ void __launch_bounds__(kEqThreads, E == 2 ? AW_EQ_WAVES : (kEqChunk <= 16 ? 4 : kEqChunk <= 32 ? 3 : 2)) aw_eq_cascade_kernel(EqParams p, const double *__restrict__ tab,
                                                                                      const double *__restrict__ plane, int n_streams) {
    extern __shared__ __align__(16) unsigned char eq_lds[];
    ScanGpuCtx ctx{reinterpret_cast<cf *>(eq_lds)};
    p.t.tab = tab;
    p.t.plane = plane;
    if constexpr (E == 2) eq_cascade_stream<ScanGpuCtx, 2>(ctx, p, (long long)blockIdx.x, 0);
    else {
        const int b = (int)blockIdx.x, stream = (b >> 4) * 8 + (b & 7);
        if (stream < n_streams) eq_cascade_stream<ScanGpuCtx, 1>(ctx, p, (long long)stream, (b >> 3) & 1);
    }
}

__global__ void aw_eq_sequential_kernel(EqParams p, int n_streams) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_streams * 2) eq_sequential(p, i >> 1, i & 1);
}

// The batch entries' equalizer stage: the two kernels above with the stream's preset looked up first (eq_stage_stream).  Same launch
// bounds, LDS and block -> (stream, ear) map; the map, the headers and the tables are `const __restrict__` arguments for the same reason.
// A workgroup whose stream is not equalized returns before it loads anything else.
template <int E>
__global__ void __launch_bounds__(kEqThreads, E == 2 ? AW_EQ_WAVES : (kEqChunk <= 16 ? 4 : kEqChunk <= 32 ? 3 : 2)) aw_eq_stage_kernel(EqStageParams sp, const int *__restrict__ map,
                                                                                      const EqStagePreset *__restrict__ presets, const double *__restrict__ tables, int n_streams) {
    extern __shared__ __align__(16) unsigned char eq_lds[];
    ScanGpuCtx ctx{reinterpret_cast<cf *>(eq_lds)};
    if constexpr (E == 2) eq_stage_stream<ScanGpuCtx, 2>(ctx, sp, map, presets, tables, (long long)blockIdx.x, 0);
    else {
        const int b = (int)blockIdx.x, stream = (b >> 4) * 8 + (b & 7);
        if (stream < n_streams) eq_stage_stream<ScanGpuCtx, 1>(ctx, sp, map, presets, tables, (long long)stream, (b >> 3) & 1);
    }
}

__global__ void aw_eq_stage_tail_kernel(EqStageParams sp, int n_streams) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_streams * 2) eq_stage_sequential(sp, i >> 1, i & 1);
}

__global__ void aw_eq_blend_kernel(const float *__restrict__ old_seg, const float *__restrict__ new_seg, float *__restrict__ out,
                                   long long seg_frames, long long out_stride, long long t_frame, long long length) {
#pragma clang fp contract(off)
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long s = blockIdx.y;
    if (f >= seg_frames) return;
    const double progress = (double)(t_frame + f + 1) / (double)length;
    const double inverse = 1 - progress;
    const float2 o = reinterpret_cast<const float2 *>(old_seg)[s * seg_frames + f];
    const float2 n = reinterpret_cast<const float2 *>(new_seg)[s * seg_frames + f];
    float2 r;
    r.x = (float)((double)o.x * inverse + (double)n.x * progress);
    r.y = (float)((double)o.y * inverse + (double)n.y * progress);
    reinterpret_cast<float2 *>(out)[s * out_stride + f] = r;
}

__global__ void aw_eq_copy_kernel(const float *__restrict__ src, long long src_stride, float *__restrict__ dst,
                                  long long dst_stride, long long frames) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long s = blockIdx.y;
    if (f < frames) reinterpret_cast<float2 *>(dst)[s * dst_stride + f] = reinterpret_cast<const float2 *>(src)[s * src_stride + f];
}

// 74 KB (both ears) / 38 KB of dynamic LDS: above the 64 KB a kernel gets without asking.  Called from aw_context_create.
hipError_t prepare_eq_kernels() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_eq_cascade_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, eq_lds_bytes(2));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_eq_cascade_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, eq_lds_bytes(1));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_eq_stage_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, eq_lds_bytes(2));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_eq_stage_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, eq_lds_bytes(1));
    return e;
}

hipError_t launch_eq_cascade(const EqParams &p, int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || p.frames <= 0) return hipSuccess;
    // split the ears over two workgroups while the per-ear grid still fits the CUs in one round (three workgroups per CU):
    // 128 streams 2.34 -> 1.76 ms, 384 streams 3.80 -> 3.42 ms; 448 streams 3.92 vs 4.53 ms and 512 streams 4.14 vs 4.61 ms
    // the other way (tools/archive/ab_eq_split.sh)
    const int cus = p.cus > 0 ? p.cus : 256, force = p.ear_split;       // from the context (read once at its creation)
    const bool split = force >= 0 ? force != 0 : 2 * n_streams <= 3 * cus;
    if (split)
        hipLaunchKernelGGL(aw_eq_cascade_kernel<1>, dim3((unsigned)((n_streams + 7) / 8) * 16), dim3(kEqThreads), eq_lds_bytes(1), stream, p, p.t.tab, p.t.plane, n_streams);
    else
        hipLaunchKernelGGL(aw_eq_cascade_kernel<2>, dim3((unsigned)n_streams), dim3(kEqThreads), eq_lds_bytes(2), stream, p, p.t.tab, p.t.plane, n_streams);
    return hipGetLastError();
}

hipError_t launch_eq_sequential(const EqParams &p, int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || p.frames <= 0) return hipSuccess;
    const int n = n_streams * 2;
    hipLaunchKernelGGL(aw_eq_sequential_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, p, n_streams);
    return hipGetLastError();
}

// launch_eq_cascade's policy and grids
hipError_t launch_eq_stage(const EqStageParams &p, int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || p.frames <= 0) return hipSuccess;
    const int cus = p.cus > 0 ? p.cus : 256, force = p.ear_split;
    const bool split = force >= 0 ? force != 0 : 2 * n_streams <= 3 * cus;
    if (split)
        hipLaunchKernelGGL(aw_eq_stage_kernel<1>, dim3((unsigned)((n_streams + 7) / 8) * 16), dim3(kEqThreads), eq_lds_bytes(1), stream, p, p.map, p.presets, p.tables, n_streams);
    else
        hipLaunchKernelGGL(aw_eq_stage_kernel<2>, dim3((unsigned)n_streams), dim3(kEqThreads), eq_lds_bytes(2), stream, p, p.map, p.presets, p.tables, n_streams);
    return hipGetLastError();
}

hipError_t launch_eq_stage_tail(const EqStageParams &p, int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || p.frames <= 0) return hipSuccess;
    const int n = n_streams * 2;
    hipLaunchKernelGGL(aw_eq_stage_tail_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, p, n_streams);
    return hipGetLastError();
}

hipError_t launch_eq_blend(const float *old_seg, const float *new_seg, float *out, int n_streams, long long seg_frames,
                           long long out_stride, long long t_frame, long long length, hipStream_t stream) {
    if (n_streams <= 0 || seg_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(aw_eq_blend_kernel, dim3((unsigned)((seg_frames + 255) / 256), (unsigned)n_streams), dim3(256), 0, stream,
                       old_seg, new_seg, out, seg_frames, out_stride, t_frame, length);
    return hipGetLastError();
}

hipError_t launch_eq_copy(const float *src, long long src_stride, float *dst, long long dst_stride, int n_streams,
                          long long frames, hipStream_t stream) {
    if (n_streams <= 0 || frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(aw_eq_copy_kernel, dim3((unsigned)((frames + 255) / 256), (unsigned)n_streams), dim3(256), 0, stream, src,
                       src_stride, dst, dst_stride, frames);
    return hipGetLastError();
}

}  // namespace awk
