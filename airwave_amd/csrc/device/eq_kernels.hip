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

// A segment of a target change's fade (eq_stage.hpp): the stage kernel's block -> (stream, ear) map; a fading stream runs both of its
// cascades on the chunk its threads hold and mixes before the one store, a stream that does not fade does what it does in
// aw_eq_stage_kernel.  More LDS than the stage kernel (the old rendering's rows, 144 / 74 KB): one workgroup per CU for both ears, two for
// one, and the launch bounds say so, which leaves each wave the registers of one / two waves per SIMD.
template <int E>
__global__ void __launch_bounds__(kEqThreads, E == 2 ? 1 : 2) aw_eq_stage_fade_kernel(EqFadeParams fp, const int *__restrict__ map,
                                                                                      const int *__restrict__ to_map, const EqStagePreset *__restrict__ presets, const double *__restrict__ tables, int n_streams) {
    extern __shared__ __align__(16) unsigned char eq_lds[];
    ScanGpuCtx ctx{reinterpret_cast<cf *>(eq_lds)};
    if constexpr (E == 2) eq_stage_fade_stream<ScanGpuCtx, 2>(ctx, fp, map, to_map, presets, tables, (long long)blockIdx.x, 0);
    else {
        const int b = (int)blockIdx.x, stream = (b >> 4) * 8 + (b & 7);
        if (stream < n_streams) eq_stage_fade_stream<ScanGpuCtx, 1>(ctx, fp, map, to_map, presets, tables, (long long)stream, (b >> 3) & 1);
    }
}

__global__ void aw_eq_stage_fade_tail_kernel(EqFadeParams fp, int n_streams) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_streams * 2) eq_stage_fade_sequential(fp, i >> 1, i & 1);
}

// The two ends of a fade, one workgroup per stream.  begin: the published entry becomes the stream's target and its second state starts
// from zero.  end: a fading stream's target and second state become its active ones.
__global__ void aw_eq_stage_turn_kernel(int begin, int *map, int *to_map, int *pending_map, double *z, double *z_to, int row_doubles) {
    const long long s = blockIdx.x;
    const int entry = begin ? pending_map[s] : to_map[s];
    __syncthreads();
    if (entry == kEqKeep) return;
    for (int i = (int)threadIdx.x; i < row_doubles; i += (int)blockDim.x) {
        if (begin) z_to[s * row_doubles + i] = 0.0;
        else z[s * row_doubles + i] = z_to[s * row_doubles + i];
    }
    if (threadIdx.x == 0) {
        if (begin) { to_map[s] = entry; pending_map[s] = kEqKeep; }
        else { map[s] = entry; to_map[s] = kEqKeep; }
    }
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
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_eq_stage_fade_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, eq_fade_lds_bytes(2));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_eq_stage_fade_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, eq_fade_lds_bytes(1));
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

// launch_eq_stage's policy and grids
hipError_t launch_eq_stage_fade(const EqFadeParams &p, int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || p.s.frames <= 0) return hipSuccess;
    const int cus = p.s.cus > 0 ? p.s.cus : 256, force = p.s.ear_split;
    const bool split = force >= 0 ? force != 0 : 2 * n_streams <= 3 * cus;
    if (split)
        hipLaunchKernelGGL(aw_eq_stage_fade_kernel<1>, dim3((unsigned)((n_streams + 7) / 8) * 16), dim3(kEqThreads), eq_fade_lds_bytes(1), stream, p, p.s.map, p.to_map, p.s.presets, p.s.tables, n_streams);
    else
        hipLaunchKernelGGL(aw_eq_stage_fade_kernel<2>, dim3((unsigned)n_streams), dim3(kEqThreads), eq_fade_lds_bytes(2), stream, p, p.s.map, p.to_map, p.s.presets, p.s.tables, n_streams);
    return hipGetLastError();
}

hipError_t launch_eq_stage_fade_tail(const EqFadeParams &p, int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || p.s.frames <= 0) return hipSuccess;
    const int n = n_streams * 2;
    hipLaunchKernelGGL(aw_eq_stage_fade_tail_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, p, n_streams);
    return hipGetLastError();
}

hipError_t launch_eq_stage_turn(bool begin, int *map, int *to_map, int *pending_map, double *z, double *z_to, int kmax, int n_streams, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    hipLaunchKernelGGL(aw_eq_stage_turn_kernel, dim3((unsigned)n_streams), dim3(64), 0, stream, begin ? 1 : 0, map, to_map, pending_map, z, z_to, kmax * 4);
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
