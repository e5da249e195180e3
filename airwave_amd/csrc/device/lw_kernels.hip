// lw_kernels.hip — the three kernels of the long-window path (tile_lw.hpp): split, rows, merge.
// Its own translation unit (built with -fno-slp-vectorize like the other tile kernels, airwave_amd/build.py).
#include "kernels.hpp"
#include "gpu_ctx.hpp"
#include "tile_lw.hpp"
#include "tile_lw16.hpp"
#include "lw_split_inst.hpp"
#include "launch_table.hpp"

namespace awk {

// Row pairs are pinned to XCDs (blockIdx % 8 labels the XCD): XCD x walks the row pairs x, x + 8, ... one after the other
// and, within a row pair, every (stream, window); its 32 workgroups therefore share one 512 KB table slice at a time.
template <int NP, bool REAL_LAST>
__global__ void __launch_bounds__(kThreads) aw_lw_rows_kernel(LwParams p, long long n_sw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpuCtx ctx{reinterpret_cast<cf *>(smem), nullptr};
    const int g = (int)gridDim.x, b = (int)blockIdx.x;
    const int xcd = b % 8, slot = b / 8;
    const int per_xcd_wg = (g - xcd + 7) / 8;
    lw_rows_tiles<GpuCtx, NP, REAL_LAST>(ctx, p, (long long)slot, (long long)per_xcd_wg, n_sw, xcd, 8);
}

// PB = 1: one exchange buffer, two workgroups per CU
template <int NP, bool REAL_LAST>
__global__ void __launch_bounds__(kThreads, 4) aw_lw_rows1_kernel(LwParams p, long long n_sw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpuCtx ctx{reinterpret_cast<cf *>(smem), nullptr};
    const int g = (int)gridDim.x, b = (int)blockIdx.x;
    const int xcd = b % 8, slot = b / 8;
    const int per_xcd_wg = (g - xcd + 7) / 8;
    lw_rows_tiles<GpuCtx, NP, REAL_LAST, 1>(ctx, p, (long long)slot, (long long)per_xcd_wg, n_sw, xcd, 8);
}

// 16 points of one row per thread, 256-thread workgroups (tile_lw16.hpp); the same XCD pinning of row pairs
#ifndef AW_R16_MIN_WAVES
#define AW_R16_MIN_WAVES 3
#endif
template <int NP, bool REAL_LAST>
__global__ void __launch_bounds__(kR16Threads, AW_R16_MIN_WAVES) aw_lw_rows16_kernel(LwParams p, long long n_sw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpuCtx ctx{reinterpret_cast<cf *>(smem), nullptr};
    const int g = (int)gridDim.x, b = (int)blockIdx.x;
    const int xcd = b % 8, slot = b / 8;
    const int per_xcd_wg = (g - xcd + 7) / 8;
    lw_rows16_tiles<GpuCtx, NP, REAL_LAST>(ctx, p, (long long)slot, (long long)per_xcd_wg, n_sw, xcd, 8);
}

template <int RA>
__global__ void __launch_bounds__(kThreads, 4) aw_lw_merge_kernel(LwParams p, long long n_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpuCtx ctx{reinterpret_cast<cf *>(smem), nullptr};
    lw_merge_tiles<GpuCtx, RA>(ctx, p, (long long)blockIdx.x, (long long)gridDim.x, n_tiles);
}

template <int RA> constexpr int lw_merge_lds_bytes() { return lw_merge_lds_elems<RA>() * (int)sizeof(cf); }
#define AW_LW_FOR_RA(X) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(12) X(14) X(15) X(16)

constexpr int kLwRows1LdsBytes = lw_rows_lds_elems<1>() * (int)sizeof(cf);

// The launch tables (launch_table.hpp).  Rows kernels, three forms: key = 2 pairs + REAL_LAST; the two-pairs-per-batch form exists for
// up to four pairs.  Merge kernels: key = RA.  Split kernels: two entry points per RA, their tables live in lw_split_a .. e.hip.
using LwEntry = KernelEntry<LwParams, long long>;
#define AW_ROW(KERNEL, LDS, NP) {2 * NP, &KERNEL<NP, false>, LDS, #KERNEL "<" #NP ", false>"}, {2 * NP + 1, &KERNEL<NP, true>, LDS, #KERNEL "<" #NP ", true>"},
#define AW_ROWS4(KERNEL, LDS) AW_ROW(KERNEL, LDS, 1) AW_ROW(KERNEL, LDS, 2) AW_ROW(KERNEL, LDS, 3) AW_ROW(KERNEL, LDS, 4)
#define AW_ROWS8(KERNEL, LDS) AW_ROWS4(KERNEL, LDS) AW_ROW(KERNEL, LDS, 5) AW_ROW(KERNEL, LDS, 6) AW_ROW(KERNEL, LDS, 7) AW_ROW(KERNEL, LDS, 8)
static const LwEntry kLwRows[] = {AW_ROWS4(aw_lw_rows_kernel, kLdsBytes)};
static const LwEntry kLwRows1[] = {AW_ROWS8(aw_lw_rows1_kernel, kLwRows1LdsBytes)};
static const LwEntry kLwRows16[] = {AW_ROWS8(aw_lw_rows16_kernel, kR16LdsBytes)};
#undef AW_ROWS8
#undef AW_ROWS4
#undef AW_ROW
#define AW_ROW(RA) {RA, &aw_lw_merge_kernel<RA>, lw_merge_lds_bytes<RA>(), "aw_lw_merge_kernel<" #RA ">"},
static const LwEntry kMerge[] = {AW_LW_FOR_RA(AW_ROW)};
#undef AW_ROW
struct LwSplitEntry {
    int ra;
    hipError_t (*prepare)();
    hipError_t (*launch)(const LwParams &, bool, int, dim3, hipStream_t, long long);
};
#define AW_ROW(RA) {RA, &lw_split_prepare<RA>, &lw_split_launch<RA>},
static const LwSplitEntry kSplit[] = {AW_LW_FOR_RA(AW_ROW)};
#undef AW_ROW

hipError_t prepare_lw_kernels() {
    hipError_t e = hipSuccess;
    for (const LwSplitEntry &k : kSplit)
        if (e == hipSuccess) e = k.prepare();
    if (e == hipSuccess) e = set_dynamic_lds(kLwRows);
    if (e == hipSuccess) e = set_dynamic_lds(kLwRows1);
    if (e == hipSuccess) e = set_dynamic_lds(kLwRows16);
    if (e == hipSuccess) e = set_dynamic_lds(kMerge);
    return e;
}

static unsigned lw_grid(long long n_tiles, const LwParams &p, int wgs_per_cu) {
    long long wgs = (long long)(p.persistent_wgs >= 8 ? p.persistent_wgs : 256) * wgs_per_cu;
    return (unsigned)(n_tiles < wgs ? n_tiles : wgs);
}

hipError_t launch_lw_split(const LwParams &p, int n_streams, hipStream_t stream, StageTimer *tm) {
    if (p.n_channels < 1 || p.n_channels > 16) return hipErrorInvalidValue;
    const int ra = p.R / 8;
    if (p.R % 8 != 0 || !lw_ra_ok(ra)) return hipErrorInvalidValue;
    const bool wide = p.n_channels > 8;              // 9-16 channels: both channel halves of a frame in one wave, 32 frames per tile
    const long long n_tiles = (long long)n_streams * p.n_windows * (wide ? kLwChunksW : kLwChunks);
    if (n_tiles <= 0) return hipSuccess;
    if (n_tiles > 0x7fffffffLL || (wide && !p.tail)) return hipErrorInvalidValue;
    const int cs = wide ? p.n_channels - 8 : p.n_channels;
    const dim3 grid(lw_grid(n_tiles, p, ra > 8 ? 1 : 2));
    if (tm) tm->begin();
    hipError_t e = hipErrorInvalidValue;
    for (const LwSplitEntry &k : kSplit)
        if (k.ra == ra) e = k.launch(p, wide, cs, grid, stream, n_tiles);
    if (tm) tm->end(wide ? "aw_lw_split_wide_kernel" : "aw_lw_split_kernel");
    return e;
}

hipError_t launch_lw_rows(const LwParams &p, int n_streams, hipStream_t stream, StageTimer *tm) {
    const long long n_sw = (long long)n_streams * p.n_windows;
    const long long n_tiles = n_sw * (p.R / 2);
    if (n_tiles <= 0) return hipSuccess;
    if (n_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const int key = 2 * p.n_pairs + (p.real_last != 0 ? 1 : 0);
    const LwEntry *k;
    unsigned grid, threads = kThreads;
    // 8 XCD groups: a grid that is a multiple of 8 (every group has the same number of workgroups), at least 8
    if (p.rows_form == 16) {
        if (!p.tab16 || !p.tw2) return hipErrorInvalidValue;
        const int per_cu = p.rows16_wgs >= 1 && p.rows16_wgs <= 4 ? p.rows16_wgs : 3;
        grid = lw_grid((n_tiles + 7) / 8 * 8, p, per_cu) / 8 * 8;
        threads = kR16Threads;
        k = find(kLwRows16, key);
    } else {
        const bool one = p.rows_pairs_per_batch == 1 || p.n_pairs > 4;          // the two-pairs-per-batch form exists for up to four pairs
        grid = lw_grid((n_tiles + 7) / 8 * 8, p, one ? 2 : 1) / 8 * 8;
        k = one ? find(kLwRows1, key) : find(kLwRows, key);
    }
    if (!k) return hipErrorInvalidValue;
    if (grid < 8) grid = 8;
    if (tm) tm->begin();
    launch(*k, dim3(grid), dim3(threads), stream, p, n_sw);
    if (tm) tm->end("aw_lw_rows_kernel");
    return hipGetLastError();
}

hipError_t launch_lw_merge(const LwParams &p, int n_streams, hipStream_t stream, StageTimer *tm) {
    const long long n_tiles = (long long)n_streams * p.n_windows * kLwChunks;
    if (n_tiles <= 0) return hipSuccess;
    if (n_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const LwEntry *k = find(kMerge, p.R / 8);
    if (!k) return hipErrorInvalidValue;
    if (tm) tm->begin();
    launch(*k, dim3(lw_grid(n_tiles, p, 2)), dim3(kThreads), stream, p, n_tiles);
    if (tm) tm->end("aw_lw_merge_kernel");
    return hipGetLastError();
}

}  // namespace awk
