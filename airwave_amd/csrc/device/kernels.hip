// kernels.hip — gfx950 kernels of the batch HRIR spatializer.
//
// The tile body lives in tile_ols.hpp (shared with the CPU emulation harness); this file adds the
// GPU execution context (LDS, barriers), the XCD-aware workgroup -> tile mapping and the small
// utility kernels (history carry, synthetic fill, planar<->interleaved).
#include <cstring>
#include "kernels.hpp"
#include "gpu_ctx.hpp"
#include "ols2_kernel.hpp"
#include "pcm.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace awk {

// INTERIOR = true: tiles [tile_lo, tile_hi) of every stream (window inside the call's input)
// INTERIOR = false: the remaining boundary tiles (history at the start, zero fill at the end)
template <int CS, int NP, bool INTERIOR, bool ACC = false>
__global__ void __launch_bounds__(kThreads) aw_fused_ols_kernel(TileParams p, long long n_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpuCtx ctx{reinterpret_cast<cf *>(smem), p.dbg ? p.dbg + (long long)blockIdx.x * kStamps : nullptr};
    ctx.stamp_thread_ = p.stamp_thread;          // diagnostic builds: which thread's wave is recorded
    const XcdShare x = xcd_share(n_tiles);          // persistent workgroups, XCD-aware (gpu_ctx.hpp)
    tiles_fused_ols<GpuCtx, CS, NP, INTERIOR, ACC>(ctx, p, x.lo + x.slot, x.wgs, x.hi);
}


// Windows [tile_lo, tile_hi) of every stream lie inside the call's input (INTERIOR), the others touch the
// history or the zero page.  p.tile_lo/hi carry the window range here.
// MODE 1: windows [tile_lo, tile_hi) (interior); MODE 2: windows [head_lo, tile_lo) (head: history + input);
// MODE 0: the rest, [0, head_lo) and [tile_hi, n_windows).  Persistent, XCD-aware like the fused kernels: each XCD group
// walks a contiguous eighth of the window list, so windows that overlap by half meet in one L2.
template <int CS, int MODE>
__global__ void __launch_bounds__(kThreads) aw_part_forward_kernel(TileParams p, long long n_ids, int head_lo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpuCtx ctx{reinterpret_cast<cf *>(smem), nullptr};
    const int n_windows = p.n_blocks + p.partitions - 1;
    const int per = MODE == 1 ? p.tile_hi - p.tile_lo : MODE == 2 ? p.tile_lo - head_lo : n_windows - (p.tile_hi - head_lo);
    const int w0 = MODE == 1 ? p.tile_lo : head_lo, skip = p.tile_hi - head_lo;
    const XcdShare x = xcd_share(n_ids);
    tiles_part_forward<GpuCtx, CS, MODE>(ctx, p, x.lo + x.slot, x.wgs, x.hi, per, w0, skip);
}

// One-pair form: workgroup id -> (stream, window, pair), pairs innermost; kInvLdsBytes of LDS, two workgroups per CU.
template <int CS, int MODE>
__global__ void __launch_bounds__(kThreads, 4) aw_part_forward1_kernel(TileParams p, long long nwg, int head_lo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpuCtx ctx{reinterpret_cast<cf *>(smem), nullptr};
    const long long id = xcd_remap((long long)blockIdx.x, nwg);
    const long long wid = id / p.n_pairs;
    const int pair = (int)(id - wid * p.n_pairs);
    const int n_windows = p.n_blocks + p.partitions - 1;
    const int per = MODE == 1 ? p.tile_hi - p.tile_lo : MODE == 2 ? p.tile_lo - head_lo : n_windows - (p.tile_hi - head_lo);
    const long long stream = wid / per;
    int w = (int)(wid - stream * per);
    if (MODE == 1) w += p.tile_lo;
    else if (MODE == 2) w += head_lo;
    else if (w >= head_lo) w += p.tile_hi - head_lo;
    tile_part_forward1<GpuCtx, CS, MODE>(ctx, p, stream, w, pair);
}

// grid = (N / kCmacThreads, block groups, streams): one thread per bin of kCmacBlocks consecutive blocks
__global__ void __launch_bounds__(kCmacThreads) aw_part_cmac_kernel(TileParams p) {
    part_cmac_bin(p, (long long)blockIdx.z, (int)blockIdx.y * kCmacBlocks, (int)(blockIdx.x * kCmacThreads + threadIdx.x));
}

__global__ void __launch_bounds__(kThreads) aw_part_inverse_kernel(TileParams p, long long nwg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpuCtx ctx{reinterpret_cast<cf *>(smem), nullptr};
    const long long id = xcd_remap((long long)blockIdx.x, nwg);
    tile_part_inverse<GpuCtx>(ctx, p, id / p.n_blocks, (int)(id % p.n_blocks));
}

// (real channels, batches): 2C pseudo-channels in batches of four
#define AW_FOR_EACH_VEC2(X) X(1, 1) X(2, 1) X(3, 2) X(5, 3) X(7, 4)      // 4, 6 and 8 channels live in ols2_even_kernels.hip (SLP on)

// Kernel variants.  Vectorised interior kernels <CS, NP, true> exist for 2-16 channels (frames that are not whole float4s are
// loaded 16 B per lane at dword alignment, zero tables cancel the lanes that run into the next frame; 9-14 channels in one
// pass over two eight-channel groups, 15-16 in two passes); the boundary tiles of every layout, and mono, run the
// generic-addressing kernels <0, NP, false> (NP = compile-time pair count 1..4; NP = 0 loops over batches of two pairs at
// run time).  The (12, 0) (14, 0) (16, 0) entries are the round-1 run-time-loop kernels (AW_WIDE_TWO_PASS=0) and the wide
// layouts' forward kernels of the partitioned path.
#define AW_FOR_EACH_VEC(X) X(2, 1) X(3, 2) X(4, 2) X(5, 3) X(6, 3) X(7, 4) X(8, 4) X(12, 0) X(14, 0) X(16, 0)
#define AW_FOR_EACH_GEN(X) X(1) X(2) X(3) X(4) X(0)
// wide layouts (interior tiles): (channels, pairs of the first pass, pairs of the accumulating second pass)
#define AW_FOR_EACH_WIDE(X) X(10, 4, 1) X(12, 4, 2) X(14, 4, 3) X(15, 4, 4) X(16, 4, 4)
// 10-14 channels in one pass: (channels, pairs).  16 channels stay on two passes (one pass: 292 B of scratch per thread,
// 13.5 against 13.9 G frames/s)
#define AW_FOR_EACH_WIDE1(X) X(9, 5) X(10, 5) X(11, 6) X(12, 6) X(13, 7) X(14, 7)
// boundary tiles of the common layouts keep whole-frame vector loads (history / zero-page selects per frame)
#define AW_FOR_EACH_BVEC(X) X(2, 1) X(4, 2) X(8, 4)

// The launch tables (launch_table.hpp): one row per instantiation, built from the lists above.  Keys: channels, or pairs for the
// generic kernels; 4 channels + MODE for the partitioned path's forward kernels, whose names are their StageTimer stage names.
#define AW_ROW(CS, NP) {CS, &aw_fused_ols_kernel<CS, NP, true>, kLdsBytes, "aw_fused_ols_kernel<" #CS ", " #NP ", true>"},
static const TileEntry kVec[] = {AW_FOR_EACH_VEC(AW_ROW)};
static const TileEntry kWide1[] = {AW_FOR_EACH_WIDE1(AW_ROW)};
#undef AW_ROW
#define AW_ROW(CS, NPA, NPB) {CS, &aw_fused_ols_kernel<CS, NPA, true, false>, kLdsBytes, "aw_fused_ols_kernel<" #CS ", " #NPA ", true>"},
static const TileEntry kWideFirst[] = {AW_FOR_EACH_WIDE(AW_ROW)};
#undef AW_ROW
#define AW_ROW(CS, NPA, NPB) {CS, &aw_fused_ols_kernel<CS, NPB, true, true>, kLdsBytes, "aw_fused_ols_kernel<" #CS ", " #NPB ", true, accumulate>"},
static const TileEntry kWideSecond[] = {AW_FOR_EACH_WIDE(AW_ROW)};
#undef AW_ROW
#define AW_ROW(CS, NP) {CS, &aw_fused_ols_kernel<CS, NP, false>, kLdsBytes, "aw_fused_ols_kernel<" #CS ", " #NP ", false>"},
static const TileEntry kBvec[] = {AW_FOR_EACH_BVEC(AW_ROW)};
#undef AW_ROW
#define AW_ROW(NP) {NP, &aw_fused_ols_kernel<0, NP, false>, kLdsBytes, "aw_fused_ols_kernel<0, " #NP ", false>"},
static const TileEntry kGen[] = {AW_FOR_EACH_GEN(AW_ROW)};
#undef AW_ROW
#define AW_ROW(NP) {NP, &aw_fused_ols_kernel<0, NP, false, true>, kLdsBytes, "aw_fused_ols_kernel<0, " #NP ", false, accumulate>"},
static const TileEntry kGenAcc[] = {AW_ROW(1) AW_ROW(2) AW_ROW(3) AW_ROW(4)};      // second pass of 9-16 channels: the pairs beyond the first four
#undef AW_ROW
#define AW_ROW(CS, NB) {CS, &aw_fused_ols2_kernel<CS, NB, true>, kLdsBytes, "aw_fused_ols2_kernel<" #CS ", " #NB ", true>"},
static const TileEntry kVec2[] = {AW_FOR_EACH_VEC2(AW_ROW)};
#undef AW_ROW
#define AW_ROW(CS, NB) {CS, &aw_fused_ols2_kernel<CS, NB, false>, kLdsBytes, "aw_fused_ols2_kernel<" #CS ", " #NB ", false>"},
static const TileEntry kBnd2[] = {AW_FOR_EACH_VEC2(AW_ROW) {0, &aw_fused_ols2_kernel<0, 0, false>, kLdsBytes, "aw_fused_ols2_kernel<0, 0, false>"}};
#undef AW_ROW
using FwdEntry = KernelEntry<TileParams, long long, int>;
#define AW_ROW(CS, NP)                                                                                         \
    {4 * CS + 1, &aw_part_forward_kernel<CS, 1>, kLdsBytes, "aw_part_forward_kernel<CS, interior>"},           \
    {4 * CS + 2, &aw_part_forward_kernel<CS, 2>, kLdsBytes, "aw_part_forward_kernel<CS, head>"},
static const FwdEntry kFwd[] = {AW_FOR_EACH_VEC(AW_ROW) {0, &aw_part_forward_kernel<0, 0>, kLdsBytes, "aw_part_forward_kernel<generic>"}};
#undef AW_ROW
#define AW_ROW(CS, NP)                                                                                         \
    {4 * CS + 1, &aw_part_forward1_kernel<CS, 1>, kInvLdsBytes, "aw_part_forward1_kernel<CS, interior>"},      \
    {4 * CS + 2, &aw_part_forward1_kernel<CS, 2>, kInvLdsBytes, "aw_part_forward1_kernel<CS, head>"},
static const FwdEntry kFwd1[] = {AW_FOR_EACH_VEC(AW_ROW) {0, &aw_part_forward1_kernel<0, 0>, kInvLdsBytes, "aw_part_forward1_kernel<generic>"}};
#undef AW_ROW

// the 16384-frame tile of a layout: the even layouts' table first (ols2_even_kernels.hip), then this unit's
static const TileEntry *find_ols2(int C, bool interior) {
    if (const TileEntry *k = find_ols2_even(C, interior)) return k;
    return interior ? find(kVec2, C) : find(kBnd2, C);
}
const char *fused_ols2_kernel_name(int C) {
    const TileEntry *k = find_ols2(C, true);
    return k ? k->name : find(kBnd2, 0)->name;
}

// the dynamic-LDS attribute of every tile kernel of this unit and of ols2_even_kernels.hip
static hipError_t set_tile_kernel_lds() {
    hipError_t e = set_dynamic_lds(kVec);
    if (e == hipSuccess) e = set_dynamic_lds(kWideFirst);
    if (e == hipSuccess) e = set_dynamic_lds(kWideSecond);
    if (e == hipSuccess) e = set_dynamic_lds(kWide1);
    if (e == hipSuccess) e = set_dynamic_lds(kGenAcc);
    if (e == hipSuccess) e = set_dynamic_lds(kGen);
    if (e == hipSuccess) e = set_dynamic_lds(kBvec);
    if (e == hipSuccess) e = set_dynamic_lds(kVec2);
    if (e == hipSuccess) e = set_dynamic_lds(kBnd2);
    if (e == hipSuccess) e = prepare_ols2_even();
    if (e == hipSuccess) e = set_dynamic_lds(kFwd);
    if (e == hipSuccess) e = set_dynamic_lds(kFwd1);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&aw_part_inverse_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kInvLdsBytes);
    return e;
}

// The device query and the AW_* knobs of a context, then the kernels' attributes: the one place of the device code that reads the environment.
hipError_t prepare_kernels(LaunchCfg *cfg) {
    if (!cfg) return set_tile_kernel_lds();
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
        cfg->cus = cus;
        cfg->persistent_wgs = cus;            // one resident workgroup per CU (152 KB LDS each)
    }
    int &g_persistent_wgs = cfg->persistent_wgs;
    if (const char *e2 = getenv("AW_PERSISTENT_WGS")) g_persistent_wgs = atoi(e2) > 0 ? atoi(e2) : g_persistent_wgs;
    // the persistent kernels deal tiles to 8 XCD groups (blockIdx % 8): a grid below 8 workgroups with more tiles than
    // workgroups would leave groups without a workgroup and their tiles uncomputed
    if (g_persistent_wgs < 8) g_persistent_wgs = 8;
    if (const char *e3 = getenv("AW_WIDE_TWO_PASS")) cfg->wide_two_pass = atoi(e3) != 0;      // A/B: 1 = two passes, 0 = run-time loop
    cfg->debug_occupancy = getenv("AW_DEBUG_OCCUPANCY") != nullptr;
    if (const char *e5 = getenv("AW_STAMP_THREAD")) cfg->stamp_thread = atoi(e5);
    if (const char *e6 = getenv("AW_EQ_EAR_SPLIT")) cfg->eq_ear_split = atoi(e6);
    if (const char *e7 = getenv("AW_LW_ROWS_PB")) cfg->lw_rows_pb = atoi(e7) == 2 ? 2 : 1;
    if (const char *e8 = getenv("AW_HOP_ALIGN")) cfg->hop_align = atoi(e8);
    if (const char *e9 = getenv("AW_LW_ROWS_FORM")) cfg->lw_rows_form = atoi(e9) == 8 ? 8 : 16;
    if (const char *e10 = getenv("AW_LW_ROWS16_WGS")) cfg->lw_rows16_wgs = atoi(e10) >= 1 && atoi(e10) <= 4 ? atoi(e10) : cfg->lw_rows16_wgs;
    if (const char *e12 = getenv("AW_LW_TABLES")) cfg->lw_tables_on_gpu = std::strcmp(e12, "host") == 0 ? 0 : 1;
    if (const char *e13 = getenv("AW_OLA_MIN_BLOCKS")) cfg->ola_min_blocks_per_wg = atoi(e13) >= 0 ? atoi(e13) : cfg->ola_min_blocks_per_wg;
    if (const char *e14 = getenv("AW_HOST_OUT_ASYNC")) cfg->host_out_async = atoi(e14) != 0;
    if (const char *e11 = getenv("AW_HOST_CHUNK_MB")) cfg->host_chunk_mb = atoi(e11) >= 1 ? atoi(e11) : cfg->host_chunk_mb;
    return set_tile_kernel_lds();
}

static bool has_vec_variant(int C) { return find(kVec, C) != nullptr; }
// 9, 10, 11, 13, 15 channels: the fused kernels only
static bool has_fused_vec_variant(int C) { return has_vec_variant(C) || find(kWide1, C) || find(kWideFirst, C); }

const char *fused_ols_kernel_name(int C) {
    if (C == 15) return "aw_fused_ols_kernel<15, 4, true> + <15, 4, true, accumulate>";
    if (C == 16) return "aw_fused_ols_kernel<16, 4, true> + <16, 4, true, accumulate>";
    if (const TileEntry *k = find(kWide1, C)) return k->name;
    if (const TileEntry *k = find(kVec, C)) return k->name;
    return "aw_fused_ols_kernel<0, NP, false>";
}

static dim3 persistent_grid(long long n_tiles, const TileParams &p) {
    const long long wgs = p.persistent_wgs >= 8 ? p.persistent_wgs : 256;
    return dim3((unsigned)(n_tiles < wgs ? n_tiles : wgs));
}

// one persistent launch over n_tiles tiles; no kernel, no launch (the callers' variant checks keep layouts without one away)
static void launch_tiles(const TileEntry *k, const TileParams &p, long long n_tiles, hipStream_t stream) {
    if (k) launch(*k, persistent_grid(n_tiles, p), dim3(kThreads), stream, p, n_tiles);
}

static void launch_vec(const TileParams &p, long long n_tiles, hipStream_t stream) {
    const TileEntry *one = p.wide_two_pass == 2 ? find(kWide1, p.n_channels) : nullptr;
    if (one) return launch_tiles(one, p, n_tiles, stream);      // 10/12/14 channels in one pass over two eight-channel groups (the default)
    const TileEntry *first = find(kWideFirst, p.n_channels);
    if ((p.wide_two_pass || p.n_channels == 10) && first) {
        // second pass: input and tables shifted by the first pass's 4 pairs (8 channels), result added to the output
        TileParams q = p;
        q.in = p.in + 8;
        q.tab = p.tab + 4 * (long long)kN;
        launch_tiles(first, p, n_tiles, stream);
        return launch_tiles(find(kWideSecond, p.n_channels), q, n_tiles, stream);
    }
    launch_tiles(find(kVec, p.n_channels), p, n_tiles, stream);
}

static void launch_gen(const TileParams &p, long long n_tiles, hipStream_t stream) {
    if (const TileEntry *k = find(kBvec, p.n_channels)) return launch_tiles(k, p, n_tiles, stream);
    if (p.n_pairs > 4 && p.n_pairs <= 8 && p.wide_two_pass) {
        // 9-16 channels: compile-time 4-pair pass, then an accumulating compile-time pass over the remaining pairs
        // (input, history and tables shifted by 8 channels; ch_base keeps the padding-channel test right)
        TileParams q = p;
        q.in = p.in + 8; q.hist = p.hist + 8; q.tab = p.tab + 4 * (long long)kN; q.ch_base = 8;
        launch_tiles(find(kGen, 4), p, n_tiles, stream);
        return launch_tiles(find(kGenAcc, p.n_pairs - 4), q, n_tiles, stream);
    }
    launch_tiles(find(kGen, p.n_pairs <= 4 ? p.n_pairs : 0), p, n_tiles, stream);
}

// Which windows of a call lie entirely inside its input.  Windows of `window` frames follow each other every `hop` frames, window 0
// starts `start` frames before the input (in the history); [lo, hi) are those that start at frame >= 0 and end at least `slack`
// frames before the input does, both clamped to `tiles`.  hi < lo when there is none: the caller says where the empty range sits.
struct TileRange { long long lo, hi; };
static TileRange interior_range(long long frames, int window, int hop, long long start, long long tiles, int slack) {
    const long long last = frames - slack - window + start;         // latest start of such a window, counted from window 0's
    TileRange r{(start + hop - 1) / hop, last >= 0 ? last / hop + 1 : 0};
    if (r.hi > tiles) r.hi = tiles;
    if (r.lo > tiles) r.lo = tiles;
    return r;
}
// 8192-frame windows: layouts whose frames are not whole float4s read up to 3 floats past a frame (load_batch): one frame of slack
static int frame_slack(int C) { return (C % 4 != 0 && C != 2) ? 1 : 0; }
static bool fits_grid(long long n) { return n <= 0x7fffffffLL; }

// Interior tiles (window entirely inside the call's input) and boundary tiles are separate launches.
hipError_t launch_fused_ols(const TileParams &p_in, int n_streams, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                            long long *dominant_tiles) {
    TileParams p = p_in;
    // tile i is interior iff  i*hop - hist_len >= 0  and  i*hop - hist_len + N <= frames
    TileRange r = interior_range(p.frames, kN, p.hop, p.hist_len, p.tiles_per_stream, frame_slack(p.n_channels));
    if (r.hi < r.lo) r.hi = r.lo;
    if (!has_fused_vec_variant(p.n_channels) || (p.wide_two_pass != 2 && p.n_channels > 8 && (p.n_channels & 1))) r = {0, 0};  // everything through the generic kernels
    p.tile_lo = (int)r.lo; p.tile_hi = (int)r.hi;
    const long long n_int = (long long)n_streams * (r.hi - r.lo);
    const long long n_bnd = (long long)n_streams * (p.tiles_per_stream - (r.hi - r.lo));
    if (!fits_grid(n_int) || !fits_grid(n_bnd)) return hipErrorInvalidValue;
    // the events bracket the DOMINANT launch only (interior tiles when the layout has a vector variant)
    const bool dom_int = n_int > 0;
    if (dominant_tiles) *dominant_tiles = dom_int ? n_int : n_bnd;
    if (ev0 && dom_int) (void)hipEventRecord(ev0, stream);
    if (n_int > 0) launch_vec(p, n_int, stream);
    if (ev1 && dom_int) (void)hipEventRecord(ev1, stream);
    if (n_bnd > 0) {
        TileParams pb = p;
        pb.dbg = nullptr;                 // diagnostic stamps describe the interior launch only
        if (ev0 && !dom_int) (void)hipEventRecord(ev0, stream);
        launch_gen(pb, n_bnd, stream);
        if (ev1 && !dom_int) (void)hipEventRecord(ev1, stream);
    }
    return hipGetLastError();
}

// 16384-frame windows: same interior / boundary split, in real frames.
hipError_t launch_fused_ols2(const TileParams &p_in, int n_streams, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                             long long *dominant_tiles) {
    TileParams p = p_in;
    // the last batch of a pseudo-frame reads up to 2 floats past it (2C not a multiple of 4): keep that much input after the window
    const int slack = ((2 * p.n_channels) % 4 != 0) ? (p.n_channels == 1 ? 2 : 1) : 0;
    TileRange r = interior_range(p.frames, kN2, p.hop, p.hist_len, p.tiles_per_stream, slack);
    if (r.hi < r.lo) r.hi = r.lo;
    const TileEntry *interior = find_ols2(p.n_channels, true);
    if (!interior) r = {0, 0};
    p.tile_lo = (int)r.lo; p.tile_hi = (int)r.hi;
    const long long n_int = (long long)n_streams * (r.hi - r.lo);
    const long long n_bnd = (long long)n_streams * (p.tiles_per_stream - (r.hi - r.lo));
    if (!fits_grid(n_int) || !fits_grid(n_bnd)) return hipErrorInvalidValue;
    const bool dom_int = n_int > 0;
    if (dominant_tiles) *dominant_tiles = dom_int ? n_int : n_bnd;
    if (n_int > 0) {
        if (ev0) (void)hipEventRecord(ev0, stream);
        launch_tiles(interior, p, n_int, stream);
        if (ev1) (void)hipEventRecord(ev1, stream);
    }
    if (n_bnd > 0) {
        p.dbg = nullptr;                 // diagnostic stamps describe the interior launch only
        if (ev0 && !dom_int) (void)hipEventRecord(ev0, stream);
        // compile-time channel and batch counts also for the boundary tiles (scalar loads) of the layouts that have an interior kernel
        const TileEntry *boundary = find_ols2(p.n_channels, false);
        launch_tiles(boundary ? boundary : find(kBnd2, 0), p, n_bnd, stream);
        if (ev1 && !dom_int) (void)hipEventRecord(ev1, stream);
    }
    return hipGetLastError();
}

hipError_t launch_part_forward(const TileParams &p_in, int n_streams, hipStream_t stream, StageTimer *tm) {
    TileParams p = p_in;
    const int n_windows = p.n_blocks + p.partitions - 1;
    if ((long long)n_streams * n_windows <= 0) return hipSuccess;
    // window w covers frames [(w - P) B, (w - P) B + N): interior iff it starts at >= 0 and ends inside the input
    // (one frame of slack for layouts whose frames are not whole float4s, see load_batch); head iff it starts in the
    // history (which reaches back P B frames: every window does) and still ends inside the input
    TileRange r = interior_range(p.frames, kN, p.hop, (long long)p.partitions * p.hop, n_windows, frame_slack(p.n_channels));
    const long long head_lo = 0;
    if (r.hi < r.lo) r.lo = r.hi;                   // short call: even some head windows run past the end
    if (!has_vec_variant(p.n_channels)) r = {0, 0};
    p.tile_lo = (int)r.lo; p.tile_hi = (int)r.hi;
    const long long n_int = (long long)n_streams * (r.hi - r.lo), n_head = (long long)n_streams * (r.lo - head_lo);
    const long long n_bnd = (long long)n_streams * (n_windows - (r.hi - head_lo));
    // one-pair form (the default): one channel pair per workgroup, two workgroups per CU; else persistent workgroups that walk all pairs
    const long long per = p.fwd_one_pair ? p.n_pairs : 1;
    if (!fits_grid(n_int) || !fits_grid(n_bnd) || !fits_grid(n_head)) return hipErrorInvalidValue;
    if (!fits_grid(n_int * per) || !fits_grid(n_bnd * per) || !fits_grid(n_head * per)) return hipErrorInvalidValue;
    // MODE 1 interior, 2 head, 0 the rest through the generic kernel
    for (const int mode : {1, 2, 0}) {
        const long long n = mode == 1 ? n_int : mode == 2 ? n_head : n_bnd;
        if (n <= 0) continue;
        const int key = mode ? 4 * p.n_channels + mode : 0;
        const FwdEntry *k = p.fwd_one_pair ? find(kFwd1, key) : find(kFwd, key);
        if (!k) return hipErrorInvalidValue;
        if (tm) tm->begin();
        launch(*k, p.fwd_one_pair ? dim3((unsigned)(n * per)) : persistent_grid(n, p), dim3(kThreads), stream, p, n * per, (int)head_lo);
        if (tm) tm->end(k->name);
    }
    return hipGetLastError();
}

hipError_t launch_part_cmac(const TileParams &p, int n_streams, hipStream_t stream, StageTimer *tm) {
    const int groups = (p.n_blocks + kCmacBlocks - 1) / kCmacBlocks;
    if (n_streams <= 0 || groups <= 0) return hipSuccess;
    if (groups > 65535 || n_streams > 65535) return hipErrorInvalidValue;
    if (tm) tm->begin();
    hipLaunchKernelGGL(aw_part_cmac_kernel, dim3(kN / kCmacThreads, (unsigned)groups, (unsigned)n_streams), dim3(kCmacThreads), 0,
                       stream, p);
    if (tm) tm->end("aw_part_cmac_kernel");
    return hipGetLastError();
}

hipError_t launch_part_inverse(const TileParams &p, int n_streams, hipStream_t stream, StageTimer *tm) {
    const long long nwg = (long long)n_streams * p.n_blocks;
    if (nwg <= 0) return hipSuccess;
    if (nwg > 0x7fffffffLL) return hipErrorInvalidValue;
    if (tm) tm->begin();
    hipLaunchKernelGGL(aw_part_inverse_kernel, dim3((unsigned)nwg), dim3(kThreads), kInvLdsBytes, stream, p, nwg);
    if (tm) tm->end("aw_part_inverse_kernel");
    return hipGetLastError();
}

// ---- history carry ---------------------------------------------------------------------------
__global__ void aw_hist_update_kernel(const float *__restrict__ in, const float *__restrict__ hist_old,
                                      float *__restrict__ hist_new, long long frames, int C, int hist_len) {
    const long long s = blockIdx.y;
    const long long per = (long long)hist_len * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long long)gridDim.x * blockDim.x) {
        const long long fi = i / C;
        const int ch = (int)(i - fi * C);
        const long long f = frames - hist_len + fi;
        const float v = f < 0 ? hist_old[s * per + (hist_len + f) * C + ch] : in[(s * frames + f) * C + ch];
        hist_new[s * per + i] = v;
    }
}

hipError_t launch_hist_update(const float *in, const float *hist_old, float *hist_new, long long frames,
                              int n_channels, int hist_len, int n_streams, hipStream_t stream) {
    if (hist_len <= 0 || n_streams <= 0) return hipSuccess;
    const long long per = (long long)hist_len * n_channels;
    unsigned gx = (unsigned)((per + 255) / 256);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(aw_hist_update_kernel, dim3(gx, (unsigned)n_streams), dim3(256), 0, stream, in, hist_old,
                       hist_new, frames, n_channels, hist_len);
    return hipGetLastError();
}

// ---- synthetic input (splitmix64: pcm.hpp, shared with the PCM encode's dither) -------------
using awp::splitmix64;

__global__ void aw_synth_fill_kernel(float *__restrict__ dst, long long per_stream, unsigned long long seed,
                                     unsigned long long first_stream) {
    const unsigned long long s = blockIdx.y;
    const unsigned long long key0 = (seed + first_stream + s) * 0x9E3779B97F4A7C15ull;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per_stream; i += (long long)gridDim.x * blockDim.x) {
        const unsigned top = (unsigned)(splitmix64(key0 + (unsigned long long)i) >> 40);
        dst[s * per_stream + i] = (float)top * (1.0f / 16777216.0f) - 0.5f;
    }
}

hipError_t launch_synth_fill(float *dst, int n_streams, long long per_stream, unsigned long long seed,
                             unsigned long long first_stream, hipStream_t stream) {
    if (n_streams <= 0 || per_stream <= 0) return hipSuccess;
    long long gx = (per_stream + 255) / 256;
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(aw_synth_fill_kernel, dim3((unsigned)gx, (unsigned)n_streams), dim3(256), 0, stream, dst,
                       per_stream, seed, first_stream);
    return hipGetLastError();
}

// ---- planar <-> interleaved stereo (plugin-shaped entry) ---------------------------------------
__global__ void aw_interleave2_kernel(const float *l, const float *r, float *dst, int frames) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < frames) { dst[2 * i] = l[i]; dst[2 * i + 1] = r[i]; }
}
__global__ void aw_deinterleave2_kernel(const float *src, float *l, float *r, int frames) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < frames) { l[i] = src[2 * i]; r[i] = src[2 * i + 1]; }
}
hipError_t launch_interleave2(const float *l, const float *r, float *dst, int frames, hipStream_t stream) {
    if (frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(aw_interleave2_kernel, dim3((frames + 255) / 256), dim3(256), 0, stream, l, r, dst, frames);
    return hipGetLastError();
}
hipError_t launch_deinterleave2(const float *src, float *l, float *r, int frames, hipStream_t stream) {
    if (frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(aw_deinterleave2_kernel, dim3((frames + 255) / 256), dim3(256), 0, stream, src, l, r, frames);
    return hipGetLastError();
}

}  // namespace awk
