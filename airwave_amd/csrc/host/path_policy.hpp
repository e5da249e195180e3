// path_policy.hpp — which kernels a spatializer runs: one table of measured crossovers per layout and three pure functions over it.
//   plan_create()   once per spatializer: fused 8192- / 16384-frame window or the partitioned path, hop, history, overlap-add rows
//   use_ola_tile()  once per fused call: the overlap-add tile or the overlap-save tile
//   lw_choose()     once per call: the long-window kernels (and on which window lengths) or the kernels of the path above
// Plain C++: no device call, no environment lookup, no allocation, no handle — runtime.cpp reads the knobs (AW_* at spatializer creation,
// LaunchCfg at context creation), calls these and keeps the side effects; tests/test_path_policy_host.py replays them on the CPU against
// the decisions recorded from the built library (tests/golden/path_policy_parent.json, written by tools/policy_table.py).
// Every number below is a measured crossover on the MI355X (G stereo frames/s); `bash tools/regen_policy.sh` re-measures all of them,
// DESIGN.md (§4.1c, §4.1b, §4.5) keeps the earlier rounds' numbers and says how to change a row.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../device/ola_layouts.hpp"
#include "../device/tile_ola.hpp"
#include "tables.hpp"

#ifndef AW_DEFAULT_WINDOW
#define AW_DEFAULT_WINDOW 8192
#endif

namespace awp {

constexpr int kNever = 1 << 30;

// One row per channel count.  tools/policy_table.py reads the rows (one `/* C */ {...},` per line) to place its grid around every value.
//   ola_need            overlap-add tile from 512 H >= ola_need x the overlap-save hop on (tools/ola_sweep.py; overlap-save / overlap-add / long-window)
//   fused2_from         16384-frame windows from this many taps on (tools/window_sweep.py; 8192 / 16384), kNever: only where 8192 frames cannot hold the HRIR
//   fused2_upto         ... up to this many, then the partitioned path (tools/path_sweep.py; 16384 / partitioned), 0: no 16384-frame kernels worth running
//   fused2_min_streams  ... and from this many streams (tools/small_batch_sweep.py, 4320 taps x 10 s; 8192 / 16384): fewer cannot fill the chip with 16384-frame tiles
//   lw_crossover_taps   path 0 without the overlap-add tile: long calls on the long-window kernels from this many taps (tools/lw_sweep.py; fused / long-window)
struct LayoutRow { double ola_need; int fused2_from, fused2_upto, fused2_min_streams, lw_crossover_taps; };
constexpr LayoutRow kLayouts[17] = {
    /*  0 */ {0.0, kNever, 0, 0, kNever},
    /*  1 */ {0.66, 0, 12289, 8, 10800},        // no overlap-add kernel; 4320 taps 93 / 202; 12 289: 79 / 49; 4 streams 67 / 55, 8: 79 / 81; 8640: 147 / 113
    /*  2 */ {0.66, 1800, 12289, 24, 9300},     // no overlap-add kernel; 1500: 180 / 171, 1800: 171 / 172; 12 289: 53 / 51; 16 streams 88 / 86, 24: 92 / 107; 8640: 93 / 89
    /*  3 */ {0.66, 1800, 12289, 12, 9000},     // no overlap-add kernel; 1500: 123 / 119, 1800: 117 / 119; to the window's limit; 12 streams; 6145: 85 / 70, 8640: 68 / 69
    /*  4 */ {0.94, 5300, 10500, 16, 5200},     // 3969: 86.3 / 86.6, 4320: 79.5 / 79.5; 5000: 59.9 / 58.5, 5300: 57.9 / 58.0; 10 000: 36.7 / 33.2, 11 000: 32.7 / 35.8; 4320: 70 / 60, 5300: 54 / 58
    /*  5 */ {0.66, 3400, 12289, 24, 7500},     // no overlap-add kernel (4320: 64.5 / 57.4); 3200: 63.7 / 60.5, 3500: 59.9 / 61.4; to the window's limit; 24 streams; 6145: 52 / 49, 8640: 41 / 48
    /*  6 */ {0.90, 4700, 12289, 16, 5500},     // 3585: 64.7 / 64.4, 4098: 58.4 / 58.0; 4320: 47.2 / 45.9, 5000: 39.4 / 44.9; 12 289: 21.0 / 20.7; 4320: 47 / 43, 5300: 38 / 43
    /*  7 */ {0.875, 4400, 11500, 16, 4700},    // 3000: 58.7 / 54.5, 3585: 53.3 / 54.2; 4320: 38.9 / 38.8, 4500: 36.4 / 36.8; 11 000: 21.1 / 19.1, 11 800: 18.2 / 19.0; 4320: 40.6 / 39.9, 5300: 37 / 40
    /*  8 */ {0.89, 5500, 11200, 16, 5200},     // 3585: 53.5 / 53.4, 3969: 49.4 / 53.3; 5300: 30.1 / 29.0, 5600: 27.4 / 28.4; 11 000: 17.4 / 17.2, 11 800: 15.5 / 17.3; 4320: 40 / 36, 5300: 32 / 36
    /*  9 */ {0.78, kNever, 0, 16, 4900},       // 3000: 42.5 / 43.1, 4320: 33.9 / 38.8 / 31.6; no 16384-frame vector kernels (6145 taps 8192 / partitioned 16.3 / 13.4); 4320: 30.2 / 29.4, 6145: 19 / 29
    /* 10 */ {0.74, kNever, 0, 16, 4900},       // 2048: 45.6 / 42.7, 3000: 40.7 / 42.7; no 16384-frame vector kernels; 4320: 29 / 27
    /* 11 */ {0.78, kNever, 0, 16, 4900},       // 4320: 29.3 / 33.4 / 28.1; no 16384-frame vector kernels
    /* 12 */ {0.80, kNever, 0, 16, 4900},       // 3000: 36.7 / 36.4, 3585: 34.1 / 36.2; no 16384-frame vector kernels (6145: 14.3 / 11.6); 4320: 26 / 24
    /* 13 */ {0.78, kNever, 0, 16, 4000},       // 4320: 24.1 / 28.6 / 24.9; no 16384-frame vector kernels
    /* 14 */ {0.89, kNever, 0, 16, 4300},       // 3000: 29.7 / 27.5, 3585: 27.5 / 27.6; no 16384-frame vector kernels (6145: 11.3 / 10.2); 3000: 25.8 / 22.3, 4320: 20.5 / 22.3
    /* 15 */ {0.62, kNever, 0, 16, 3200},       // 2048: 24.6 / 26.7, 4320: 17.7 / 24.2 / 21.7; no 16384-frame vector kernels (6145: 9.2 / 8.9); 3900: 18.6 / 21.7 (two-pass layout)
    /* 16 */ {0.66, kNever, 0, 16, 3200},       // 2048: 24.1 / 24.5, 4320: 17.6 / 22.7 / 20.6; no 16384-frame vector kernels; 3000: 20.1 / 19.7, 4320: 16.4 / 19.6
};
// (layouts of more than 16 channels have neither overlap-add nor long-window kernels: the columns they use are those of the last row)
constexpr const LayoutRow &layout_row(int channels) { return kLayouts[std::min(std::max(channels, 0), 16)]; }

// Blocks per persistent workgroup from which a call runs the overlap-add tile: every run pays ceil(hist / hop) <= 2 warm-up blocks, which
// must stay below what the tile gains over the overlap-save tile — 2 - 10 % for layouts of up to eight channels, 10 - 40 % for wider ones.
constexpr int ola_min_blocks_default(int channels) { return channels <= 8 ? 48 : 16; }
// Partitioned kernels, fabric-byte equivalents per output frame of a long call: ~110 + 13 C up to eight channels (measured 20-23 G frames/s
// for C = 7, 29 for C = 2), ~30 C for the one-pair forward kernels of wider layouts (tools/lw_calls_sweep.py).
constexpr double part_bytes_per_frame(int C) { return C <= 8 ? 110.0 + 13.0 * C : 30.0 * C; }

// The rules that do not depend on the layout.
constexpr int kPartitionedFromChannels = 16, kPartitionedFromTaps = 6000;   // 8192-frame tile against the partitioned path near the window's end: 16 channels cross at ~6000 taps (5800: 10.1 / 9.5; 6145: 9.1 / 9.4; tools/path_sweep.py), 9 - 15 stay fused
constexpr int kOlaWindowMinStreams = 48;      // smaller batches keep the window policy: their calls rarely have the blocks per workgroup the overlap-add tile needs
constexpr int kOlaLwCrossoverTaps = 5122;     // spatializers on the overlap-add tile (blocks of 8 / 7 / 6 rows up to 4097 / 4609 / 5121 taps): faster than the long-window kernels wherever it is chosen (tools/ola_sweep.py)
constexpr long long kLwMinRowTiles = 32;      // long-window kernels from 32 row tiles on (ONE stream x 10 s, 64 row tiles: 7 channels x 32768 taps 8.2 against 3.9 partitioned)
constexpr long long kLwFusedRowTilesPerCu = 2;   // path 0: a small batch stays on the fused tiles (cfg 1: 9.7) until its row tiles cover the CUs twice
constexpr double kLwFusedFill = 1.25;         // path 0 past the crossover: the long call only has to fill its windows to 80 %
constexpr double kLwGroupPenalty = 2.0e8;     // a second group of windows: three more launches and their ramps, ~40 us in the cost's currency (bytes at ~5 TB/s), shared by the streams
// Window lengths of the long-window kernels in rows of kLwM frames: R = 8 RA, RA = 4 .. 16 without 11 and 13, so that the padded length
// sum(N) stays close to frames + windows x history for every call length.
constexpr int kLwRowChoices[] = {32, 40, 48, 56, 64, 72, 80, 96, 112, 120, 128};
constexpr int kLwRowChoiceCount = (int)(sizeof(kLwRowChoices) / sizeof(kLwRowChoices[0]));

struct Layout { int channels, taps, streams; };
// An integer knob of the environment: whether it was set, and atoi of it.
struct Knob { bool set = false; int value = 0; };
struct Knobs {
    Knob window;                        // AW_WINDOW: 8192 | 16384 force the fused window, 4096 the partitioned path
    Knob ola;                           // AW_OLA: 0 never the overlap-add tile, 1 wherever a kernel exists
    Knob lw;                            // AW_LW: 0 never the long-window kernels, 32 .. 128 force that window
    bool part_cmac_group = false;       // AW_PART_CMAC=group
    Knob part_fwd;                      // AW_PART_FWD: 1 | 2 force the forward kernel's form
    Knob part_herm;                     // AW_PART_HERM: 0 stores the last pair's redundant half too
    int hop_align = 64;                 // LaunchCfg::hop_align (AW_HOP_ALIGN)
    int ola_min_blocks_per_wg = -1;     // LaunchCfg::ola_min_blocks_per_wg (AW_OLA_MIN_BLOCKS); < 0: per layout
};
struct CreatePlan {
    int path = 0;                       // 0 fused, 1 partitioned
    bool fused2 = false;                // path 0 on 16384-frame windows
    int hop = 0, hist_len = 0, partitions = 1, n_pairs = 0;
    int ola_h = 0;                      // path 0 on 8192-frame windows: block rows of the overlap-add tile, 0: never
    bool cmac_group = false, fwd_one_pair = false, herm_ok = true;       // partitioned path: kernel forms
    int lw_mode = -1;                   // -1 the cost model of lw_choose(), 0 never, R forces that window length
};

// Tiles start on 64-frame boundaries of the timeline: a shorter hop costs < 2 % more tiles and makes every tile's
// loads and stores start line-aligned (measured cfg 2: 1.555 -> 1.530 ms per call).  hop_align is AW_HOP_ALIGN's atoi, unchecked: below 2
// it is off, and so is a value the hop is not sixteen times as long as.  The 8192-frame and the overlap-add tile run any hop; the 16384-frame
// tile needs an even one (plan_create).
constexpr int align_hop(int hop_align, int hop) { return (hop_align > 1 && hop > 16 * hop_align) ? hop - hop % hop_align : hop; }

// Overlap-add tile or overlap-save tile for a path-0 spatializer on 8192-frame windows?  Block rows H (0: overlap-save).  `rows_carried`:
// awk::ola_rows_carried() of the layout and HRIR length; `hist_len` = rows of the history buffer the spatializer will keep (the window
// minus the aligned overlap-save hop >= taps - 1): the block's tail must fit behind its hop.  The overlap-add block is cheaper per
// transform (whole frames in registers, every input line read once, no boundary launch) but shorter than the overlap-save hop (512 H
// against 8193 - taps rounded down to 64), so it wins from a layout's ratio of the two on.
inline int ola_rows(int channels, const Knob &ola, int rows_carried, int hist_len) {
    const int mode = ola.set ? ola.value : -1;
    if (mode == 0) return 0;
    int H = rows_carried;
    while (H >= 6 && hist_len > awk::kN - 512 * H) --H;          // (the aligned history may be a few rows longer than taps - 1)
    if (H < 6) return 0;
    if (mode > 0) return H;
    const int hop_ols = awk::kN - hist_len;
    const double need = layout_row(channels).ola_need;
    return 512.0 * H >= need * hop_ols ? H : 0;
}

inline CreatePlan plan_create(const Layout &l, const Knobs &k, int ola_rows_carried) {
    CreatePlan p;
    const int N = awk::kN, C = l.channels, taps = l.taps;
    const LayoutRow &row = layout_row(C);
    p.n_pairs = (C + 1) / 2;
    int window = k.window.set ? k.window.value : 0;
    const int hist2 = awh::poly_history_frames(taps);          // 16384-frame windows (tile_ols2.hpp)
    const bool fits1 = taps - 1 <= N - 2048, fits2 = hist2 <= awk::kN2 - 4096;
    const bool fused2_ok = fits2 && taps <= row.fused2_upto;
    const int hop1 = align_hop(k.hop_align, N - (taps - 1));
    // the overlap-add tile is measured against BOTH overlap-save windows (ola_need); the choice between it and the overlap-save tile
    // of the window chosen here is per call (use_ola_tile)
    const int ola_h = (window == 0 || window == N) ? ola_rows(C, k.ola, ola_rows_carried, N - hop1) : 0;
    if (ola_h && window == 0 && l.streams >= kOlaWindowMinStreams) window = N;
    if (window == 0) {
        window = (taps >= row.fused2_from && fused2_ok) ? awk::kN2 : AW_DEFAULT_WINDOW;
        if (window == awk::kN2 && l.streams < row.fused2_min_streams && fits1) window = N;
    }
    const bool prefer_partitioned = !k.window.set && C >= kPartitionedFromChannels && taps >= kPartitionedFromTaps;
    const bool force_partitioned = window == 4096 || prefer_partitioned;
    if (!force_partitioned && ((window == awk::kN2 && fits2) || (!fits1 && fused2_ok))) {
        p.path = 0; p.fused2 = true;
        p.hop = align_hop(k.hop_align, awk::kN2 - hist2);
        p.hop -= p.hop & 1;                                          // an odd AW_HOP_ALIGN: the tile stores frames in pairs from an even window position on (tile_ols2.hpp: first_valid is even), an odd history would drop the first new frame of every tile
        p.hist_len = awk::kN2 - p.hop;                               // even, >= 2 * floor(taps / 2)
        p.n_pairs = (2 * C + 1) / 2;                                 // pseudo-pairs of the half-rate 2C-channel view
    } else if (fits1 && !force_partitioned) {
        p.path = 0;
        p.hop = hop1;
        p.hist_len = N - p.hop;
        p.ola_h = ola_h;
    } else {
        p.path = 1;
        p.hop = N / 2;
        p.partitions = (taps + p.hop - 1) / p.hop;
        p.hist_len = p.partitions * p.hop;
        p.cmac_group = p.n_pairs > 8 || k.part_cmac_group;           // the marched kernel's lane groups hold up to 8 channel pairs
        // forward kernel form: all pairs of a window in one workgroup up to 4 pairs (cfg 3: 11.2 against 12.1 ms); with more pairs
        // the four-channel batches of 56-byte-or-wider frames each re-read every line (14 channels: fabric reads 4.3x the input),
        // and one pair per workgroup — the pairs of a window side by side on one XCD — wins (27.0 -> 22.7 ms)
        p.fwd_one_pair = k.part_fwd.set ? k.part_fwd.value == 1 : p.n_pairs > 4;
        if (k.part_herm.set) p.herm_ok = k.part_herm.value != 0;
    }
    if (k.lw.set) p.lw_mode = k.lw.value;
    if (C > 16) p.lw_mode = 0;                                       // the long-window kernels hold up to eight channel pairs
    return p;
}

// Per call of a path-0 spatializer with ola_h: every workgroup of the overlap-add tile walks ONE contiguous run of blocks and pays
// ceil(hist / hop) warm-up blocks per run and per stream start; a call needs ola_min_blocks blocks per workgroup for that to stay a few
// per cent (cfg 2: 67).  Shorter calls, and streams too long for 32-bit byte offsets, run the overlap-save tile on the same tables and
// history.  `l.streams`: every stream of the spatializer, not a staged chunk's, so that every entry runs the same tile.
inline bool use_ola_tile(const CreatePlan &p, const Layout &l, int64_t frames, int persistent_wgs, int ola_min_blocks_knob) {
    if (!p.ola_h || p.fused2) return false;
    const int hop_ola = 512 * p.ola_h;
    const long long blocks = (long long)l.streams * ((frames + hop_ola - 1) / hop_ola);
    const long long wgs = std::max(1, persistent_wgs);
    const int min_blocks = ola_min_blocks_knob >= 0 ? ola_min_blocks_knob : ola_min_blocks_default(l.channels);
    return blocks >= (long long)min_blocks * wgs && frames * l.channels * 4LL <= awk::kOlaMaxBytes;
}

// A call runs as at most two groups of windows: `n` windows of R_a rows, then one window of R_b rows for what is left (either may be
// absent) — the reference's cost per frame does not depend on the stream length (uniform partitions, ConvolutionEngine.swift:93,232-367),
// and with three window lengths and one length per call this path's did (x 1.49 at 11 s).
struct LwGroup { int R; int n_windows; long long frame0, frame_end; };
struct LwCallPlan { int n_groups; LwGroup g[2]; double cost; };
struct LwInputs {
    Layout layout;
    CreatePlan plan;
    int cus;                            // compute units of the device
    int64_t reserved_frames;            // calls of up to this many frames never build tables: only window lengths whose tables exist are candidates
    uint32_t have;                      // bit i: the tables of kLwRowChoices[i] exist
};

// Long-window kernels (windows of N = R x kLwM frames, hop = N - hist_len) or the spatializer's own path, by a cost model in fabric
// bytes: the long-window kernels move 12 C + 24 bytes per WINDOW frame (input + rows written, rows read + s1/s2
// written, s1/s2 read + stereo out), whatever the HRIR length.  n_groups == 0: the spatializer's own path.
// for_reserve: every window length is a candidate (aw_spatializer_reserve builds the tables of the plan).
inline LwCallPlan lw_choose(const LwInputs &in, int64_t frames, bool for_reserve = false) {
    LwCallPlan none{};
    const Layout &l = in.layout;
    const CreatePlan &p = in.plan;
    if (p.lw_mode == 0 || l.channels > 16) return none;
    if (p.path == 0 && p.lw_mode < 0 && l.taps < (p.ola_h ? kOlaLwCrossoverTaps : layout_row(l.channels).lw_crossover_taps)) return none;
    const bool existing_only = !for_reserve && frames <= in.reserved_frames;
    auto usable = [&](int i) {
        const int R = kLwRowChoices[i];
        const long long N = (long long)R * awk::kLwM, hop = N - p.hist_len;
        if (hop < N / 4) return false;                                  // the window must be mostly new frames
        if (p.lw_mode > 0 && p.lw_mode != R) return false;
        if (existing_only && !(in.have >> i & 1u)) return false;
        return true;
    };
    const int C = l.channels;
    const double per_frame = 12.0 * C + 24.0;
    const double group_penalty = kLwGroupPenalty / (double)std::max(1, l.streams);
    LwCallPlan best{};
    for (int ia = 0; ia < kLwRowChoiceCount; ++ia) {
        if (!usable(ia)) continue;
        const int Ra = kLwRowChoices[ia];
        const long long Na = (long long)Ra * awk::kLwM, hopa = Na - p.hist_len;
        {   // one group
            const long long n = (frames + hopa - 1) / hopa;
            const double cost = (double)n * (double)Na * per_frame;
            if (!best.n_groups || cost < best.cost) { best = LwCallPlan{1, {{Ra, (int)n, 0, frames}, {}}, cost}; }
        }
        if (p.lw_mode > 0) continue;                                   // a forced window length: one group
        for (int ib = 0; ib < ia; ++ib) {                               // (the choices ascend: every shorter window)
            if (!usable(ib)) continue;
            const int Rb = kLwRowChoices[ib];
            const long long Nb = (long long)Rb * awk::kLwM, hopb = Nb - p.hist_len;
            const long long n = frames > hopb ? (frames - hopb + hopa - 1) / hopa : 0;
            if (n < 1) continue;                                        // (the remainder window alone: the one-group case of Rb)
            const long long rest = frames - n * hopa;
            if (rest <= 0) continue;
            const double cost = ((double)n * (double)Na + (double)Nb) * per_frame + group_penalty;
            if (cost < best.cost) best = LwCallPlan{2, {{Ra, (int)n, 0, n * hopa}, {Rb, 1, n * hopa, frames}}, cost};
        }
    }
    if (!best.n_groups || p.lw_mode > 0) return best;
    long long row_tiles = 0;
    for (int i = 0; i < best.n_groups; ++i) row_tiles += (long long)l.streams * best.g[i].n_windows * (best.g[i].R / 2);
    if (row_tiles < kLwMinRowTiles) return none;
    // path 0: the crossovers of the table were measured on batches that fill the chip
    if (p.path == 0 && row_tiles < kLwFusedRowTilesPerCu * in.cus) return none;
    double other_cost;
    if (p.path == 0) {
        other_cost = kLwFusedFill * (double)frames * per_frame;
    } else {
        // Partitioned kernels, in the same currency: 86 % of their bytes per input WINDOW (forward transform + marched CMAC) — and a call
        // of n blocks transforms n + P - 1 windows, which is what makes short calls expensive there — and 14 % per output block.
        // tools/lw_calls_sweep.py (partitioned / long-window, 128 streams x 7 channels x 32768 taps): 16 384 frames 6.2 / 5.9,
        // 32 768: 9.9 / 10.9, 49 152: 11.5 / 15.6, 65 536: 13.1 / 20.0, 131 072: 15.8 / 21.0, 480 000: 20.0 / 35.8.
        const double b_part = part_bytes_per_frame(C);
        const long long blocks = (frames + p.hop - 1) / p.hop;
        other_cost = (double)p.hop * b_part * (0.86 * (double)(blocks + p.partitions - 1) + 0.14 * (double)blocks);
    }
    return best.cost < other_cost ? best : none;
}

}  // namespace awp
