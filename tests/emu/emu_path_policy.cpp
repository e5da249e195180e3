// TEST-ONLY: a C interface over the kernel-path planner (airwave_amd/csrc/host/path_policy.hpp) and the library's overlap-add kernel list
// (device/ola_layouts.hpp), compiled with plain g++ for tests/test_path_policy_host.py.  Plans travel as int arrays:
//   knobs [13]: window.set, window.value, ola.set, ola.value, lw.set, lw.value, part_cmac_group, part_fwd.set, part_fwd.value,
//               part_herm.set, part_herm.value, hop_align, ola_min_blocks_per_wg
//   plan  [11]: path, fused2, hop, hist_len, partitions, n_pairs, ola_h, cmac_group, fwd_one_pair, herm_ok, lw_mode
#include "../../airwave_amd/csrc/host/path_policy.hpp"

static awp::CreatePlan plan_of(const int *v) {
    awp::CreatePlan p;
    p.path = v[0]; p.fused2 = v[1] != 0; p.hop = v[2]; p.hist_len = v[3]; p.partitions = v[4]; p.n_pairs = v[5]; p.ola_h = v[6];
    p.cmac_group = v[7] != 0; p.fwd_one_pair = v[8] != 0; p.herm_ok = v[9] != 0; p.lw_mode = v[10];
    return p;
}

extern "C" {

void pp_plan_create(int channels, int taps, int streams, const int *k, int *out) {
    awp::Knobs knobs;
    knobs.window = {k[0] != 0, k[1]}; knobs.ola = {k[2] != 0, k[3]}; knobs.lw = {k[4] != 0, k[5]};
    knobs.part_cmac_group = k[6] != 0; knobs.part_fwd = {k[7] != 0, k[8]}; knobs.part_herm = {k[9] != 0, k[10]};
    knobs.hop_align = k[11]; knobs.ola_min_blocks_per_wg = k[12];
    const awp::CreatePlan p = awp::plan_create(awp::Layout{channels, taps, streams}, knobs, awk::ola_rows_carried(channels, taps));
    const int v[11] = {p.path, p.fused2, p.hop, p.hist_len, p.partitions, p.n_pairs, p.ola_h, p.cmac_group, p.fwd_one_pair, p.herm_ok, p.lw_mode};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}

int pp_use_ola_tile(const int *plan, int channels, int taps, int streams, long long frames, int persistent_wgs, int ola_min_blocks_knob) {
    return awp::use_ola_tile(plan_of(plan), awp::Layout{channels, taps, streams}, frames, persistent_wgs, ola_min_blocks_knob) ? 1 : 0;
}

// out [5]: n_groups, R and windows of the first group, R and windows of the second
void pp_lw_choose(const int *plan, int channels, int taps, int streams, int cus, long long reserved_frames, unsigned have, long long frames,
                  int for_reserve, int *out) {
    const awp::LwInputs in{awp::Layout{channels, taps, streams}, plan_of(plan), cus, reserved_frames, have};
    const awp::LwCallPlan c = awp::lw_choose(in, frames, for_reserve != 0);
    out[0] = c.n_groups;
    for (int i = 0; i < 2; ++i) { out[1 + 2 * i] = i < c.n_groups ? c.g[i].R : 0; out[2 + 2 * i] = i < c.n_groups ? c.g[i].n_windows : 0; }
}

// the window lengths in the order of LwInputs::have's bits; 0 past the last
int pp_lw_rows(int i) { return i >= 0 && i < awp::kLwRowChoiceCount ? awp::kLwRowChoices[i] : 0; }
long long pp_ola_max_bytes() { return awk::kOlaMaxBytes; }

}  // extern "C"
