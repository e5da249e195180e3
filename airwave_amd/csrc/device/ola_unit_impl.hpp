// ola_unit_impl.hpp — body of one ola_kernels_<x>.hip unit: define AW_OLA_UNIT_LIST, AW_OLA_UNIT_LAUNCH and AW_OLA_UNIT_PREPARE, then include.
#include "ola_inst.hpp"
#include "ola_kernel.hpp"

namespace awk {

// the unit's launch table, key = 16 channels + H
#define AW_ROW(CS, H) {16 * CS + H, &aw_fused_ola_kernel<CS, (CS + 1) / 2, H>, kLdsBytes, "aw_fused_ola_kernel<" #CS ", (" #CS " + 1) / 2, " #H ">"},
static const TileEntry kOla[] = {AW_OLA_UNIT_LIST(AW_ROW)};
#undef AW_ROW

hipError_t AW_OLA_UNIT_PREPARE() { return set_dynamic_lds(kOla); }

bool AW_OLA_UNIT_LAUNCH(const TileParams &p, int H, dim3 grid, long long n_tiles, hipStream_t stream) {
    const auto *k = find(kOla, 16 * p.n_channels + H);
    if (k) launch(*k, grid, dim3(kThreads), stream, p, n_tiles);
    return k != nullptr;
}

}  // namespace awk
