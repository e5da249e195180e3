// ols2_even_kernels.hip — the 16384-frame-window kernels of 4, 6 and 8 channels, in a translation unit of their
// own: through round 3 they kept hipcc's SLP vectoriser (see ols2_kernel.hpp; since the half-wave row transform of round 4 they are
// built without it like everything else, build.py), and the unit builds beside kernels.hip.  Everything else about them is in kernels.hip.
#include "ols2_kernel.hpp"

namespace awk {

#define AW_FOR_EACH_VEC2_EVEN(X) X(4, 2) X(6, 3) X(8, 4)

// key = 2 channels + INTERIOR
#define AW_ROW(CS, NB)                                                                                                          \
    {2 * CS + 1, &aw_fused_ols2_kernel<CS, NB, true>, kLdsBytes, "aw_fused_ols2_kernel<" #CS ", " #NB ", true>"},               \
    {2 * CS, &aw_fused_ols2_kernel<CS, NB, false>, kLdsBytes, "aw_fused_ols2_kernel<" #CS ", " #NB ", false>"},
static const TileEntry kEven[] = {AW_FOR_EACH_VEC2_EVEN(AW_ROW)};
#undef AW_ROW

hipError_t prepare_ols2_even() { return set_dynamic_lds(kEven); }
const TileEntry *find_ols2_even(int n_channels, bool interior) { return find(kEven, 2 * n_channels + (interior ? 1 : 0)); }

}  // namespace awk
