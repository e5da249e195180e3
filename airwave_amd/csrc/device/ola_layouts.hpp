// ola_layouts.hpp — which overlap-add tile kernels (tile_ola.hpp) the library carries: the (channels, rows) list the translation units
// of ola_inst.hpp instantiate, readable by host code and by CPU tests (plain C++).
// (channels, rows H of 512 frames per block): hop = 512 H, HRIRs of up to 8193 - 512 H taps.  H = 8 serves 3585 .. 4097 taps (the bundled
// HRIRs at 44.1 kHz: 3969) and everything shorter that the policy sends here, H = 7 4098 .. 4609 (the bundled HRIRs at 48 kHz: 4320),
// Layouts: 4 and 6 - 16 channels (mono, stereo, 3 and 5 channels run faster on their 16384-frame overlap-save tiles: 5 channels measured 0.80 - 0.99,
// profiles/round6_v5/ola_sweep_odd.txt).  H = 6 up to 5121 taps — beyond that the long-window kernels (or the 16384-frame tile) measure faster for every layout: blocks of 5 rows
// were built and measured (profiles/round6_v1/ola_sweep.txt: 0.88 - 1.02 of the best alternative) and are not carried.
#pragma once
#include "tile_ols.hpp"

#define AW_OLA_FOR_H(X, CS) X(CS, 6) X(CS, 7) X(CS, 8)
#define AW_OLA_LAYOUTS_A(X) AW_OLA_FOR_H(X, 4) AW_OLA_FOR_H(X, 6)
#define AW_OLA_LAYOUTS_B(X) AW_OLA_FOR_H(X, 7) AW_OLA_FOR_H(X, 8)
#define AW_OLA_LAYOUTS_C(X) AW_OLA_FOR_H(X, 10) AW_OLA_FOR_H(X, 12)
#define AW_OLA_LAYOUTS_D(X) AW_OLA_FOR_H(X, 14) AW_OLA_FOR_H(X, 13)
#define AW_OLA_LAYOUTS_E(X) AW_OLA_FOR_H(X, 16) AW_OLA_FOR_H(X, 15)
#define AW_OLA_LAYOUTS_F(X) AW_OLA_FOR_H(X, 9) AW_OLA_FOR_H(X, 11)

namespace awk {
// whether one of the units carries the (channels, H) kernel
constexpr bool ola_has_kernel(int n_channels, int rows) {
#define AW_ROW(CS, H) if (n_channels == CS && rows == H) return true;
    AW_OLA_LAYOUTS_A(AW_ROW) AW_OLA_LAYOUTS_B(AW_ROW) AW_OLA_LAYOUTS_C(AW_ROW) AW_OLA_LAYOUTS_D(AW_ROW) AW_OLA_LAYOUTS_E(AW_ROW) AW_OLA_LAYOUTS_F(AW_ROW)
#undef AW_ROW
    return false;
}
// rows H of the block a layout's HRIR length maps to (0: no kernel): the largest H <= 8 whose window still holds the tail
constexpr int ola_rows_carried(int n_channels, int taps) {
    if (taps < 2) return 0;
    int H = (kN - (taps - 1)) / 512;
    if (H > 8) H = 8;
    return ola_has_kernel(n_channels, H) ? H : 0;
}
}  // namespace awk
