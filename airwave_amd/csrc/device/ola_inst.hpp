// ola_inst.hpp — the translation units that build the overlap-add tile kernels (tile_ola.hpp) of the list in ola_layouts.hpp.
#pragma once
#include "kernels.hpp"
#include "ola_layouts.hpp"

namespace awk {
// each returns false when the (channels, H) pair is not one of its unit's
bool launch_ola_a(const TileParams &p, int H, dim3 grid, long long n_tiles, hipStream_t stream);
bool launch_ola_b(const TileParams &p, int H, dim3 grid, long long n_tiles, hipStream_t stream);
bool launch_ola_c(const TileParams &p, int H, dim3 grid, long long n_tiles, hipStream_t stream);
bool launch_ola_d(const TileParams &p, int H, dim3 grid, long long n_tiles, hipStream_t stream);
bool launch_ola_e(const TileParams &p, int H, dim3 grid, long long n_tiles, hipStream_t stream);
bool launch_ola_f(const TileParams &p, int H, dim3 grid, long long n_tiles, hipStream_t stream);
hipError_t prepare_ola_a();
hipError_t prepare_ola_b();
hipError_t prepare_ola_c();
hipError_t prepare_ola_d();
hipError_t prepare_ola_e();
hipError_t prepare_ola_f();
}  // namespace awk
