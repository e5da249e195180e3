// shard_plan.hpp — how a batch of independent streams is cut over the shards of a multi-device handle (aw_multi, multi_runtime.cpp).
// Pure host arithmetic: no device call and no environment lookup, so tests/emu/emu_shard_plan.cpp checks it with plain g++.
//
// The rule is airwave_amd/sharding.py's shard_streams: contiguous shards in stream order, the first total % world of them one stream
// longer.  A shard of zero streams is legal (more shards than streams): it owns nothing and every range skips it.
#pragma once
#include <cstdint>

namespace awsh {

struct Shard { int32_t first = 0, count = 0; };

// shard `rank` of `world` over streams [0, total): world >= 1, 0 <= rank < world, total >= 0
inline Shard shard_streams(int32_t total, int32_t world, int32_t rank) {
    const int32_t q = total / world, r = total % world;
    return Shard{rank * q + (rank < r ? rank : r), q + (rank < r ? 1 : 0)};
}

// One piece of a global stream range: streams [global_first, global_first + count) are streams [local_first, local_first + count) of
// shard `shard`.
struct Piece { int32_t shard = 0, global_first = 0, local_first = 0, count = 0; };

// Cuts the global range [first_stream, first_stream + n) (inside [0, total), n >= 0) into its per-shard pieces, in stream order; empty
// pieces are left out.  Returns the number of pieces written to `out`, which holds up to `world` of them.  Every getter and every sliced
// setter of the multi handle walks these.
inline int32_t shard_ranges(int32_t total, int32_t world, int32_t first_stream, int32_t n, Piece *out) {
    int32_t k = 0;
    const int64_t lo = first_stream, hi = (int64_t)first_stream + n;
    for (int32_t i = 0; i < world; ++i) {
        const Shard s = shard_streams(total, world, i);
        const int64_t a = lo > s.first ? lo : s.first, b = hi < (int64_t)s.first + s.count ? hi : (int64_t)s.first + s.count;
        if (b > a) out[k++] = Piece{i, (int32_t)a, (int32_t)(a - s.first), (int32_t)(b - a)};
    }
    return k;
}

// the shard that owns `stream` (0 <= stream < total)
inline int32_t shard_of(int32_t total, int32_t world, int32_t stream) {
    Piece p;
    return shard_ranges(total, world, stream, 1, &p) == 1 ? p.shard : -1;
}

}  // namespace awsh
