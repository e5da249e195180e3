// TEST-ONLY: C entry points over airwave_amd/csrc/host/shard_plan.hpp for tests/test_shard_plan_host.py (plain g++, no device code).
#include "../../airwave_amd/csrc/host/shard_plan.hpp"

extern "C" {

void sp_shard_streams(int total, int world, int rank, int *first, int *count) {
    const awsh::Shard s = awsh::shard_streams(total, world, rank);
    *first = s.first;
    *count = s.count;
}

// out: [world][4] = shard, global first, local first, count; returns the number of pieces
int sp_shard_ranges(int total, int world, int first_stream, int n, int *out) {
    awsh::Piece pieces[64];
    const int k = awsh::shard_ranges(total, world, first_stream, n, pieces);
    for (int j = 0; j < k; ++j) {
        out[4 * j + 0] = pieces[j].shard;
        out[4 * j + 1] = pieces[j].global_first;
        out[4 * j + 2] = pieces[j].local_first;
        out[4 * j + 3] = pieces[j].count;
    }
    return k;
}

int sp_shard_of(int total, int world, int stream) { return awsh::shard_of(total, world, stream); }

}  // extern "C"
