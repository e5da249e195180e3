// TEST-ONLY: a C interface over the scratch and chunk planner (airwave_amd/csrc/host/scratch_plan.hpp), compiled with plain g++ for
// tests/test_scratch_plan_host.py.  Plans travel as the int arrays of emu_path_policy.cpp (plan [11]); a call plan as
//   call [5]: n_groups, R and windows of the first group, R and windows of the second
// and every result as an array of long long, in the field order of emu_scratch_plan.py.
#include "../../airwave_amd/csrc/host/scratch_plan.hpp"
#include "emu_path_policy.cpp"

typedef long long ll;

static awp::LwCallPlan call_of(const ll *c) {
    awp::LwCallPlan p{};
    p.n_groups = (int)c[0];
    for (int i = 0; i < p.n_groups; ++i) { p.g[i].R = (int)c[1 + 2 * i]; p.g[i].n_windows = (int)c[2 + 2 * i]; }
    return p;
}
static void call_to(const awp::LwCallPlan &c, ll *out) {
    out[0] = c.n_groups;
    for (int i = 0; i < 2; ++i) { out[1 + 2 * i] = i < c.n_groups ? c.g[i].R : 0; out[2 + 2 * i] = i < c.n_groups ? c.g[i].n_windows : 0; }
}
// out [7]: n_blocks, n_windows, per_stream, per_stream_w, chunk, need, wspec_at
static void part_to(const awp::PartScratch &s, ll *out) {
    const ll v[7] = {s.n_blocks, s.n_windows, (ll)s.per_stream, (ll)s.per_stream_w, s.chunk, (ll)s.need, (ll)s.wspec_at()};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
}
// out [10]: chunk, need of the plan, then per group: spec_per_sw, per_stream, the group's own chunk, wrows_at(the plan's chunk)
static void lw_to(const awp::LwCallPlan &c, const awp::LwPlanScratch &all, ll *out) {
    out[0] = all.chunk; out[1] = (ll)all.need;
    for (int i = 0; i < 2; ++i) {
        const bool on = i < c.n_groups;
        const awp::LwScratch &g = all.g[i];
        const ll v[4] = {on ? g.spec_per_sw : 0, on ? (ll)g.per_stream : 0, on ? g.chunk : 0, on ? (ll)g.wrows_at(all.chunk) : 0};
        for (int k = 0; k < 4; ++k) out[2 + 4 * i + k] = v[k];
    }
}
// the scratch of one call, whichever kernels run it: out [5 + 7 + 10] = the call plan, part_to (path 1 without groups), lw_to (groups)
static void call_scratch(const awp::LwInputs &in, int64_t frames, size_t budget, size_t held, ll *out) {
    for (int i = 0; i < 22; ++i) out[i] = 0;
    const awp::LwCallPlan c = awp::lw_choose(in, frames);
    call_to(c, out);
    if (c.n_groups) {
        lw_to(c, awp::lw_plan_scratch(in.layout, c, budget, held), out + 12);
    } else if (in.plan.path == 1) {
        part_to(awp::part_scratch(in.layout, in.plan, frames, budget, held), out + 5);
    }
}
static unsigned have_of(const awp::LwCallPlan &c, unsigned have) {
    for (int g = 0; g < c.n_groups; ++g)
        for (int i = 0; i < awp::kLwRowChoiceCount; ++i)
            if (awp::kLwRowChoices[i] == c.g[g].R) have |= 1u << i;
    return have;
}

extern "C" {

ll sp_stream_chunk(ll budget_elems, ll held_elems, ll per_stream, ll streams, ll cap) {
    return awp::stream_chunk((size_t)budget_elems, (size_t)held_elems, (size_t)per_stream, streams, cap < 0 ? awp::kNoChunkCap : cap);
}
void sp_part_scratch(const int *plan, int channels, int taps, int streams, ll frames, ll budget, ll held, ll *out) {
    part_to(awp::part_scratch(awp::Layout{channels, taps, streams}, plan_of(plan), frames, (size_t)budget, (size_t)held), out);
}
void sp_lw_plan_scratch(int channels, int taps, int streams, const ll *call, ll budget, ll held, ll *out) {
    const awp::LwCallPlan c = call_of(call);
    lw_to(c, awp::lw_plan_scratch(awp::Layout{channels, taps, streams}, c, (size_t)budget, (size_t)held), out);
}
ll sp_default_budget(int known, ll free_bytes) { return (ll)awp::default_budget(known != 0, (size_t)free_bytes); }
ll sp_part_longest_call(const int *plan, int channels, int taps, int streams, int cus, ll max_frames) {
    return awp::part_longest_call(awp::LwInputs{awp::Layout{channels, taps, streams}, plan_of(plan), cus, 0, 0u}, max_frames);
}
// out [2]: need, chunk.  `call`: the reserve plan (lw_choose of the frames asked for, for_reserve).
void sp_reserve_need(const int *plan, int channels, int taps, int streams, int cus, const ll *call, ll reserved_frames, ll budget, ll *out) {
    const awp::LwInputs in{awp::Layout{channels, taps, streams}, plan_of(plan), cus, 0, 0u};
    const awp::ReserveNeed r = awp::reserve_need(in, call_of(call), reserved_frames, (size_t)budget);
    out[0] = (ll)r.need; out[1] = r.chunk;
}
ll sp_host_chunk_streams(int streams, int channels, ll frames, int in_bytes, int host_chunk_mb) {
    return awp::host_chunk_streams(streams, channels, frames, (size_t)in_bytes, host_chunk_mb);
}
ll sp_staged_chunk_streams(int streams, int channels, ll frames, int in_bytes, int host_chunk_mb, ll reserved_frames, ll reserved_chunk) {
    return awp::staged_chunk_streams(streams, channels, frames, (size_t)in_bytes, host_chunk_mb, reserved_frames, reserved_chunk);
}
ll sp_staged_streams(ll chunk, int streams) { return (ll)awp::staged_streams(chunk, streams); }

// The grid of tests/test_scratch_plan_host.py for one layout with the default knobs: for every stream count, budget (bytes) and reserve,
// the reserve — and for every call length (from 1 to the reserve in `steps` steps, then reserve - 1 and reserve) the call on the reserve's
// tables, inside its pool (held = its need) and on a handle that was never reserved (no tables wanted, held = 0).  One record of
// kGridFields per call; returns the records written (at most `capacity`).
//   [0..5]    channels, taps, streams, budget, reserve, frames
//   [6..10]   plan: path, hop, partitions, n_pairs, hist_len
//   [11..15]  the reserve plan (call [5])      [16] part_longest_call      [17] reserve need      [18] reserve chunk
//   [19..40]  the reserved call (call_scratch)   [41..62]  the unreserved call
enum { kGridFields = 63 };
int sp_grid_fields() { return kGridFields; }
ll sp_grid(int channels, int taps, int cus, const int *streams, int n_streams, const ll *budgets, int n_budgets, const ll *reserves, int n_reserves,
           int steps, ll *out, ll capacity) {
    ll n = 0;
    for (int si = 0; si < n_streams; ++si) {
        const awp::Layout l{channels, taps, streams[si]};
        const awp::CreatePlan p = awp::plan_create(l, awp::Knobs{}, awk::ola_rows_carried(channels, taps));
        for (int ri = 0; ri < n_reserves; ++ri) {
            const ll reserve = reserves[ri];
            const awp::LwInputs fresh{l, p, cus, 0, 0u};
            const awp::LwCallPlan res = awp::lw_choose(fresh, reserve, true);
            const awp::LwInputs reserved{l, p, cus, reserve, have_of(res, 0u)};
            const ll longest = awp::part_longest_call(fresh, reserve);
            for (int bi = 0; bi < n_budgets; ++bi) {
                const size_t budget = (size_t)budgets[bi];
                const awp::ReserveNeed need = awp::reserve_need(fresh, res, reserve, budget);
                for (int k = 0; k <= steps + 1; ++k) {
                    const ll frames = k < steps ? 1 + (reserve - 1) * k / steps : k == steps ? reserve - 1 : reserve;
                    if (frames < 1 || n >= capacity) continue;
                    ll *r = out + n++ * kGridFields;
                    const ll head[11] = {channels, taps, l.streams, (ll)budget, reserve, frames, p.path, p.hop, p.partitions, p.n_pairs, p.hist_len};
                    for (int i = 0; i < 11; ++i) r[i] = head[i];
                    call_to(res, r + 11);
                    r[16] = longest; r[17] = (ll)need.need; r[18] = need.chunk;
                    call_scratch(reserved, frames, budget, need.need, r + 19);
                    call_scratch(fresh, frames, budget, 0, r + 41);
                }
            }
        }
    }
    return n;
}

}  // extern "C"
