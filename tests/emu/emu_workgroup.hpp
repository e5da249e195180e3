#pragma once
// emu_workgroup.hpp — TEST-ONLY: the workgroup runner of the CPU emulation, the only place that starts threads.  A call site builds its
// execution context (emu_ctx.hpp, emu_stage_ctx.hpp) from `t` and loops over its grid around the call.
#include <thread>
#include <vector>

namespace {

// one emulated workgroup: fn(t) for t in [0, threads) on a std::thread each, joined before the return
template <class Fn> void emu_workgroup(int threads, Fn &&fn) {
    std::vector<std::thread> th;
    th.reserve((size_t)threads);
    for (int t = 0; t < threads; ++t) th.emplace_back([&fn, t]() { fn(t); });
    for (auto &x : th) x.join();
}

}  // namespace
