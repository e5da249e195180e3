// device_buf_check.cpp — airwave_amd/csrc/host/device_buf.hpp (the real header) over tests/harness/hip_stub, built with the host
// sanitizers and run by tests/test_device_buf_host.py: what awr::Buf and awr::Event call, in which order, and that nothing stays live.
// Prints every mismatch and exits non-zero if there was one; LeakSanitizer reports what the live counts would miss.
#include <cstdio>
#include <vector>

#include "host/device_buf.hpp"

using awr::Buf;
using awr::Counter;
using awr::Event;
using awr::Kind;
namespace st = hip_stub;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)
static std::string calls() { std::string l; l.swap(st::log); return l; }          // the calls since the last look

static void grow_and_alloc() {
    Counter n{0};
    {
        Buf<float> b;
        CHECK(!b && b.get() == nullptr && b.capacity() == 0 && b.bytes() == 0);
        CHECK(b.grow(8, &n) == hipSuccess && calls() == "m" && n == 1);
        CHECK(b && b.capacity() == 8 && b.bytes() == 32 && st::live[0] == 1);
        float *const p = b.get();
        CHECK(b.grow(8, &n) == hipSuccess && b.grow(3, &n) == hipSuccess && b.grow(0, &n) == hipSuccess);          // below capacity: no call
        CHECK(calls() == "" && n == 1 && b.get() == p && b.capacity() == 8);
        CHECK(b.grow(9, &n) == hipSuccess && calls() == "fm" && n == 2 && b.capacity() == 9 && st::live[0] == 1);  // free, THEN allocate
        CHECK(b.grow(20, nullptr) == hipSuccess && calls() == "fm" && n == 2 && b.capacity() == 20);               // not counted
        st::fail_at = 1;
        CHECK(b.grow(100, &n) == hipErrorOutOfMemory && calls() == "fm");                                           // a failed growth:
        CHECK(!b && b.get() == nullptr && b.capacity() == 0 && b.bytes() == 0 && n == 2 && st::live[0] == 0);       // empty, not counted
        CHECK(b.grow(4, &n) == hipSuccess && calls() == "m" && n == 3 && b.capacity() == 4);                        // and usable again
        CHECK(b.alloc(2, &n) == hipSuccess && calls() == "fm" && n == 4 && b.capacity() == 2);                      // exact size, also downwards
        st::fail_at = 1;
        CHECK(b.alloc(2, &n) == hipErrorOutOfMemory && !b && b.capacity() == 0 && n == 4);
        calls();
        CHECK(b.reset() == hipSuccess && b.reset() == hipSuccess && calls() == "");                                 // nothing held: no call
        CHECK(b.alloc(5, &n) == hipSuccess && b.reset() == hipSuccess && b.reset() == hipSuccess && calls() == "mf" && !b && b.capacity() == 0);
        CHECK(b.alloc(6, &n) == hipSuccess && calls() == "m");
    }
    CHECK(calls() == "f" && st::live[0] == 0);          // the destructor
}

static void *freed_block = nullptr, *held_at_free = nullptr;
static Buf<int> *watched = nullptr;
static void moves() {
    {
        Buf<int> x;
        CHECK(x.alloc(4, nullptr) == hipSuccess);
        int *const p = x.get();
        Buf<int> y(std::move(x));
        CHECK(!x && x.capacity() == 0 && y.get() == p && y.capacity() == 4 && calls() == "m");
    }
    CHECK(calls() == "f" && st::live[0] == 0);          // freed once, by the one that holds it
    {
        Buf<int> a, b;
        CHECK(a.alloc(4, nullptr) == hipSuccess && b.alloc(7, nullptr) == hipSuccess && calls() == "mm");
        int *const pa = a.get(), *const pb = b.get();
        watched = &a;
        st::on_free = [](void *p) { freed_block = p; held_at_free = watched->get(); };
        a = std::move(b);
        st::on_free = nullptr;
        CHECK(calls() == "f" && st::live[0] == 1 && a.get() == pb && a.capacity() == 7 && !b && b.capacity() == 0);
        CHECK(freed_block == pa && held_at_free == pb);          // the old block went AFTER the new one was taken
        Buf<int> &same = a;
        a = std::move(same);
        CHECK(calls() == "" && a.get() == pb && a.capacity() == 7);
        a = Buf<int>();                                           // an empty right side drops what the left held
        CHECK(calls() == "f" && !a && st::live[0] == 0);
    }
    CHECK(calls() == "" && st::live[0] == 0);
}

static void pinned_kind() {
    Counter n{0};
    {
        Buf<double, Kind::pinned> h;
        CHECK(h.grow(3, &n) == hipSuccess && calls() == "M" && st::live[1] == 1 && st::live[0] == 0 && h.bytes() == 24);
        CHECK(h.grow(4, &n) == hipSuccess && calls() == "FM" && n == 2);
        Buf<double, Kind::pinned> g(std::move(h));
        CHECK(g.reset() == hipSuccess && calls() == "F" && st::live[1] == 0);
        CHECK(g.alloc(1, &n) == hipSuccess && calls() == "M");
    }
    CHECK(calls() == "F" && st::live[1] == 0 && st::wrong_kind == 0);
}

static void uploads() {
    Counter allocs{0}, copies{0};
    const int src[3] = {5, 6, 7};
    Buf<int> b;
    CHECK(b.upload(src, 3, &allocs, &copies) == hipSuccess && calls() == "mc" && allocs == 1 && copies == 1);
    CHECK(b.capacity() == 3 && b.get()[0] == 5 && b.get()[2] == 7);
    CHECK(b.upload(src, 2, nullptr, nullptr) == hipSuccess && calls() == "fmc" && allocs == 1 && copies == 1 && b.capacity() == 2);
    st::fail_copy = true;          // a buffer that was never written does not stay behind; both counters have moved, as the calls were made
    CHECK(b.upload(src, 3, &allocs, &copies) == hipErrorUnknown && calls() == "fmcf" && !b && allocs == 2 && copies == 2 && st::live[0] == 0);
    st::fail_at = 1;
    CHECK(b.upload(src, 3, &allocs, &copies) == hipErrorOutOfMemory && calls() == "m" && !b && allocs == 2 && copies == 2);
}

// aw_spatializer::LwPlan's shape: eight buffers built in a chain that stops at the first failure; a half-built one just goes out of scope
struct Plan { int R = 0; Buf<long> tab; Buf<double> tab16; Buf<float> tw2, coarse, fine, step, tw_r, tw1m; };
static hipError_t build(Plan &p, Counter *n) {
    hipError_t e = p.tab.alloc(3, n);
    if (e == hipSuccess) e = p.tab16.alloc(5, n);
    for (Buf<float> *b : {&p.tw2, &p.coarse, &p.fine, &p.step, &p.tw_r, &p.tw1m})
        if (e == hipSuccess) e = b->alloc(7, n);
    return e;
}
static void aggregate() {
    for (int k = 1; k <= 8; ++k) {
        Counter n{0};
        st::fail_at = k;
        {
            Plan p;
            CHECK(build(p, &n) == hipErrorOutOfMemory && n == k - 1 && st::live[0] == k - 1);
        }
        CHECK(st::live[0] == 0 && st::fail_at == 0);
    }
    {
        std::vector<Plan> plans;
        plans.reserve(2);
        Counter n{0};
        Plan p;
        p.R = 32;
        CHECK(build(p, &n) == hipSuccess && n == 8);
        float *const tw2 = p.tw2.get();
        plans.push_back(std::move(p));
        CHECK(st::live[0] == 8 && plans.back().R == 32 && plans.back().tw2.get() == tw2 && !p.tab && !p.tw1m);
        calls();
    }
    CHECK(calls() == "ffffffff" && st::live[0] == 0);
}

static void events() {
    {
        Event a, b;
        CHECK(!a && a.get() == nullptr);
        CHECK(a.create() == hipSuccess && b.create(hipEventDisableTiming) == hipSuccess && a && b && st::events == 2 && calls() == "ee");
        hipEvent_t const h = a.get();
        Event c(std::move(a));
        CHECK(!a && c.get() == h && st::events == 2);
    }
    CHECK(calls() == "EE" && st::events == 0);          // each destroyed exactly once (a second time is a double free under the sanitizer)
}

int main() {
    grow_and_alloc();
    moves();
    pinned_kind();
    uploads();
    aggregate();
    events();
    CHECK(st::live[0] == 0 && st::live[1] == 0 && st::events == 0 && st::wrong_kind == 0 && st::log.empty());
    std::printf(failures ? "device_buf_check: %d mismatches\n" : "device_buf_check: ok\n", failures);
    return failures ? 1 : 0;
}
