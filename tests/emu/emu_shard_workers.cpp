// TEST-ONLY: a stand-alone program over airwave_amd/csrc/host/shard_workers.hpp (tests/test_shard_plan_host.py builds it with a thread
// sanitizer and runs it as a plain process).  It checks what aw_multi relies on:
//   - every worker runs every job exactly once, with its own shard index;
//   - run() returns the status and the message of the LOWEST-index failing shard, 0 when none failed, the thrown status for a job that throws;
//   - no job runs outside run(): each job looks at a flag the driver holds up only around run(), and the counts are final once the
//     workers are destroyed;
//   - workers can be created and destroyed in a loop, used or not.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../airwave_amd/csrc/host/shard_workers.hpp"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (++failures < 20) std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                     \
    } while (0)

struct Job {
    std::atomic<bool> *inside;              // true only while the driver is inside run()
    std::atomic<long> *outside_calls;       // jobs that ran while it was false
    std::vector<long> *calls;               // per shard index (each worker writes its own element; the driver reads after run())
    int fail_a, fail_b, throw_at;           // shard indices that fail (status 100 + shard) or throw; -1: none
    int operator()(int shard, char *message, size_t capacity) {
        if (!inside->load()) outside_calls->fetch_add(1);
        (*calls)[(size_t)shard] += 1;
        if (shard == throw_at) throw std::runtime_error("thrown on purpose");
        if (shard == fail_a || shard == fail_b) {
            std::snprintf(message, capacity, "shard %d failed on purpose", shard);
            return 100 + shard;
        }
        return 0;
    }
};

int main() {
    constexpr int kThrown = 77;
    std::atomic<bool> inside{false};
    std::atomic<long> outside_calls{0};
    long rounds_total = 0;
    unsigned rng = 12345u;
    auto next = [&rng](unsigned n) { rng = rng * 1664525u + 1013904223u; return (rng >> 8) % n; };
    for (int n = 1; n <= 8; ++n) {
        std::vector<int> shards;
        for (int i = 0; i < n; ++i) shards.push_back(2 * i + 1);          // shard indices with gaps: empty shards have no worker
        std::vector<long> calls(2 * (size_t)n + 1, 0);
        const int rounds = 500;
        {
            awsh::Workers w(shards, kThrown);
            EXPECT(w.size() == (size_t)n);
            for (int r = 0; r < rounds; ++r) {
                Job job{&inside, &outside_calls, &calls, -1, -1, -1};
                const unsigned kind = next(4);
                if (kind >= 1) job.fail_a = shards[next((unsigned)n)];                    // one deliberately failing shard
                if (kind == 2) job.fail_b = shards[next((unsigned)n)];                    // sometimes a second: the lowest index is reported
                if (kind == 3 && next(4) == 0) { job.throw_at = job.fail_a; job.fail_a = -1; }
                inside.store(true);
                const awsh::Workers::Result res = w.run(job);
                inside.store(false);
                int lowest = -1;
                for (int s : shards)
                    if (lowest < 0 && (s == job.fail_a || s == job.fail_b || s == job.throw_at)) lowest = s;
                if (lowest < 0) {
                    EXPECT(res.status == 0 && res.shard == -1 && res.message[0] == 0);
                } else if (lowest == job.throw_at) {
                    EXPECT(res.status == kThrown && res.shard == lowest && std::strstr(res.message, "exception") != nullptr);
                } else {
                    char want[64];
                    std::snprintf(want, sizeof want, "shard %d failed on purpose", lowest);
                    EXPECT(res.status == 100 + lowest && res.shard == lowest && std::strcmp(res.message, want) == 0);
                }
                for (int s : shards) EXPECT(calls[(size_t)s] == r + 1);                  // every worker, exactly once, before run() returned
            }
            rounds_total += rounds;
        }
        for (size_t s = 0; s < calls.size(); ++s) EXPECT(calls[s] == ((s & 1) ? rounds : 0));      // final after the workers are gone
    }
    for (int k = 0; k < 300; ++k) {          // create / destroy in a loop, with and without a job in between
        const int n = 1 + (int)next(8);
        std::vector<int> shards;
        for (int i = 0; i < n; ++i) shards.push_back(i);
        std::vector<long> calls((size_t)n, 0);
        awsh::Workers w(shards, kThrown);
        for (unsigned r = next(3); r > 0; --r) {
            Job job{&inside, &outside_calls, &calls, n - 1, -1, -1};
            inside.store(true);
            const awsh::Workers::Result res = w.run(job);
            inside.store(false);
            EXPECT(res.status == 100 + n - 1 && res.shard == n - 1);
            ++rounds_total;
        }
    }
    { awsh::Workers none(std::vector<int>{}, kThrown); Job job{&inside, &outside_calls, nullptr, -1, -1, -1}; EXPECT(none.run(job).status == 0); }
    EXPECT(outside_calls.load() == 0);
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok: %ld rounds\n", rounds_total);
    return 0;
}
