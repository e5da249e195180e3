// shard_workers.hpp — the threads of a multi-device handle (aw_multi, multi_runtime.cpp): one persistent thread per non-empty shard,
// started when the handle is created and parked on a condition variable between calls.  Pure host code with no device call, so
// tests/emu/emu_shard_workers.cpp runs it under a thread sanitizer as a plain program.
//
//   run(job)  hands the same callable to every worker with that worker's shard index and returns when ALL of them have finished, also
//             when one fails: no job is running once run() has returned.  The result is the status of the lowest-index failing shard
//             with the text that worker left, or {0, -1, ""}.  run() allocates nothing: the job is passed by address, every worker writes
//             its message into a buffer it owns.
//   job       int job(int shard, char *message, size_t capacity): 0 = ok; otherwise it leaves a NUL-terminated text in message.  A job
//             that throws counts as failed with the status given to the constructor.
// One caller at a time (the handle is single-owner, like every handle of the library).
#pragma once
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace awsh {

class Workers {
  public:
    static constexpr size_t kMessage = 512;
    struct Result { int status; int shard; const char *message; };      // message: the failing worker's buffer, valid until the next run()

    // one worker per entry of `shards` (the shard index it reports); throws what std::thread throws, after joining the threads it started
    Workers(const std::vector<int> &shards, int thrown_status) : slots_(shards.size()), thrown_status_(thrown_status) {
        for (size_t i = 0; i < slots_.size(); ++i) slots_[i].shard = shards[i];
        try {
            for (Slot &s : slots_) s.thread = std::thread([this, &s] { loop(s); });
        } catch (...) {
            shutdown();
            throw;
        }
    }
    ~Workers() { shutdown(); }
    Workers(const Workers &) = delete;
    Workers &operator=(const Workers &) = delete;
    size_t size() const { return slots_.size(); }

    template <class Job> Result run(Job &job) {
        std::unique_lock<std::mutex> lk(m_);
        job_ = &job;
        call_ = [](void *j, int shard, char *msg, size_t cap) { return (*static_cast<Job *>(j))(shard, msg, cap); };
        pending_ = (int)slots_.size();
        ++generation_;
        cv_work_.notify_all();
        cv_done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
        for (const Slot &s : slots_)          // (slots are in shard order)
            if (s.status != 0) return Result{s.status, s.shard, s.message};
        return Result{0, -1, ""};
    }

  private:
    struct Slot {
        std::thread thread;
        int shard = 0, status = 0;
        char message[kMessage] = {0};
    };
    void loop(Slot &s) {
        unsigned long long seen = 0;
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
            cv_work_.wait(lk, [&] { return stop_ || generation_ != seen; });
            if (stop_) return;
            seen = generation_;
            void *job = job_;
            int (*call)(void *, int, char *, size_t) = call_;
            lk.unlock();
            int status;
            s.message[0] = 0;
            try {
                status = call(job, s.shard, s.message, kMessage);
            } catch (...) {
                status = thrown_status_;
                std::strncpy(s.message, "exception in a shard worker", kMessage - 1);
            }
            s.message[kMessage - 1] = 0;
            lk.lock();
            s.status = status;
            if (--pending_ == 0) cv_done_.notify_one();
        }
    }
    void shutdown() {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_work_.notify_all();
        for (Slot &s : slots_) if (s.thread.joinable()) s.thread.join();
    }

    std::vector<Slot> slots_;          // sized once: the workers hold references into it
    const int thrown_status_;
    std::mutex m_;
    std::condition_variable cv_work_, cv_done_;
    void *job_ = nullptr;
    int (*call_)(void *, int, char *, size_t) = nullptr;
    unsigned long long generation_ = 0;
    int pending_ = 0;
    bool stop_ = false;
};

}  // namespace awsh
