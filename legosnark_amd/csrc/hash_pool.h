// legosnark_amd/csrc/hash_pool.h -- the CRS cache's hashing threads (crs_cache.hip).  Host code only, no HIP:
// tests/cpp/test_crs_index.cc runs it under the address, undefined-behaviour and thread sanitizers.
#pragma once
#include <stdlib.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#include "crs_index.h"

namespace lsa {

// persistent workers hashing the chunks of one vector; the caller thread joins in at finish()
class HashPool {
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, cv_done_;
    const uint8_t *base_ = nullptr;
    size_t unit_bytes_ = 0, units_per_task_ = 1, total_bytes_ = 0, nunits_ = 0, ntasks_ = 0;
    uint64_t *out_ = nullptr;
    std::atomic<size_t> next_{0};
    size_t active_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;

    void work() {
        for (;;) {
            size_t t = next_.fetch_add(1);
            if (t >= ntasks_) break;
            size_t u1 = (t + 1) * units_per_task_ < nunits_ ? (t + 1) * units_per_task_ : nunits_;
            for (size_t u = t * units_per_task_; u < u1; u++) {
                size_t lo = u * unit_bytes_, hi = lo + unit_bytes_ < total_bytes_ ? lo + unit_bytes_ : total_bytes_;
                out_[u] = hash_words(reinterpret_cast<const uint64_t *>(base_ + lo), (hi - lo) / 8);   // never past total_bytes_
            }
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
            }
            work();
            {
                std::lock_guard<std::mutex> lk(m_);
                if (--active_ == 0) cv_done_.notify_all();
            }
        }
    }

  public:
    ~HashPool() { stop(); }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) if (t.joinable()) t.join();
        th_.clear();
        // back to the initial state: workers started later begin with seen = 0 and must find gen_ = 0, or each
        // would take a phantom first generation and decrement active_ once too often (lsa_shutdown -> lsa_init)
        std::lock_guard<std::mutex> lk(m_);
        stop_ = false;
        gen_ = 0;
        active_ = 0;
    }
    // starts hashing `bytes` bytes (a multiple of 8) in units of unit_bytes (the last one may be
    // short); out: one u64 per unit; a task = units_per_task consecutive units
    void begin(const void *p, size_t bytes, size_t unit_bytes, size_t units_per_task, uint64_t *out) {
        base_ = (const uint8_t *)p; total_bytes_ = bytes; unit_bytes_ = unit_bytes; units_per_task_ = units_per_task; out_ = out;
        nunits_ = (bytes + unit_bytes - 1) / unit_bytes;
        ntasks_ = (nunits_ + units_per_task - 1) / units_per_task;
        next_.store(0);
        if (ntasks_ < 8) return;                     // small: the caller does it alone in finish()
        {
            // workers are spawned inside the block that publishes the generation: none can observe a
            // half-initialised pool
            std::lock_guard<std::mutex> lk(m_);
            if (th_.empty()) {
                unsigned hw = std::thread::hardware_concurrency();
                const char *e = getenv("LSA_HASH_THREADS");
                unsigned want = e ? (unsigned)atoi(e) : (hw > 16 ? 15 : (hw > 1 ? hw - 1 : 0));
                for (unsigned i = 0; i < want; i++) th_.emplace_back([this] { loop(); });
            }
            if (th_.empty()) return;
            active_ = th_.size();
            gen_++;
        }
        cv_.notify_all();
    }
    void finish() {
        work();
        std::unique_lock<std::mutex> lk(m_);
        cv_done_.wait(lk, [&] { return active_ == 0; });
    }
};

}  // namespace lsa
