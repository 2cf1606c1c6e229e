// ec_worker.hpp — the launch thread's job queue and the latch of the shard group (ec_sharded.hip), in plain C++: nothing from
// HIP or from this library, so that host/test_worker_queue.cpp can run the handshake alone under a thread sanitizer.
//
// The protocol: a push happens under `mu`, and `pending` is counted under `mu`.  A worker that has just run a job polls `pending`
// for kWorkerSpin without the lock, then takes `mu`; it sets `sleeping` under `mu` only after finding the queue empty.  `post`
// notifies only if `sleeping`: a job pushed before the flag was set is found by the worker's own look at the queue, one pushed
// after it sees the flag.  A stop drains the queue before `run` returns.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>

namespace ecd {

// How long a launch thread polls its queue after a job before it goes to sleep on the condition variable.
constexpr auto kWorkerSpin = std::chrono::microseconds(60);

struct Worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::function<void()>> q;
    std::atomic<int> pending{0};      // jobs in q (read by the polling worker without the lock)
    std::atomic<bool> sleeping{false};
    bool stop = false;

    void run() {
        for (;;) {
            std::function<void()> job;
            if (pending.load(std::memory_order_acquire) == 0) {  // poll, then sleep
                const auto until = std::chrono::steady_clock::now() + kWorkerSpin;
                while (pending.load(std::memory_order_acquire) == 0 && std::chrono::steady_clock::now() < until) __builtin_ia32_pause();
            }
            {
                std::unique_lock<std::mutex> lk(mu);
                if (q.empty()) {
                    sleeping.store(true, std::memory_order_release);
                    cv.wait(lk, [&] { return stop || !q.empty(); });
                    sleeping.store(false, std::memory_order_release);
                    if (q.empty()) return;  // stop requested and drained
                }
                job = std::move(q.front());
                q.pop_front();
                pending.fetch_sub(1, std::memory_order_acq_rel);
            }
            job();
        }
    }
    void post(std::function<void()> job) {
        {
            std::lock_guard<std::mutex> lk(mu);
            q.push_back(std::move(job));
            pending.fetch_add(1, std::memory_order_acq_rel);
        }
        if (sleeping.load(std::memory_order_acquire)) cv.notify_one();  // a polling worker sees `pending`
    }
    // no more posts: the thread runs what is queued and returns
    void stop_and_join() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_one();
        if (th.joinable()) th.join();
    }
};

struct Latch {
    std::mutex mu;
    std::condition_variable cv;
    int left;
    explicit Latch(int n) : left(n) {}
    void arrive() {
        std::lock_guard<std::mutex> lk(mu);
        if (--left == 0) cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return left == 0; });
    }
};

}  // namespace ecd
