// test_worker_queue.cpp — the launch thread's queue handshake (csrc/ec_worker.hpp) on its own: no HIP, nothing from the
// library, so it runs under a thread sanitizer (make test_worker_queue_tsan).
//
//   1. order and completeness: one posting thread feeds four workers 50,000 jobs each, with pauses of none / 20 µs / 200 µs
//      between posts (kWorkerSpin is 60 µs: every worker is caught polling and asleep many times); every job ran exactly once,
//      in posting order per worker.
//   2. drain on stop: a stop issued while jobs are still queued runs them all before the thread returns.
//   3. Latch(4) releases its waiter only after the fourth arrive.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "ec_worker.hpp"

using ecd::Latch;
using ecd::Worker;

static int g_failures = 0;
#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            ++g_failures;                   \
            std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");     \
        }                                   \
    } while (0)

static void start(Worker& w) { w.th = std::thread([&w] { w.run(); }); }

static void pause_for(std::chrono::microseconds us) {  // busy: a sleep of 20 µs would last far longer
    const auto until = std::chrono::steady_clock::now() + us;
    while (std::chrono::steady_clock::now() < until) __builtin_ia32_pause();
}

static void order_and_completeness() {
    constexpr int kWorkers = 4, kJobs = 50000;
    Worker w[kWorkers];
    std::vector<int> ran[kWorkers];  // ran[i] is written by worker i alone, read after its join
    for (int i = 0; i < kWorkers; ++i) {
        ran[i].reserve(kJobs);
        start(w[i]);
    }
    std::thread poster([&] {
        uint64_t x = 0x9E3779B97F4A7C15ull;  // xorshift: the pause before each round of posts
        for (int seq = 0; seq < kJobs; ++seq) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const unsigned r = static_cast<unsigned>(x >> 33) % 100;  // 200 µs 1 %, 20 µs 9 %, none 90 %
            if (r == 0) pause_for(std::chrono::microseconds(200));
            else if (r < 10) pause_for(std::chrono::microseconds(20));
            for (int i = 0; i < kWorkers; ++i) w[i].post([&ran, i, seq] { ran[i].push_back(seq); });
        }
    });
    poster.join();
    for (int i = 0; i < kWorkers; ++i) w[i].stop_and_join();
    for (int i = 0; i < kWorkers; ++i) {
        CHECK(ran[i].size() == size_t(kJobs), "worker %d ran %zu of %d jobs", i, ran[i].size(), kJobs);
        size_t bad = 0;
        for (size_t k = 0; k < ran[i].size(); ++k) bad += ran[i][k] != int(k);
        CHECK(bad == 0, "worker %d: %zu jobs out of posting order (or run twice)", i, bad);
        CHECK(w[i].pending.load() == 0 && w[i].q.empty(), "worker %d: queue not empty after stop", i);
    }
}

static void drain_on_stop() {
    constexpr int kJobs = 2000;
    Worker w;
    std::atomic<bool> held{false}, go{false};
    int ran = 0;  // the worker's alone until the join
    start(w);
    w.post([&] {  // holds the worker: the rest queue up
        held.store(true, std::memory_order_release);
        while (!go.load(std::memory_order_acquire)) __builtin_ia32_pause();
    });
    while (!held.load(std::memory_order_acquire)) __builtin_ia32_pause();
    for (int k = 0; k < kJobs; ++k) w.post([&ran] { ++ran; });
    std::thread stopper([&] { w.stop_and_join(); });
    while (true) {  // release the worker only once the stop has been requested, with the queue still full
        std::lock_guard<std::mutex> lk(w.mu);
        if (w.stop) break;
    }
    CHECK(w.pending.load() == kJobs, "%d jobs queued at the stop, expected %d", w.pending.load(), kJobs);
    go.store(true, std::memory_order_release);
    stopper.join();
    CHECK(ran == kJobs, "a stop with %d jobs queued ran %d of them", kJobs, ran);
}

static void latch_waits_for_all() {
    Latch latch(4);
    std::atomic<int> arrived{0};
    std::atomic<int> seen_at_release{-1};
    std::thread waiter([&] {
        latch.wait();
        seen_at_release.store(arrived.load());
    });
    for (int k = 1; k <= 4; ++k) {
        if (k == 4) {  // three arrivals are in: the waiter must still be waiting
            pause_for(std::chrono::microseconds(2000));
            CHECK(seen_at_release.load() == -1, "Latch(4) released its waiter after %d arrivals", seen_at_release.load());
        }
        arrived.fetch_add(1);
        latch.arrive();
    }
    waiter.join();
    CHECK(seen_at_release.load() == 4, "the waiter saw %d arrivals at its release", seen_at_release.load());
}

int main() {
    order_and_completeness();
    drain_on_stop();
    latch_waits_for_all();
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::puts("worker queue: all checks passed");
    return 0;
}
