// cycle_pool.h -- the worker threads of env_cycle_many (runtime_api.hip).  No HIP in here: tests/native/pool_tsan.cc includes this
// header alone and runs the class under ThreadSanitizer.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace magent_amd {

// Worker threads of env_cycle_many: started once, parked on a condition variable between rounds (creating threads
// per call cost more than a small world's whole step).  One round at a time (rounds are serialised by `round_mutex`).
class CyclePool {
public:
    void run(int n_threads, int n_items, const std::function<void(int)> &fn) {
        std::lock_guard<std::mutex> round(round_mutex);
        {
            std::unique_lock<std::mutex> lk(m);
            while ((int)workers.size() < n_threads - 1) workers.emplace_back([this] { loop(); });
            job = &fn; total = n_items; next = 0; pending = std::min(n_threads - 1, (int)workers.size()); active = pending; epoch++;
            ran.store(0, std::memory_order_relaxed);
        }
        cv.notify_all();
        int mine = 0;
        for (int e; (e = next.fetch_add(1)) < n_items; mine++) fn(e);     // the calling thread works too
        count(mine, false);
        std::unique_lock<std::mutex> lk(m);
        done_cv.wait(lk, [this] { return pending == 0; });
        job = nullptr;
        n_rounds.fetch_add(1, std::memory_order_relaxed);
        const long long threads = ran.load(std::memory_order_relaxed);
        if (threads > most_threads.load(std::memory_order_relaxed)) most_threads.store(threads, std::memory_order_relaxed);
    }
    // env_cycle_pool_stats (include/magent_runtime_api.h): rounds, items, items run by workers, most threads that ran an item in one round
    void stats(long long out[4]) const {
        out[0] = n_rounds.load(std::memory_order_relaxed); out[1] = n_items_run.load(std::memory_order_relaxed);
        out[2] = n_worker_items.load(std::memory_order_relaxed); out[3] = most_threads.load(std::memory_order_relaxed);
    }
    ~CyclePool() {
        { std::unique_lock<std::mutex> lk(m); quit = true; }
        cv.notify_all();
        for (auto &t : workers) t.join();
    }
private:
    void loop() {
        unsigned seen = 0;
        std::unique_lock<std::mutex> lk(m);
        while (true) {
            cv.wait(lk, [&] { return quit || (epoch != seen && active > 0); });
            if (quit) return;
            seen = epoch; active--;
            const std::function<void(int)> *fn = job;
            const int n = total;
            lk.unlock();
            int mine = 0;
            for (int e; (e = next.fetch_add(1)) < n; mine++) (*fn)(e);
            count(mine, true);
            lk.lock();
            if (--pending == 0) done_cv.notify_one();
        }
    }
    void count(int mine, bool worker) {       // (counters only: nothing reads them but stats())
        if (mine == 0) return;
        n_items_run.fetch_add(mine, std::memory_order_relaxed);
        if (worker) n_worker_items.fetch_add(mine, std::memory_order_relaxed);
        ran.fetch_add(1, std::memory_order_relaxed);
    }
    std::mutex m, round_mutex;
    std::condition_variable cv, done_cv;
    std::vector<std::thread> workers;
    const std::function<void(int)> *job = nullptr;
    std::atomic<int> next{0};
    int total = 0, pending = 0, active = 0;
    unsigned epoch = 0;
    bool quit = false;
    std::atomic<long long> n_rounds{0}, n_items_run{0}, n_worker_items{0}, most_threads{0}, ran{0};
};

}  // namespace magent_amd
