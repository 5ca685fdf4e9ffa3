// pool_tsan.cc -- a stand-alone program (tests/test_cycle_threads.py builds it with -fsanitize=thread and runs it): the host-thread pool
// of env_cycle_many (magent_amd/csrc/cycle_pool.h) and tune() (magent_amd/csrc/tune.h) under contention.  No HIP, no engine.
//   pool : 3,000 rounds per caller, n_threads cycling through 1..9, item counts through 0, 1, 2, 7, 40; every round's fn counts
//          hits[round][item] (plain ints: a pool that lets a round's items overlap its return is a data race ThreadSanitizer reports, and
//          one that runs an item twice or never a wrong count), notes which threads ran an item, and after run() every item of the round
//          must have been run exactly once by at most n_threads threads.  Two callers do this on ONE pool at once; then one phase grows
//          the pool to 8 workers and calls it with 2.
//   tune : MAGENT_TUNE=pipe_own=3,render=1,batch_cycle=0; eight threads released together, each asks for a key of its own 1,000 times.
// Exit code 0: everything held (ThreadSanitizer's own reports end the process with the exit code TSAN_OPTIONS names).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "cycle_pool.h"
#include "tune.h"

static std::atomic<int> failures{0};
#define CHECK(cond, ...) do { if (!(cond) && failures.fetch_add(1) < 20) { char msg[256]; std::snprintf(msg, sizeof msg, __VA_ARGS__); std::fprintf(stderr, "pool_tsan: %s\n", msg); } } while (0)

static const int ITEMS[5] = {0, 1, 2, 7, 40};

// rounds [0, n_rounds) of one caller on `pool`; n_threads_of(r) threads asked for in round r
template <class F> static void caller(magent_amd::CyclePool &pool, const char *who, int n_rounds, F n_threads_of) {
    std::vector<std::vector<int>> hits(n_rounds);
    for (int r = 0; r < n_rounds; r++) {
        const int n_items = ITEMS[r % 5], n_threads = n_threads_of(r);
        std::vector<int> &h = hits[r];
        h.assign(n_items, 0);
        std::mutex ids_lock;
        std::set<std::thread::id> ids;
        pool.run(n_threads, n_items, [&](int e) {
            h[e]++;
            std::lock_guard<std::mutex> g(ids_lock);
            ids.insert(std::this_thread::get_id());
        });
        for (int e = 0; e < n_items; e++)
            CHECK(h[e] == 1, "%s round %d (n_threads %d, %d items): item %d was run %d times", who, r, n_threads, n_items, e, h[e]);
        CHECK((int)ids.size() <= (n_threads < 1 ? 1 : n_threads), "%s round %d: %d threads ran items, %d were asked for", who, r, (int)ids.size(), n_threads);
    }
    // (a round that went on behind its run(): every count once more, after all rounds)
    for (int r = 0; r < n_rounds; r++)
        for (int e = 0; e < (int)hits[r].size(); e++) CHECK(hits[r][e] == 1, "%s round %d: item %d counted %d at the end", who, r, e, hits[r][e]);
}

static void spin_barrier(std::atomic<int> &arrived, int n) {
    arrived.fetch_add(1);
    while (arrived.load() < n) std::this_thread::yield();
}

int main() {
    // ---- the pool: two callers at once, n_threads 1..9
    {
        magent_amd::CyclePool pool;
        long long before[4], after[4];
        pool.stats(before);
        std::atomic<int> arrived{0};
        std::thread second([&] { spin_barrier(arrived, 2); caller(pool, "second caller", 3000, [](int r) { return 9 - r % 9; }); });
        spin_barrier(arrived, 2);
        caller(pool, "first caller", 3000, [](int r) { return 1 + r % 9; });
        second.join();
        pool.stats(after);
        long long items = 0;
        for (int r = 0; r < 3000; r++) items += 2 * ITEMS[r % 5];
        CHECK(after[0] - before[0] == 6000, "stats: %lld rounds counted, 6000 run", after[0] - before[0]);
        CHECK(after[1] - before[1] == items, "stats: %lld items counted, %lld run", after[1] - before[1], items);
        CHECK(after[2] <= after[1] && after[3] <= 9, "stats: %lld of %lld items by workers, %lld threads in one round", after[2], after[1], after[3]);
    }
    // ---- a pool grown to 8 workers, then asked for 2 (and 1, and 4): never more threads than asked for
    {
        magent_amd::CyclePool pool;
        caller(pool, "growing", 50, [](int) { return 9; });
        caller(pool, "grown, asked for 2", 500, [](int) { return 2; });
        static const int widths[6] = {1, 4, 2, 9, 3, 2};
        caller(pool, "grown, changing", 600, [](int r) { return widths[r % 6]; });
    }
    // ---- tune() from eight threads at once, each on its own key
    {
        setenv("MAGENT_TUNE", "pipe_own=3,render=1,batch_cycle=0", 1);
        static const struct { const char *key; int dflt, want; } K[8] = {
            {"pipe_own", 48, 3}, {"render", -1, 1}, {"batch_cycle", 1, 0}, {"batch_pipe", 1, 1},
            {"attack_pairs", 7, 7}, {"host_shuffle", 0, 0}, {"pipe_sweep", -1, -1}, {"solo_max", 1536, 1536}};
        std::atomic<int> arrived{0};
        std::vector<std::thread> T;
        for (int t = 0; t < 8; t++)
            T.emplace_back([&, t] {
                spin_barrier(arrived, 8);
                for (int k = 0; k < 1000; k++) {
                    const int got = magent_amd::tune(K[t].key, K[t].dflt);
                    CHECK(got == K[t].want, "tune(\"%s\", %d) returned %d in thread %d, call %d: %d expected", K[t].key, K[t].dflt, got, t, k, K[t].want);
                }
            });
        for (auto &t : T) t.join();
    }
    if (failures.load()) { std::fprintf(stderr, "pool_tsan: %d checks failed\n", failures.load()); return 1; }
    std::printf("pool_tsan ok\n");
    return 0;
}
