// Stand-alone program (CPU only): replay_returns of magent_amd/csrc/replay.hip, compiled as plain C++ against tests/hipemu, under
// AddressSanitizer and UndefinedBehaviorSanitizer.  Two record calls, a close and a pack through the C-ABI of include/magent_replay.h
// (tests/native/replay_asan.cc checks those), then replay_returns and replay_returns_direct with out_ret a heap block of exactly
// n_trans floats and boot one of exactly the tracked count; the result is compared on bits with a loop written here.
// tests/test_replay_returns.py builds and runs it (clang++ -fsanitize=address,undefined -ffp-contract=off: replay_emu.cc,
// emu_runtime.cc, this file).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "magent_replay.h"

namespace {

template <class T>
T *block(size_t n) {      // exactly n elements, 16-byte aligned
    void *p = nullptr;
    if (posix_memalign(&p, 16, std::max<size_t>(n * sizeof(T), 1))) abort();
    memset(p, 0x5A, n * sizeof(T));
    return (T *)p;
}

constexpr int ROWS = 12, CAP = 6, MAX_T = 16, VIEW = 5, FEAT = 4;

#define CHECK(what)                                                      \
    do {                                                                 \
        if (!(what)) {                                                   \
            fprintf(stderr, "replay_returns_asan: %s:%d: %s\n", __FILE__, __LINE__, #what); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

struct Call { std::vector<int> ids, begin, count; };

}  // namespace

int main() {
    ReplayState st{};
    st.capacity = CAP; st.max_transitions = MAX_T; st.view_row_bytes = VIEW * 4; st.feat_row_bytes = FEAT * 4;
    st.key_of_slot = block<long long>(CAP); st.sorted_keys = block<long long>(CAP); st.sorted_slot = block<int>(CAP);
    st.row_of_slot = block<int>(CAP); st.len = block<int>(CAP); st.flags = block<int>(CAP); st.src_row = block<int>(CAP);
    st.blk = block<int>((CAP + REPLAY_SCAN_BLOCK - 1) / REPLAY_SCAN_BLOCK); st.counters = block<int>(REPLAY_COUNTERS);
    st.log_view = block<float>(MAX_T * VIEW); st.log_feat = block<float>(MAX_T * FEAT); st.log_act = block<int>(MAX_T); st.log_rew = block<float>(MAX_T);
    st.log_slot = block<int>(MAX_T); st.log_ord = block<int>(MAX_T);
    for (int s = 0; s < CAP; s++) { st.key_of_slot[s] = st.sorted_keys[s] = REPLAY_NO_KEY; st.row_of_slot[s] = -1; st.len[s] = st.flags[s] = 0; }
    memset(st.counters, 0, REPLAY_COUNTERS * sizeof(int));

    // replay_asan.cc's two worlds: world 0 loses id 1 between the calls (an episode of length 1 beside episodes of length 2)
    std::vector<Call> calls = {{{0, 1, 2, 3, 9, 9, 9, 9, 0, 1, 2, 3}, {0, 8}, {4, 4}}, {{0, 2, 3, 3, 9, 9, 9, 9, 0, 1, 2, 3}, {0, 8}, {3, 4}}};
    Call after = {{0, 2, 3, 3, 9, 9, 9, 9, 0, 1, 2, 3}, {0, 8}, {2, 4}};
    const int order[ROWS] = {11, 3, 5, 0, 8, 2, 7, 1, 9, 4, 10, 6};
    long long *row_key = block<long long>(ROWS), *cand = block<long long>(ROWS), *cand_sorted = block<long long>(ROWS), *cand_pos = block<long long>(ROWS);
    int *row_slot = block<int>(ROWS), *first = block<int>(ROWS), *ids = block<int>(ROWS), *order_dev = block<int>(ROWS), *acts = block<int>(ROWS);
    float *view = block<float>(ROWS * VIEW), *feat = block<float>(ROWS * FEAT), *rews = block<float>(ROWS);
    memcpy(order_dev, order, sizeof(order));
    memset(view, 0, ROWS * VIEW * sizeof(float)); memset(feat, 0, ROWS * FEAT * sizeof(float)); memset(acts, 0, ROWS * sizeof(int));

    int call_no = 0;
    for (size_t t = 0; t < calls.size(); t++, call_no++) {
        const Call &c = calls[t];
        memcpy(ids, c.ids.data(), ROWS * sizeof(int));
        for (int r = 0; r < ROWS; r++) rews[r] = (r % 2 ? -1.0f : 1.0f) * (0.3f + 0.7f * r + 5.1f * t);      // (both signs)
        CHECK(replay_find(&st, ids, ROWS, c.begin.data(), c.count.data(), 2, row_key, row_slot, 0, nullptr) == 0);
        CHECK(replay_candidates(&st, row_key, row_slot, order_dev, ROWS, cand, nullptr) == 0);
        std::vector<long long> pos(ROWS);
        std::iota(pos.begin(), pos.end(), 0);
        std::stable_sort(pos.begin(), pos.end(), [&](long long a, long long b) { return cand[a] < cand[b]; });
        for (int i = 0; i < ROWS; i++) { cand_pos[i] = pos[i]; cand_sorted[i] = cand[pos[i]]; }
        CHECK(replay_admit(&st, cand, cand_sorted, cand_pos, ROWS, first, nullptr) == 0);
        std::vector<int> by_key(CAP);
        std::iota(by_key.begin(), by_key.end(), 0);
        std::stable_sort(by_key.begin(), by_key.end(), [&](int a, int b) { return st.key_of_slot[a] < st.key_of_slot[b]; });
        for (int i = 0; i < CAP; i++) { st.sorted_slot[i] = by_key[i]; st.sorted_keys[i] = st.key_of_slot[by_key[i]]; }
        CHECK(replay_find(&st, ids, ROWS, c.begin.data(), c.count.data(), 2, nullptr, nullptr, 1, nullptr) == 0);
        CHECK(replay_step(&st, call_no, 1, 8, view, feat, acts, rews, nullptr) == 0);
    }
    memcpy(ids, after.ids.data(), ROWS * sizeof(int));
    CHECK(replay_find(&st, ids, ROWS, after.begin.data(), after.count.data(), 2, nullptr, nullptr, 1, nullptr) == 0);
    CHECK(replay_step(&st, call_no++, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    const int tracked = st.counters[REPLAY_C_TRACKED], n = st.counters[REPLAY_C_FILL(call_no & 1)];
    CHECK(tracked == CAP && n > CAP && n <= MAX_T);
    float *out_view = block<float>(n * VIEW), *out_feat = block<float>(n * FEAT), *out_rew = block<float>(n), *out_mask = block<float>(n);
    int *out_act = block<int>(n), *base = block<int>(CAP), *dst = block<int>(n);
    unsigned char *out_term = block<unsigned char>(n);
    CHECK(replay_pack(&st, n, out_view, out_feat, out_act, out_rew, out_term, out_mask, base, dst, nullptr) == 0);

    float *boot = block<float>(tracked), *out_ret = block<float>(n), *want = block<float>(n);
    const double gamma = 0.99;
    int ones = 0, at = 0;
    for (int s = 0; s < tracked; s++) {
        boot[s] = (s % 2 ? 1.0f : -1.0f) * (1.5f + s);
        CHECK(base[s] == at);
        ones += st.len[s] == 1;
        volatile double keep = boot[s];                  // (volatile: the product is stored before it is added, whatever the flags)
        for (int i = st.len[s] - 1; i >= 0; i--) {
            volatile double scaled = keep * gamma;
            keep = scaled + (double)out_rew[at + i];
            want[at + i] = (float)keep;
        }
        at += st.len[s];
    }
    CHECK(at == n && ones >= 1);
    for (int direct = 0; direct < 2; direct++) {
        memset(out_ret, 0x5A, n * sizeof(float));
        CHECK((direct ? replay_returns_direct : replay_returns)(&st, tracked, n, base, out_rew, boot, gamma, out_ret, nullptr) == 0);
        CHECK(memcmp(out_ret, want, n * sizeof(float)) == 0);
    }
    // refused calls enqueue nothing; calls with nothing to do write nothing
    memset(out_ret, 0x5A, n * sizeof(float));
    CHECK(replay_returns(&st, tracked, n, base, out_rew, nullptr, gamma, out_ret, nullptr) == 1);
    CHECK(replay_returns(&st, tracked, n, base, out_rew, boot, gamma, nullptr, nullptr) == 1);
    CHECK(replay_returns(&st, CAP + 1, n, base, out_rew, boot, gamma, out_ret, nullptr) == 1);
    CHECK(replay_returns(&st, tracked, -1, base, out_rew, boot, gamma, out_ret, nullptr) == 1);
    CHECK(replay_returns(&st, 0, n, base, out_rew, boot, gamma, out_ret, nullptr) == 0);
    CHECK(replay_returns(&st, tracked, 0, base, out_rew, boot, gamma, out_ret, nullptr) == 0);
    for (int i = 0; i < n; i++) CHECK(((unsigned char *)(out_ret + i))[0] == 0x5A && ((unsigned char *)(out_ret + i))[3] == 0x5A);
    for (void *p : {(void *)st.key_of_slot, (void *)st.sorted_keys, (void *)st.sorted_slot, (void *)st.row_of_slot, (void *)st.len, (void *)st.flags,
                    (void *)st.src_row, (void *)st.blk, (void *)st.counters, st.log_view, st.log_feat, (void *)st.log_act, (void *)st.log_rew,
                    (void *)st.log_slot, (void *)st.log_ord, (void *)row_key, (void *)cand, (void *)cand_sorted, (void *)cand_pos, (void *)row_slot,
                    (void *)first, (void *)ids, (void *)order_dev, (void *)acts, (void *)view, (void *)feat, (void *)rews, (void *)out_view,
                    (void *)out_feat, (void *)out_rew, (void *)out_mask, (void *)out_act, (void *)base, (void *)dst, (void *)out_term, (void *)boot,
                    (void *)out_ret, (void *)want})
        free(p);
    printf("replay_returns_asan ok: %d returns of %d agents\n", n, tracked);
    return 0;
}
