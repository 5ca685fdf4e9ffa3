// Stand-alone program (CPU only): the host code and the kernels of magent_amd/csrc/replay.hip, compiled as plain C++ against tests/hipemu,
// under AddressSanitizer and UndefinedBehaviorSanitizer.  Two record calls, a close and a pack through the C-ABI of
// include/magent_replay.h, every buffer a heap block of exactly the size the ABI states, the result compared with a loop written here.
// tests/test_replay_kernels.py builds and runs it (clang++ -fsanitize=address,undefined: replay_emu.cc, emu_runtime.cc, this file).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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

constexpr int ROWS = 12, CAP = 6, MAX_T = 16, VIEW = 5, FEAT = 4;      // view rows of 20 bytes (4-byte units), feature rows of 16 (16-byte units)

#define CHECK(what)                                                      \
    do {                                                                 \
        if (!(what)) {                                                   \
            fprintf(stderr, "replay_asan: %s:%d: %s\n", __FILE__, __LINE__, #what); \
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

    // two worlds at rows 0 and 8; world 0 loses id 1 between the calls and id 3 after them, world 1 offers more agents than slots are left
    std::vector<Call> calls = {{{0, 1, 2, 3, 9, 9, 9, 9, 0, 1, 2, 3}, {0, 8}, {4, 4}}, {{0, 2, 3, 3, 9, 9, 9, 9, 0, 1, 2, 3}, {0, 8}, {3, 4}}};
    Call after = {{0, 2, 3, 3, 9, 9, 9, 9, 0, 1, 2, 3}, {0, 8}, {2, 4}};
    const int order[ROWS] = {11, 3, 5, 0, 8, 2, 7, 1, 9, 4, 10, 6};
    long long *row_key = block<long long>(ROWS), *cand = block<long long>(ROWS), *cand_sorted = block<long long>(ROWS), *cand_pos = block<long long>(ROWS);
    int *row_slot = block<int>(ROWS), *first = block<int>(ROWS), *ids = block<int>(ROWS), *order_dev = block<int>(ROWS), *acts = block<int>(ROWS);
    float *view = block<float>(ROWS * VIEW), *feat = block<float>(ROWS * FEAT), *rews = block<float>(ROWS);
    memcpy(order_dev, order, sizeof(order));

    std::map<long long, int> slot;                       // the restatement: key -> slot, per slot the codes of its transitions
    std::vector<std::vector<int>> want(CAP);
    std::vector<bool> died(CAP, false), recorded(CAP, false);
    int call_no = 0;
    for (size_t t = 0; t < calls.size(); t++, call_no++) {
        const Call &c = calls[t];
        memcpy(ids, c.ids.data(), ROWS * sizeof(int));
        for (int r = 0; r < ROWS; r++) {
            const int code = 100 * (int)(t + 1) + r;
            for (int e = 0; e < VIEW; e++) view[r * VIEW + e] = code + 0.125f * e;
            for (int e = 0; e < FEAT; e++) feat[r * FEAT + e] = -code - 0.25f * e;
            acts[r] = code * 3; rews[r] = code + 0.5f;
        }
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
        // the restatement
        std::map<long long, int> last;
        std::vector<long long> key_of_row(ROWS, -1);
        for (int s = 0; s < 2; s++)
            for (int r = c.begin[s]; r < c.begin[s] + c.count[s]; r++) last[key_of_row[r] = ((long long)s << 32) | (unsigned)c.ids[r]] = r;
        for (int p = 0; p < ROWS && (int)slot.size() < CAP; p++)
            if (key_of_row[order[p]] >= 0 && !slot.count(key_of_row[order[p]])) { const int s = (int)slot.size(); slot[key_of_row[order[p]]] = s; }
        std::vector<bool> now(CAP, false);
        for (auto &kv : last)
            if (slot.count(kv.first)) { now[slot[kv.first]] = true; want[slot[kv.first]].push_back(100 * (int)(t + 1) + kv.second); }
        for (int s = 0; s < CAP; s++) { if (recorded[s] && !now[s]) died[s] = true; recorded[s] = now[s]; }
    }
    memcpy(ids, after.ids.data(), ROWS * sizeof(int));
    CHECK(replay_find(&st, ids, ROWS, after.begin.data(), after.count.data(), 2, nullptr, nullptr, 1, nullptr) == 0);
    CHECK(replay_step(&st, call_no++, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    {
        std::map<long long, int> last;
        for (int s = 0; s < 2; s++)
            for (int r = after.begin[s]; r < after.begin[s] + after.count[s]; r++) last[((long long)s << 32) | (unsigned)after.ids[r]] = r;
        for (auto &kv : slot)
            if (recorded[kv.second] && !last.count(kv.first)) died[kv.second] = true;
    }
    CHECK((int)slot.size() == CAP && st.counters[REPLAY_C_TRACKED] == CAP);
    const int n = st.counters[REPLAY_C_FILL(call_no & 1)];
    int n_want = 0;
    for (auto &w : want) n_want += (int)w.size();
    CHECK(n == n_want && n > CAP && st.counters[REPLAY_C_OVERFLOW(call_no & 1)] == 0);
    float *out_view = block<float>(n * VIEW), *out_feat = block<float>(n * FEAT), *out_rew = block<float>(n), *out_mask = block<float>(n);
    int *out_act = block<int>(n), *base = block<int>(CAP), *dst = block<int>(n);
    unsigned char *out_term = block<unsigned char>(n);
    CHECK(replay_pack(&st, n, out_view, out_feat, out_act, out_rew, out_term, out_mask, base, dst, nullptr) == 0);
    int at = 0, terminals = 0;
    for (int s = 0; s < CAP; s++)
        for (size_t t = 0; t < want[s].size(); t++, at++) {
            const int code = want[s][t];
            const bool lastone = t + 1 == want[s].size();
            for (int e = 0; e < VIEW; e++) CHECK(out_view[at * VIEW + e] == code + 0.125f * e);
            for (int e = 0; e < FEAT; e++) CHECK(out_feat[at * FEAT + e] == -code - 0.25f * e);
            CHECK(out_act[at] == code * 3 && out_rew[at] == code + 0.5f);
            CHECK(out_term[at] == (lastone && died[s]) && out_mask[at] == (lastone && !died[s] ? 0.0f : 1.0f));
            terminals += out_term[at];
        }
    CHECK(terminals >= 1);
    // a refused table enqueues nothing; a call that does not fit sets the flag and records nothing
    const int bad_begin[2] = {0, 2}, bad_count[2] = {4, 4};
    CHECK(replay_find(&st, ids, ROWS, bad_begin, bad_count, 2, nullptr, nullptr, 1, nullptr) == 1);
    st.max_transitions = n + 1;
    CHECK(replay_find(&st, ids, ROWS, after.begin.data(), after.count.data(), 2, nullptr, nullptr, 1, nullptr) == 0);
    CHECK(replay_step(&st, call_no++, 1, 8, view, feat, acts, rews, nullptr) == 0);
    CHECK(st.counters[REPLAY_C_OVERFLOW(call_no & 1)] == 1 && st.counters[REPLAY_C_FILL(call_no & 1)] == n);
    for (void *p : {(void *)st.key_of_slot, (void *)st.sorted_keys, (void *)st.sorted_slot, (void *)st.row_of_slot, (void *)st.len, (void *)st.flags,
                    (void *)st.src_row, (void *)st.blk, (void *)st.counters, st.log_view, st.log_feat, (void *)st.log_act, (void *)st.log_rew,
                    (void *)st.log_slot, (void *)st.log_ord, (void *)row_key, (void *)cand, (void *)cand_sorted, (void *)cand_pos, (void *)row_slot,
                    (void *)first, (void *)ids, (void *)order_dev, (void *)acts, (void *)view, (void *)feat, (void *)rews, (void *)out_view,
                    (void *)out_feat, (void *)out_rew, (void *)out_mask, (void *)out_act, (void *)base, (void *)dst, (void *)out_term})
        free(p);
    printf("replay_asan ok: %d transitions of %d agents, %d terminal\n", n, CAP, terminals);
    return 0;
}
