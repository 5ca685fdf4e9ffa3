// replay.hip -- the device episode recorder of a packed EnvBatch (include/magent_replay.h; host side: magent_amd/replay.py).
//
// One call per cycle and side records the rows of the tracked agents, keyed by (segment, id) as the segmented DRQN table keys its states
// (policy_f32_dev.h: drqn_key).  All state is in the caller's ReplayState; nothing waits for the host.
//
//   k_replay_find        one thread per row: the row's segment (the table travels by value, policy_f32_dev.h: A2cSegTable) -> key -> binary
//                        search in the tracked keys (state_row_of_key) -> slot.  mark: row_of_slot[slot] = max(row): the LAST row of a
//                        duplicated key is the agent's, whatever the scheduling.
//   k_replay_candidates  the untracked in-segment rows in `order`'s order; the caller sorts them stably by key, k_replay_first marks the
//   k_replay_first       first offer of every key, and
//   k_replay_admit       ONE workgroup ranks the offers by a running scan and appends the keys while slots are free.
//   k_replay_count       per block of REPLAY_SCAN_BLOCK slots, the slots with a row (the step) or the transitions (the pack) ...
//   k_replay_place       ... and the scan over them: a present slot's place in the step-major log, its ordinal (the episode's length so
//                        far), the deaths (recorded by the previous call, absent from this one) and the overflow decision.  Every
//                        workgroup takes the decision from the same words (the counters of the call's parity) and workgroup 0 writes
//                        the other parity's: no workgroup reads a word that another one of the launch writes.
//   k_replay_copy        the hot one: a wave owns whole rows.  Rows whose size is a multiple of 16 bytes (bf16 cells, most feature rows)
//                        move as 16-byte units, 1 KiB per wave instruction; the others (a float32 view of 13 x 13 x 7 is 4732 bytes: the
//                        segment is 16-byte aligned, the row is not) as 4-byte words, 256 contiguous bytes per instruction.  Four
//                        independent loads are in flight per lane before the first store.  The grid comes from the host's bound; the
//                        number of rows is read on the device.  The pack's scatter is the same kernel with the indices swapped.
//   k_replay_base        exclusive scan of the episode lengths -> every slot's first row of the packed arrays
//   k_replay_dst         log row j -> base[slot] + ordinal; terminal and mask from "ordinal == len - 1" and the died flag
//   k_replay_returns     the A2C's discounted returns over the packed rewards: one lane per slot, from the episode's last row to its
//                        first, keep = keep * gamma + r in double with the product and the sum rounded separately
//
// No floating-point atomics and no atomic whose result depends on the order (the one atomic is k_replay_find's integer maximum).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/magent_policy.h"
#include "../../include/magent_replay.h"
#include "policy_f32_dev.h"
#include "policy_host.h"

namespace magent_amd {
namespace {

constexpr int RP_THREADS = 256, RP_SCAN = REPLAY_SCAN_BLOCK, RP_ADMIT_PER_THREAD = 8, RP_COPY_MAX_BLOCKS = 8192;
constexpr int RP_RET_SLOTS = 128, RP_RET_LDS = 8192;            // k_replay_returns: slots per workgroup; the rows (float32) its LDS stage takes

// Exclusive scan of v over the RP_SCAN threads of the workgroup, *total: the sum (Hillis-Steele on two LDS rows; buf: int [2 * RP_SCAN]).
// Ends with a barrier: buf may be reused at once.
__device__ __forceinline__ int block_scan(int v, int *buf, int *total) {
    const int tid = threadIdx.x;
    int *a = buf, *b = buf + RP_SCAN;
    a[tid] = v;
    __syncthreads();
    for (int d = 1; d < RP_SCAN; d <<= 1) {
        b[tid] = a[tid] + (tid >= d ? a[tid - d] : 0);
        __syncthreads();
        int *t = a; a = b; b = t;
    }
    const int incl = a[tid];
    *total = a[RP_SCAN - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(RP_THREADS) k_replay_find(A2cSegTable t, int seg_first, int row_lo, int row_hi, const int *ids, ReplayState st,
                                                           long long *row_key, int *row_slot, int mark) {
    const int r = row_lo + blockIdx.x * RP_THREADS + threadIdx.x;
    if (r >= row_hi) return;
    int lo = 0, hi = t.n_seg;                                    // lo: the first segment that begins behind r (drqn_lookup_row's search)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t.begin[mid] <= r) lo = mid + 1;
        else hi = mid;
    }
    const int s = lo - 1;
    if (s < 0 || r >= t.begin[s] + t.count[s]) {
        if (row_key) { row_key[r] = REPLAY_NO_KEY; row_slot[r] = -2; }
        return;
    }
    const long long key = f32::drqn_key(seg_first + s, ids[r]);
    const int slot = f32::state_row_of_key(key, st.sorted_keys, st.sorted_slot, st.counters[REPLAY_C_TRACKED]);
    if (row_key) { row_key[r] = key; row_slot[r] = slot; }
    if (mark && slot >= 0 && slot < st.capacity) atomicMax(&st.row_of_slot[slot], r);
}

__global__ void __launch_bounds__(RP_THREADS) k_replay_candidates(const long long *row_key, const int *row_slot, const int *order, int n, long long *cand_key) {
    const int p = blockIdx.x * RP_THREADS + threadIdx.x;
    if (p >= n) return;
    const int r = order ? order[p] : p;
    cand_key[p] = r >= 0 && r < n && row_slot[r] == -1 ? row_key[r] : REPLAY_NO_KEY;
}

__global__ void __launch_bounds__(RP_THREADS) k_replay_first(const long long *sorted_cand, const long long *cand_pos, int n, int *first) {
    const int i = blockIdx.x * RP_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long key = sorted_cand[i], p = cand_pos[i];
    if (p >= 0 && p < n) first[p] = key != REPLAY_NO_KEY && (i == 0 || sorted_cand[i - 1] != key);
}

// one workgroup: thread t of a pass takes RP_ADMIT_PER_THREAD consecutive positions of `order`
__global__ void __launch_bounds__(RP_SCAN) k_replay_admit(ReplayState st, const long long *cand_key, const int *first, int n) {
    __shared__ int buf[2 * RP_SCAN];
    int running = st.counters[REPLAY_C_TRACKED];
    const int start = running;
    for (int base = 0; base < n && running < st.capacity; base += RP_SCAN * RP_ADMIT_PER_THREAD) {
        const int p0 = base + threadIdx.x * RP_ADMIT_PER_THREAD;
        int mine = 0;
        for (int e = 0; e < RP_ADMIT_PER_THREAD; e++) mine += p0 + e < n && first[p0 + e] != 0;
        int total;
        int rank = running + block_scan(mine, buf, &total);
        for (int e = 0; e < RP_ADMIT_PER_THREAD && mine > 0; e++)
            if (p0 + e < n && first[p0 + e] != 0) {
                if (rank < st.capacity) st.key_of_slot[rank] = cand_key[p0 + e];
                rank++;
            }
        running += total;
    }
    __syncthreads();                                             // (every thread has read the counter)
    if (threadIdx.x == 0 && running != start) st.counters[REPLAY_C_TRACKED] = min(running, st.capacity);
}

// blk[b] = the slots of block b that have a row in this call (lengths == 0) or the transitions recorded of them (lengths != 0)
__global__ void __launch_bounds__(RP_SCAN) k_replay_count(ReplayState st, int lengths) {
    __shared__ int buf[2 * RP_SCAN];
    const int s = blockIdx.x * RP_SCAN + threadIdx.x, tracked = st.counters[REPLAY_C_TRACKED];
    int v = 0;
    if (s < st.capacity && s < tracked) v = lengths ? st.len[s] : st.row_of_slot[s] >= 0;
    int total;
    block_scan(v, buf, &total);
    if (threadIdx.x == 0) st.blk[blockIdx.x] = total;
}

// (the sum of blk in front of this block, the sum of all of blk)
__device__ __forceinline__ void blocks_before(const int *blk, int *buf, int *before, int *all) {
    int mine_before = 0, mine_all = 0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += RP_SCAN) {
        const int v = blk[i];
        mine_all += v;
        if (i < (int)blockIdx.x) mine_before += v;
    }
    block_scan(mine_before, buf, before);
    block_scan(mine_all, buf, all);
}

__global__ void __launch_bounds__(RP_SCAN) k_replay_place(ReplayState st, int call, int record) {
    __shared__ int buf[2 * RP_SCAN];
    const int par = call & 1, tracked = st.counters[REPLAY_C_TRACKED];
    const int fill = st.counters[REPLAY_C_FILL(par)], over = st.counters[REPLAY_C_OVERFLOW(par)];
    const int s = blockIdx.x * RP_SCAN + threadIdx.x;
    const bool mine = s < st.capacity && s < tracked;
    const int row = mine ? st.row_of_slot[s] : -1;
    int before, k, total;
    blocks_before(st.blk, buf, &before, &k);
    const int at = before + block_scan(row >= 0, buf, &total);
    const bool over_now = over != 0 || (record && (long long)fill + k > (long long)st.max_transitions);
    if (mine && !over_now) {
        const int f = st.flags[s];
        if (row >= 0) {
            if (record) {
                const int ord = st.len[s];
                st.src_row[at] = row;
                st.log_slot[fill + at] = s;
                st.log_ord[fill + at] = ord;
                st.len[s] = ord + 1;
                st.flags[s] = (f & REPLAY_F_DIED) | REPLAY_F_RECORDED;
            }
        } else if (f & REPLAY_F_RECORDED) {
            st.flags[s] = REPLAY_F_DIED;
        }
    }
    if (s < st.capacity) st.row_of_slot[s] = -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st.counters[REPLAY_C_FILL(par ^ 1)] = record && !over_now ? fill + k : fill;
        st.counters[REPLAY_C_OVERFLOW(par ^ 1)] = over_now;
    }
}

__global__ void __launch_bounds__(RP_SCAN) k_replay_base(ReplayState st, int *base) {
    __shared__ int buf[2 * RP_SCAN];
    const int s = blockIdx.x * RP_SCAN + threadIdx.x, tracked = st.counters[REPLAY_C_TRACKED];
    const int v = s < st.capacity && s < tracked ? st.len[s] : 0;
    int before, all, total;
    blocks_before(st.blk, buf, &before, &all);
    const int at = before + block_scan(v, buf, &total);
    if (s < st.capacity) base[s] = at;
}

__global__ void __launch_bounds__(RP_THREADS) k_replay_dst(ReplayState st, int n_trans, const int *base, int *dst, unsigned char *terminal, float *mask) {
    const int j = blockIdx.x * RP_THREADS + threadIdx.x;
    if (j >= n_trans) return;
    const int s = st.log_slot[j], ord = st.log_ord[j];
    int d = -1;
    if (s >= 0 && s < st.capacity) {
        d = base[s] + ord;
        if (d < 0 || d >= n_trans) d = -1;
    }
    dst[j] = d;
    if (d < 0) return;
    const bool last = ord == st.len[s] - 1, died = (st.flags[s] & REPLAY_F_DIED) != 0;
    terminal[d] = last && died;
    mask[d] = last && !died ? 0.0f : 1.0f;
}

// ---------------------------------------------------------------------------------------------------- the row copy
struct RowCopy {
    const char *src_view, *src_feat;
    const int *src_act;
    const float *src_rew;
    char *dst_view, *dst_feat;
    int *dst_act;
    float *dst_rew;
    int view_bytes, feat_bytes, view_vec, feat_vec;              // *_vec: rows and bases are multiples of 16 bytes
};

// one wave, one row: lane l takes units l, l + 64, ...; four loads in flight before the first store
template <class Unit>
__device__ __forceinline__ void copy_units(const Unit *s, Unit *d, int n, int lane) {
    int i = lane;
    for (; i + 192 < n; i += 256) {
        const Unit a = s[i], b = s[i + 64], c = s[i + 128], e = s[i + 192];
        d[i] = a; d[i + 64] = b; d[i + 128] = c; d[i + 192] = e;
    }
    for (; i < n; i += 64) d[i] = s[i];
}
__device__ __forceinline__ void copy_row(const char *s, char *d, int bytes, int vec, int lane) {
    if (vec) copy_units((const uint4 *)s, (uint4 *)d, bytes >> 4, lane);
    else copy_units((const unsigned *)s, (unsigned *)d, bytes >> 2, lane);
}

// STEP: rows src_row[j] -> log row fill + j, j < the rows this call recorded (the two parities' fills).  !STEP (the pack): log row j ->
// packed row idx[j], j < n_host; idx[j] < 0: no row.
template <bool STEP>
__global__ void __launch_bounds__(RP_THREADS) k_replay_copy(RowCopy c, const int *counters, int call, int n_host, const int *idx) {
    int k = n_host, fill = 0;
    if (STEP) {
        fill = counters[REPLAY_C_FILL(call & 1)];
        k = min(counters[REPLAY_C_FILL((call & 1) ^ 1)] - fill, n_host);
    }
    const int lane = threadIdx.x & 63, waves = gridDim.x * (RP_THREADS / 64);
    for (int j = blockIdx.x * (RP_THREADS / 64) + (threadIdx.x >> 6); j < k; j += waves) {
        const int other = idx[j];
        if (other < 0) continue;
        const size_t from = STEP ? (size_t)other : (size_t)j, to = STEP ? (size_t)fill + j : (size_t)other;
        copy_row(c.src_view + from * c.view_bytes, c.dst_view + to * c.view_bytes, c.view_bytes, c.view_vec, lane);
        copy_row(c.src_feat + from * c.feat_bytes, c.dst_feat + to * c.feat_bytes, c.feat_bytes, c.feat_vec, lane);
        if (lane == 0) c.dst_act[to] = c.src_act[from];
        if (lane == 1) c.dst_rew[to] = c.src_rew[from];
    }
}

// ---------------------------------------------------------------------------------------------------- the discounted returns
// One step of the A2C's recurrence in IEEE double, the product and the sum rounded separately, as the host's `keep * gamma + r[i]` is:
// the pragma keeps the compiler from contracting the two into an FMA (device code is contracted by default).
__device__ __forceinline__ double returns_step(double keep, double gamma, float r) {
#pragma clang fp contract(off)
    const double scaled = keep * gamma;
    return scaled + (double)r;
}

// One lane per slot, serial inside the episode (a scan of composed affine maps would round differently).  A lane whose rows are not
// inside the packed arrays -- a base that replay_pack did not leave -- writes nothing.
//   STAGED: the packed rows of a workgroup's RP_RET_SLOTS consecutive slots are one contiguous range.  Where it is at most RP_RET_LDS
//   rows, the rewards come into LDS coalesced, the lanes run the recurrence there (float32 overwritten in place, keep a double in a
//   register) and the range leaves coalesced; a longer range takes the direct form, decided per workgroup.
template <bool STAGED>
__global__ void __launch_bounds__(RP_RET_SLOTS) k_replay_returns(ReplayState st, int n_slots, int n_trans, const int *__restrict__ base,
                                                                const float *__restrict__ rew, const float *__restrict__ boot, double gamma,
                                                                float *__restrict__ out) {
    __shared__ float lds[STAGED ? RP_RET_LDS : 1];
    const int s0 = blockIdx.x * RP_RET_SLOTS, s = s0 + threadIdx.x;
    int b = 0, m = 0;
    if (s < n_slots) {
        b = base[s];
        m = st.len[s];
        if (m < 0 || b < 0 || (long long)b + m > (long long)n_trans) m = 0;
    }
    if (STAGED) {
        const int s1 = min(s0 + RP_RET_SLOTS, n_slots) - 1;      // (s0 < n_slots: the grid covers n_slots)
        const int lo = base[s0], hi = base[s1] + st.len[s1];
        if (lo >= 0 && hi >= lo && hi <= n_trans && hi - lo <= RP_RET_LDS) {       // (the same words in every lane: no lane leaves the others at a barrier)
            for (int i = threadIdx.x; i < hi - lo; i += RP_RET_SLOTS) lds[i] = rew[lo + i];
            __syncthreads();
            if (m > 0 && b >= lo && b + m <= hi) {
                float *mine = lds + (b - lo);
                double keep = (double)boot[s];
                for (int i = m - 1; i >= 0; i--) {
                    keep = returns_step(keep, gamma, mine[i]);
                    mine[i] = (float)keep;
                }
            }
            __syncthreads();
            for (int i = threadIdx.x; i < hi - lo; i += RP_RET_SLOTS) out[lo + i] = lds[i];
            return;
        }
    }
    if (m <= 0) return;
    double keep = (double)boot[s];
#pragma unroll 4
    for (int i = m - 1; i >= 0; i--) {
        keep = returns_step(keep, gamma, rew[b + i]);
        out[b + i] = (float)keep;
    }
}

inline bool state_ok(const ReplayState *st) {
    return st && st->capacity > 0 && st->max_transitions > 0 && st->key_of_slot && st->sorted_keys && st->sorted_slot && st->row_of_slot && st->len &&
           st->flags && st->src_row && st->blk && st->counters && st->log_view && st->log_feat && st->log_act && st->log_rew && st->log_slot &&
           st->log_ord && st->view_row_bytes > 0 && st->feat_row_bytes > 0 && st->view_row_bytes % 4 == 0 && st->feat_row_bytes % 4 == 0;
}
inline int scan_blocks(const ReplayState *st) { return (st->capacity + RP_SCAN - 1) / RP_SCAN; }
inline int vec16(const void *a, const void *b, int bytes) { return bytes % 16 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }
inline int copy_blocks(int rows) { return std::min((rows + RP_THREADS / 64 - 1) / (RP_THREADS / 64), RP_COPY_MAX_BLOCKS); }

}  // namespace
}  // namespace magent_amd

using namespace magent_amd;

extern "C" {

int replay_find(const ReplayState *st, const int *ids, int n, const int *seg_begin, const int *seg_count, int n_seg, long long *row_key,
                int *row_slot, int mark, void *stream) {
    if (!state_ok(st) || n < 0 || n_seg < 0 || (n_seg > 0 && !(seg_begin && seg_count)) || (row_key == nullptr) != (row_slot == nullptr)) return 1;
    long long at = 0;                                            // a2c_seg_table's rules, for a table of any length
    for (int s = 0; s < n_seg; s++) {
        const long long b = seg_begin[s], c = seg_count[s];
        if (b < 0 || c < 0 || b < at || b + c > (long long)n) return 1;
        at = b + c;
    }
    if (n == 0) return 0;
    if (!ids) return 1;
    hipStream_t hs = (hipStream_t)stream;
    StreamDevice on(hs);
    if (!on.ok) return 2;
    for (int s0 = 0; s0 == 0 || s0 < n_seg; s0 += A2C_MAX_SEGMENTS) {
        // the rows of this launch: from the end of the launch before to the end of this one's last segment; the last takes the rest
        A2cSegTable table;
        const int s1 = std::min(s0 + A2C_MAX_SEGMENTS, n_seg);
        table.n_seg = s1 - s0;
        for (int s = s0; s < s1; s++) { table.begin[s - s0] = seg_begin[s]; table.count[s - s0] = seg_count[s]; }
        const int row_lo = s0 == 0 ? 0 : seg_begin[s0 - 1] + seg_count[s0 - 1];
        const int row_hi = s1 >= n_seg ? n : seg_begin[s1 - 1] + seg_count[s1 - 1];
        if (row_hi > row_lo && (row_key || table.n_seg > 0))
            hipLaunchKernelGGL(k_replay_find, dim3((row_hi - row_lo + RP_THREADS - 1) / RP_THREADS), dim3(RP_THREADS), 0, hs, table, s0, row_lo, row_hi, ids,
                               *st, row_key, row_slot, mark);
    }
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int replay_candidates(const ReplayState *st, const long long *row_key, const int *row_slot, const int *order, int n, long long *cand_key,
                      void *stream) {
    if (!state_ok(st) || n < 0) return 1;
    if (n == 0) return 0;
    if (!row_key || !row_slot || !cand_key) return 1;
    hipStream_t hs = (hipStream_t)stream;
    StreamDevice on(hs);
    if (!on.ok) return 2;
    hipLaunchKernelGGL(k_replay_candidates, dim3((n + RP_THREADS - 1) / RP_THREADS), dim3(RP_THREADS), 0, hs, row_key, row_slot, order, n, cand_key);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int replay_admit(const ReplayState *st, const long long *cand_key, const long long *sorted_cand, const long long *cand_pos, int n, int *first,
                 void *stream) {
    if (!state_ok(st) || n < 0) return 1;
    if (n == 0) return 0;
    if (!cand_key || !sorted_cand || !cand_pos || !first) return 1;
    hipStream_t hs = (hipStream_t)stream;
    StreamDevice on(hs);
    if (!on.ok) return 2;
    hipLaunchKernelGGL(k_replay_first, dim3((n + RP_THREADS - 1) / RP_THREADS), dim3(RP_THREADS), 0, hs, sorted_cand, cand_pos, n, first);
    hipLaunchKernelGGL(k_replay_admit, dim3(1), dim3(RP_SCAN), 0, hs, *st, cand_key, (const int *)first, n);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int replay_copy(const ReplayState *st, const int *counters, int call, int max_rows, const void *view, const void *feat, const int *acts,
                const float *rewards, const int *src_row, void *stream) {
    if (!state_ok(st) || call < 0 || max_rows < 0 || max_rows > st->max_transitions) return 1;
    if (max_rows == 0) return 0;
    if (!counters || !view || !feat || !acts || !rewards || !src_row) return 1;
    hipStream_t hs = (hipStream_t)stream;
    StreamDevice on(hs);
    if (!on.ok) return 2;
    RowCopy c{(const char *)view, (const char *)feat, acts, rewards, (char *)st->log_view, (char *)st->log_feat, st->log_act, st->log_rew,
              st->view_row_bytes, st->feat_row_bytes, vec16(view, st->log_view, st->view_row_bytes), vec16(feat, st->log_feat, st->feat_row_bytes)};
    hipLaunchKernelGGL(k_replay_copy<true>, dim3(copy_blocks(max_rows)), dim3(RP_THREADS), 0, hs, c, counters, call, max_rows, src_row);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int replay_step(const ReplayState *st, int call, int record, int max_rows, const void *view, const void *feat, const int *acts,
                const float *rewards, void *stream) {
    if (!state_ok(st) || call < 0 || max_rows < 0) return 1;
    if (record && max_rows > 0 && !(view && feat && acts && rewards)) return 1;
    hipStream_t hs = (hipStream_t)stream;
    StreamDevice on(hs);
    if (!on.ok) return 2;
    const int nb = scan_blocks(st);
    hipLaunchKernelGGL(k_replay_count, dim3(nb), dim3(RP_SCAN), 0, hs, *st, 0);
    hipLaunchKernelGGL(k_replay_place, dim3(nb), dim3(RP_SCAN), 0, hs, *st, call, record);
    const int rows = std::min(max_rows, std::min(st->capacity, st->max_transitions));      // (more cannot be recorded by one call)
    if (record && rows > 0) return replay_copy(st, st->counters, call, rows, view, feat, acts, rewards, st->src_row, stream);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int replay_pack(const ReplayState *st, int n_trans, void *out_view, void *out_feat, int *out_act, float *out_rew, unsigned char *out_terminal,
                float *out_mask, int *base, int *dst, void *stream) {
    if (!state_ok(st) || n_trans < 0 || n_trans > st->max_transitions) return 1;
    if (n_trans == 0) return 0;
    if (!out_view || !out_feat || !out_act || !out_rew || !out_terminal || !out_mask || !base || !dst) return 1;
    hipStream_t hs = (hipStream_t)stream;
    StreamDevice on(hs);
    if (!on.ok) return 2;
    const int nb = scan_blocks(st);
    hipLaunchKernelGGL(k_replay_count, dim3(nb), dim3(RP_SCAN), 0, hs, *st, 1);
    hipLaunchKernelGGL(k_replay_base, dim3(nb), dim3(RP_SCAN), 0, hs, *st, base);
    hipLaunchKernelGGL(k_replay_dst, dim3((n_trans + RP_THREADS - 1) / RP_THREADS), dim3(RP_THREADS), 0, hs, *st, n_trans, (const int *)base, dst, out_terminal,
                       out_mask);
    RowCopy c{(const char *)st->log_view, (const char *)st->log_feat, st->log_act, st->log_rew, (char *)out_view, (char *)out_feat, out_act, out_rew,
              st->view_row_bytes, st->feat_row_bytes, vec16(st->log_view, out_view, st->view_row_bytes), vec16(st->log_feat, out_feat, st->feat_row_bytes)};
    hipLaunchKernelGGL(k_replay_copy<false>, dim3(copy_blocks(n_trans)), dim3(RP_THREADS), 0, hs, c, (const int *)st->counters, 0, n_trans, (const int *)dst);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

static int returns_launch(bool staged, const ReplayState *st, int n_slots, int n_trans, const int *base, const float *rew, const float *boot,
                          double gamma, float *out_ret, void *stream) {
    if (!state_ok(st) || n_slots < 0 || n_trans < 0 || n_slots > st->capacity || n_trans > st->max_transitions) return 1;
    if (!base || !rew || !boot || !out_ret) return 1;
    if (n_slots == 0 || n_trans == 0) return 0;
    hipStream_t hs = (hipStream_t)stream;
    StreamDevice on(hs);
    if (!on.ok) return 2;
    const dim3 grid((n_slots + RP_RET_SLOTS - 1) / RP_RET_SLOTS), block(RP_RET_SLOTS);
    if (staged) hipLaunchKernelGGL(k_replay_returns<true>, grid, block, 0, hs, *st, n_slots, n_trans, base, rew, boot, gamma, out_ret);
    else hipLaunchKernelGGL(k_replay_returns<false>, grid, block, 0, hs, *st, n_slots, n_trans, base, rew, boot, gamma, out_ret);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

int replay_returns(const ReplayState *st, int n_slots, int n_trans, const int *base, const float *rew, const float *boot, double gamma,
                   float *out_ret, void *stream) {
    return returns_launch(true, st, n_slots, n_trans, base, rew, boot, gamma, out_ret, stream);
}

int replay_returns_direct(const ReplayState *st, int n_slots, int n_trans, const int *base, const float *rew, const float *boot, double gamma,
                          float *out_ret, void *stream) {
    return returns_launch(false, st, n_slots, n_trans, base, rew, boot, gamma, out_ret, stream);
}

}  // extern "C"
