// policy_f32_dev.h -- what the float32 policy translation units share (internal; not part of the C-ABI):
//   policy_f32.hip       the DQN: k_dqn_conv_f32 + k_dqn_head_f32, and the trunk launcher below
//   policy_drqn_f32.hip  the DRQN: the DQN's trunk, then k_drqn_gru_f32 + k_drqn_head_f32
//   policy_a2c_f32.hip   the A2C: k_a2c_trunk_f32, k_a2c_layer_f32 (+ the column sums), k_a2c_head_f32
// Operand and fragment conventions: policy_f32.hip's header comment and include/magent_policy.h ("f32 fragment order").
// The building blocks, each written once:
//   out_of                                           which output a result register holds
//   dense_main, stage_features, dense_emb,
//   hidden_out with the sinks ToX / ToHid            the 128 agents x 256 outputs dense pair (k_dqn_head_f32, k_a2c_trunk_f32)
//   head_gemm512                                     the one-wave K = 512, 32-output head GEMM (k_drqn_head_f32, k_a2c_head_f32)
//   q_epilogue                                       the dueling combination, torch.argmax's pick, the stores (k_dqn_head_f32, k_drqn_head_f32)
//   policy_epilogue                                  softmax, clamp, the stores and the inverse-CDF draw (k_a2c_head_f32, k_a2c_head_bf16)
//   pingpong                                         the streamed-row double buffering (k_drqn_gru_f32, k_a2c_layer_f32, head_gemm512_bf16)
//   state_row                                        the id table's look-up (k_drqn_gru_f32, k_drqn_gru_bf16)
//   drqn_key, state_row_of_key, drqn_lookup_row      the (segment, id) table's look-up (policy_host.h: k_drqn_lookup_seg)
//   colsum_rows, colsum_blocks                       the CommNet column sums' bodies (policy_host.h: the k_a2c_colsum* kernels)
//   seg_map, colsum_part_seg, colsum_blocks_seg, seg_of_row   the segmented A2C call's maps and sums (k_a2c_segmap, the *_seg kernels, the layers)
// The bf16 files take their float32 side from here too (policy_bf16_dev.h includes this header): policy.hip the vector types, out_of
// and q_before; policy_drqn_bf16.hip out_of, sigmoid, q_epilogue and state_row (its gates, blend and epilogue are float32);
// policy_a2c_bf16.hip out_of, relu, policy_epilogue and the column sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/magent_policy.h"

namespace magent_amd {

// The A2C: rows of A2C_HID units; column sums over blocks of A2C_CS_BLOCK agents.  The segmented call's table (policy_a2c_infer*_seg: n
// packed rows and segments (begin, count)) travels to the device by value, as the argument of k_a2c_segmap (policy_host.h).
constexpr int A2C_HID = 512, A2C_CS_BLOCK = 256, A2C_MAX_SEGMENTS = POLICY_A2C_MAX_SEGMENTS;
struct A2cSegTable { int n_seg; int begin[A2C_MAX_SEGMENTS]; int count[A2C_MAX_SEGMENTS]; };

namespace f32 {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ f32x16 mfma4(const f32x4 &w, const f32x4 &x, f32x16 acc) {     // the four k-steps of one group of 8 K-values
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[0], x[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[1], x[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[2], x[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[3], x[3], acc, 0, 0, 0);
    return acc;
}
// the output (of a 32-wide tile) that result register r of a lane of group g = lane >> 5 holds: a lane owns 8 q + 4 g + 0..3 for q = 0..3
__device__ __forceinline__ int out_of(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }
// relu that keeps a NaN a NaN, as torch.relu does (fmaxf is IEEE maxNum: fmaxf(NaN, 0) = 0, and a poisoned view or a diverged network would
// then act on finite garbage).  IEEE 754-2019 maximum: one v_maximum3_f32 on gfx950, the cost of the v_max_f32 it replaces; -0 gives +0.
__device__ __forceinline__ float relu(float x) { return __builtin_elementwise_maximum(x, 0.0f); }
// the GRU gates' sigmoid (k_drqn_gru_f32, k_drqn_gru_bf16): nothing launders a NaN
__device__ __forceinline__ float sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ f32x4 relu4(const f32x16 &acc, int q) {
    return f32x4{relu(acc[4 * q]), relu(acc[4 * q + 1]), relu(acc[4 * q + 2]), relu(acc[4 * q + 3])};
}
// torch.argmax's order of a Q row: a NaN above everything (the first NaN wins), then the larger value, the lower index among equals.  Does
// (v, o) come before (best, arg)?
__device__ __forceinline__ bool q_before(float v, int o, float best, int arg) {
    return v != v ? (best == best || o < arg) : (best == best && (v > best || (v == best && o < arg)));
}

// ---------------------------------------------------------------------------------------------------- the 128 x 256 dense pair
// dense K -> 256 as a GEMM over 128 agents per workgroup of 8 waves: wave w owns outputs 32 w .. 32 w + 31 for all four agent tiles (per
// group of 8 K-values ONE weight float4 from L2 and four activation float4 from LDS feed 16 MFMAs), activations double buffered through
// LDS a 64-value chunk at a time; then the feature embedding K = FK -> 256 from an LDS image of the features.  How a chunk reaches LDS,
// when the features are staged, where the two halves of the hidden layer go and what lies between them is the calling kernel's.
constexpr int DENSE_THREADS = 512, DENSE_M = 128, DENSE_KC = 64;      // 128 agents per workgroup of 8 waves; K staged 64 values at a time
constexpr int DENSE_ABUF = DENSE_M * (DENSE_KC / 4);                  // float4 units of one activation buffer: 128 agents x 16 = 32 KB

// LDS images: rows of 16 float4 (activation chunk) / 64 float4 (hidden half), the unit index xor-ed with the row's low bits so that the 16
// lanes of a ds_read_b128 service group (16 consecutive agents, one unit) cover all 16 columns
__device__ __forceinline__ int act_slot(int row, int unit) { return row * 16 + (unit ^ (row & 15)); }
__device__ __forceinline__ int hid_slot(int row, int unit) { return row * 64 + (unit ^ (row & 15)); }

// acc[j] (agent tile j, output tile w) = the dense layer over n_groups groups of 8 K-values (8 per chunk; the last chunk may be short).
// s_act: [2][128 agents][16 units], swizzled (act_slot).  aload(c) requests chunk c into the caller's registers, astore(buf) puts the
// requested chunk into s_act + buf * DENSE_ABUF; a chunk's weights are fetched a chunk ahead of their use.  Ends behind a barrier:
// nobody reads the activation buffers any more.
template <class ALoad, class AStore>
__device__ __forceinline__ void dense_main(f32x16 (&acc)[4], const f32x4 *s_act, const f32x4 *wv, int n_groups, const ALoad &aload, const AStore &astore) {
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 5, r32 = l & 31;
    const int total = (n_groups + 7) / 8;
    const f32x4 *wbase = wv + (size_t)w * 64 + l;          // fragment (group m, tile w) = wbase[m * 8 * 64]
    f32x4 wr[2][8];          // the wave's weight fragments: this chunk's and the next one's
    auto wload = [&](int c, f32x4 (&dst)[8]) {
#pragma unroll
        for (int m = 0; m < 8; m++) dst[m] = wbase[(size_t)min(c * 8 + m, n_groups - 1) * 8 * 64];
    };
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = f32x16{0};

    aload(0);
    wload(0, wr[0]);
    astore(0);
    if (total > 1) aload(1);
    __syncthreads();
    auto chunk = [&](int c, f32x4 (&wc)[8], f32x4 (&wn)[8]) __attribute__((always_inline)) {
        const int buf = c & 1;
        const int groups = min(8, n_groups - c * 8);
        if (c + 1 < total) wload(c + 1, wn);                 // a chunk (16 x 8 MFMAs per wave) ahead of its use
        f32x4 x[2][4];
        auto xread = [&](int m, f32x4 (&dst)[4]) {
#pragma unroll
            for (int j = 0; j < 4; j++) dst[j] = s_act[buf * DENSE_ABUF + act_slot(32 * j + r32, 2 * m + g)];
        };
        xread(0, x[0]);
#pragma unroll
        for (int m = 0; m < 8; m++) {
            if (m < 7) xread(m + 1, x[(m + 1) & 1]);
            if (m < groups) {
#pragma unroll
                for (int j = 0; j < 4; j++) acc[j] = mfma4(wc[m], x[m & 1][j], acc[j]);
            }
            if (m == 1 && c + 1 < total) astore(buf ^ 1);    // the next chunk, requested a chunk ago (its buffer was last read two barriers back)
        }
        if (c + 2 < total) aload(c + 2);
        __syncthreads();
    };
    for (int c = 0; c < total; c += 2) {
        chunk(c, wr[0], wr[1]);
        if (c + 1 < total) chunk(c + 1, wr[1], wr[0]);
    }
}
// the features of the workgroup's agents a0 .. a0 + 127 to LDS as [128 agents][FK] (FK: F padded to 8 with zeros; rows past n are zeros)
__device__ __forceinline__ void stage_features(float *s_feat, const float *feat, int a0, int n, int F, int FK) {
    const int tid = threadIdx.x;
    for (int k = tid; k < DENSE_M * FK; k += DENSE_THREADS) {
        const int row = k / FK, f = k - row * FK;
        s_feat[k] = (f < F && a0 + row < n) ? feat[(size_t)(a0 + row) * F + f] : 0.0f;
    }
}
// acc[j] = the feature embedding, K = FK, all eight waves (output tile w, four agent tiles); we: [FK / 8][8 tiles][64]
__device__ __forceinline__ void dense_emb(f32x16 (&acc)[4], const float *s_feat, const f32x4 *we, int FK) {
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 5, r32 = l & 31;
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = f32x16{0};
    for (int m = 0; m < FK / 8; m++) {
        const f32x4 wm = we[((size_t)m * 8 + w) * 64 + l];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const f32x4 x = *(const f32x4 *)(s_feat + (32 * j + r32) * FK + 8 * m + 4 * g);
            acc[j] = mfma4(wm, x, acc[j]);
        }
    }
}
// relu(acc + bias) -> sink(j, r32, w, q, g, v): lane (agent 32 j + r32, g) of output tile w holds units 32 w + 8 q + 4 g + 0..3 (bias: [256], natural order)
template <class Sink>
__device__ __forceinline__ void hidden_out(const f32x16 (&acc)[4], const float *bias, const Sink &sink) {
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 5, r32 = l & 31;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const f32x4 b = *(const f32x4 *)(bias + 32 * w + 8 * q + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const f32x4 v = {relu(acc[j][4 * q] + b[0]), relu(acc[j][4 * q + 1] + b[1]), relu(acc[j][4 * q + 2] + b[2]), relu(acc[j][4 * q + 3] + b[3])};
            sink(j, r32, w, q, g, v);
        }
    }
}
struct ToX {          // half `half` of x float[n][512], agents a0 .. of the workgroup; rows past n are not stored
    float *x;
    int a0, n, half;
    __device__ __forceinline__ void operator()(int j, int r32, int w, int q, int g, const f32x4 &v) const {
        if (a0 + 32 * j + r32 < n) *(f32x4 *)(x + (size_t)(a0 + 32 * j + r32) * 512 + 256 * half + 32 * w + 8 * q + 4 * g) = v;
    }
};
struct ToHid {        // the LDS image of one half of the hidden layer, [128 agents][64 units] (hid_slot)
    f32x4 *s_hid;
    __device__ __forceinline__ void operator()(int j, int r32, int w, int q, int g, const f32x4 &v) const { s_hid[hid_slot(32 * j + r32, 8 * w + 2 * q + g)] = v; }
};

// ---------------------------------------------------------------------------------------------------- the heads
// [32 outputs] x [32 agents] of one wave over K = 512: wh = the packed head ([64 groups][64 lanes]), l the lane, hp = the agent's row + g
// (group m at hp[2 m]); the operands of the next group load while the current one's four MFMAs run
__device__ __forceinline__ f32x16 head_gemm512(const f32x4 *wh, int l, const f32x4 *hp) {
    f32x16 acc = {0};
    f32x4 hw[2], hx[2];
    hw[0] = wh[l];
    hx[0] = hp[0];
    for (int m = 0; m < 64; m++) {
        if (m + 1 < 64) { hw[(m + 1) & 1] = wh[(m + 1) * 64 + l]; hx[(m + 1) & 1] = hp[2 * (m + 1)]; }
        acc = mfma4(hw[m & 1], hx[m & 1], acc);
    }
    return acc;
}
// The Q row of a lane pair and its action.  Lane (agent, g) holds outputs out_of(r, g) of h; its partner lane ^ 32 the other sixteen.
// dueling: outputs 0..n_action-1 are the advantage, output n_action the value, Q = h + shift_of(value, sum of the advantages) -- the shift
// is the caller's arithmetic; else Q = h.  The action is the argmax of the Q row itself in torch.argmax's order (q_before): a NaN anywhere
// in the network reaches the row, and then its first NaN is chosen, as the PyTorch path chooses it; every action lies in [0, n_action)
// whatever the input.  live lanes store the action (g == 0) and, if q, their outputs of the row.  Whole waves call this (shuffles).
template <class ShiftOf>
__device__ __forceinline__ void q_epilogue(const f32x16 &h, int g, int n_action, bool dueling, const ShiftOf &shift_of, bool live, int agent,
                                           int *actions, float *q) {
    float shift = 0.0f;
    if (dueling) {
        float sum = 0.0f, value = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int o = out_of(r, g);
            if (o < n_action) sum += h[r];
            if (o == n_action) value = h[r];
        }
        sum += __shfl_xor(sum, 32);
        value += __shfl_xor(value, 32);
        shift = shift_of(value, sum);
    }
    float best = -INFINITY;
    int arg = n_action;           // (not an action: every output of the row comes before it)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int o = out_of(r, g);
        if (o < n_action && q_before(h[r] + shift, o, best, arg)) { best = h[r] + shift; arg = o; }
    }
    const float obest = __shfl_xor(best, 32);
    const int oarg = __shfl_xor(arg, 32);
    if (q_before(obest, oarg, best, arg)) { best = obest; arg = oarg; }
    if (live) {
        if (g == 0) actions[agent] = arg;
        if (q) {
#pragma unroll
            for (int r = 0; r < 16; r++) { const int o = out_of(r, g); if (o < n_action) q[(size_t)agent * n_action + o] = h[r] + shift; }
        }
    }
}

// The probability row of a lane pair and its draw (k_a2c_head_f32, k_a2c_head_bf16).  Lane (agent, g) holds the outputs out_of(r, g) of acc
// = logits + bias (outputs 0..n_action-1) and the value (output n_action); its partner lane ^ 32 the other sixteen.  p = clamp(softmax
// with the row maximum subtracted, 1e-10, 1 - 1e-10); the row goes through `row` (POLICY_ROW_PITCH floats of LDS per agent, the lane
// pair's own) to the lane that holds the agent's action 0, which draws: c_0 = p_0, c_a = c_(a-1) + p_a, t = u c_(A-1), the smallest a with
// c_a > t, else A - 1.  live lanes store p (if policy), the value (if value) and the action.  EVERY wave of the workgroup calls this (a
// barrier stands between the row's stores and the draw).
constexpr int POLICY_ROW_PITCH = 33;
__device__ __forceinline__ void policy_epilogue(const f32x16 &acc, int g, int n_action, float *row, bool live, int agent, const float *u,
                                                int *actions, float *policy, float *value) {
    float top = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int o = out_of(r, g);
        if (o < n_action) top = fmaxf(top, acc[r]);            // (a NaN is passed over here and reaches the sum through its own exp)
    }
    top = fmaxf(top, __shfl_xor(top, 32));
    float e[16], sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int o = out_of(r, g);
        e[r] = o < n_action ? expf(acc[r] - top) : 0.0f;
        sum += e[r];
    }
    sum += __shfl_xor(sum, 32);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int o = out_of(r, g);
        float p = e[r] / sum;
        p = p < 1e-10f ? 1e-10f : (p > (float)(1.0 - 1e-10) ? (float)(1.0 - 1e-10) : p);      // torch.clamp: a NaN stays
        if (o < n_action) {
            row[o] = p;
            if (live && policy) policy[(size_t)agent * n_action + o] = p;
        }
        if (o == n_action && live && value) value[agent] = acc[r];
    }
    __syncthreads();
    if (g == 0 && live) {
        float c = row[0];
        for (int a = 1; a < n_action; a++) c += row[a];
        const float t = u[agent] * c;
        int act = n_action - 1;                                // (no c_a > t: rounding, or a NaN in the row)
        c = row[0];
        for (int a = 0; a < n_action - 1; a++) {
            if (c > t) { act = a; break; }
            c += row[a + 1];
        }
        actions[agent] = act;
    }
}

// ---------------------------------------------------------------------------------------------------- streamed rows
// NC chunks of operands through two register buffers: the next chunk loads while the current one's MFMAs run (NC even)
template <int NC, class Buf, class Load, class Run>
__device__ __forceinline__ void pingpong(Buf (&op)[2], const Load &load, const Run &run) {
    load(0, op[0]);
    for (int c = 0; c < NC; c += 2) {
        load(c + 1, op[1]);
        run(op[0]);
        if (c + 2 < NC) load(c + 2, op[0]);
        run(op[1]);
    }
}

// ---------------------------------------------------------------------------------------------------- the DRQN's id table
// The state row (`pitch` floats) of agent `id`: the row of the LAST entry equal to id of the previous call's ids sorted stably (binary
// search; duplicates -- the dict's last occurrence), or null if there is none (the agent starts from zeros).
__device__ __forceinline__ const float *state_row(int id, const int *prev_ids, const int *rows, int count, const float *states, int pitch) {
    int lo = 0, hi = count;                                      // lo: the first entry above id
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prev_ids[mid] <= id) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && prev_ids[lo - 1] == id ? states + (size_t)rows[lo - 1] * pitch : nullptr;
}

// The segmented call's table (policy_drqn_lookup_seg*): the key of agent `id` of segment `seg` is (seg << 32) | uint32(id) -- every world
// of a packed batch numbers its agents from 0, the segment keeps them apart.  A row in no segment (a pad row, a stale row) takes
// DRQN_NO_KEY, which no look-up produces (segment 2^31 - 1 is refused) and which sorts behind every key: such rows stay in the table,
// at its end, and nobody finds them.
constexpr long long DRQN_NO_KEY = 0x7FFFFFFFFFFFFFFFLL;
__device__ __forceinline__ long long drqn_key(int seg, int id) { return (long long)(((unsigned long long)(unsigned)seg << 32) | (unsigned)id); }
// state_row's search on the 64-bit keys: the row of `states` of the LAST entry of prev_keys (ascending; equal keys in that call's order)
// equal to key, or -1
__device__ __forceinline__ int state_row_of_key(long long key, const long long *prev_keys, const int *rows, int count) {
    int lo = 0, hi = count;                                      // lo: the first entry above key
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prev_keys[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && prev_keys[lo - 1] == key ? rows[lo - 1] : -1;
}
// One row of the look-up launch: its segment is the last one that begins at or in front of it, if the row is inside it (the table
// ascends without overlap: an empty segment in front of it with the same begin is passed over).  from_row[r]: the row of the previous
// call's states that holds this agent's state, -1 for an agent the table does not know and for a row in no segment; keys[r]: its key in
// THIS call's table.  seg_first: the number of the table's segment 0 among the call's segments (a call of more than A2C_MAX_SEGMENTS
// segments goes through several look-ups).
__device__ __forceinline__ void drqn_lookup_row(int r, const int *ids, const A2cSegTable &t, int seg_first, const long long *prev_keys,
                                                const int *rows, int count, int *from_row, long long *keys) {
    int lo = 0, hi = t.n_seg;                                    // lo: the first segment that begins behind r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t.begin[mid] <= r) lo = mid + 1;
        else hi = mid;
    }
    const int s = lo - 1;
    if (s < 0 || r >= t.begin[s] + t.count[s]) {
        from_row[r] = -1;
        keys[r] = DRQN_NO_KEY;
        return;
    }
    const long long key = drqn_key(seg_first + s, ids[r]);
    from_row[r] = state_row_of_key(key, prev_keys, rows, count);
    keys[r] = key;
}

// ---------------------------------------------------------------------------------------------------- column sums in a fixed order
// Workgroups of A2C_HID threads, thread c = column c.  colsum_rows: rows beg .. end - 1 of h [n][A2C_HID] (an element as float32: row_f32
// of its type) added in row order into row `part_row` of part -- the plain call's block b: agents A2C_CS_BLOCK b .. + A2C_CS_BLOCK - 1,
// a segmented call's: see below; colsum_blocks: one workgroup adds the blocks in block order.
__device__ __forceinline__ float row_f32(float v) { return v; }
__device__ __forceinline__ float row_f32(unsigned short v) { return __uint_as_float((unsigned)v << 16); }      // a stored bf16 value
template <class Row>
__device__ __forceinline__ void colsum_rows(const Row *h, int beg, int end, float *part, int part_row) {
    const int c = threadIdx.x;
    float s = 0.0f;
#pragma unroll 16
    for (int a = beg; a < end; a++) s += row_f32(h[(size_t)a * A2C_HID + c]);
    part[(size_t)part_row * A2C_HID + c] = s;
}
__device__ __forceinline__ void colsum_blocks(const float *part, int n_blocks, float *sum) {
    const int c = threadIdx.x;
    float s = 0.0f;
#pragma unroll 32
    for (int b = 0; b < n_blocks; b++) s += part[(size_t)b * A2C_HID + c];
    sum[c] = s;
}

// The same sums per segment of a segmented call (A2cSegTable above; policy_host.h: a2c_layout).  Segment s is cut into blocks of
// A2C_CS_BLOCK agents counted from ITS first row; a block is added in agent order, a segment's blocks in block order: the partition and
// the order of the plain call's blocks on that segment alone, so the sums have that call's bits.
// seg_map: workgroup s (of max(n_seg, 1), any size) writes segment s's entry of seg_tab, its blocks' entries of blk_map, and row_seg of
// the segment's rows and of the rows between it and the next segment (-1; workgroup 0 also the rows in front of the first segment).
__device__ __forceinline__ void seg_map(const A2cSegTable &t, int n, int *row_seg, int *seg_tab, int *blk_map) {
    const int s = blockIdx.x, tid = threadIdx.x, step = blockDim.x;
    if (t.n_seg == 0) {
        for (int r = tid; r < n; r += step) row_seg[r] = -1;
        return;
    }
    const int beg = t.begin[s], cnt = t.count[s], nblk = (cnt + A2C_CS_BLOCK - 1) / A2C_CS_BLOCK;
    const int next = s + 1 < t.n_seg ? t.begin[s + 1] : n;
    int blk0 = 0;
    for (int k = 0; k < s; k++) blk0 += (t.count[k] + A2C_CS_BLOCK - 1) / A2C_CS_BLOCK;
    if (tid == 0) {
        seg_tab[4 * s] = beg; seg_tab[4 * s + 1] = cnt; seg_tab[4 * s + 2] = blk0; seg_tab[4 * s + 3] = nblk;
    }
    for (int b = tid; b < nblk; b += step) { blk_map[2 * (blk0 + b)] = s; blk_map[2 * (blk0 + b) + 1] = b; }
    for (int r = (s == 0 ? 0 : beg) + tid; r < next; r += step) row_seg[r] = (r >= beg && r < beg + cnt) ? s : -1;
}
// workgroup b of sum over s of ceil(count_s / A2C_CS_BLOCK): the partial row of block blk_map[b]
template <class Row>
__device__ __forceinline__ void colsum_part_seg(const Row *h, const int *seg_tab, const int *blk_map, float *part) {
    const int s = blk_map[2 * blockIdx.x], beg = seg_tab[4 * s] + blk_map[2 * blockIdx.x + 1] * A2C_CS_BLOCK;
    colsum_rows(h, beg, min(beg + A2C_CS_BLOCK, seg_tab[4 * s] + seg_tab[4 * s + 1]), part, blockIdx.x);
}
// workgroup s: segment s's blocks in block order -> sum[s][A2C_HID] (an empty segment: zeros, never read)
__device__ __forceinline__ void colsum_blocks_seg(const float *part, const int *seg_tab, float *sum) {
    const int s = blockIdx.x;
    colsum_blocks(part + (size_t)seg_tab[4 * s + 2] * A2C_HID, seg_tab[4 * s + 3], sum + (size_t)s * A2C_HID);
}
// what a lane of the segmented CommNet layer takes from its agent's segment: the sum row, the divisor count - 1 and whether the agent is
// alone (count == 1, or a row in no segment: row_seg < 0 -- then the sum row is segment 0's, loaded and not used)
struct SegOfRow { int sum_row; float others_div; bool alone; };
__device__ __forceinline__ SegOfRow seg_of_row(const int *row_seg, const int *seg_tab, int agent) {
    const int s = row_seg[agent];
    if (s < 0) return SegOfRow{0, 1.0f, true};
    const int cnt = seg_tab[4 * s + 1];
    return SegOfRow{s, (float)(cnt - 1), cnt == 1};
}

// The DQN's trunk for the DRQN: k_dqn_conv_f32, then k_dqn_head_f32 stopped after its hidden layer, which it stores as
// x float[n][512] = relu(dense_view) || relu(dense_emb), natural unit order, one 2 KB row per agent.  `w->head` and `w->value_bias` are
// not read.  act_workspace: policy_dqn_f32_act_bytes(s, n).  Enqueues two kernels on `stream`; 0, or non-zero as policy_dqn_infer_f32.
int dqn_f32_trunk(const PolicyDqnShape *s, const PolicyDqnWeightsF32 *w, const float *view, const float *feat, int n, void *act_workspace,
                  float *x, void *stream);

}  // namespace f32
}  // namespace magent_amd
