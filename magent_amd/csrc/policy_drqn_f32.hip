// policy_drqn_f32.hip -- the deep recurrent Q network's acting step (magent_amd/builtin/torch_model/drqn.py: _RecurrentQNet.forward with
// one step per agent), inference only, in float32 on v_mfma_f32_32x32x2_f32, with the recurrent state of every agent id kept in HBM.
//
//   network:  the DQN's trunk (policy_f32.hip: conv3x3 relu -> conv3x3 relu -> dense 256 relu || dense 256 relu on the features) -> x [512]
//             GRU cell (torch.nn.GRU, gates r, z, n):  r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)
//                                                      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//                                                      n = tanh(W_in x + b_in + r * (W_hn h + b_hn))
//                                                      h' = (1 - z) * n + z * h
//             head over h': dueling  Q = value(h') + adv(h') - mean(adv(h'))  (advantage without bias), or  Q = value(h')  (n_action outputs)
//
// Operands and fragments as in policy_f32.hip: A = weights (lane l: output l & 31), B = activations (lane l: agent l & 31), a lane group g
// reads values 4 g .. 4 g + 3 of a group of 8 K-values as one float4 that feeds four MFMAs; a result lane (agent, g) holds outputs
// 8 q + 4 g + 0..3 of its 32-wide tile, natural order.
//
// k_dqn_conv_f32 + k_dqn_head_f32<true> (policy_f32_dev.h: dqn_f32_trunk): x as float[n][512], one 2 KB row per agent.
// k_drqn_gru_f32 : [n agents] x [3 x 512 gate outputs] over K = 512 (x) + 512 (h).  A wave owns 32 agents x 32 hidden units (tile T) and
//   four accumulators: r and z over all of K, n_x over x, n_h over h (r multiplies n_h alone) -- 64 VGPRs.  The packed weights put the
//   three gate tiles of a hidden tile side by side ([K / 8][16 tiles][3 gates][64 lanes]): per group of 8 K-values a lane loads its
//   activation float4 and three weight float4, which feed 12 MFMAs (768 cycles); operands of the next four groups load while the
//   current four's 48 MFMAs run (policy_f32_dev.h: pingpong, shared with k_a2c_layer_f32).  A workgroup is 8 waves = 256 agents on ONE hidden tile, so its waves read the same weights (L1/L2) and
//   the x rows of an agent group are read by the 16 hidden tiles' workgroups (L2).  The gates are applied in registers and h' goes
//   straight to the new state table.
//   The previous state of an agent is the row of the previous call whose id is the LAST equal entry of that call's ids sorted stably
//   (policy_f32_dev.h: state_row, the bf16 kernel's too -- binary search: duplicates, the dict's last occurrence); an id not found starts from zeros.  With an empty table the <false>
//   variant skips the h half and takes the biases of a zero state (W_h 0 + b_h, which the host computes: NaN where W_h holds a
//   non-finite weight, as torch's W_h @ 0).
// k_drqn_head_f32 : [32 outputs] x [32 agents] per wave over K = 512 state units (policy_f32_dev.h: head_gemm512, shared with
//   k_a2c_head_f32), then the dueling combination and torch.argmax's order (q_epilogue, shared with k_dqn_head_f32).
//
// NaN contract: nothing launders a NaN -- sigmoid is 1 / (1 + exp(-v)), tanhf, relu is IEEE maximum; a NaN anywhere in an
// agent's inputs or state reaches its Q row and its new state, and its action is the first NaN of that row, as the PyTorch path's argmax.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/magent_policy.h"
#include "policy_f32_dev.h"
#include "policy_host.h"

namespace {

using namespace magent_amd::f32;      // the vector types, mfma4, and the shared blocks: pingpong, head_gemm512, q_epilogue, sigmoid

constexpr int STATE = 512, GRU_TILES = STATE / 32;
constexpr int GRU_WAVES = 8, GRU_THREADS = 64 * GRU_WAVES, GRU_CHUNK = 4;     // groups of 8 K-values a wave has in flight per buffer
constexpr int QH_WAVES = 4, QH_THREADS = 64 * QH_WAVES;

struct GruArgs {
    const float *x;           // [n][512] the trunk's hidden layer
    const int *ids;           // [n] this call's agent ids
    const int *prev_ids;      // [count] the previous call's ids, ascending (equal ids in that call's order)
    const int *rows;          // [count] their rows of `states`
    const float *states;      // [.][512] the previous call's output states
    const int *from_row;      // [n] or null; not null (the *_rows entry): agent i's row of `states`, < 0 none -- ids, prev_ids, rows are not read
    int count, n;
    const f32x4 *w;           // [128 groups][16 tiles][3 gates][64]: K = x's 512, then h's 512; gates r, z, n
    const float *bias;        // [4][512] b_ir + b_hr, b_iz + b_hz, b_in, b_hn
    float *out;               // [n][512] h'
};

template <bool HAS_H>
__global__ void __launch_bounds__(GRU_THREADS) k_drqn_gru_f32(GruArgs A) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    const int tile0 = (blockIdx.x * GRU_WAVES + w) * 32;
    if (tile0 >= A.n) return;                                    // (whole waves: the MFMAs below see every lane)
    const int T = blockIdx.y;
    const int agent = min(tile0 + r32, A.n - 1);
    const float *hrow = nullptr;
    if (HAS_H) {
        if (A.from_row) {                                        // (uniform: the look-up ran in its own launch, policy_drqn_lookup_seg_f32)
            const int row = A.from_row[agent];
            hrow = row >= 0 ? A.states + (size_t)row * STATE : nullptr;
        } else hrow = state_row(A.ids[agent], A.prev_ids, A.rows, A.count, A.states, STATE);
    }
    const bool have = hrow != nullptr;
    const f32x4 *xp = (const f32x4 *)(A.x + (size_t)agent * STATE) + g;       // group m: xp[2 m] = x[8 m + 4 g .. + 3]
    const f32x4 *hp = have ? (const f32x4 *)hrow + g : xp;                    // (a lane without a state reads x and takes zeros)
    const f32x4 *wp = A.w + (size_t)T * 3 * 64 + l;                           // (group m, gate) at wp[(m * 48 + gate) * 64]
    f32x16 ar = {0}, az = {0}, anx = {0}, anh = {0};
    f32x4 op[2][GRU_CHUNK][4];                                                // [buffer][group][activation, w_r, w_z, w_n]
    auto phase = [&](auto is_h) __attribute__((always_inline)) {
        constexpr bool H = decltype(is_h)::value;
        const f32x4 *src = H ? hp : xp;
        const f32x4 *wph = wp + (H ? (size_t)64 * 48 * 64 : 0);
        auto load = [&](int c, f32x4 (&d)[GRU_CHUNK][4]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < GRU_CHUNK; j++) {
                const int m = c * GRU_CHUNK + j;
                const f32x4 v = src[2 * m];
                d[j][0] = (!H || have) ? v : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int gate = 0; gate < 3; gate++) d[j][1 + gate] = wph[((size_t)m * 48 + gate) * 64];
            }
        };
        auto run = [&](const f32x4 (&d)[GRU_CHUNK][4]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < GRU_CHUNK; j++) {
                ar = mfma4(d[j][1], d[j][0], ar);
                az = mfma4(d[j][2], d[j][0], az);
                if (H) anh = mfma4(d[j][3], d[j][0], anh);
                else anx = mfma4(d[j][3], d[j][0], anx);
            }
        };
        pingpong<64 / GRU_CHUNK>(op, load, run);
    };
    phase(std::integral_constant<bool, false>{});
    if (HAS_H) phase(std::integral_constant<bool, true>{});
    // the gates, in registers: lane (agent, g) holds units u = 32 T + 8 q + 4 g + i in result register 4 q + i
    const bool live = tile0 + r32 < A.n;
    float *orow = A.out + (size_t)agent * STATE + 32 * T + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int u = 32 * T + 8 * q + 4 * g;
        const f32x4 br = *(const f32x4 *)(A.bias + u), bz = *(const f32x4 *)(A.bias + STATE + u);
        const f32x4 bn = *(const f32x4 *)(A.bias + 2 * STATE + u), bhn = *(const f32x4 *)(A.bias + 3 * STATE + u);
        f32x4 hold = {0.0f, 0.0f, 0.0f, 0.0f};
        if (HAS_H && have) hold = *(const f32x4 *)(hrow + u);
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = 4 * q + i;
            const float rg = sigmoid(ar[r] + br[i]);
            const float zg = sigmoid(az[r] + bz[i]);
            const float ng = tanhf(anx[r] + bn[i] + rg * (anh[r] + bhn[i]));
            o[i] = (1.0f - zg) * ng + zg * hold[i];
        }
        if (live) *(f32x4 *)(orow + 8 * q) = o;
    }
}

struct QHeadArgs {
    const float *h;           // [n][512] h'
    const f32x4 *wh;          // [64][64]: K = 512 state units; dueling: outputs 0..n_action-1 advantage, n_action value; else value's n_action
    const float *bh;          // [32] per-output biases (dueling: the value's at n_action, zeros elsewhere)
    int n, n_action, dueling;
    int *actions;             // [n]
    float *q;                 // [n][n_action] or null
};

__global__ void __launch_bounds__(QH_THREADS) k_drqn_head_f32(QHeadArgs A) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    const int tile0 = (blockIdx.x * QH_WAVES + w) * 32;
    if (tile0 >= A.n) return;
    const int agent = min(tile0 + r32, A.n - 1);
    f32x16 acc = head_gemm512(A.wh, l, (const f32x4 *)(A.h + (size_t)agent * STATE) + g);
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] += A.bh[out_of(r, g)];
    // Q = acc + value - mean(advantage) (dueling) or acc, the argmax and the stores: q_epilogue
    q_epilogue(acc, g, A.n_action, A.dueling != 0, [&](float value, float sum) { return value - sum / (float)A.n_action; },
               tile0 + r32 < A.n, agent, A.actions, A.q);
}

static size_t x_offset(const PolicyDqnShape *s, int n) { return magent_amd::drqn_x_offset(policy_dqn_f32_act_bytes, s, n); }      // policy_host.h

}  // namespace

extern "C" {

int policy_drqn_f32_supported(const PolicyDqnShape *s) { return policy_dqn_f32_supported(s); }

int policy_drqn_f32_workspace_bytes(const PolicyDqnShape *s, int n, size_t *bytes) {
    n = n < 0 ? 0 : n;
    *bytes = x_offset(s, n) + (size_t)n * STATE * sizeof(float);
    return 0;
}

}  // extern "C"

namespace {

// Both entries behind their argument checks.  The state of agent i: the id table's look-up (from_row null; count == 0: an empty table),
// or row from_row[i] of `states` (the *_rows entry; states null: an empty table).
int drqn_infer_f32(const PolicyDqnShape *s, const PolicyDrqnWeightsF32 *w, const float *view, const float *feat, int n, const int *ids,
                   const int *prev_sorted_ids, const int *rows, const int *from_row, const float *states, int count, float *new_states,
                   void *workspace, int *actions, float *q, void *stream) {
    const bool has_h = from_row ? states != nullptr : count > 0;
    if (((uintptr_t)new_states | (uintptr_t)states | (uintptr_t)workspace) & 15) return 1;      // (rows are read and written as float4)
    float *x = (float *)((char *)workspace + x_offset(s, n));
    int rc = magent_amd::f32::dqn_f32_trunk(s, &w->trunk, view, feat, n, workspace, x, stream);
    if (rc != 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    magent_amd::StreamDevice on(st);
    if (!on.ok) return 2;
    GruArgs G{};
    G.x = x; G.ids = ids; G.prev_ids = prev_sorted_ids; G.rows = rows; G.states = states; G.from_row = from_row; G.count = count; G.n = n;
    G.w = (const f32x4 *)w->gru; G.bias = has_h ? w->gru_bias : w->gru_bias0; G.out = new_states;
    const dim3 ggrid((n + 32 * GRU_WAVES - 1) / (32 * GRU_WAVES), GRU_TILES);
    if (has_h) hipLaunchKernelGGL(k_drqn_gru_f32<true>, ggrid, dim3(GRU_THREADS), 0, st, G);
    else hipLaunchKernelGGL(k_drqn_gru_f32<false>, ggrid, dim3(GRU_THREADS), 0, st, G);
    QHeadArgs Q{};
    Q.h = new_states; Q.wh = (const f32x4 *)w->head; Q.bh = w->head_bias; Q.n = n; Q.n_action = s->n_action; Q.dueling = w->dueling != 0;
    Q.actions = actions; Q.q = q;
    hipLaunchKernelGGL(k_drqn_head_f32, dim3((n + 32 * QH_WAVES - 1) / (32 * QH_WAVES)), dim3(QH_THREADS), 0, st, Q);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

struct LookupF32;         // (the tag of this file family's copy of k_drqn_lookup_seg)

}  // namespace

extern "C" {

int policy_drqn_infer_f32(const PolicyDqnShape *s, const PolicyDrqnWeightsF32 *w, const float *view, const float *feat, int n, const int *ids,
                          const int *prev_sorted_ids, const int *rows, const float *states, int count, float *new_states, void *workspace,
                          int *actions, float *q, void *stream) {
    if (!policy_drqn_f32_supported(s) || count < 0 || (count > 0 && !(prev_sorted_ids && rows && states))) return 1;
    if (n <= 0) return 0;
    if (!ids || !new_states || !actions || !workspace) return 1;
    return drqn_infer_f32(s, w, view, feat, n, ids, prev_sorted_ids, rows, nullptr, states, count, new_states, workspace, actions, q, stream);
}

int policy_drqn_lookup_seg_f32(const int *ids, int n, const int *seg_begin, const int *seg_count, int n_seg, int seg_first,
                               const long long *prev_sorted_keys, const int *rows, int count, int *from_row, long long *keys, void *stream) {
    return magent_amd::drqn_lookup_seg<LookupF32>(ids, n, seg_begin, seg_count, n_seg, seg_first, prev_sorted_keys, rows, count, from_row, keys, stream);
}

int policy_drqn_infer_f32_rows(const PolicyDqnShape *s, const PolicyDrqnWeightsF32 *w, const float *view, const float *feat, int n,
                               const int *from_row, const float *states, float *new_states, void *workspace, int *actions, float *q, void *stream) {
    if (!policy_drqn_f32_supported(s)) return 1;
    if (n <= 0) return 0;
    if (!from_row || !new_states || !actions || !workspace) return 1;
    return drqn_infer_f32(s, w, view, feat, n, nullptr, nullptr, nullptr, from_row, states, 0, new_states, workspace, actions, q, stream);
}

}  // extern "C"
