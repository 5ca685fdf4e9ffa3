// policy_drqn_bf16.hip -- the deep recurrent Q network's acting step (magent_amd/builtin/torch_model/drqn.py: _RecurrentQNet.forward with
// one step per agent), inference only, with bf16 matrix operands on v_mfma_f32_32x32x16_bf16: the opt-in sibling of policy_drqn_f32.hip,
// as policy.hip is of policy_f32.hip.  The recurrent state of every agent id stays FLOAT32 in HBM, in the f32 path's own table format.
//
//   network:  the DQN's bf16 trunk (policy.hip: k_dqn_conv, then k_dqn_head<., true>, which stops after the hidden layer) -> x [512] bf16
//             GRU cell (torch.nn.GRU, gates r, z, n):  r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)
//                                                      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//                                                      n = tanh(W_in x + b_in + r * (W_hn h + b_hn))
//                                                      h' = (1 - z) * n + z * h
//             head over h': dueling  Q = value(h') + adv(h') - mean(adv(h'))  (advantage without bias), or  Q = value(h')  (n_action outputs)
//   rounding: to bf16 (nearest even) -- the views, the features, every weight matrix, conv1's bias (it rides in the MFMA), the two conv
//             outputs, the two hidden halves (x), h AS THE GRU's OPERAND and h' AS THE HEAD's OPERAND.  Nothing else: products accumulate in
//             float32, the other biases, the gates (policy_f32_dev.h: sigmoid; tanhf) and the blend are float32, and the blend's z * h takes
//             the UNROUNDED float32 h of the table.  h' is stored as float32: bf16 error does not compound through the blend from call to
//             call, and a model can move between this path and the f32 one with its states.
//
// Operands: A = weights in fragment order (lane l: output l & 31, k = 8 (l >> 5) + 0..7 of a 16-wide k-step), B = activations (lane l: agent
// l & 31, the same eight k); a result lane (agent, g = l >> 5) holds outputs 8 q + 4 g + 0..3 of its 32-wide tile (policy_f32_dev.h: out_of).
//
// k_drqn_gru_bf16 : [n agents] x [3 x 512 gate outputs] over K = 512 (x, hidden slot order) + 512 (h).  A wave owns 32 agents x 32 hidden units
//   (tile T) and the f32 kernel's four accumulators: r and z over all of K, n_x over x, n_h over h -- 64 VGPRs.  The packed weights put the
//   three gate tiles of a hidden tile side by side ([64 k-steps][16 tiles][3 gates][64 lanes] x 16 bytes): per k-step a lane loads its
//   activation (16 bytes of x; 32 bytes of float32 h, rounded in registers on their way into the MFMA) and three weight fragments, which
//   feed 3 MFMAs; operands are requested four k-steps (12 MFMAs) ahead of their use, two k-steps at a time (ring3).
//   Work split: a workgroup is 8 waves = 256 agents on ONE hidden tile (its waves read the same 192 KB of weights through one L1); the 16
//   tiles of an agent group are 16 workgroups dealt to the SAME XCD (workgroups go round-robin over the 8 XCDs), one after another: every
//   L2 then holds the whole 3 MB of weights and fetches an agent group's x and h rows once for its 16 readers.
//   The placement is policy_bf16_dev.h: xcd_place / xcd_grid, shared with the A2C's two GEMM kernels.
//   State look-up as k_drqn_gru_f32 (policy_f32_dev.h: state_row): the LAST entry of the stably sorted previous ids equal to the agent's
//   id, zeros if there is none; with an empty table the <false> variant skips the h half and takes gru_bias0.
// k_drqn_head_bf16 : [32 outputs] x [32 agents] per wave over K = 512 state units (policy_bf16_dev.h: head_gemm512_bf16, shared with
//   k_a2c_head_bf16; h' rounded as the operand), float32 biases, then the dueling combination and torch.argmax's order
//   (policy_f32_dev.h: q_epilogue, the f32 heads' own).
//
// Whole waves exit early; lanes past n repeat the last agent (their own columns of the MFMA, never stored).  NaN contract:
// a NaN or Inf in an agent's inputs or state stays in that agent's MFMA column: it reaches its Q row and its new state and no other agent's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/magent_policy.h"
#include "policy_bf16_dev.h"
#include "policy_f32_dev.h"
#include "policy_host.h"

namespace {

using namespace magent_amd::bf16;         // the vector types, the conversions, xcd_place / xcd_grid, ring3, head_gemm512_bf16
using magent_amd::f32::q_epilogue;
using magent_amd::f32::out_of;
using magent_amd::f32::sigmoid;
using magent_amd::f32::state_row;

constexpr int STATE = 512, GRU_TILES = STATE / 32, KSTEPS = STATE / 16;
constexpr int GRU_WAVES = 8, GRU_THREADS = 64 * GRU_WAVES, GRU_CHUNK = 2;     // k-steps per register buffer; a wave has three buffers (ring3)
constexpr int QH_WAVES = 4, QH_THREADS = 64 * QH_WAVES;

struct GruArgs {
    const bf16x8 *x;          // [n][64 units of 8]: the trunk's hidden layer, slot order
    const int *ids;           // [n] this call's agent ids
    const int *prev_ids;      // [count] the previous call's ids, ascending (equal ids in that call's order)
    const int *rows;          // [count] their rows of `states`
    const float *states;      // [.][512] the previous call's output states, float32
    const int *from_row;      // [n] or null; not null (the *_rows entries): agent i's row of `states`, < 0 none -- ids, prev_ids, rows are not read
    int count, n, groups;     // groups: agent groups of 32 GRU_WAVES
    const bf16x8 *w;          // [64 k-steps][16 tiles][3 gates][64]: K = x's 512 slots, then h's 512 units; gates r, z, n
    const float *bias;        // [4][512] b_ir + b_hr, b_iz + b_hz, b_in, b_hn
    float *out;               // [n][512] h', float32
};

struct XOp { bf16x8 a, w[3]; };            // one k-step of the x half: the operand as stored
struct HOp { f32x4 a[2]; bf16x8 w[3]; };   // one k-step of the h half: eight float32 of the state, rounded when they are used

template <bool HAS_H>
__global__ void __launch_bounds__(GRU_THREADS) k_drqn_gru_bf16(GruArgs A) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    int T, group;                                                // (policy_bf16_dev.h: the 16 tiles of an agent group on one XCD)
    xcd_place(GRU_TILES, T, group);
    const int tile0 = (group * GRU_WAVES + w) * 32;
    if (group >= A.groups || tile0 >= A.n) return;               // (whole waves: the MFMAs below see every lane)
    const int agent = min(tile0 + r32, A.n - 1);
    const float *hrow = nullptr;
    if (HAS_H) {
        if (A.from_row) {                                        // (uniform: the look-up ran in its own launch, policy_drqn_lookup_seg)
            const int row = A.from_row[agent];
            hrow = row >= 0 ? A.states + (size_t)row * STATE : nullptr;
        } else hrow = state_row(A.ids[agent], A.prev_ids, A.rows, A.count, A.states, STATE);
    }
    const bool have = hrow != nullptr;
    const bf16x8 *xp = A.x + (size_t)agent * (STATE / 8) + g;                 // k-step s: xp[2 s] = x[16 s + 8 g .. + 7]
    const f32x4 *hp = have ? (const f32x4 *)hrow + 2 * g : (const f32x4 *)xp; // k-step s: hp[4 s], hp[4 s + 1] = h[16 s + 8 g .. + 7]
    const int hstep = have ? 4 : 0;                                           // (a lane without a state re-reads one address and takes zeros)
    const bf16x8 *wp = A.w + (size_t)T * 3 * 64 + l;                          // (k-step s, gate) at wp[(s * 48 + gate) * 64]
    f32x16 ar = {0}, az = {0}, anx = {0}, anh = {0};
    {
        XOp op[3][GRU_CHUNK];
        auto load = [&](int c, XOp (&d)[GRU_CHUNK]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < GRU_CHUNK; k++) {
                const int s = c * GRU_CHUNK + k;
                d[k].a = xp[2 * s];
#pragma unroll
                for (int gate = 0; gate < 3; gate++) d[k].w[gate] = wp[((size_t)s * 48 + gate) * 64];
            }
        };
        auto run = [&](const XOp (&d)[GRU_CHUNK]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < GRU_CHUNK; k++) {
                ar = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[k].w[0], d[k].a, ar, 0, 0, 0);
                az = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[k].w[1], d[k].a, az, 0, 0, 0);
                anx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[k].w[2], d[k].a, anx, 0, 0, 0);
            }
        };
        ring3<KSTEPS / GRU_CHUNK>(op, load, run);
    }
    if (HAS_H) {
        HOp op[3][GRU_CHUNK];
        const bf16x8 *wph = wp + (size_t)KSTEPS * 48 * 64;
        auto load = [&](int c, HOp (&d)[GRU_CHUNK]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < GRU_CHUNK; k++) {
                const int s = c * GRU_CHUNK + k;
                d[k].a[0] = hp[hstep * s];
                d[k].a[1] = hp[hstep * s + 1];
#pragma unroll
                for (int gate = 0; gate < 3; gate++) d[k].w[gate] = wph[((size_t)s * 48 + gate) * 64];
            }
        };
        auto run = [&](const HOp (&d)[GRU_CHUNK]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < GRU_CHUNK; k++) {
                const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
                const bf16x8 hb = round_bf16x8(have ? d[k].a[0] : zero, have ? d[k].a[1] : zero);
                ar = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[k].w[0], hb, ar, 0, 0, 0);
                az = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[k].w[1], hb, az, 0, 0, 0);
                anh = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[k].w[2], hb, anh, 0, 0, 0);
            }
        };
        ring3<KSTEPS / GRU_CHUNK>(op, load, run);
    }
    // the gates, in registers, float32: lane (agent, g) holds units u = 32 T + 8 q + 4 g + i in result register 4 q + i
    const bool live = tile0 + r32 < A.n;
    float *orow = A.out + (size_t)agent * STATE + 32 * T + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int u = 32 * T + 8 * q + 4 * g;
        const f32x4 br = *(const f32x4 *)(A.bias + u), bz = *(const f32x4 *)(A.bias + STATE + u);
        const f32x4 bn = *(const f32x4 *)(A.bias + 2 * STATE + u), bhn = *(const f32x4 *)(A.bias + 3 * STATE + u);
        f32x4 hold = {0.0f, 0.0f, 0.0f, 0.0f};
        if (HAS_H && have) hold = *(const f32x4 *)(hrow + u);        // the table's float32 h, unrounded
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
    const float *h;           // [n][512] h', float32
    const bf16x8 *wh;         // [32 k-steps][64]: K = 512 state units; dueling: outputs 0..n_action-1 advantage, n_action value; else value's n_action
    const float *bh;          // [32] per-output biases (dueling: the value's at n_action, zeros elsewhere)
    int n, n_action, dueling;
    int *actions;             // [n]
    float *q;                 // [n][n_action] or null
};

__global__ void __launch_bounds__(QH_THREADS) k_drqn_head_bf16(QHeadArgs A) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    const int tile0 = (blockIdx.x * QH_WAVES + w) * 32;
    if (tile0 >= A.n) return;
    const int agent = min(tile0 + r32, A.n - 1);
    const f32x4 *hp = (const f32x4 *)(A.h + (size_t)agent * STATE) + 2 * g;       // k-step s: hp[4 s], hp[4 s + 1]
    f32x16 acc = head_gemm512_bf16(A.wh, l, [&](int s) { return F8{{hp[4 * s], hp[4 * s + 1]}}; }, [](const F8 &v) { return round_bf16x8(v); });
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] += A.bh[out_of(r, g)];
    // Q = acc + value - mean(advantage) (dueling) or acc, the argmax and the stores: q_epilogue
    q_epilogue(acc, g, A.n_action, A.dueling != 0, [&](float value, float sum) { return value - sum / (float)A.n_action; },
               tile0 + r32 < A.n, agent, A.actions, A.q);
}

static size_t x_offset(const PolicyDqnShape *s, int n) { return magent_amd::drqn_x_offset(policy_dqn_act_bytes, s, n); }      // policy_host.h
struct LookupBf16;        // (the tag of this file family's copy of k_drqn_lookup_seg)

// All five entries.  The state of agent i: the id table's look-up (from_row null; count == 0: an empty table), or row from_row[i] of
// `states` (rows_form, the *_rows entries; states null: an empty table).
static int drqn_infer(const PolicyDqnShape *s, const PolicyDrqnWeights *w, const void *view_any, bool cells16, const float *feat, int n,
                      const int *ids, const int *prev_sorted_ids, const int *rows, bool rows_form, const int *from_row, const float *states,
                      int count, float *new_states, void *workspace, int *actions, float *q, void *stream) {
    if (!policy_drqn_supported(s)) return 1;
    if (!rows_form && (count < 0 || (count > 0 && !(prev_sorted_ids && rows && states)))) return 1;
    if (n <= 0) return 0;
    if (!view_any || !feat || !(rows_form ? (const void *)from_row : (const void *)ids) || !new_states || !actions || !workspace) return 1;
    const bool has_h = rows_form ? states != nullptr : count > 0;
    if (((uintptr_t)new_states | (uintptr_t)states | (uintptr_t)workspace) & 15) return 1;      // (rows are read and written as float4)
    if (cells16 && ((uintptr_t)view_any & 15)) return 1;                                         // (a cell is one 16-byte load)
    void *x = (char *)workspace + x_offset(s, n);
    int rc = magent_amd::bf16::dqn_trunk(s, &w->trunk, view_any, cells16, feat, n, workspace, x, stream);
    if (rc != 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    magent_amd::StreamDevice on(st);
    if (!on.ok) return 2;
    GruArgs G{};
    G.x = (const bf16x8 *)x; G.ids = ids; G.prev_ids = prev_sorted_ids; G.rows = rows; G.states = states; G.from_row = rows_form ? from_row : nullptr;
    G.count = count; G.n = n;
    G.groups = (n + 32 * GRU_WAVES - 1) / (32 * GRU_WAVES);
    G.w = (const bf16x8 *)w->gru; G.bias = has_h ? w->gru_bias : w->gru_bias0; G.out = new_states;
    const dim3 ggrid(xcd_grid(G.groups, GRU_TILES));
    if (has_h) hipLaunchKernelGGL(k_drqn_gru_bf16<true>, ggrid, dim3(GRU_THREADS), 0, st, G);
    else hipLaunchKernelGGL(k_drqn_gru_bf16<false>, ggrid, dim3(GRU_THREADS), 0, st, G);
    QHeadArgs Q{};
    Q.h = new_states; Q.wh = (const bf16x8 *)w->head; Q.bh = w->head_bias; Q.n = n; Q.n_action = s->n_action; Q.dueling = w->dueling != 0;
    Q.actions = actions; Q.q = q;
    hipLaunchKernelGGL(k_drqn_head_bf16, dim3((n + 32 * QH_WAVES - 1) / (32 * QH_WAVES)), dim3(QH_THREADS), 0, st, Q);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" {

int policy_drqn_supported(const PolicyDqnShape *s) { return policy_dqn_supported(s); }

int policy_drqn_workspace_bytes(const PolicyDqnShape *s, int n, size_t *bytes) {
    n = n < 0 ? 0 : n;
    *bytes = x_offset(s, n) + (size_t)n * STATE * 2;
    return 0;
}

int policy_drqn_infer(const PolicyDqnShape *s, const PolicyDrqnWeights *w, const float *view, const float *feat, int n, const int *ids,
                      const int *prev_sorted_ids, const int *rows, const float *states, int count, float *new_states, void *workspace,
                      int *actions, float *q, void *stream) {
    return drqn_infer(s, w, view, false, feat, n, ids, prev_sorted_ids, rows, false, nullptr, states, count, new_states, workspace, actions, q, stream);
}

int policy_drqn_infer_bf16(const PolicyDqnShape *s, const PolicyDrqnWeights *w, const void *view_cells, const float *feat, int n, const int *ids,
                           const int *prev_sorted_ids, const int *rows, const float *states, int count, float *new_states, void *workspace,
                           int *actions, float *q, void *stream) {
    return drqn_infer(s, w, view_cells, true, feat, n, ids, prev_sorted_ids, rows, false, nullptr, states, count, new_states, workspace, actions, q, stream);
}

int policy_drqn_lookup_seg(const int *ids, int n, const int *seg_begin, const int *seg_count, int n_seg, int seg_first,
                           const long long *prev_sorted_keys, const int *rows, int count, int *from_row, long long *keys, void *stream) {
    return magent_amd::drqn_lookup_seg<LookupBf16>(ids, n, seg_begin, seg_count, n_seg, seg_first, prev_sorted_keys, rows, count, from_row, keys, stream);
}

int policy_drqn_infer_rows(const PolicyDqnShape *s, const PolicyDrqnWeights *w, const float *view, const float *feat, int n, const int *from_row,
                           const float *states, float *new_states, void *workspace, int *actions, float *q, void *stream) {
    return drqn_infer(s, w, view, false, feat, n, nullptr, nullptr, nullptr, true, from_row, states, 0, new_states, workspace, actions, q, stream);
}

int policy_drqn_infer_bf16_rows(const PolicyDqnShape *s, const PolicyDrqnWeights *w, const void *view_cells, const float *feat, int n,
                                const int *from_row, const float *states, float *new_states, void *workspace, int *actions, float *q, void *stream) {
    return drqn_infer(s, w, view_cells, true, feat, n, nullptr, nullptr, nullptr, true, from_row, states, 0, new_states, workspace, actions, q, stream);
}

}  // extern "C"
