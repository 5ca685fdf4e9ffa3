// policy_a2c_f32.hip -- one acting step of the advantage actor-critic (magent_amd/builtin/torch_model/a2c.py: _ActorCritic.forward, then
// the action draw), inference only, in float32 on v_mfma_f32_32x32x2_f32.
//
//   network:  xv = relu(flat(view) Wv^T + bv) [256] || xe = relu(feature We^T + be) [256]  ->  h = relu([xv | xe] Wd^T + bd) [512]
//             CommNet (use_comm), twice:  h <- tanh(others C_s^T + h H_s^T + skip),  skip = the h above,
//                                         others_i = (sum_j h_j - h_i) / (n - 1) over ALL n agents of the call (zeros for n == 1)
//             logits = h Wp^T + bp [A],  value = h Wval^T + bval;   p = clamp(softmax(logits), 1e-10, 1 - 1e-10)
//             draw:  c_0 = p_0, c_a = c_(a-1) + p_a, t = u c_(A-1);  action = the smallest a with c_a > t, else A - 1
//
// Operands and fragments as in policy_f32.hip: A = weights (lane l: output l & 31), B = activations (lane l: agent l & 31), a lane group g
// reads values 4 g .. 4 g + 3 of a group of 8 K-values as one float4 that feeds four MFMAs; a result lane (agent, g) holds outputs
// 8 q + 4 g + 0..3 of its 32-wide tile, natural order.  Every result column (agent) of an MFMA depends on that agent's operands alone, so
// an agent's row does not depend on where in a tile, a workgroup or a launch it sits.
//
// k_a2c_trunk_f32 : the two input layers by the loops k_dqn_head_f32 does its dense layer with (policy_f32_dev.h: dense_main,
//   stage_features, dense_emb, hidden_out) -- 128 agents per workgroup of 8 waves, wave w owns output tile w for all four agent tiles (one
//   weight float4 from L2 and four activation float4 from LDS feed 16 MFMAs); this kernel supplies the chunk stager.  The view rows are K =
//   H W C floats, 4-byte aligned only (battle: 1183), so a K-chunk of 64 values per agent goes through registers into LDS by 4-byte
//   loads -- a wave reads 64 consecutive floats of one row -- double buffered; values past K are zeros (K is padded to a multiple of 8 with
//   zero weights), rows past n repeat row n - 1 and are not stored.  x = [xv | xe] goes to HBM as float[n][512].
// k_a2c_layer_f32 : a [n] x [512] layer over K = 512 (<false>: h = relu(x Wd^T + bd)) or K = 1024 (<true>: one CommNet step as ONE GEMM,
//   [others | h] against [C_s | H_s] side by side; others is formed from the h row and the column sums as the operand is fed, tanh in
//   registers).  A wave owns 32 agents x 4 output tiles (four accumulators: per group of 8 K-values one activation float4 and four weight
//   float4 feed 16 MFMAs), operands of the next two groups load while the current two's 32 MFMAs run (policy_f32_dev.h: pingpong, the
//   driver k_drqn_gru_f32 uses), from L2 / HBM.
// k_a2c_colsum_part<float> + k_a2c_colsum : the CommNet column sums without float atomics, in a fixed order; the segmented call
//   (policy_a2c_infer_f32_seg) has k_a2c_segmap and k_a2c_colsum_part_seg<float> + k_a2c_colsum_seg in their place, and
//   k_a2c_layer_f32<true, true> takes the sum row, the divisor and `alone` per lane from the lane's agent's segment (a row in no
//   segment: alone).  Those kernels, the workspace layout (a2c_layout) and the driver of the launches (a2c_infer) are
//   policy_host.h's, the bf16 path's too; this file gives the driver the trait F32.
// k_a2c_head_f32 : [32 outputs] x [32 agents] per wave over K = 512 (head_gemm512; outputs 0..A-1 the policy's, output A the value's), softmax with the
//   row maximum subtracted, clamp, and the draw by the lane that holds the agent's action 0 (the row goes through LDS: a lane pair holds it).
//
// NaN contract: relu is IEEE maximum, tanhf and expf keep a NaN, the clamp is two comparisons (a NaN fails both and stays);
// the row maximum ignores a NaN (fmaxf) but the NaN reaches the row's sum through its own exp, so the whole row is NaN as F.softmax's.  A
// row with a NaN draws action A - 1 (no c_a > t holds).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/magent_policy.h"
#include "policy_f32_dev.h"
#include "policy_host.h"

namespace {

using namespace magent_amd::f32;      // the vector types, mfma4, relu, and the shared blocks: the dense pair, pingpong, head_gemm512, out_of, policy_epilogue

constexpr int HID = magent_amd::A2C_HID;
// ---------------------------------------------------------------------------------------------------- the input layers
constexpr int TR_THREADS = DENSE_THREADS, TR_M = DENSE_M, TR_KC = DENSE_KC, TR_ABUF = DENSE_ABUF;      // the shared dense pair's workgroup (policy_f32_dev.h)
constexpr int TR_FMAX = 64;                                          // most features (padded to 8)
constexpr int TR_KMAX = 4096;                                        // most view values: the packed dense_view (K x 256 floats) stays inside one 4 MB L2
constexpr size_t TR_LDS = ((size_t)2 * TR_ABUF + (size_t)TR_M * (TR_FMAX / 4)) * 16;      // two activation buffers + the features: 96 KB

struct TrunkArgs {
    const float *view;        // [n][K]
    const float *feat;        // [n][F]
    const f32x4 *wv;          // dense_view, f32 fragment order [KG][8 tiles][64]     (KG = K rounded up to 8, in groups)
    const f32x4 *we;          // dense_emb,  [FK / 8][8 tiles][64]                     (FK = F rounded up to 8)
    const float *bv, *be;     // [256] biases, natural order
    int n, K, KG, F, FK;
    float *x;                 // [n][512] relu(dense_view) || relu(dense_emb)
};

__global__ void __launch_bounds__(TR_THREADS) k_a2c_trunk_f32(TrunkArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    f32x4 *s_act = (f32x4 *)s_raw;                         // [2][128 agents][16 units], swizzled
    float *s_feat = (float *)(s_act + 2 * TR_ABUF);        // [128 agents][FK]
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const int a0 = blockIdx.x * TR_M;
    stage_features(s_feat, A.feat, a0, A.n, A.F, A.FK);
    // staging: wave w moves value l of the chunk for rows w, w + 8, .. w + 120 (64 consecutive floats of a row per load)
    float ar[16];
    auto aload = [&](int c) {
        const int k = c * TR_KC + l;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float *row = A.view + (size_t)min(a0 + w + 8 * i, A.n - 1) * A.K;
            ar[i] = k < A.K ? row[k] : 0.0f;
        }
    };
    auto astore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 16; i++) ((float *)(s_act + buf * TR_ABUF + act_slot(w + 8 * i, l >> 2)))[l & 3] = ar[i];
    };
    f32x16 acc[4];
    dense_main(acc, s_act, A.wv, A.KG, aload, astore);
    hidden_out(acc, A.bv, ToX{A.x, a0, A.n, 0});
    dense_emb(acc, s_feat, A.we, A.FK);
    hidden_out(acc, A.be, ToX{A.x, a0, A.n, 1});
}

// ---------------------------------------------------------------------------------------------------- dense 512 and the CommNet step
constexpr int LY_WAVES = 8, LY_THREADS = 64 * LY_WAVES, LY_TILES = 4, LY_CHUNK = 2;     // groups of 8 K-values a wave has in flight per buffer

struct LayerArgs {
    const float *in;          // [n][512] x (dense) or h (CommNet step)
    const float *sum;         // [512] column sums of `in` over the call (CommNet step)
    const float *skip;        // [n][512] (CommNet step)
    const f32x4 *w;           // [64 groups][16 tiles][64] (dense) / [128 groups][16 tiles][64]: K = others' 512, then h's 512 (CommNet step)
    const float *bias;        // [512] (dense)
    float *out;               // [n][512]
    int n;
    const int *row_seg;       // [n], seg_tab [n_seg][4]: the segmented call's maps (policy_host.h: k_a2c_segmap); `sum` is then [n_seg][512]
    const int *seg_tab;
};

// <COMM, SEG>: SEG is the CommNet step of a segmented call -- the sum row, the divisor and `alone` are the lane's agent's segment's
template <bool COMM, bool SEG = false>
__global__ void __launch_bounds__(LY_THREADS) k_a2c_layer_f32(LayerArgs A) {
    static_assert(COMM || !SEG, "only the CommNet step has a segmented form");
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    const int tile0 = (blockIdx.x * LY_WAVES + w) * 32;
    if (tile0 >= A.n) return;                                    // (whole waves: the MFMAs below see every lane)
    const int T0 = blockIdx.y * LY_TILES;
    const int agent = min(tile0 + r32, A.n - 1);
    const f32x4 *xp = (const f32x4 *)(A.in + (size_t)agent * HID) + g;        // group m: xp[2 m] = in[8 m + 4 g .. + 3]
    const f32x4 *sp = COMM ? (const f32x4 *)A.sum + g : xp;
    const f32x4 *wp = A.w + (size_t)T0 * 64 + l;                              // (group m, tile T0 + t) at wp[(m * 16 + t) * 64]
    float others_div = (float)(A.n - 1);
    bool alone = A.n == 1;
    if (SEG) {                                                   // per lane: a wave may straddle any number of segments
        const SegOfRow so = seg_of_row(A.row_seg, A.seg_tab, agent);
        sp += (size_t)so.sum_row * (HID / 4);
        others_div = so.others_div;
        alone = so.alone;
    }
    f32x16 acc[LY_TILES];
#pragma unroll
    for (int t = 0; t < LY_TILES; t++) acc[t] = f32x16{0};
    f32x4 op[2][LY_CHUNK][2 + LY_TILES];                                      // [buffer][group][row values, column sums, weights]
    auto phase = [&](auto is_others) __attribute__((always_inline)) {
        constexpr bool O = decltype(is_others)::value;
        const f32x4 *wph = wp + ((COMM && !O) ? (size_t)64 * 16 * 64 : 0);
        auto load = [&](int c, f32x4 (&d)[LY_CHUNK][2 + LY_TILES]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < LY_CHUNK; j++) {
                const int m = c * LY_CHUNK + j;
                d[j][0] = xp[2 * m];
                if (O) d[j][1] = sp[2 * m];
#pragma unroll
                for (int t = 0; t < LY_TILES; t++) d[j][2 + t] = wph[((size_t)m * 16 + t) * 64];
            }
        };
        auto run = [&](const f32x4 (&d)[LY_CHUNK][2 + LY_TILES]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < LY_CHUNK; j++) {
                f32x4 x = d[j][0];
                if (O) x = alone ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : (d[j][1] - x) / others_div;      // the mean of the OTHER agents
#pragma unroll
                for (int t = 0; t < LY_TILES; t++) acc[t] = mfma4(d[j][2 + t], x, acc[t]);
            }
        };
        pingpong<64 / LY_CHUNK>(op, load, run);
    };
    if (COMM) phase(std::integral_constant<bool, true>{});
    phase(std::integral_constant<bool, false>{});
    // lane (agent, g) holds units u = 32 (T0 + t) + 8 q + 4 g + i in result register 4 q + i of tile t
    const bool live = tile0 + r32 < A.n;
#pragma unroll
    for (int t = 0; t < LY_TILES; t++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int u = 32 * (T0 + t) + 8 * q + 4 * g;
            const f32x4 add = COMM ? *(const f32x4 *)(A.skip + (size_t)agent * HID + u) : *(const f32x4 *)(A.bias + u);
            f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = COMM ? tanhf(acc[t][4 * q + i] + add[i]) : relu(acc[t][4 * q + i] + add[i]);
            if (live) *(f32x4 *)(A.out + (size_t)agent * HID + u) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the heads and the draw
constexpr int PH_WAVES = 4, PH_THREADS = 64 * PH_WAVES, PH_PITCH = POLICY_ROW_PITCH;

struct PHeadArgs {
    const float *h;           // [n][512]
    const f32x4 *wh;          // [64][64]: K = 512; outputs 0..n_action-1 the policy's, n_action the value's, the rest zero
    const float *bh;          // [32] per-output biases
    const float *u;           // [n] uniform in [0, 1)
    int n, n_action;
    int *actions;             // [n]
    float *policy;            // [n][n_action] or null
    float *value;             // [n] or null
};

__global__ void __launch_bounds__(PH_THREADS) k_a2c_head_f32(PHeadArgs A) {
    __shared__ float s_p[PH_WAVES * 32 * PH_PITCH];               // the probability rows of the workgroup's agents
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    const int tile0 = (blockIdx.x * PH_WAVES + w) * 32;
    const int agent = min(tile0 + r32, A.n - 1);                 // (waves past n repeat the last agent and store nothing)
    const bool live = tile0 + r32 < A.n;
    f32x16 acc = head_gemm512(A.wh, l, (const f32x4 *)(A.h + (size_t)agent * HID) + g);
    // lane (agent, g) holds outputs out_of(r, g); its partner lane ^ 32 the other sixteen
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] += A.bh[out_of(r, g)];
    // softmax, clamp, the stores and the draw: policy_epilogue (policy_f32_dev.h), the bf16 head's too
    policy_epilogue(acc, g, A.n_action, s_p + (w * 32 + r32) * PH_PITCH, live, agent, A.u, A.actions, A.policy, A.value);
}

// ---------------------------------------------------------------------------------------------------- the launches
// the float32 trait of policy_host.h: a2c_infer, which owns the checks, the workspace and the order of the launches
struct F32 {
    typedef float Row;
    typedef PolicyA2cWeightsF32 Weights;
    bool supported(const PolicyDqnShape *s) const { return policy_a2c_f32_supported(s) != 0; }
    const void *view_weights(const Weights *w) const { return w->dense_view; }
    bool view_ok(const void *) const { return true; }            // (view rows are read by 4-byte loads)
    bool device_ready(int dev) const {
        static magent_amd::LdsAllowance lds_ok;
        return lds_ok.grant(dev, {{reinterpret_cast<const void *>(k_a2c_trunk_f32), (int)TR_LDS}});
    }
    void trunk(hipStream_t st, const PolicyDqnShape *s, const Weights *w, const void *view, const float *feat, int n, float *x) const {
        TrunkArgs T{};
        T.view = (const float *)view; T.feat = feat; T.wv = (const f32x4 *)w->dense_view; T.we = (const f32x4 *)w->dense_emb;
        T.bv = w->dense_view_bias; T.be = w->dense_emb_bias;
        T.n = n; T.K = s->view_h * s->view_w * s->view_c; T.KG = (T.K + 7) / 8; T.F = s->feat; T.FK = (s->feat + 7) / 8 * 8; T.x = x;
        hipLaunchKernelGGL(k_a2c_trunk_f32, dim3((n + TR_M - 1) / TR_M), dim3(TR_THREADS), TR_LDS, st, T);
    }
    void layer(hipStream_t st, magent_amd::A2cLayerKind kind, int n, const magent_amd::A2cLayerIo<float> &io) const {
        LayerArgs A{};
        A.in = io.in; A.sum = io.sum; A.skip = io.skip; A.w = (const f32x4 *)io.w; A.bias = io.bias; A.out = io.out; A.n = n;
        A.row_seg = io.row_seg; A.seg_tab = io.seg_tab;
        const dim3 grid((n + 32 * LY_WAVES - 1) / (32 * LY_WAVES), HID / 32 / LY_TILES), block(LY_THREADS);
        if (kind == magent_amd::A2C_DENSE) hipLaunchKernelGGL(k_a2c_layer_f32<false>, grid, block, 0, st, A);
        else if (kind == magent_amd::A2C_COMM) hipLaunchKernelGGL(k_a2c_layer_f32<true>, grid, block, 0, st, A);
        else hipLaunchKernelGGL((k_a2c_layer_f32<true, true>), grid, block, 0, st, A);
    }
    void head(hipStream_t st, const PolicyDqnShape *s, const Weights *w, const float *h, const float *u, int n, int *actions, float *policy,
              float *value) const {
        PHeadArgs P{};
        P.h = h; P.wh = (const f32x4 *)w->head; P.bh = w->head_bias; P.u = u; P.n = n; P.n_action = s->n_action;
        P.actions = actions; P.policy = policy; P.value = value;
        hipLaunchKernelGGL(k_a2c_head_f32, dim3((n + 32 * PH_WAVES - 1) / (32 * PH_WAVES)), dim3(PH_THREADS), 0, st, P);
    }
};

}  // namespace

extern "C" {

int policy_a2c_f32_supported(const PolicyDqnShape *s) {
    return s->view_h >= 1 && s->view_w >= 1 && s->view_c >= 1 && (long long)s->view_h * s->view_w * s->view_c <= TR_KMAX && s->feat >= 1 &&
           s->feat <= TR_FMAX && s->n_action >= 1 && s->n_action <= 31;
}

int policy_a2c_f32_workspace_bytes(const PolicyDqnShape *, int n, int use_comm, size_t *bytes) {
    *bytes = magent_amd::a2c_workspace_bytes(n, use_comm, sizeof(float), -1);
    return 0;
}

int policy_a2c_infer_f32(const PolicyDqnShape *s, const PolicyA2cWeightsF32 *w, const float *view, const float *feat, int n, const float *u,
                         void *workspace, int *actions, float *policy, float *value, void *stream) {
    return magent_amd::a2c_infer(F32{}, s, w, view, feat, n, u, workspace, actions, policy, value, stream, {});
}

int policy_a2c_f32_workspace_bytes_seg(const PolicyDqnShape *, int n, int use_comm, int n_seg, size_t *bytes) {
    *bytes = magent_amd::a2c_workspace_bytes(n, use_comm, sizeof(float), n_seg < 0 ? 0 : n_seg);
    return 0;
}

int policy_a2c_infer_f32_seg(const PolicyDqnShape *s, const PolicyA2cWeightsF32 *w, const float *view, const float *feat, int n, const float *u,
                             void *workspace, int *actions, float *policy, float *value, void *stream, const int *seg_begin,
                             const int *seg_count, int n_seg) {
    return magent_amd::a2c_infer(F32{}, s, w, view, feat, n, u, workspace, actions, policy, value, stream, {true, seg_begin, seg_count, n_seg});
}

}  // extern "C"
