// policy_a2c_bf16.hip -- one acting step of the advantage actor-critic (magent_amd/builtin/torch_model/a2c.py: _ActorCritic.forward, then
// the action draw), inference only, with bf16 matrix operands on v_mfma_f32_32x32x16_bf16: the opt-in sibling of policy_a2c_f32.hip, as
// policy_drqn_bf16.hip is of policy_drqn_f32.hip.
//
//   network:  xv = relu(flat(view) Wv^T + bv) [256] || xe = relu(feature We^T + be) [256]  ->  h = relu([xv | xe] Wd^T + bd) [512]
//             CommNet (use_comm), twice:  h <- tanh(others C_s^T + h H_s^T + skip),  skip = the h above,
//                                         others_i = (sum_j h_j - h_i) / (n - 1) over ALL n agents of the call (zeros for n == 1)
//             logits = h Wp^T + bp [A],  value = h Wval^T + bval;   p = clamp(softmax(logits), 1e-10, 1 - 1e-10);  the f32 path's draw
//   rounding: to bf16 (nearest even) -- the views (the cells entry takes the engine's cells as they are), the features, every weight
//             matrix, and every inter-layer activation ONCE, when it is stored: x = [xv | xe], h0 = relu(dense), each CommNet step's
//             output, as rows bf16[n][512] in natural unit order.  The stored row is what everything downstream reads: the next layer's
//             operand, the skip term, the column sums.  others_i is formed in float32 from the float32 column sum and the stored row and
//             then rounded as the operand.  Nothing else: products accumulate in float32, all biases are float32 epilogue adds, relu,
//             tanh, the column sums, the logits, the softmax, the clamp, the value and the draw are float32.
//
// Operands as in policy_drqn_bf16.hip: A = weights in fragment order (lane l: output l & 31, k = 8 (l >> 5) + 0..7 of a 16-wide k-step), B =
// activations (lane l: agent l & 31, the same eight k); a result lane (agent, g = l >> 5) holds outputs out_of(r, g) of its 32-wide tile.
// Every result column (agent) of an MFMA depends on that agent's operands alone.
//
// Work split of the two GEMM kernels, k_drqn_gru_bf16's: a wave owns 32 agents x 4 output tiles (four accumulators); per k-step a lane loads
// its 16 bytes of the agent's row and four weight fragments, which feed 4 MFMAs.  A workgroup is 8 waves = 256 agents on ONE group of four
// tiles (its waves read the same weights through one L1); the tile groups of an agent group are workgroups dealt to the SAME XCD
// (workgroups go round-robin over the 8 XCDs), one after another: every L2 then holds the layer's whole weight matrix and fetches an agent
// group's rows once for all of their readers.
// k_a2c_trunk_bf16<CELLS> : the two input layers, 8 + 8 output tiles in two tile groups.  <false>: float[n][K] views, rows 4-byte aligned
//   only (battle: 1183 floats): a lane loads its eight values of a k-step one by one and rounds them on their way into the MFMA; values
//   past K are zeros (K is padded to a multiple of 16 with zero weights).  <true>: the engine's cells bf16[n][H][W][8]: one cell is one
//   16-byte load and one half of a k-step, K' = 8 H W against the cell-order packing of dense_view; the half k-step behind an odd H W
//   is zeros.  The features are float[n][F], rounded the same way.  Two register buffers of two k-steps (K is a run-time number here).
// k_a2c_layer_bf16<COMM> : [n] x [512] over K = 512 (<false>: h = relu(x Wd^T + bd)) or K = 1024 (<true>: one CommNet step as ONE GEMM,
//   [others | h] against [C_s | H_s]; others is formed from the stored row and the column sums -- in LDS -- as the operand is fed; the
//   skip row and tanh in the epilogue).  Three register buffers of two k-steps (policy_bf16_dev.h: ring3).  Both GEMM kernels take
//   their (tile group, agent group) from policy_bf16_dev.h: xcd_place, and their grid from xcd_grid.
// k_a2c_colsum_part<bf16_t> + k_a2c_colsum, and the segmented call's k_a2c_segmap, k_a2c_colsum_part_seg<bf16_t> + k_a2c_colsum_seg
//   (policy_a2c_infer_seg, policy_a2c_infer_bf16_seg): the f32 path's kernels (policy_host.h) over the bf16 rows,
//   added in float32.  k_a2c_layer_bf16<true, true>: the sum row, the divisor and `alone` per lane.  Its sums do not go through LDS (a
//   workgroup may touch as many segments as it has agents): a lane loads the eight float32 sums of a k-step from its segment's row with
//   the k-step's operands, through three register buffers of ONE k-step.
// k_a2c_head_bf16 : [32 outputs] x [32 agents] per wave over K = 512 (policy_bf16_dev.h: head_gemm512_bf16, shared with
//   k_drqn_head_bf16; the operand as stored), float32 biases, then policy_f32_dev.h: policy_epilogue, the f32 head's own softmax, clamp
//   and draw.  The workspace layout (a2c_layout, the f32 path's with 2-byte row elements) and the driver of the launches (a2c_infer) are
//   policy_host.h's; this file gives the driver the trait Bf16.
//
// Whole waves exit early (the head's stay for its barrier); lanes past n repeat the last agent (their own columns of the MFMA, never stored).
// NaN contract: relu is IEEE maximum, tanhf keeps a NaN, the roundings keep a NaN; without CommNet a NaN or Inf in an
// agent's inputs stays in that agent's MFMA column; with CommNet a non-finite h reaches every agent through the sum, as in PyTorch.  An
// action is always inside [0, n_action).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/magent_policy.h"
#include "policy_bf16_dev.h"
#include "policy_f32_dev.h"
#include "policy_host.h"

namespace {

using namespace magent_amd::bf16;         // the vector types, the conversions, xcd_place / xcd_grid, ring3, head_gemm512_bf16
using magent_amd::f32::out_of;
using magent_amd::f32::policy_epilogue;
using magent_amd::f32::POLICY_ROW_PITCH;
using magent_amd::f32::relu;

typedef unsigned short bf16_t;           // a stored bf16 value (rows are addressed by element)

constexpr int HID = magent_amd::A2C_HID, KSTEPS = HID / 16;
constexpr int GEMM_WAVES = 8, GEMM_THREADS = 64 * GEMM_WAVES, GEMM_TILES = 4;      // a wave: 32 agents x 4 output tiles; a workgroup: 256 agents

// ---------------------------------------------------------------------------------------------------- the input layers
constexpr int TR_TG = 256 / 32 / GEMM_TILES, TR_CHUNK = 2;      // two tile groups per half of x; k-steps per register buffer
constexpr int TR_FMAX = 64, TR_KMAX = 4096;                     // the f32 path's region

struct TrunkArgs {
    const void *view;         // float[n][K], or the cells bf16[n][HW][8]
    const float *feat;        // [n][F]
    const bf16x8 *wv;         // dense_view (or its cell-order packing), fragment order [KS][8 tiles][64]
    const bf16x8 *we;         // dense_emb, [FS][8 tiles][64]
    const float *bv, *be;     // [256] biases, natural order
    int n, groups;            // groups: agent groups of 32 GEMM_WAVES
    int K, HW, KS;            // view values (float32 views), cells (cells), and the k-steps of either: K / 16 or HW / 2, rounded up
    int F, FS;                // features and their k-steps
    bf16_t *x;                // [n][512] relu(dense_view) || relu(dense_emb), bf16
};

// acc[t] += over `ksteps` k-steps: the lane's operand of k-step s is conv(aload(s)); (k-step s, tile t) of the weights at wp[(s * 8 + t) * 64].
// aload takes any s up to ksteps (it clamps its addresses).  The next two k-steps load while the current two's 8 MFMAs run.
template <class Raw, class ALoad, class Conv>
__device__ __forceinline__ void trunk_rows(f32x16 (&acc)[GEMM_TILES], const bf16x8 *wp, int ksteps, const ALoad &aload, const Conv &conv) {
    struct Op { Raw a; bf16x8 w[GEMM_TILES]; };
    Op op[2][TR_CHUNK];
    const int nc = (ksteps + TR_CHUNK - 1) / TR_CHUNK;
    auto load = [&](int c, Op (&d)[TR_CHUNK]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < TR_CHUNK; j++) {
            const int s = c * TR_CHUNK + j;
            d[j].a = aload(s);
#pragma unroll
            for (int t = 0; t < GEMM_TILES; t++) d[j].w[t] = wp[((size_t)min(s, ksteps - 1) * 8 + t) * 64];
        }
    };
    auto run = [&](int c, const Op (&d)[TR_CHUNK]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < TR_CHUNK; j++) {
            if (c * TR_CHUNK + j < ksteps) {                     // (the same for every lane: whole waves take the MFMAs)
                const bf16x8 b = conv(d[j].a);
#pragma unroll
                for (int t = 0; t < GEMM_TILES; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[j].w[t], b, acc[t], 0, 0, 0);
            }
        }
    };
    load(0, op[0]);
    for (int c = 0; c < nc; c += 2) {
        if (c + 1 < nc) load(c + 1, op[1]);
        run(c, op[0]);
        if (c + 2 < nc) load(c + 2, op[0]);
        if (c + 1 < nc) run(c + 1, op[1]);
    }
}
// eight float32 k0 .. k0 + 7 of a row of `len` values (4-byte aligned); values past the row are zeros (and not read)
__device__ __forceinline__ F8 load_f8(const float *row, int k0, int len) {
    F8 v;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float f = row[min(k0 + e, len - 1)];
        v.a[e >> 2][e & 3] = k0 + e < len ? f : 0.0f;
    }
    return v;
}
// relu(acc + bias) of the wave's four tiles, rounded, to the agent's row: lane (agent, g) holds units 32 t + 8 q + 4 g + 0..3 of tile t
__device__ __forceinline__ void trunk_out(const f32x16 (&acc)[GEMM_TILES], const float *bias, bf16_t *orow, int g, bool live) {
#pragma unroll
    for (int t = 0; t < GEMM_TILES; t++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int u = 32 * t + 8 * q + 4 * g;
            const f32x4 b = *(const f32x4 *)(bias + u);
            f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = relu(acc[t][4 * q + i] + b[i]);
            if (live) *(u32x2 *)(orow + u) = round_bf16x4(o);
        }
    }
}

template <bool CELLS>
__global__ void __launch_bounds__(GEMM_THREADS) k_a2c_trunk_bf16(TrunkArgs A) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    int tg, group;
    xcd_place(TR_TG, tg, group);
    const int tile0 = (group * GEMM_WAVES + w) * 32;
    if (group >= A.groups || tile0 >= A.n) return;               // (whole waves: the MFMAs below see every lane)
    const int agent = min(tile0 + r32, A.n - 1);
    const bool live = tile0 + r32 < A.n;
    const int T0 = tg * GEMM_TILES;
    bf16_t *orow = A.x + (size_t)agent * HID + 32 * T0;
    f32x16 acc[GEMM_TILES];
#pragma unroll
    for (int t = 0; t < GEMM_TILES; t++) acc[t] = f32x16{0};
    const bf16x8 *wvp = A.wv + (size_t)T0 * 64 + l;
    if (CELLS) {
        const bf16x8 *row = (const bf16x8 *)A.view + (size_t)agent * A.HW;       // cell c is the half k-step c
        trunk_rows<bf16x8>(acc, wvp, A.KS,
                           [&](int s) {
                               const int c = 2 * s + g;
                               const bf16x8 v = row[min(c, A.HW - 1)];
                               return c < A.HW ? v : bf16x8{0};                    // (behind an odd H W, and never another agent's cell)
                           },
                           [](const bf16x8 &v) { return v; });
    } else {
        const float *row = (const float *)A.view + (size_t)agent * A.K;
        trunk_rows<F8>(acc, wvp, A.KS, [&](int s) { return load_f8(row, 16 * s + 8 * g, A.K); },
                       [](const F8 &v) { return round_bf16x8(v); });
    }
    trunk_out(acc, A.bv + 32 * T0, orow, g, live);
#pragma unroll
    for (int t = 0; t < GEMM_TILES; t++) acc[t] = f32x16{0};
    const float *frow = A.feat + (size_t)agent * A.F;
    trunk_rows<F8>(acc, A.we + (size_t)T0 * 64 + l, A.FS, [&](int s) { return load_f8(frow, 16 * s + 8 * g, A.F); },
                   [](const F8 &v) { return round_bf16x8(v); });
    trunk_out(acc, A.be + 32 * T0, orow + 256, g, live);
}

// ---------------------------------------------------------------------------------------------------- dense 512 and the CommNet step
constexpr int LY_TG = HID / 32 / GEMM_TILES, LY_CHUNK = 2;      // four tile groups; k-steps per register buffer, a wave has three (ring3)

struct LayerArgs {
    const bf16x8 *in;         // [n][64 units of 8] x (dense) or h (CommNet step)
    const float *sum;         // [512] column sums of `in` over the call (CommNet step)
    const bf16_t *skip;       // [n][512] (CommNet step)
    const bf16x8 *w;          // [32 k-steps][16 tiles][64] (dense) / [64][16][64]: K = others' 512, then h's 512 (CommNet step)
    const float *bias;        // [512] (dense)
    bf16_t *out;              // [n][512]
    int n, groups;
    const int *row_seg;       // [n], seg_tab [n_seg][4]: the segmented call's maps (policy_host.h: k_a2c_segmap); `sum` is then [n_seg][512]
    const int *seg_tab;
};

// one k-step: the lane's 16 bytes of the row as stored, four weight fragments; <true>, the segmented step's: and the eight column sums of
// the k-step, loaded with the operands from the lane's segment's row of the table
template <bool SEG> struct XOp { bf16x8 a, w[GEMM_TILES]; };
template <> struct XOp<true> { bf16x8 a, w[GEMM_TILES]; f32x4 s[2]; };
__device__ __forceinline__ void load_sums(XOp<false> &, const f32x4 *, int) {}
__device__ __forceinline__ void load_sums(XOp<true> &d, const f32x4 *gsp, int s) { d.s[0] = gsp[4 * s]; d.s[1] = gsp[4 * s + 1]; }
__device__ __forceinline__ void held_sums(const XOp<false> &, f32x4 &, f32x4 &) {}
__device__ __forceinline__ void held_sums(const XOp<true> &d, f32x4 &lo, f32x4 &hi) { lo = d.s[0]; hi = d.s[1]; }

// <COMM, SEG>: SEG is the CommNet step of a segmented call -- the sum row, the divisor and `alone` are the lane's agent's segment's.  The
// call's single sum row goes through LDS; a workgroup of 256 agents of a segmented call may touch as many segments as it has agents, so
// there each lane loads its own segment's sums from global memory (n_seg rows of 2 KB: L2) beside the operands of the same k-step.
template <bool COMM, bool SEG = false>
__global__ void __launch_bounds__(GEMM_THREADS) k_a2c_layer_bf16(LayerArgs A) {
    static_assert(COMM || !SEG, "only the CommNet step has a segmented form");
    __shared__ __attribute__((aligned(16))) float s_sum[SEG ? 4 : HID];
    if (COMM && !SEG) {                                          // (before any wave leaves: GEMM_THREADS == HID)
        s_sum[threadIdx.x] = A.sum[threadIdx.x];
        __syncthreads();
    }
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    int tg, group;
    xcd_place(LY_TG, tg, group);
    const int tile0 = (group * GEMM_WAVES + w) * 32;
    if (group >= A.groups || tile0 >= A.n) return;               // (whole waves: the MFMAs below see every lane)
    const int agent = min(tile0 + r32, A.n - 1);
    const int T0 = tg * GEMM_TILES;
    const bf16x8 *xp = A.in + (size_t)agent * (HID / 8) + g;                  // k-step s: xp[2 s] = in[16 s + 8 g .. + 7]
    const bf16x8 *wp = A.w + (size_t)T0 * 64 + l;                             // (k-step s, tile T0 + t) at wp[(s * 16 + t) * 64]
    float others_div = (float)(A.n - 1);
    bool alone = A.n == 1;
    const f32x4 *gsp = nullptr;                                  // SEG: the lane's segment's sum row, k-step s at gsp[4 s], gsp[4 s + 1]
    if constexpr (SEG) {                                         // per lane: a wave may straddle any number of segments
        const magent_amd::f32::SegOfRow so = magent_amd::f32::seg_of_row(A.row_seg, A.seg_tab, agent);
        gsp = (const f32x4 *)(A.sum + (size_t)so.sum_row * HID) + 2 * g;
        others_div = so.others_div;
        alone = so.alone;
    }
    f32x16 acc[GEMM_TILES];
#pragma unroll
    for (int t = 0; t < GEMM_TILES; t++) acc[t] = f32x16{0};
    // k-steps per register buffer: the segmented step's buffers also hold the sums, eight float32 per k-step, and three buffers of two
    // k-steps no longer fit 256 VGPRs beside the accumulators (38 spilled) -- it runs three buffers of one k-step
    constexpr int CH = SEG ? 1 : LY_CHUNK;
    typedef XOp<SEG> Op;
    Op op[3][CH];
    auto phase = [&](auto is_others) __attribute__((always_inline)) {
        constexpr bool O = decltype(is_others)::value;
        const bf16x8 *wph = wp + ((COMM && !O) ? (size_t)KSTEPS * 16 * 64 : 0);
        int at = 0;                                              // the chunk `run` is at (ring3 is fully unrolled: a constant)
        auto load = [&](int c, Op (&d)[CH]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < CH; k++) {
                const int s = c * CH + k;
                d[k].a = xp[2 * s];
                if (SEG && O) load_sums(d[k], gsp, s);
#pragma unroll
                for (int t = 0; t < GEMM_TILES; t++) d[k].w[t] = wph[((size_t)s * 16 + t) * 64];
            }
        };
        auto run = [&](const Op (&d)[CH]) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < CH; k++) {
                bf16x8 b = d[k].a;
                if (O) {                                         // the mean of the OTHER agents, float32, then rounded as the operand
                    f32x4 slo, shi;
                    if (SEG) held_sums(d[k], slo, shi);
                    else {
                        const float *sp = s_sum + 16 * (at * CH + k) + 8 * g;
                        slo = *(const f32x4 *)sp; shi = *(const f32x4 *)(sp + 4);
                    }
                    const u32x4 raw = __builtin_bit_cast(u32x4, d[k].a);
                    f32x4 lo = widen(u32x2{raw[0], raw[1]}), hi = widen(u32x2{raw[2], raw[3]});
                    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
                    lo = alone ? zero : (slo - lo) / others_div;
                    hi = alone ? zero : (shi - hi) / others_div;
                    b = round_bf16x8(lo, hi);
                }
#pragma unroll
                for (int t = 0; t < GEMM_TILES; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[k].w[t], b, acc[t], 0, 0, 0);
            }
            at++;
        };
        ring3<KSTEPS / CH>(op, load, run);
    };
    if (COMM) phase(std::integral_constant<bool, true>{});
    phase(std::integral_constant<bool, false>{});
    // lane (agent, g) holds units u = 32 (T0 + t) + 8 q + 4 g + i in result register 4 q + i of tile t
    const bool live = tile0 + r32 < A.n;
#pragma unroll
    for (int t = 0; t < GEMM_TILES; t++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int u = 32 * (T0 + t) + 8 * q + 4 * g;
            const f32x4 add = COMM ? widen(*(const u32x2 *)(A.skip + (size_t)agent * HID + u)) : *(const f32x4 *)(A.bias + u);
            f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = COMM ? tanhf(acc[t][4 * q + i] + add[i]) : relu(acc[t][4 * q + i] + add[i]);
            if (live) *(u32x2 *)(A.out + (size_t)agent * HID + u) = round_bf16x4(o);      // rounded once, here
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the heads and the draw
constexpr int PH_WAVES = 4, PH_THREADS = 64 * PH_WAVES;

struct PHeadArgs {
    const bf16x8 *h;          // [n][64 units of 8]
    const bf16x8 *wh;         // [32 k-steps][64]: K = 512; outputs 0..n_action-1 the policy's, n_action the value's, the rest zero
    const float *bh;          // [32] per-output biases
    const float *u;           // [n] uniform in [0, 1)
    int n, n_action;
    int *actions;             // [n]
    float *policy;            // [n][n_action] or null
    float *value;             // [n] or null
};

__global__ void __launch_bounds__(PH_THREADS) k_a2c_head_bf16(PHeadArgs A) {
    __shared__ float s_p[PH_WAVES * 32 * POLICY_ROW_PITCH];      // the probability rows of the workgroup's agents
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, g = l >> 5, r32 = l & 31;
    const int tile0 = (blockIdx.x * PH_WAVES + w) * 32;
    const int agent = min(tile0 + r32, A.n - 1);                 // (waves past n repeat the last agent and store nothing)
    const bool live = tile0 + r32 < A.n;
    const bf16x8 *xp = A.h + (size_t)agent * (HID / 8) + g;                   // k-step s: xp[2 s], the operand as stored
    f32x16 acc = head_gemm512_bf16(A.wh, l, [&](int s) { return xp[2 * s]; }, [](const bf16x8 &v) { return v; });
    // lane (agent, g) holds outputs out_of(r, g); its partner lane ^ 32 the other sixteen
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] += A.bh[out_of(r, g)];
    policy_epilogue(acc, g, A.n_action, s_p + (w * 32 + r32) * POLICY_ROW_PITCH, live, agent, A.u, A.actions, A.policy, A.value);
}

// ---------------------------------------------------------------------------------------------------- the launches
static bool cells_supported(const PolicyDqnShape *s) { return s->view_c <= 7 && 8LL * s->view_h * s->view_w <= TR_KMAX; }

// the bf16 trait of policy_host.h: a2c_infer, which owns the checks, the workspace and the order of the launches.  `cells`: the view
// is the engine's cells (policy_a2c_infer_bf16*), not float32 views
struct Bf16 {
    typedef bf16_t Row;
    typedef PolicyA2cWeights Weights;
    bool cells;
    bool supported(const PolicyDqnShape *s) const { return policy_a2c_supported(s) && (!cells || cells_supported(s)); }
    const void *view_weights(const Weights *w) const { return cells ? w->dense_view_cells : w->dense_view; }
    bool view_ok(const void *view) const { return !cells || !((uintptr_t)view & 15); }      // (a cell is one 16-byte load)
    bool device_ready(int) const { return true; }
    static int groups(int n) { return (n + 32 * GEMM_WAVES - 1) / (32 * GEMM_WAVES); }
    void trunk(hipStream_t st, const PolicyDqnShape *s, const Weights *w, const void *view, const float *feat, int n, bf16_t *x) const {
        TrunkArgs T{};
        T.view = view; T.feat = feat; T.wv = (const bf16x8 *)view_weights(w); T.we = (const bf16x8 *)w->dense_emb;
        T.bv = w->dense_view_bias; T.be = w->dense_emb_bias; T.n = n; T.groups = groups(n);
        T.K = s->view_h * s->view_w * s->view_c; T.HW = s->view_h * s->view_w; T.KS = cells ? (T.HW + 1) / 2 : (T.K + 15) / 16;
        T.F = s->feat; T.FS = (s->feat + 15) / 16; T.x = x;
        if (cells) hipLaunchKernelGGL(k_a2c_trunk_bf16<true>, dim3(xcd_grid(T.groups, TR_TG)), dim3(GEMM_THREADS), 0, st, T);
        else hipLaunchKernelGGL(k_a2c_trunk_bf16<false>, dim3(xcd_grid(T.groups, TR_TG)), dim3(GEMM_THREADS), 0, st, T);
    }
    void layer(hipStream_t st, magent_amd::A2cLayerKind kind, int n, const magent_amd::A2cLayerIo<bf16_t> &io) const {
        LayerArgs A{};
        A.in = (const bf16x8 *)io.in; A.sum = io.sum; A.skip = io.skip; A.w = (const bf16x8 *)io.w; A.bias = io.bias; A.out = io.out;
        A.n = n; A.groups = groups(n); A.row_seg = io.row_seg; A.seg_tab = io.seg_tab;
        const dim3 grid(xcd_grid(A.groups, LY_TG)), block(GEMM_THREADS);
        if (kind == magent_amd::A2C_DENSE) hipLaunchKernelGGL(k_a2c_layer_bf16<false>, grid, block, 0, st, A);
        else if (kind == magent_amd::A2C_COMM) hipLaunchKernelGGL(k_a2c_layer_bf16<true>, grid, block, 0, st, A);
        else hipLaunchKernelGGL((k_a2c_layer_bf16<true, true>), grid, block, 0, st, A);
    }
    void head(hipStream_t st, const PolicyDqnShape *s, const Weights *w, const bf16_t *h, const float *u, int n, int *actions, float *policy,
              float *value) const {
        PHeadArgs P{};
        P.h = (const bf16x8 *)h; P.wh = (const bf16x8 *)w->head; P.bh = w->head_bias; P.u = u; P.n = n; P.n_action = s->n_action;
        P.actions = actions; P.policy = policy; P.value = value;
        hipLaunchKernelGGL(k_a2c_head_bf16, dim3((n + 32 * PH_WAVES - 1) / (32 * PH_WAVES)), dim3(PH_THREADS), 0, st, P);
    }
};

}  // namespace

extern "C" {

int policy_a2c_supported(const PolicyDqnShape *s) {
    const bool views = s->view_h >= 1 && s->view_w >= 1 && s->view_c >= 1 && (long long)s->view_h * s->view_w * s->view_c <= TR_KMAX && s->feat >= 1 &&
                       s->feat <= TR_FMAX && s->n_action >= 1 && s->n_action <= 31;
    return views ? (cells_supported(s) ? 3 : 1) : 0;
}

int policy_a2c_workspace_bytes(const PolicyDqnShape *, int n, int use_comm, size_t *bytes) {
    *bytes = magent_amd::a2c_workspace_bytes(n, use_comm, sizeof(bf16_t), -1);
    return 0;
}

int policy_a2c_infer(const PolicyDqnShape *s, const PolicyA2cWeights *w, const float *view, const float *feat, int n, const float *u,
                     void *workspace, int *actions, float *policy, float *value, void *stream) {
    return magent_amd::a2c_infer(Bf16{false}, s, w, view, feat, n, u, workspace, actions, policy, value, stream, {});
}

int policy_a2c_infer_bf16(const PolicyDqnShape *s, const PolicyA2cWeights *w, const void *view_cells, const float *feat, int n, const float *u,
                          void *workspace, int *actions, float *policy, float *value, void *stream) {
    return magent_amd::a2c_infer(Bf16{true}, s, w, view_cells, feat, n, u, workspace, actions, policy, value, stream, {});
}

int policy_a2c_workspace_bytes_seg(const PolicyDqnShape *, int n, int use_comm, int n_seg, size_t *bytes) {
    *bytes = magent_amd::a2c_workspace_bytes(n, use_comm, sizeof(bf16_t), n_seg < 0 ? 0 : n_seg);
    return 0;
}

int policy_a2c_infer_seg(const PolicyDqnShape *s, const PolicyA2cWeights *w, const float *view, const float *feat, int n, const float *u,
                         void *workspace, int *actions, float *policy, float *value, void *stream, const int *seg_begin,
                         const int *seg_count, int n_seg) {
    return magent_amd::a2c_infer(Bf16{false}, s, w, view, feat, n, u, workspace, actions, policy, value, stream, {true, seg_begin, seg_count, n_seg});
}

int policy_a2c_infer_bf16_seg(const PolicyDqnShape *s, const PolicyA2cWeights *w, const void *view_cells, const float *feat, int n,
                              const float *u, void *workspace, int *actions, float *policy, float *value, void *stream,
                              const int *seg_begin, const int *seg_count, int n_seg) {
    return magent_amd::a2c_infer(Bf16{true}, s, w, view_cells, feat, n, u, workspace, actions, policy, value, stream, {true, seg_begin, seg_count, n_seg});
}

}  // extern "C"
