// policy_bf16_dev.h -- what the bf16 policy translation units share (internal; not part of the C-ABI):
//   policy.hip            the DQN: k_dqn_conv + k_dqn_head, and the trunk launcher below
//   policy_drqn_bf16.hip  the DRQN: the DQN's trunk, then k_drqn_gru_bf16 + k_drqn_head_bf16
//   policy_a2c_bf16.hip   the A2C: k_a2c_trunk_bf16, k_a2c_layer_bf16 (+ the column sums), k_a2c_head_bf16
// The building blocks, each written once:
//   bf16x8, round_bf16x2 / x4 / x8, bf_lo, bf_hi, widen   the operand type and the conversions (all three)
//   xcd_place, xcd_grid                                   tile groups of an agent group on ONE XCD (k_drqn_gru_bf16, k_a2c_trunk_bf16, k_a2c_layer_bf16)
//   ring3                                                 the streamed-row triple buffering (k_drqn_gru_bf16, k_a2c_layer_bf16)
//   head_gemm512_bf16                                     the one-wave K = 512, 32-output head GEMM (k_drqn_head_bf16, k_a2c_head_bf16)
// The float32 side of these kernels (out_of, q_before, relu, sigmoid, the epilogues, pingpong, the id table, the column sums) is
// policy_f32_dev.h's, included here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/magent_policy.h"
#include "policy_f32_dev.h"

namespace magent_amd {
namespace bf16 {

using f32::f32x16;
using f32::f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// two float32 rounded to a 32-bit word of two bf16, the first in the low half: one v_cvt_pk_bf16_f32 (nearest even; a NaN stays a NaN)
__device__ __forceinline__ unsigned round_bf16x2(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2{a, b}), bf16x2));
}
// four float32 to four stored bf16, and eight (k = 8 g + 0..7 of a k-step) to the MFMA's operand
__device__ __forceinline__ u32x2 round_bf16x4(const f32x4 &v) { return u32x2{round_bf16x2(v[0], v[1]), round_bf16x2(v[2], v[3])}; }
__device__ __forceinline__ bf16x8 round_bf16x8(const f32x4 &a, const f32x4 &b) {
    return __builtin_bit_cast(bf16x8, u32x4{round_bf16x2(a[0], a[1]), round_bf16x2(a[2], a[3]), round_bf16x2(b[0], b[1]), round_bf16x2(b[2], b[3])});
}
struct F8 { f32x4 a[2]; };    // the eight float32 of a lane's half k-step as loaded, rounded when they are used
__device__ __forceinline__ bf16x8 round_bf16x8(const F8 &v) { return round_bf16x8(v.a[0], v.a[1]); }
// the two bf16 values of a 32-bit word as float32 (exact)
__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }
__device__ __forceinline__ f32x4 widen(const u32x2 &w) { return f32x4{bf_lo(w[0]), bf_hi(w[0]), bf_lo(w[1]), bf_hi(w[1])}; }

// The streamed-row GEMMs' placement: a workgroup is 256 agents (an agent group) on one of TG tile groups, and the TG workgroups of an
// agent group are dealt to the SAME XCD, one after another.  Workgroup L runs on XCD L % 8 (workgroups go round-robin over the 8 XCDs);
// the j = L / 8 -th workgroup of an XCD is tile group j % TG of the XCD's (j / TG)-th agent group.  The grid covers whole rounds of 8
// agent groups: a kernel returns where group >= its number of groups.
constexpr int XCDS = 8;
__device__ __forceinline__ void xcd_place(int TG, int &tg, int &group) {
    const int j = blockIdx.x / XCDS;
    tg = j % TG;
    group = (j / TG) * XCDS + blockIdx.x % XCDS;
}
inline unsigned xcd_grid(int groups, int TG) { return (unsigned)((groups + XCDS - 1) / XCDS * XCDS * TG); }

// NC chunks of operands through three register buffers: chunk c + 2 loads while chunk c's MFMAs run -- the look-ahead of two ping-pong
// buffers of twice the size (four k-steps, 12 MFMAs) in three quarters of their registers: with the h half's float32 operands two buffers of
// four k-steps did not fit 256 VGPRs beside the four accumulators.  Fully unrolled: no branch for the wait counts to merge over.
template <int NC, class Buf, class Load, class Run>
__device__ __forceinline__ void ring3(Buf (&op)[3], const Load &load, const Run &run) {
    load(0, op[0]);
    load(1, op[1]);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if (c + 2 < NC) load(c + 2, op[(c + 2) % 3]);
        run(op[c % 3]);
    }
}

// [32 outputs] x [32 agents] of one wave over K = 512: wh = the packed head ([32 k-steps][64 lanes]), l the lane; the lane's operand of
// k-step s is conv(load(s)) -- load fetches its eight values as they lie in memory (float32, or bf16 as stored), conv makes the MFMA's
// operand of them when it is used.  The operands of the next two k-steps load while the current two's MFMAs run (pingpong).
template <class Load, class Conv>
__device__ __forceinline__ f32x16 head_gemm512_bf16(const bf16x8 *wh, int l, const Load &load, const Conv &conv) {
    struct Op { decltype(load(0)) a; bf16x8 w; };
    Op op[2][2];
    f32x16 acc = {0};
    auto fetch = [&](int c, Op (&d)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int s = 2 * c + k;
            d[k].a = load(s);
            d[k].w = wh[s * 64 + l];
        }
    };
    auto run = [&](const Op (&d)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 2; k++) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d[k].w, conv(d[k].a), acc, 0, 0, 0);
    };
    f32::pingpong<512 / 16 / 2>(op, fetch, run);
    return acc;
}

// The DQN's trunk for the DRQN: k_dqn_conv (float32 views, or with cells16 the engine's bf16 cells), then k_dqn_head stopped after its
// hidden layer (k_dqn_head<., true>), which it stores as x bf16[n][512] = relu(dense_view) || relu(dense_emb), one 1 KB row per agent:
// the values the DQN's head would read from LDS, rounded once.  Order of a row: hidden SLOT order -- value 256 half + 32 T + s is unit
// 256 half + 32 T + (s & 3) + 8 ((s & 15) >> 2) + 4 (s >> 4) of torch's concatenated hidden layer (include/magent_policy.h: "slot"); the
// GRU's packed weight_ih absorbs the permutation, as dense_view's absorbs conv2's.  `w->head` and `w->value_bias` are not read.
// act_workspace: policy_dqn_act_bytes(s, n); x: 16-byte aligned.  Enqueues two kernels on `stream`; 0, or non-zero as policy_dqn_infer.
int dqn_trunk(const PolicyDqnShape *s, const PolicyDqnWeights *w, const void *view_any, bool cells16, const float *feat, int n,
              void *act_workspace, void *x, void *stream);

}  // namespace bf16
}  // namespace magent_amd
