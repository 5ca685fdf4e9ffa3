// policy_bf16_dev.h -- what the bf16 policy translation units share (internal; not part of the C-ABI):
//   policy.hip            the DQN: k_dqn_conv + k_dqn_head, and the trunk launcher below
//   policy_drqn_bf16.hip  the DRQN: the DQN's trunk, then k_drqn_gru_bf16 + k_drqn_head_bf16
//   policy_a2c_bf16.hip   the A2C: k_a2c_trunk_bf16, k_a2c_layer_bf16 (+ the column sums), k_a2c_head_bf16
// and the two device building blocks the streamed-row kernels of the last two are made of: round_bf16x8 and ring3.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/magent_policy.h"
#include "policy_f32_dev.h"

namespace magent_amd {
namespace bf16 {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// eight float32 (k = 8 g + 0..7 of a k-step) rounded to the MFMA's operand: four v_cvt_pk_bf16_f32 (nearest even; a NaN stays a NaN)
__device__ __forceinline__ bf16x8 round_bf16x8(const f32::f32x4 &a, const f32::f32x4 &b) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    u32x4 u;
    u[0] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2{a[0], a[1]}), bf16x2));
    u[1] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2{a[2], a[3]}), bf16x2));
    u[2] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2{b[0], b[1]}), bf16x2));
    u[3] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2{b[2], b[3]}), bf16x2));
    return __builtin_bit_cast(bf16x8, u);
}

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
