// policy_f32_dev.h -- what the float32 policy translation units share (internal; not part of the C-ABI):
//   policy_f32.hip       the DQN: k_dqn_conv_f32 + k_dqn_head_f32, and the trunk launcher below
//   policy_drqn_f32.hip  the DRQN: the DQN's trunk, then k_drqn_gru_f32 + k_drqn_head_f32
// Operand and fragment conventions: policy_f32.hip's header comment and include/magent_policy.h ("f32 fragment order").
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/magent_policy.h"

namespace magent_amd {
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
// relu that keeps a NaN a NaN, as torch.relu does (fmaxf is IEEE maxNum: fmaxf(NaN, 0) = 0, and a poisoned view or a diverged network would
// then act on finite garbage).  IEEE 754-2019 maximum: one v_maximum3_f32 on gfx950, the cost of the v_max_f32 it replaces; -0 gives +0.
__device__ __forceinline__ float relu(float x) { return __builtin_elementwise_maximum(x, 0.0f); }
__device__ __forceinline__ f32x4 relu4(const f32x16 &acc, int q) {
    return f32x4{relu(acc[4 * q]), relu(acc[4 * q + 1]), relu(acc[4 * q + 2]), relu(acc[4 * q + 3])};
}
// torch.argmax's order of a Q row: a NaN above everything (the first NaN wins), then the larger value, the lower index among equals.  Does
// (v, o) come before (best, arg)?
__device__ __forceinline__ bool q_before(float v, int o, float best, int arg) {
    return v != v ? (best == best || o < arg) : (best == best && (v > best || (v == best && o < arg)));
}

// The DQN's trunk for the DRQN: k_dqn_conv_f32, then k_dqn_head_f32 stopped after its hidden layer, which it stores as
// x float[n][512] = relu(dense_view) || relu(dense_emb), natural unit order, one 2 KB row per agent.  `w->head` and `w->value_bias` are
// not read.  act_workspace: policy_dqn_f32_act_bytes(s, n).  Enqueues two kernels on `stream`; 0, or non-zero as policy_dqn_infer_f32.
int dqn_f32_trunk(const PolicyDqnShape *s, const PolicyDqnWeightsF32 *w, const float *view, const float *feat, int n, void *act_workspace,
                  float *x, void *stream);

}  // namespace f32
}  // namespace magent_amd
