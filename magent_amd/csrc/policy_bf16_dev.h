// policy_bf16_dev.h -- what the bf16 policy translation units share (internal; not part of the C-ABI):
//   policy.hip            the DQN: k_dqn_conv + k_dqn_head, and the trunk launcher below
//   policy_drqn_bf16.hip  the DRQN: the DQN's trunk, then k_drqn_gru_bf16 + k_drqn_head_bf16
#pragma once
#include <stddef.h>

#include "../../include/magent_policy.h"

namespace magent_amd {
namespace bf16 {

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
