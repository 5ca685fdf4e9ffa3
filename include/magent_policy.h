/*
 * magent_policy.h -- C-ABI of the inference path of the reference's deep Q network on MI355X (libmagent.so).
 *
 * What it replaces: the forward pass of python/magent/builtin/tf_model/dqn.py:151-189 (2 x conv3x3(32, valid, relu) ->
 * dense 256 || dense 256 -> dueling head) as DeepQNetwork.infer_action calls it (dqn.py:191-228) between
 * GridWorld.get_observation and GridWorld.set_action -- BASELINE config 5's policy step.  Additive: the reference has no
 * C entry point here (its model is a TensorFlow graph); the Python binding is magent_amd/builtin/torch_model/hip_policy.py.
 *
 * Further down: the same network in float32, the deep recurrent Q network's acting step in float32 and with bf16 operands
 * (policy_drqn_infer_f32, policy_drqn_infer), the actor-critic's in float32 and with bf16 operands (policy_a2c_infer_f32,
 * policy_a2c_infer), and the actor-critic's segmented form for packed batches (policy_a2c_infer_f32_seg, policy_a2c_infer_seg).
 *
 * All pointers are DEVICE pointers; the call enqueues two kernels on `stream` and returns.  Inputs are the engine's own
 * observation tensors (env_get_observation_device): view float[n][view_h][view_w][view_c], feature float[n][feat].
 * Numerics: inputs, weights and inter-layer activations are rounded to bf16, products accumulate in f32 (MFMA).
 */
#ifndef MAGENT_AMD_POLICY_H
#define MAGENT_AMD_POLICY_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int view_h, view_w, view_c;   /* view_c <= 7 (the eighth channel of a window cell carries conv1's bias); view_h * view_w <= 256 */
    int feat;                     /* <= 64 */
    int n_action;                 /* <= 31 */
} PolicyDqnShape;

/* Weights in "fragment order" (bf16, 16-byte units of 8 values): for k-step s (16 values of the reduction dimension) and
 * 32-wide output tile T, lane l (0..63) holds W[out = 32 T + (l & 31)][k = 16 s + 8 (l >> 5) + 0..7].
 * The reduction index k of each layer:
 *   conv1      : j * 8 + channel, j = 0..9 standing for tap (ky * 3 + kx) 0, 3, 1, 4, 2, 5, 6, 7, 8, padding -- the two taps of
 *                a k-step lie a constant number of window cells apart (channels padded to 8: 5 k-steps)       [5][64][8]
 *                its bias is the weight of (tap 0, channel 7): the kernel feeds a constant 1.0 there
 *   conv2      : tap * 32 + slot                          (18 k-steps)                                         [18][64][8]
 *   dense_view : position (y * (view_w - 4) + x) * 32 + slot                                                    [K/16][8][64][8]
 *   dense_emb  : feature index (padded to a multiple of 16)                                                     [FK/16][8][64][8]
 *   head       : hidden slot (tile T' of dense_view / 256 + tile T' of dense_emb: 32 T' + slot); outputs 0..n_action-1 =
 *                advantage, output n_action = value, the rest zero                                              [32][64][8]
 * A "slot" s of a 32-wide tile stands for its channel / output (s & 3) + 8 ((s & 15) >> 2) + 4 (s >> 4): the order in which
 * a lane of the MFMA result holds them (magent_amd/csrc/policy.hip: ch_of).  Biases are float[tiles][32] in slot order. */
typedef struct {
    const void *conv1, *conv2, *dense_view, *dense_emb, *head;
    const float *conv2_bias, *dense_view_bias, *dense_emb_bias;
    float value_bias;
} PolicyDqnWeights;

/* 1 if the kernels take this shape */
int policy_dqn_supported(const PolicyDqnShape *shape);
/* size of the activation workspace (conv2's output, bf16) for n agents */
int policy_dqn_act_bytes(const PolicyDqnShape *shape, int n, size_t *bytes);
/* actions[i] = argmax_a Q(view[i], feature[i]); q (optional, may be NULL) = float[n][n_action].  Returns 0, or non-zero if the
 * shape is not supported / a launch failed (nothing is written then). */
int policy_dqn_infer(const PolicyDqnShape *shape, const PolicyDqnWeights *weights, const float *view, const float *feature, int n,
                     void *act_workspace, int *actions, float *q, void *stream);

/* the same with the views as the engine's bf16 cells (env_get_observation_device_bf16: [n][view_h][view_w][8], channel 7 = 1.0):
 * they ARE conv1's operands -- nothing is converted, and the kernel reads 16 bytes per window cell instead of 4 * view_c */
int policy_dqn_infer_bf16(const PolicyDqnShape *shape, const PolicyDqnWeights *weights, const void *view_cells, const float *feature, int n,
                          void *act_workspace, int *actions, float *q, void *stream);

/* ---- the same network in the reference's own arithmetic: float32 inputs, weights, activations and accumulation, on the f32 matrix
 * instruction (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered chain of fmaf) -- magent_amd/csrc/policy_f32.hip.
 * Weights in "f32 fragment order" (float, 16-byte units of 4 values): the reduction index is cut into groups of 8; for group m and 32-wide
 * output tile T, lane l (0..63) holds W[out = 32 T + (l & 31)][k = 8 m + 4 (l >> 5) + 0..3].  The reduction index k of each layer:
 *   conv1      : tap (ky * 3 + kx) * 8 + channel (channels padded to 8); the bias is the weight of (tap 0, channel 7): the kernel
 *                feeds a constant 1.0 there                                                                     [9][64][4]
 *   conv2      : tap * 32 + channel                                                                              [36][64][4]
 *   dense_view : position (y * (view_w - 4) + x) * 32 + channel                                                  [K/8][8][64][4]
 *   dense_emb  : feature index (padded to a multiple of 8)                                                       [FK/8][8][64][4]
 *   head       : hidden unit (dense_view's 256, then dense_emb's 256); outputs 0..n_action-1 = advantage, output n_action = value,
 *                the rest zero                                                                                   [64][64][4]
 * Channels, hidden units and biases are in their natural order (float[32], float[256], float[256]). */
typedef struct {
    const void *conv1, *conv2, *dense_view, *dense_emb, *head;
    const float *conv2_bias, *dense_view_bias, *dense_emb_bias;
    float value_bias;
} PolicyDqnWeightsF32;

/* 1 if the f32 kernels take this shape (view_c <= 7, feat <= 56, n_action <= 31, views up to ~19 x 19: the conv kernel's LDS images of
 * two agents must fit 160 KB) */
int policy_dqn_f32_supported(const PolicyDqnShape *shape);
/* size of the activation workspace (conv2's output, float32) for n agents */
int policy_dqn_f32_act_bytes(const PolicyDqnShape *shape, int n, size_t *bytes);
/* as policy_dqn_infer: view float[n][view_h][view_w][view_c], feature float[n][feat] as env_get_observation_device writes them */
int policy_dqn_infer_f32(const PolicyDqnShape *shape, const PolicyDqnWeightsF32 *weights, const float *view, const float *feature, int n,
                         void *act_workspace, int *actions, float *q, void *stream);

/* ---- the deep recurrent Q network's acting step (magent_amd/builtin/torch_model/drqn.py: _RecurrentQNet, one GRU step per agent) in
 * float32 -- magent_amd/csrc/policy_drqn_f32.hip.  The trunk is the DQN's (the f32 entries above); a GRU(512) cell follows, then the head
 * over its output h'.  Weights in f32 fragment order:
 *   gru  : torch's weight_ih_l0 and weight_hh_l0 [3 x 512][512] (gates r, z, n) side by side, K = x's 512 units, then h's 512;
 *          the three gate tiles of hidden tile T are adjacent: group m, tile T, gate G at [m][3 T + G]                  [128][48][64][4]
 *   head : K = the 512 state units; dueling: outputs 0..n_action-1 = advantage, output n_action = value; otherwise outputs
 *          0..n_action-1 = value; the rest zero                                                                       [64][64][4]
 * gru_bias  float[4][512]: b_ir + b_hr, b_iz + b_hz, b_in, b_hn (the gates' biases; b_hn stays inside the reset gate's product)
 * gru_bias0 the same for a zero state: W_h* 0 added to each hidden bias (0, or NaN where a row of weight_hh_l0 is not finite, as torch's
 *           W_h @ 0) -- used when the state table is empty
 * head_bias float[32]: per output (dueling: the value's bias at n_action, zeros elsewhere) */
typedef struct {
    PolicyDqnWeightsF32 trunk;    /* conv1 .. dense_emb and their biases as for policy_dqn_infer_f32; trunk.head and trunk.value_bias are not read */
    const void *gru;
    const float *gru_bias, *gru_bias0;
    const void *head;
    const float *head_bias;
    int dueling;
} PolicyDrqnWeightsF32;

/* 1 if the DRQN kernels take this shape: policy_dqn_f32_supported's region (the state is 512 wide) */
int policy_drqn_f32_supported(const PolicyDqnShape *shape);
/* size of the workspace of one call with n agents (the trunk's activations, then the GRU's input float[n][512]) */
int policy_drqn_f32_workspace_bytes(const PolicyDqnShape *shape, int n, size_t *bytes);
/* One step of n agents.  ids int[n]: this call's agent ids.  The state table of the previous call: prev_sorted_ids int[count] its ids
 * sorted ascending (stably: equal ids in that call's order), rows int[count] the row of `states` float[.][512] holding each one's state.
 * Agent i starts from the row of the LAST entry of prev_sorted_ids equal to ids[i] (the last occurrence of a duplicated id), or from
 * zeros if there is none; count == 0 is an empty table.  new_states float[n][512]: h' of agent i in row i (must not overlap `states`).
 * states, new_states and the workspace are 16-byte aligned (a call with one that is not is refused).
 * actions[i] = torch.argmax of Q row i (a NaN first, then the larger value, then the lower index); q (optional) float[n][n_action].
 * Enqueues four kernels on `stream` and returns 0, or non-zero if the shape is not supported / a pointer is missing / a launch failed. */
int policy_drqn_infer_f32(const PolicyDqnShape *shape, const PolicyDrqnWeightsF32 *weights, const float *view, const float *feature, int n,
                          const int *ids, const int *prev_sorted_ids, const int *rows, const float *states, int count, float *new_states,
                          void *workspace, int *actions, float *q, void *stream);

/* ---- the same recurrent network with bf16 matrix operands (v_mfma_f32_32x32x16_bf16) -- magent_amd/csrc/policy_drqn_bf16.hip: an opt-in,
 * as policy_dqn_infer is beside policy_dqn_infer_f32.  The trunk is the bf16 DQN's (k_dqn_conv, then k_dqn_head stopped after its hidden
 * layer); it leaves x = relu(dense_view) || relu(dense_emb) as bf16[n][512] in the workspace, in hidden SLOT order (value 32 T' + s of a
 * row is hidden unit 32 T' + slot s's output, T' = 0..15: the order PolicyDqnWeights' head reads).
 * Rounded to bf16 (nearest even): the views, the features, every weight matrix, conv1's bias, the conv outputs, the two hidden halves,
 * h as the GRU's operand and h' as the head's operand.  Everything else is float32: accumulation, the other biases, the gates and the
 * blend h' = (1 - z) n + z h, which takes the UNROUNDED h.  The state table is the f32 entry's, float[.][512]: the two paths can hand
 * their states to each other, and bf16 error does not compound through the blend.
 * Weights in (bf16) fragment order:
 *   gru  : torch's weight_ih_l0 and weight_hh_l0 [3 x 512][512] (gates r, z, n) side by side; K = x's 512 hidden SLOTS (weight_ih_l0's
 *          columns permuted: column 32 T' + s is the weight of unit 32 T' + (s & 3) + 8 ((s & 15) >> 2) + 4 (s >> 4)), then h's 512 units in
 *          natural order; the three gate tiles of hidden tile T are adjacent: k-step s, tile T, gate G at [s][3 T + G]; outputs (hidden
 *          units) in natural order                                                                                       [64][48][64][8]
 *   head : K = the 512 state units, natural order; outputs as for PolicyDrqnWeightsF32's head                           [32][64][8]
 * gru_bias, gru_bias0, head_bias: float, as for PolicyDrqnWeightsF32 (gru_bias0's NaN marks a row of the bf16-ROUNDED weight_hh_l0 that is
 * not finite) */
typedef struct {
    PolicyDqnWeights trunk;       /* conv1 .. dense_emb and their biases as for policy_dqn_infer; trunk.head and trunk.value_bias are not read */
    const void *gru;
    const float *gru_bias, *gru_bias0;
    const void *head;
    const float *head_bias;
    int dueling;
} PolicyDrqnWeights;

/* 1 if the bf16 DRQN kernels take this shape: policy_dqn_supported's region */
int policy_drqn_supported(const PolicyDqnShape *shape);
/* size of the workspace of one call with n agents (the trunk's activations, then x bf16[n][512]) */
int policy_drqn_workspace_bytes(const PolicyDqnShape *shape, int n, size_t *bytes);
/* One step of n agents: the arguments, the state table's look-up (the last equal entry; an absent id starts from zeros; count == 0 takes
 * gru_bias0), the alignment rule (states, new_states, workspace: 16 bytes), the actions' order and the return codes of
 * policy_drqn_infer_f32.  Four kernels on `stream`; a refused call has written nothing. */
int policy_drqn_infer(const PolicyDqnShape *shape, const PolicyDrqnWeights *weights, const float *view, const float *feature, int n,
                      const int *ids, const int *prev_sorted_ids, const int *rows, const float *states, int count, float *new_states,
                      void *workspace, int *actions, float *q, void *stream);
/* the same with the views as the engine's bf16 cells ([n][view_h][view_w][8], channel 7 = 1.0; 16-byte aligned), as policy_dqn_infer_bf16 */
int policy_drqn_infer_bf16(const PolicyDqnShape *shape, const PolicyDrqnWeights *weights, const void *view_cells, const float *feature, int n,
                           const int *ids, const int *prev_sorted_ids, const int *rows, const float *states, int count, float *new_states,
                           void *workspace, int *actions, float *q, void *stream);

/* ---- the segmented DRQN step: one call over the packed rows of many worlds (EnvBatch.packed_offsets), every world with its own id
 * namespace.  The state table is keyed by (segment, id): it holds int64 keys (segment << 32) | uint32(id), sorted ascending (stably),
 * in place of the plain entries' sorted ids.  Segment s of a call is world s; the plain entries' table is segment 0's.  Two steps:
 *
 * 1. policy_drqn_lookup_seg_f32 / policy_drqn_lookup_seg (one kernel, exported by either file family) -- ONE small launch over all n rows:
 *      ids int[n]; the table seg_begin / seg_count / n_seg (HOST arrays) in policy_a2c_infer_f32_seg's format, with its validation and its
 *      cap POLICY_A2C_MAX_SEGMENTS (it travels by value in the kernel's arguments); seg_first: the number of table segment 0 among the
 *      call's segments (a call of more segments than the cap makes several look-ups over row ranges; 0 <= seg_first < 2^31 - 257);
 *      prev_sorted_keys int64[count], rows int[count]: the previous call's table (count == 0: empty).
 *    Writes from_row int[n]: for a row in a segment the row of the previous `states` that the LAST entry of prev_sorted_keys equal to its
 *    key names (the plain entries' duplicate rule), -1 if there is none; -1 for a row in no segment.  Writes keys int64[n]: the row's key
 *    in THIS call's table; a row in no segment gets 0x7FFFFFFFFFFFFFFF, which no look-up produces and which sorts to the end: pad and
 *    stale rows stay in the table, nobody finds them, and no host synchronisation is needed to drop them.
 *    Returns 0; 1 for a refused table or argument -- nothing is written --, 2 / 3 as the entries above.
 * 2. policy_drqn_infer_f32_rows / policy_drqn_infer_rows / policy_drqn_infer_bf16_rows -- the plain entries with (ids, prev_sorted_ids,
 *    rows, states, count) replaced by (from_row, states): agent i starts from row from_row[i] of `states`, or from zeros if from_row[i] < 0;
 *    states == NULL is the empty table (gru_bias0, from_row is not read but must be given).  Rows are independent: any row range of the
 *    call can go to a call of its own (from_row + beg).  Trunk, head, alignment rule (states, new_states, workspace: 16 bytes), return
 *    codes and "a refused call has written nothing" are the plain entries'; the GRU kernels are the plain entries' own. */
int policy_drqn_lookup_seg_f32(const int *ids, int n, const int *seg_begin, const int *seg_count, int n_seg, int seg_first,
                               const long long *prev_sorted_keys, const int *rows, int count, int *from_row, long long *keys, void *stream);
int policy_drqn_lookup_seg(const int *ids, int n, const int *seg_begin, const int *seg_count, int n_seg, int seg_first,
                           const long long *prev_sorted_keys, const int *rows, int count, int *from_row, long long *keys, void *stream);
int policy_drqn_infer_f32_rows(const PolicyDqnShape *shape, const PolicyDrqnWeightsF32 *weights, const float *view, const float *feature, int n,
                               const int *from_row, const float *states, float *new_states, void *workspace, int *actions, float *q, void *stream);
int policy_drqn_infer_rows(const PolicyDqnShape *shape, const PolicyDrqnWeights *weights, const float *view, const float *feature, int n,
                           const int *from_row, const float *states, float *new_states, void *workspace, int *actions, float *q, void *stream);
int policy_drqn_infer_bf16_rows(const PolicyDqnShape *shape, const PolicyDrqnWeights *weights, const void *view_cells, const float *feature, int n,
                                const int *from_row, const float *states, float *new_states, void *workspace, int *actions, float *q, void *stream);

/* ---- one acting step of the advantage actor-critic (magent_amd/builtin/torch_model/a2c.py: _ActorCritic.forward, then the action draw)
 * in float32 -- magent_amd/csrc/policy_a2c_f32.hip.  No convolution: the flattened view (K = view_h * view_w * view_c values, in the
 * order env_get_observation_device writes them) feeds a dense layer.  Weights in f32 fragment order, biases in natural order:
 *   dense_view : K padded to a multiple of 8 with zero weights                                                        [KP/8][8][64][4]
 *   dense_emb  : feature index (padded to a multiple of 8)                                                            [FK/8][8][64][4]
 *   dense      : K = dense_view's 256 units, then dense_emb's 256                                                     [64][16][64][4]
 *   comm[s]    : CommNet step s = 0, 1 (use_comm): C_s and H_s [512][512] side by side, K = the 512 means of the OTHER agents' units,
 *                then the agent's own 512; NULL without use_comm                                                      [128][16][64][4]
 *   head       : K = the 512 hidden units; outputs 0..n_action-1 = policy logits, output n_action = value, the rest zero  [64][64][4]
 * dense_view_bias, dense_emb_bias float[256]; dense_bias float[512]; head_bias float[32] per output of `head`. */
typedef struct {
    const void *dense_view, *dense_emb, *dense;
    const void *comm[2];
    const void *head;
    const float *dense_view_bias, *dense_emb_bias, *dense_bias, *head_bias;
    int use_comm;
} PolicyA2cWeightsF32;

/* 1 if the A2C kernels take this shape: view_h, view_w, view_c >= 1 with view_h * view_w * view_c <= 4096 (view_c is NOT limited to 7:
 * there is no convolution; the bound keeps the packed dense_view inside one 4 MB L2), 1 <= feat <= 64, 1 <= n_action <= 31 (the policy's
 * outputs and the value share one 32-wide tile) */
int policy_a2c_f32_supported(const PolicyDqnShape *shape);
/* size of the workspace of one call with n agents: two (use_comm: three) float[n][512] layers, and with use_comm the column sums'
 * partial blocks */
int policy_a2c_f32_workspace_bytes(const PolicyDqnShape *shape, int n, int use_comm, size_t *bytes);
/* One step of n agents.  u float[n]: one uniform number in [0, 1) per agent.  policy (optional) float[n][n_action] = clamp(softmax(logits),
 * 1e-10, 1 - 1e-10); value (optional) float[n].  The draw, in float32 and in this order: c_0 = p_0, c_a = c_(a-1) + p_a,
 * t = u * c_(n_action-1); actions[i] = the smallest a with c_a > t, or n_action - 1 if there is none (rounding, a NaN in the row): always
 * inside [0, n_action).  With use_comm the means run over ALL n agents of the call; the column sums are taken over blocks of 256 agents
 * in agent order and then over the blocks in order (no atomics), so the result is a function of the inputs alone.  The workspace is
 * 16-byte aligned.  Enqueues its kernels (3, with use_comm 9) on `stream` and returns 0, or non-zero with nothing written if the shape is
 * not supported / a pointer is missing / the workspace is misaligned / a launch failed. */
int policy_a2c_infer_f32(const PolicyDqnShape *shape, const PolicyA2cWeightsF32 *weights, const float *view, const float *feature, int n,
                         const float *u, void *workspace, int *actions, float *policy, float *value, void *stream);

/* ---- the same actor-critic step with bf16 matrix operands (v_mfma_f32_32x32x16_bf16) -- magent_amd/csrc/policy_a2c_bf16.hip: an opt-in, as
 * policy_drqn_infer is beside policy_drqn_infer_f32.
 * Rounded to bf16 (nearest even): the views (the cells entry takes the engine's cells as they are), the features, every weight matrix, and
 * every inter-layer activation ONCE, when it is stored: x = [relu(dense_view) | relu(dense_emb)], h0 = relu(dense), each CommNet step's
 * output -- rows bf16[n][512] in natural unit order (no slot permutation anywhere).  The stored row is what everything downstream reads:
 * the next layer's operand, the CommNet `skip` term and the column sums.  others_i = (sum - h_i) / (n - 1) is formed in float32 from the
 * float32 column sum and the stored row, then rounded as the operand (zeros for n == 1).  Everything else is float32: accumulation, all
 * biases (added behind the MFMA), relu and tanh, the column sums (over blocks of 256 agents in agent order, then over the blocks in order:
 * no atomics), the logits, the softmax, the clamp, the value and the draw (policy_a2c_infer_f32's, the same code).
 * Weights in (bf16) fragment order (PolicyDqnWeights: k-step s, tile T, lane l holds W[32 T + (l & 31)][16 s + 8 (l >> 5) + 0..7]),
 * outputs and biases in natural order:
 *   dense_view       : K = view_h * view_w * view_c in the float32 view's order, padded to a multiple of 16 with zero weights   [KP/16][8][64][8]
 *   dense_view_cells : the same matrix for the engine's cells [view_h][view_w][8]: K' = 8 view_h view_w, k = 8 cell + channel, padded to a
 *                      multiple of 16 (one cell); zero weights for channels >= view_c, so the cells' constant 1.0 in channel 7 meets
 *                      a zero.  NULL where the shape has no cells (view_c > 7 or K' > 4096)                             [K'P/16][8][64][8]
 *   dense_emb        : feature index, padded to a multiple of 16                                                         [FK/16][8][64][8]
 *   dense            : K = dense_view's 256 units, then dense_emb's 256                                                  [32][16][64][8]
 *   comm[s]          : CommNet step s = 0, 1 (use_comm): C_s and H_s side by side, K = the 512 means of the OTHER agents' units, then the
 *                      agent's own 512; NULL without use_comm                                                            [64][16][64][8]
 *   head             : K = the 512 hidden units; outputs 0..n_action-1 = policy logits, output n_action = value, the rest zero  [32][1][64][8]
 * dense_view_bias, dense_emb_bias float[256]; dense_bias float[512]; head_bias float[32]: as for PolicyA2cWeightsF32. */
typedef struct {
    const void *dense_view, *dense_view_cells, *dense_emb, *dense;
    const void *comm[2];
    const void *head;
    const float *dense_view_bias, *dense_emb_bias, *dense_bias, *head_bias;
    int use_comm;
} PolicyA2cWeights;

/* 0 if the bf16 A2C kernels do not take this shape; otherwise bit 0 is set: policy_a2c_infer (float32 views) takes it --
 * policy_a2c_f32_supported's region, view_h * view_w * view_c <= 4096, 1 <= feat <= 64, 1 <= n_action <= 31 -- and bit 1 says whether
 * policy_a2c_infer_bf16 (cells) takes it too: additionally view_c <= 7 and 8 * view_h * view_w <= 4096.  So 0, 1 or 3. */
int policy_a2c_supported(const PolicyDqnShape *shape);
/* size of the workspace of one call with n agents: two (use_comm: three) bf16[n][512] layers, and with use_comm the column sums' partial
 * blocks (float32) */
int policy_a2c_workspace_bytes(const PolicyDqnShape *shape, int n, int use_comm, size_t *bytes);
/* One step of n agents: the arguments, the draw, the span of the CommNet means (ALL n agents of the call), the alignment rule (workspace:
 * 16 bytes) and the return codes of policy_a2c_infer_f32.  Enqueues its kernels (3, with use_comm 9) on `stream`; a refused call has
 * written nothing. */
int policy_a2c_infer(const PolicyDqnShape *shape, const PolicyA2cWeights *weights, const float *view, const float *feature, int n,
                     const float *u, void *workspace, int *actions, float *policy, float *value, void *stream);
/* the same with the views as the engine's bf16 cells ([n][view_h][view_w][8], channel 7 = 1.0; 16-byte aligned: a cell is one load and one
 * half of a k-step, nothing is converted); needs weights->dense_view_cells */
int policy_a2c_infer_bf16(const PolicyDqnShape *shape, const PolicyA2cWeights *weights, const void *view_cells, const float *feature, int n,
                          const float *u, void *workspace, int *actions, float *policy, float *value, void *stream);

/* ---- the segmented form of the actor-critic step, float32 and bf16: ONE call over n packed rows that belong to several independent
 * groups of agents (the environments of an EnvBatch: packed_offsets / packed_segments), every CommNet mean taken inside the agent's own
 * group.  The arguments of the plain entries, then the table: seg_begin int[n_seg], seg_count int[n_seg] -- HOST arrays, read before the
 * call returns -- segment s is rows seg_begin[s] .. seg_begin[s] + seg_count[s] - 1.
 *   others_i = (sum over the rows j of i's segment of h_j - h_i) / (count - 1), zeros for count == 1.  The column sums of segment s are
 *   taken over blocks of 256 agents counted from the segment's OWN first row, in agent order, then over the blocks in order (no atomics):
 *   the partition and order of the plain entry called on rows seg_begin[s] .. of view, feature and u alone, so every output of a
 *   segment's rows has that call's bits, wherever the segment lies in the packed buffers.
 *   A row in no segment (a pad row between two segments, a stale row behind a world's living agents) is a segment of one: others = 0.
 *   Its outputs are written like any row's -- an action inside [0, n_action) -- and it enters no sum: a NaN there reaches nobody.
 *   An empty segment (count == 0) is allowed and costs nothing; n_seg == 0: every row is alone.  Without use_comm the table is checked
 *   and otherwise not looked at: the outputs are the plain entry's bits.  One segment (0, n) gives the plain entry's bits too.
 * Refused (1 returned, nothing written) unless 0 <= n_seg <= POLICY_A2C_MAX_SEGMENTS, every seg_begin >= 0 and seg_count >= 0,
 * seg_begin[s] + seg_count[s] <= n, and the segments ascend without overlap: seg_begin[s] >= seg_begin[s - 1] + seg_count[s - 1]; and
 * for whatever the plain entry refuses.  A longer table is cut at segment boundaries into several calls (segments are independent).
 * The table reaches the device as a kernel argument: no allocation, no copy from the host arrays, no wait.  With use_comm the call
 * enqueues 10 kernels (the plain 9 and the one that spreads the table), fewer where no segment has an agent; without, the plain 3.
 * The workspace (16-byte aligned) holds, beside the plain call's rows, one sum row per segment, at most n / 256 + n_seg partial rows
 * and the row -> segment map: policy_a2c_*workspace_bytes_seg(shape, n, use_comm, n_seg). */
#define POLICY_A2C_MAX_SEGMENTS 256
int policy_a2c_f32_workspace_bytes_seg(const PolicyDqnShape *shape, int n, int use_comm, int n_seg, size_t *bytes);
int policy_a2c_infer_f32_seg(const PolicyDqnShape *shape, const PolicyA2cWeightsF32 *weights, const float *view, const float *feature, int n,
                             const float *u, void *workspace, int *actions, float *policy, float *value, void *stream,
                             const int *seg_begin, const int *seg_count, int n_seg);
int policy_a2c_workspace_bytes_seg(const PolicyDqnShape *shape, int n, int use_comm, int n_seg, size_t *bytes);
int policy_a2c_infer_seg(const PolicyDqnShape *shape, const PolicyA2cWeights *weights, const float *view, const float *feature, int n,
                         const float *u, void *workspace, int *actions, float *policy, float *value, void *stream,
                         const int *seg_begin, const int *seg_count, int n_seg);
/* the same with the views as the engine's bf16 cells, as policy_a2c_infer_bf16 */
int policy_a2c_infer_bf16_seg(const PolicyDqnShape *shape, const PolicyA2cWeights *weights, const void *view_cells, const float *feature, int n,
                              const float *u, void *workspace, int *actions, float *policy, float *value, void *stream,
                              const int *seg_begin, const int *seg_count, int n_seg);

#ifdef __cplusplus
}
#endif
#endif /* MAGENT_AMD_POLICY_H */
