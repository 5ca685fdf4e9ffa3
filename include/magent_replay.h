/* magent_replay.h -- the C-ABI of the device episode recorder (magent_amd/csrc/replay.hip; host side: magent_amd/replay.py).
 *
 * A recorder collects the transitions of the tracked agents of ONE side of a packed EnvBatch during one round: per cycle the rows of
 * the packed observation, action and reward buffers that belong to tracked agents are copied into a step-major log on the device, and
 * at the round's end the log is scattered into episode order.  Agents are keyed by (segment << 32) | uint32(id), the segmented DRQN
 * table's key (include/magent_policy.h: policy_drqn_lookup_seg).  Nothing here allocates, copies to the host or waits for the device:
 * all storage is the caller's (ReplayState), all work is enqueued on `stream`.
 *
 * Return values of every entry: 0; 1: a refused argument (nothing was enqueued); 2: the runtime refused the stream's device;
 * 3: a launch failed.
 */
#ifndef MAGENT_REPLAY_H
#define MAGENT_REPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REPLAY_NO_KEY 0x7FFFFFFFFFFFFFFFLL /* the key of an empty slot and of a row in no segment: sorts behind every key */
#define REPLAY_SCAN_BLOCK 1024             /* slots per workgroup of the scans; blk holds one int per such block */
/* counters (int32 [REPLAY_COUNTERS]).  The transitions in the log and the sticky overflow flag are kept twice: call number c reads
 * the pair of parity c & 1 and writes the pair of parity (c + 1) & 1, so no workgroup reads a word another one of its launch writes. */
#define REPLAY_COUNTERS 8
#define REPLAY_C_TRACKED 0
#define REPLAY_C_FILL(parity) (2 + 2 * (parity))
#define REPLAY_C_OVERFLOW(parity) (3 + 2 * (parity))
/* flags of a slot */
#define REPLAY_F_RECORDED 1 /* the agent was recorded in the previous call */
#define REPLAY_F_DIED 2     /* the agent was recorded in one call and absent from the next */

/* The recorder's device storage.  Before the first call (and to reset): key_of_slot and sorted_keys filled with REPLAY_NO_KEY,
 * row_of_slot with -1, len, flags and counters with 0. */
typedef struct ReplayState {
    long long *key_of_slot; /* [capacity] the tracked keys in admission order (the slot number is the admission rank) */
    long long *sorted_keys; /* [capacity] the same keys ascending ...                                                 */
    int *sorted_slot;       /* [capacity] ... and the slot of each (a stable sort's indices, as int32)                */
    int *row_of_slot;       /* [capacity] the row of this call that holds the slot's agent, -1: absent                */
    int *len;               /* [capacity] transitions recorded of the slot's agent                                    */
    int *flags;             /* [capacity] REPLAY_F_*                                                                  */
    int *src_row;           /* [capacity] the rows recorded by this call, in slot order                               */
    int *blk;               /* [ceil(capacity / REPLAY_SCAN_BLOCK)] per-block sums of the scans                       */
    int *counters;          /* [REPLAY_COUNTERS]                                                                      */
    void *log_view;         /* [max_transitions][view_row_bytes] the log, step-major: a call appends its rows         */
    void *log_feat;         /* [max_transitions][feat_row_bytes]                                                      */
    int *log_act;           /* [max_transitions]                                                                      */
    float *log_rew;         /* [max_transitions]                                                                      */
    int *log_slot;          /* [max_transitions] the slot of a log row ...                                            */
    int *log_ord;           /* [max_transitions] ... and its number within that slot's episode                        */
    int capacity, max_transitions;
    int view_row_bytes, feat_row_bytes; /* multiples of 4; the buffers are 16-byte aligned                            */
} ReplayState;

/* The look-up of one call: ids int32 [n] (device); (seg_begin, seg_count)[n_seg] the host table of magent_policy.h's segmented entries
 * (begin, count >= 0, begin + count <= n, ascending without overlap) with any n_seg >= 0: a table of more than
 * POLICY_A2C_MAX_SEGMENTS segments is cut at segment boundaries into several launches.  Segment s of the table is world s.
 *   row_key [n], row_slot [n] (both or neither): per row its key and the slot that tracks it, -1 for an untracked key; a row in no
 *     segment takes REPLAY_NO_KEY and -2.
 *   mark != 0: row_of_slot[slot] = the LAST row of the call that holds the slot's key (an integer maximum). */
int replay_find(const ReplayState *st, const int *ids, int n, const int *seg_begin, const int *seg_count, int n_seg, long long *row_key,
                int *row_slot, int mark, void *stream);

/* Admission, in three steps around two sorts that are the caller's.
 * replay_candidates: cand_key[p] = the key of row order[p] if that row is in a segment and untracked, else REPLAY_NO_KEY (order:
 *   int32 [n] on the device, a permutation of the rows -- an entry outside 0 .. n - 1 offers nothing --; NULL: row order).
 * The caller sorts cand_key STABLY ascending into (sorted_cand, cand_pos int64).
 * replay_admit: the first entry of every run of equal keys is that key's first offer in `order`'s order; the offers are ranked in that
 *   order and, while slots are free, appended to key_of_slot; counters[REPLAY_C_TRACKED] grows.  first: int32 [n] workspace.
 * The caller then sorts key_of_slot stably into (sorted_keys, sorted_slot). */
int replay_candidates(const ReplayState *st, const long long *row_key, const int *row_slot, const int *order, int n, long long *cand_key,
                      void *stream);
int replay_admit(const ReplayState *st, const long long *cand_key, const long long *sorted_cand, const long long *cand_pos, int n, int *first,
                 void *stream);

/* The step of call number `call` (0, 1, ... since the reset), after replay_find(.., mark = 1).
 * record != 0: every tracked agent with a row appends one transition (view row, feature row, action, reward) to the log; one that was
 *   recorded by the previous call and has no row died.  If the call's transitions do not all fit, nothing at all is recorded or
 *   detected by this and every later call, and the overflow flag is set.  max_rows: the host's upper bound of the rows the call can
 *   record (it sizes the copy's grid; the true number is read on the device).
 * record == 0 (close): the deaths are detected, nothing is recorded and no agent becomes "recorded by the previous call".
 * row_of_slot is -1 everywhere afterwards. */
int replay_step(const ReplayState *st, int call, int record, int max_rows, const void *view, const void *feat, const int *acts,
                const float *rewards, void *stream);

/* replay_step's copy launch on its own (tools/replay_rate.py times it): rows src_row[j] of the four arrays go to log rows fill + j for
 * j < min(counters[REPLAY_C_FILL((call & 1) ^ 1)] - fill, max_rows), fill = counters[REPLAY_C_FILL(call & 1)] -- `counters` and
 * `src_row` are the caller's here, not the state's.  The caller answers for src_row's entries being rows of the arrays and for the log
 * taking fill + max_rows rows. */
int replay_copy(const ReplayState *st, const int *counters, int call, int max_rows, const void *view, const void *feat, const int *acts,
                const float *rewards, const int *src_row, void *stream);

/* The round's end, after `calls` steps: the n_trans rows of the log (the caller read counters[REPLAY_C_FILL(calls & 1)]) go to episode
 * order -- slots ascending, each slot's transitions in time order.  terminal (1 byte per row): the last transition of an agent that
 * died; mask: 0.0 on the last transition of one that did not, else 1.0.  base: int32 [capacity], dst: int32 [n_trans] workspace. */
int replay_pack(const ReplayState *st, int n_trans, void *out_view, void *out_feat, int *out_act, float *out_rew, unsigned char *out_terminal,
                float *out_mask, int *base, int *dst, void *stream);

/* The A2C's discounted returns of the packed round, after replay_pack: `base` as replay_pack left it, rew float32 [n_trans] the packed
 * rewards, boot float32 [n_slots] one bootstrap value per slot, out_ret float32 [n_trans] (not overlapping rew).  For every slot
 * s < n_slots (<= capacity) with len[s] > 0:
 *     keep = (double)boot[s];  for i = len[s] - 1 down to 0:  keep = keep * gamma + (double)rew[base[s] + i];  out_ret[base[s] + i] = (float)keep
 * in IEEE double with the product and the sum rounded SEPARATELY (no fused multiply-add), rounded once to float32: bit for bit what
 * AdvantageActorCritic.train computes on the host.  A slot of length 0 writes nothing and its boot entry is not read.  A NULL pointer,
 * a negative count, n_slots > capacity or n_trans > max_transitions is refused (1); n_slots == 0 or n_trans == 0 returns 0 and writes
 * nothing.
 * replay_returns stages a workgroup's contiguous rows in LDS where they fit; replay_returns_direct is the same function with every lane
 * on global memory (tools/a2c_train_rate.py times both). */
int replay_returns(const ReplayState *st, int n_slots, int n_trans, const int *base, const float *rew, const float *boot, double gamma,
                   float *out_ret, void *stream);
int replay_returns_direct(const ReplayState *st, int n_slots, int n_trans, const int *base, const float *rew, const float *boot, double gamma,
                          float *out_ret, void *stream);

#ifdef __cplusplus
}
#endif
#endif
