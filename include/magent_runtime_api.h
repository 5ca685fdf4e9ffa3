/*
 * magent_runtime_api.h -- C-ABI of the MI355X-native grid-world step engine (libmagent.so).
 *
 * This is the drop-in boundary.  Every symbol in PART 1 replaces, with the same name, argument order,
 * argument meaning and return value (always 0), the function the reference exports from
 * /root/reference/src/runtime_api.h:20-56 and that python/magent/gridworld.py binds through ctypes
 * (python/magent/c_lib.py:11-21 loads "<pkg>/../../build/libmagent.so").  Plain pointers and ints only:
 * no torch / HIP types appear in any signature.
 *
 * Ownership (same as the reference): the caller owns every data buffer and sizes it from
 * env_get_info("num") x the *_space infos; the engine owns the opaque EnvHandle until env_delete_game.
 * PART 1 buffers are HOST memory; each call is synchronous (outputs valid on return).
 * PART 2 is additive: the same operations on DEVICE pointers, asynchronous on the environment's HIP stream.
 * PART 3 holds the reference's three rule-based actors (host, runtime_api.h:64-73) and their device entry.
 *
 * Errors: like the reference (LOG(FATAL) -> std::terminate under ctypes, utility.h:77-80) an invalid
 * argument or an unsupported feature prints "magent-amd FATAL: ..." to stderr and aborts; nothing returns
 * non-zero expecting the caller to look.
 */
#ifndef MAGENT_AMD_RUNTIME_API_H
#define MAGENT_AMD_RUNTIME_API_H

#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *EnvHandle;  /* reference: Environment*  (Environment.h:36) */
typedef int GroupHandle;  /* reference: Environment.h:12; -1 = walls / "no group" (GridWorld.cc:184) */

/* ---------------------------------------------------------------------------------------------------
 * PART 1 -- the reference C-ABI (host buffers, synchronous)
 * ------------------------------------------------------------------------------------------------- */

/* runtime_api.h:21  name must be "GridWorld" ("DiscreteSnake" is a different game: FATAL unsupported). */
int env_new_game(EnvHandle *game, const char *name);
/* runtime_api.h:22 */
int env_delete_game(EnvHandle game);
/* runtime_api.h:23 -> GridWorld::set_config (GridWorld.cc:120-149).  keys: map_width,map_height (int*),
 * food_mode,turn_mode,minimap_mode,goal_mode (bool*), embedding_size (int*), render_dir (char*), seed (int*).
 * (turn_mode and food_mode are implemented; so is goal_mode, "deprecated" at GridWorld.cc:137 and set by no shipped game: what it
 * does in the reference is add two feature slots that nothing ever writes, GridWorld.cc:926-934.)
 * Additive key: device_id (int*) selects the HIP device (before env_reset). */
int env_config_game(EnvHandle game, const char *name, void *p_value);

/* runtime_api.h:26 -> GridWorld::reset (GridWorld.cc:72-118) */
int env_reset(EnvHandle game);
/* runtime_api.h:27 -> GridWorld::get_observation (GridWorld.cc:292-401)
 * buffer[0] = view   float[n][view_h][view_w][n_channel], buffer[1] = feature float[n][feature_size] */
int env_get_observation(EnvHandle game, GroupHandle group, float **buffer);
/* runtime_api.h:28 -> GridWorld::set_action (GridWorld.cc:403-454); actions int32[n].
 * A SECOND set_action for the same group before env_step appends, as in the reference: every agent of the group then acts once per
 * call (two entries in the shuffled attack list, two turns / moves in list order), and last_action is the latest call's.  No caller of the
 * reference does that, so it is served off the hot path: the step runs the reference's sequential loops on one lane of the device
 * (exact, about a microsecond per list entry; every game).  The same loops run a step in which a can_absorb group ("goals") was given
 * actions: such goals move like any agent in the reference (Map.cc:313-358), which the parallel move resolution does not cover.
 * An action outside [0, n_action) is reported at env_step (FATAL; the reference indexes out of range). */
int env_set_action(EnvHandle game, GroupHandle group, const int *actions);
/* runtime_api.h:29 -> GridWorld::step (GridWorld.cc:456-631) */
int env_step(EnvHandle game, int *done);
/* runtime_api.h:30 -> GridWorld::get_reward (GridWorld.cc:694-704); buffer float[n] */
int env_get_reward(EnvHandle game, GroupHandle group, float *buffer);

/* runtime_api.h:33 -> GridWorld::get_info (GridWorld.cc:709-894).  names: num,id,pos,alive,global_minimap,
 * walls_info,render_window_info,attack_event,action_space,view_space,feature_space,view2attack,attack_base,
 * groups_info,both_attack,mean_info ("deprecated" in the reference, GridWorld.cc:765-786: float[2 + n_action] = mean x,
 * mean y, share of every action; served since round 5 -- only ask for groups that have been given actions: the reference
 * counts an agent that never acted one past the end of a heap array).
 * Additive names (tuning / tests): engine_stats -> int32[8], round_hist -> int32[9] (magent_amd/gridworld.py). */
int env_get_info(EnvHandle game, GroupHandle group, const char *name, void *buffer);

/* runtime_api.h:36-37 -> RenderGenerator (text video dump; host-side, off the hot path) */
int env_render(EnvHandle game);
int env_render_next_file(EnvHandle game);

/* runtime_api.h:43 -> AgentType::AgentType (AgentType.cc:30-123) */
int gridworld_register_agent_type(EnvHandle game, const char *name, int n, const char **keys, float *values);
/* runtime_api.h:44 -> GridWorld::new_group (GridWorld.cc:160-169) */
int gridworld_new_group(EnvHandle game, const char *agent_type_name, GroupHandle *group);
/* runtime_api.h:45-46 -> GridWorld::add_agents (GridWorld.cc:180-290); method = random|custom|fill */
int gridworld_add_agents(EnvHandle game, GroupHandle group, int n, const char *method,
                         const int *pos_x, const int *pos_y, const int *dir);

/* runtime_api.h:49 -> GridWorld::clear_dead (GridWorld.cc:633-665) */
int gridworld_clear_dead(EnvHandle game);
/* runtime_api.h:50 -> GridWorld::set_goal (GridWorld.cc:667-679; deprecated in the reference).  method "random" draws a goal position
 * for every agent of the group from the engine's generator (two draws each, the uncleared dead included); nothing in the reference
 * reads a goal back, so the call's whole effect is on the generator -- on every shuffle and random placement after it -- with or
 * without goal_mode.  Any other method is FATAL, as there.  linear_buffer is unused, as there. */
int gridworld_set_goal(EnvHandle game, GroupHandle group, const char *method, const int *linear_buffer);

/* runtime_api.h:53-56 -> RewardEngine.cc:28-69 */
int gridworld_define_agent_symbol(EnvHandle game, int no, int group, int index);
int gridworld_define_event_node(EnvHandle game, int no, int op, int *inputs, int n_inputs);
int gridworld_add_reward_rule(EnvHandle game, int on, int *receiver, float *value, int n_receiver,
                              bool is_terminal, bool auto_value);

/* runtime_api.h:61-62: the second game of the reference; exported so that the symbol table matches,
 * FATAL "unsupported" when called. */
int discrete_snake_clear_dead(EnvHandle game);
int discrete_snake_add_object(EnvHandle game, int obj_id, int n, const char *method, const int *linear_buffer);

/* ---------------------------------------------------------------------------------------------------
 * PART 2 -- additive MI355X extensions (device-resident buffers; SURVEY.md 8b "extensions allowed")
 * All pointers below are DEVICE pointers on the environment's device.  Calls enqueue work on the
 * environment's HIP stream and return without waiting; env_sync() waits for the stream.
 * Observation views come in two formats: float32 [n][view_h][view_w][n_channel], the layout of env_get_observation
 * (env_get_observation_device, env_cycle_many), and bf16 cells [n][view_h][view_w][8], one 16-byte vector per window cell
 * (env_get_observation_device_bf16; per entry in env_cycle_many_cells).  Feature rows are float32 in both.
 * ------------------------------------------------------------------------------------------------- */

/* same layout as env_get_observation, written straight into caller-owned device memory */
int env_get_observation_device(EnvHandle game, GroupHandle group, float **device_buffer);
/* the same observation in the policy kernels' input format (include/magent_policy.h): device_buffer[0] = view as bf16
 * [n][view_h][view_w][8] -- the n_channel (<= 7) channels of env_get_observation rounded to nearest even, zeros, and 1.0 in
 * channel 7; 16-byte aligned -- device_buffer[1] = feature float[n][feature_size] as above.  2.7 KB per agent instead of 4.7:
 * the render is HBM-write bound, and a policy that computes in bf16 reads these cells as its MFMA operands. */
int env_get_observation_device_bf16(EnvHandle game, GroupHandle group, void **device_buffer);
/* actions int32[n] in device memory */
int env_set_action_device(EnvHandle game, GroupHandle group, const int *device_actions);
/* rewards float[n] in device memory */
int env_get_reward_device(EnvHandle game, GroupHandle group, float *device_buffer);
/* name = id (int32[n]) | pos (int32[n][2]) | alive (uint8[n]) | hp (float[n]) into device memory */
int env_get_info_device(EnvHandle game, GroupHandle group, const char *name, void *device_buffer);
/* env_step for n independent environments at once: all steps are enqueued (each on its environment's stream) before
 * the first is waited for, so their device work overlaps; done[i] as env_step */
int env_step_many(EnvHandle *games, int n, int *done);
/* One full cycle of n_env independent environments, exactly the call sequence
 *   for g: env_get_observation_device(e, g, {view, feat});   for g: env_set_action_device(e, g, actions);
 *   env_step(e, &done[e]);   for g: env_get_reward_device(e, g, rewards);   gridworld_clear_dead(e)
 * Device pointer arrays are indexed [e * n_group + g]; a NULL entry skips that call for that group.
 * Three forms, chosen per environment:
 *   - worlds small enough for the one-launch step -- <= 1536 agents for an environment cycled on its own (n_env == 1), <= 16384 as one
 *     of a batch (n_env >= 2); MAGENT_TUNE solo_max / batch_solo_max -- run the whole cycle in TWO launches (observation render of
 *     all groups; everything else), and with n_env >= 2 ALL such environments share one pair of launches on the first one's stream
 *     (one workgroup per environment for the step): small worlds are launch-latency bound, many of them fill the GPU;
 *   - with n_env >= 2, worlds of >= 1537 agents (MAGENT_TUNE batch_pipe_min) whose game the pipeline of plain games takes (one-cell
 *     bodies, no turn_mode / food_mode / goals / kill_supply, rules that pay the attacker: battle, gather) share ONE chain of launches,
 *     one per phase for all of them, without a host round trip inside the cycle (pipe.hip; MAGENT_TUNE batch_pipe=0 switches it off);
 *   - every other world runs the calls one after the other on n_threads host threads inside the library.
 * `actions` must hold the actions BEFORE the call (they are read by the second launch, in
 * stream order after the render -- the caller's policy reads the observation of the PREVIOUS cycle, or orders its own
 * stream with env_get_stream); the outputs are complete when the call returns (the host has waited for `done`).
 * Concurrent calls from several host threads over disjoint sets of environments are supported (the library's worker threads serve one
 * call's round at a time). */
int env_cycle_many(EnvHandle *games, int n_env, int n_group, float **view, float **feat, const int **actions,
                   float **rewards, int *done, int n_threads);
/* env_cycle_many with the view format chosen PER ENTRY: view_cells[e * n_group + g] != 0 says that view[e * n_group + g] is a bf16-cell
 * buffer [n][view_h][view_w][8] in env_get_observation_device_bf16's format (the channels rounded to nearest even, zeros up to channel
 * 6, 1.0 in channel 7; 16-byte aligned), 0 that it is float32 as in env_cycle_many; view_cells == NULL: every entry is float32 -- that
 * is env_cycle_many itself, which is this call with NULL.  One side of a game may feed a bf16 network while the other feeds a rule actor
 * (actor_infer_action_device reads float32 views).  Everything else -- NULL entries, when `actions` are read, what is complete at
 * return, which of the three forms an environment takes (a cell row is 16 * view_h * view_w bytes: of a packed buffer's segments only the
 * feature pointer can still miss the 16-byte alignment the batched forms ask for) -- is env_cycle_many's, and so is the number of
 * launches: a render launch writes every (environment, group) slot in the slot's own format.  A cell entry for a game with more than
 * 7 channels, or one that is not 16-byte aligned, is FATAL as in env_get_observation_device_bf16. */
int env_cycle_many_cells(EnvHandle *games, int n_env, int n_group, void **view, const unsigned char *view_cells,
                         float **feat, const int **actions, float **rewards, int *done, int n_threads);
/* What the library's host-thread pool -- the workers of env_cycle_many(_cells) that run the environments of the third form -- has done in
 * this process so far: out[0] rounds (calls that handed two or more environments to it with n_threads >= 2), out[1] environment cycles
 * ("items") run in them, out[2] those of them run by worker threads and not by the calling thread, out[3] the most distinct threads that
 * ran at least one item in one round.  Relaxed counters, read-only, for tests and tuning; no device work. */
int env_cycle_pool_stats(long long out[4]);
/* out[e * n_group + g] = number of agents of group g in environment e (env_get_info "num" for a whole batch; host only) */
int env_num_many(EnvHandle *games, int n_env, int n_group, int *out);
/* env_get_info_device(e, g, "id", out[e * n_group + g]) for a whole batch in one launch: out[e * n_group + g] is a device pointer to
 * int32[n of that group]; a NULL entry skips that group, and so does an empty group.  `name` is "id" only (anything else is FATAL).
 * The (source, destination, n) items travel by value in the kernel's arguments, 192 to a launch (a larger batch takes several); no
 * allocation, no copy, no host wait.  Unlike the calls above, the work is enqueued on `stream`, the CALLER's hipStream_t (NULL: the null
 * stream): a caller that orders its stream behind the engine's (env_streams_many) reads the ids where it reads the observations.
 * Which ids describe which rows: env_cycle_many renders the observation of the population as it stands when the cycle STARTS, then steps
 * and compacts.  The ids (and env_num_many's counts) of the rows a cycle's render writes are therefore the ones taken BEFORE that cycle. */
int env_info_many(EnvHandle *games, int n_env, int n_group, const char *name, void **out, void *stream);
/* wait until everything enqueued on the environment's stream has finished */
int env_sync(EnvHandle game);
/* the environment's hipStream_t, as an opaque pointer (for event timing / interop by the caller) */
int env_get_stream(EnvHandle game, void **stream);
/* the hipStream_t on which the NEXT env_set_action_device will read its actions.  Worlds too large for the one-launch step
 * run set_action and the read-only head of env_step (attack shuffle, hit gather, death-rank fixed point) on a second
 * stream, beside the observation renders on env_get_stream's stream; a caller that produces actions
 * asynchronously on a stream of its own orders THIS stream behind it.  Equal to env_get_stream's for small worlds or
 * with MAGENT_TUNE overlap=0 (the default).  All outputs (observations, rewards, infos) are ordered on env_get_stream's stream as before. */
int env_get_action_stream(EnvHandle game, void **stream);
/* both streams of n_env environments in one call (out: 2 * n_env pointers, [2 e] = env_get_stream, [2 e + 1] = env_get_action_stream):
 * what a batch of environments needs to order its inputs once per DISTINCT stream -- environments cycled together share one */
int env_streams_many(EnvHandle *games, int n_env, void **out);

/* Kernel timing with HIP events recorded on the environment's stream.
 * env_profile_enable(game, 1) starts recording one event pair per launch of each named kernel; (game, 2) records
 * only the observation render launches ("render", "features") -- an event pair costs ~10 us of stream time, so this
 * is the level to leave on inside a timed region; (game, 0) stops.  env_profile_read returns, for kernel `name` ("render", "paint", "minimap", "attack", "move", ...),
 * the number of recorded launches and their total duration in milliseconds, and resets the counters. */
int env_profile_enable(EnvHandle game, int on);
int env_profile_read(EnvHandle game, const char *name, int *n_launches, float *total_ms);

/* ---------------------------------------------------------------------------------------------------
 * PART 3 -- rule-based actors (reference src/temp_c_booster.cc; magent_amd/csrc/actors.hip)
 * ------------------------------------------------------------------------------------------------- */

/* runtime_api.h:64-73, with the reference's exact signatures and, unlike the reference, as C symbols.  HOST buffers:
 * obs_buf = view float[n][height][width][n_channel], feature_buf / hp_buf = feature float[n][feature_size], act_buf = int32[n],
 * view2attack_buf = int32[height][width].  One sequential loop over the agents in ascending order, drawing from libc's own
 * random() / rand() at exactly the reference's points: for the same libc state, the actions and the state afterwards equal the
 * reference's run on one thread.  Two definitions of the product: rush_prey's threshold test reads feature_buf[i], the i-th
 * float of the flattened feature array (as the reference does); gather's minimap step with no minimap cell -- a division
 * by zero in the reference -- draws rand() % attack_base. */
void runaway_infer_action(float *obs_buf, float *feature_buf, int n, int height, int width, int n_channel,
                          int attack_base, int *act_buf, int away_channel, int move_back);
void rush_prey_infer_action(float *obs_buf, float *feature_buf, int n, int height, int width, int n_channel,
                            int *act_buf, int attack_channel, int attack_base,
                            int *view2attack_buf, float threshold);
void gather_infer_action(float *obs_buf, float *hp_buf, int n, int height, int width, int n_channel,
                         int *act_buf, int attack_base, int *view2attack_buf);

/* The same three policies on DEVICE observations. */
enum { MAGENT_ACTOR_RUNAWAY = 0, MAGENT_ACTOR_RUSH_PREY = 1, MAGENT_ACTOR_GATHER = 2 };
typedef struct MagentActorArgs {
    int kind;                       /* MAGENT_ACTOR_* */
    int n, height, width, n_channel;
    int attack_base;
    int channel;                    /* runaway: away_channel; rush_prey: attack_channel; gather: unused (channels 3, 4, 6) */
    int move_back;                  /* runaway */
    float threshold;                /* rush_prey */
    unsigned long long seed, counter;   /* the device's draws: DESIGN.md 3.16 */
} MagentActorArgs;
/* view float[n][height][width][n_channel], feature float[n][feature_size], view2attack int32[height * width] (unused by runaway),
 * actions int32[n], drew uint8[n] or NULL: all DEVICE pointers.  Enqueued on `stream` (a hipStream_t; NULL = the null stream);
 * no synchronisation, no allocation; n == 0 does nothing.  Every agent whose reference action involves no draw gets exactly the
 * reference's action and drew[i] = 0; an agent whose action comes from a draw gets drew[i] = 1 and an action uniform over the set
 * the reference draws from, drawn from a stateless stream of (seed, counter, agent, slot) instead of libc's state. */
int actor_infer_action_device(const MagentActorArgs *args, const float *view, const float *feature, const int *view2attack,
                              int *actions, unsigned char *drew, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MAGENT_AMD_RUNTIME_API_H */
