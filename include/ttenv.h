/* ttenv.h -- C ABI of libttenv.so: the batched truck-trailer backing environment on MI355X.
 *
 * The reference (pain7576/ddpg-trucktrailer) has no FFI; the interface its callers use for
 * this path is the gym-style Python surface of `Truck_trailer_Env_2`
 * (truck_trailer_sim/simv2.py:20-101, 459-545) plus the public attributes they read and
 * write (DDPG/trainv2.py:488-531, DDPG/test.py:96-115, DDPG/heatmap.py:79-168).  Each entry
 * point below names the reference interface it replaces; INTEGRATION.md shows the ctypes
 * stub that binds them behind that Python surface.
 *
 * Conventions
 *  - plain C: opaque handle, plain pointers and sizes, no C++/torch types;
 *  - every call returns 0 (TT_OK) or a negative TT_E* code and never throws;
 *    tt_last_error() returns a message owned by the handle (or by the library for a NULL handle);
 *  - every array pointer is a DEVICE pointer owned by the caller (e.g. torch `data_ptr()`),
 *    layouts as stated per argument; N = number of envs of the handle;
 *  - no entry point reads or writes outside the extents stated per argument.  A pointer needs the natural alignment of its
 *    element type, and 16 bytes -- what any torch allocation has -- where the kernels use 16-byte accesses: the parameter
 *    tensors of a tt_mlp_weights (w1, the per-neuron vectors, w2, w3, wa, ba), the [B,400] and [B,300] arrays of tt_mlp_saved
 *    and tt_mlp_bwd_ws (their [B] arrays rstd1, rstd2 and dpre are accessed as scalars), z_state, bias_corr_out, split_ws and
 *    fc2_img.  Gradient tensors (a tt_mlp_weights of gradients) and Adam moments may sit at their offsets in ONE flat,
 *    16-byte-aligned f32 buffer in tt_mlp_weights order (so wa and ba are only 4-byte aligned); observation, action, reward
 *    and done arrays may be slot views of a ring (4- and 1-byte aligned: the env's observation stores test the address);
 *  - work is enqueued on the caller's stream (`tt_stream_t` is `hipStream_t`; NULL = the
 *    default stream) and is asynchronous; nothing here synchronises or allocates after create;
 *  - one host thread per handle; handles are independent (one process per GPU, one handle per
 *    process is the multi-GPU model).
 */
#ifndef TTENV_H
#define TTENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT_VERSION 3
#define TT_OBS_DIM 23 /* simv2.py:76 */
#define TT_MAX_EPISODE_STEPS 4095 /* steps and max_episode_steps are 12-bit packed counters; larger values are TT_EINVAL */

enum { TT_OK = 0, TT_EINVAL = -1, TT_ENOMEM = -2, TT_EHIP = -3, TT_ENODEV = -4 };

/* termination causes, one bit each, in the order of simv2.py:528-541; bit 6 = reward-side success */
enum {
    TT_F_JACKKNIFE = 1, TT_F_OUT_OF_MAP = 2, TT_F_MAX_STEPS = 4, TT_F_GOAL_REACHED = 8,
    TT_F_GOAL_PASSED = 16, TT_F_EXCESSIVE_BACK = 32, TT_F_SUCCESS = 64
};
#define TT_TERM_SIMV2 0x3F /* all six causes end an episode (simv2.py:541) */
#define TT_TERM_SIMV1 0x0F /* jackknife | out of map | max steps | goal (simv1.py:432) */

/* `violation_type` of reward_functionv1.py:378-419, last writer wins */
enum {
    TT_V_NONE = 0, TT_V_JACKKNIFE, TT_V_JACKKNIFE_WARNING, TT_V_MAJOR_BOUNDARY, TT_V_MINOR_BOUNDARY,
    TT_V_PAST_THE_GOAL, TT_V_MAX_STEP, TT_V_EXCESSIVE_BACKWARD
};

/* rows of tt_info.comp, the reward_info dict of reward_functionv1.py:489-504 */
enum {
    TT_I_TOTAL = 0, TT_I_PROGRESS, TT_I_HEADING, TT_I_ORIENT, TT_I_STAGED, TT_I_SAFETY, TT_I_EXPLORE,
    TT_I_FINAL, TT_I_BACKWARD, TT_I_SMOOTH, TT_I_CUMBACK, TT_I_BUDGET, TT_NINFO
};

typedef struct ihipStream_t *tt_stream_t; /* == hipStream_t */
typedef struct tt_env tt_env;

/* Constants of Truck_trailer_Env_2.__init__ (simv2.py:23-101); variant 1 = simv1.py:23-99. */
typedef struct tt_params {
    double L1, L2;             /* wheelbase, trailer length (L2 is the default; per-env via tt_env_set_pose) */
    double hitch_offset, v1x;  /* 0.0, -5.012 */
    double dt;                 /* 0.08: one fixed Dormand-Prince step per env step */
    double map_min_x, map_max_x, map_min_y, map_max_y; /* -40..40 */
    double max_steer;          /* np.radians(45) */
    double position_threshold, orientation_threshold; /* 0.5, deg2rad(15) */
    double step_length;        /* 0.40096 (simv2.py:265) */
    int32_t extra_steps;       /* 75 */
    int32_t fixed_max_steps;   /* 0 = int(d0/step_length)+extra_steps (simv2); 300 (simv1.py:95) */
    uint32_t term_mask;        /* which TT_F_* bits end an episode */
    int32_t variant;           /* 0 simv2, 1 simv1 */
    int32_t stateless_reward;  /* 0: the reward carry persists over the episode (simv2.py:347-373);
                                  1: a fresh RewardFunction every step, nothing carried (simv1.py:435) */
    int32_t reserved_;
    double goal[3];            /* default goal x, y, yaw: 0, -30, pi/2 (simv2.py:335-337) */
    double reset_lo[3], reset_hi[3]; /* start x, y, yaw ~ U(lo, hi) (simv2.py:331-333) */
} tt_params;

/* Optional per-step detail: the `info` dict of env.step (reward_functionv1.py:489-504) and the
 * public flags callers read afterwards (heatmap.py:159-168).  Any member may be NULL. */
typedef struct tt_info {
    double *comp;       /* [TT_NINFO, N] f64, row-major by component (row TT_I_TOTAL = f64 reward) */
    uint8_t *violation; /* [N] TT_V_* */
    uint8_t *flags;     /* [N] TT_F_* bits, before masking with term_mask */
} tt_info;

int tt_version(void);
const char *tt_last_error(const tt_env *env);

/* Truck_trailer_Env_2() / Truck_trailer_Env_1(): fills `out` with the reference constants. */
int tt_params_default(int variant, tt_params *out);

/* Truck_trailer_Env_2.__init__ for N envs on HIP device `device` (simv2.py:23-101). */
int tt_env_create(int n_envs, int device, const tt_params *params, tt_env **out);
int tt_env_destroy(tt_env *env);
int tt_env_num_envs(const tt_env *env);

/* env.reset(seed) (simv2.py:459-498) for the envs whose mask byte is non-zero (NULL = all):
 * start pose ~ reset_lo/hi from counter-based Philox keyed by (seed, env, episode number) (distributional
 * parity with np.random.seed; the bit-exact seeded pose is tt_env_set_pose's job).  A full reset (mask NULL)
 * restarts every env at episode 0, so the poses are a pure function of `seed`; state stored
 * f32-rounded, step counter and reward carry cleared, obs rows written with steering 0.
 * Also fixes the seed used by tt_env_step's auto-reset.  obs_out [N,23] f32 may be NULL. */
int tt_env_reset(tt_env *env, const uint8_t *mask, uint64_t seed, float *obs_out, tt_stream_t stream);

/* Start-pose pool for resets (simv1.py:255-282 draws poses by rejection sampling against a Dubins-path
 * feasibility test, which is host logic): when a pool of m >= 1 poses [m,3] f64 (x, y, yaw) is set, tt_env_reset
 * and the in-kernel auto-reset draw uniformly from it instead of from reset_lo/hi.  The pool stays owned by the
 * caller and must outlive its use; m = 0 (or pool NULL) goes back to the box distribution. */
int tt_env_set_reset_pool(tt_env *env, const double *pool, int m);

/* The callers' pose-override pattern (DDPG/test.py:96-115, heatmap.py:79-122): for j < k set
 * env idx[j] (idx NULL = env j) to start[j] = (startx, starty, startyaw), optional goal[j] and
 * L2[j], state = trailer pose with the truck L2 ahead rounded to f32, max_episode_steps =
 * compute_max_steps(), episode cleared; writes obs rows idx[j] of obs_out [N,23] if non-NULL. */
int tt_env_set_pose(tt_env *env, const int32_t *idx, int k, const double *start /*[k,3]*/,
                    const double *goal /*[k,3] or NULL*/, const double *L2 /*[k] or NULL*/, float *obs_out,
                    tt_stream_t stream);

/* Plain attribute writes `env.startx/starty/startyaw = ...`, `env.goalx/goaly/goalyaw = ...`,
 * `env.L2 = ...` (heatmap.py:79-89): like tt_env_set_pose's arguments (each may be NULL = keep)
 * but WITHOUT touching the kinematic state, the step counter or the reward carry. */
int tt_env_set_attrs(tt_env *env, const int32_t *idx, int k, const double *start /*[k,3] or NULL*/,
                     const double *goal /*[k,3] or NULL*/, const double *L2 /*[k] or NULL*/, tt_stream_t stream);

/* `env.state = ...` / `env.state` (simv2.py:489, trainv2.py:499,522): raw f64 kinematic state
 * psi1, psi2, x1, y1, x2, y2.  set: state [k,6] row-major for envs idx[j]; get: [6,N] SoA. */
int tt_env_set_state(tt_env *env, const int32_t *idx, int k, const double *state, tt_stream_t stream);
int tt_env_get_state(tt_env *env, double *state_out, tt_stream_t stream);

/* `env.max_episode_steps = ...` (heatmap.py:96) for envs idx[j].  Values outside [0, TT_MAX_EPISODE_STEPS] are refused
 * with TT_EINVAL and nothing is written; to check them this call copies max_steps to the host and waits for `stream`
 * (a setter, not a hot call; not capturable). */
int tt_env_set_max_steps(tt_env *env, const int32_t *idx, int k, const int32_t *max_steps, tt_stream_t stream);

/* `env.episode_steps = ...` (simv2.py:94, 523-530; written by a caller at DDPG/episode_replay_collectorv2.py:269) for envs
 * idx[j]: the step counter that the exploration tiers, the max-step penalty and `max_steps_reached` read.  Like the
 * reference's attribute write it leaves the reward carry alone (reward_state: previous distance, backward-movement count,
 * stage latches -- only reset / tt_env_set_pose clear it).  Range-checked and synchronising like tt_env_set_max_steps. */
int tt_env_set_steps(tt_env *env, const int32_t *idx, int k, const int32_t *steps, tt_stream_t stream);

/* Episode bookkeeping read-back; any pointer may be NULL.  steps/max_steps [N] i32;
 * start, goal [3,N] f64 (startx.., goalx..: trainv2.py:503-508); L2 [N] f64. */
int tt_env_get_episode(tt_env *env, int32_t *steps, int32_t *max_steps, double *start, double *goal, double *L2,
                       tt_stream_t stream);

/* env.compute_observation(env.state, steering) (simv2.py:103-181) for all envs;
 * steering [N] f32 radians or NULL for 0.  obs_out [N,23] f32 row-major. */
int tt_env_observe(tt_env *env, const float *steering, float *obs_out, tt_stream_t stream);

/* env.step(action) for all N envs (simv2.py:499-545): clip to +-max_steer, one DP5 step of the
 * kinematic ODE in f64, 23-dim observation, reward_functionv1 reward with its carry, flags.
 *   action [N] f32 radians; obs [N,23] f32 row-major; reward [N] f32; done [N] u8;
 *   info optional (NULL or members NULL).
 * auto_reset != 0: an env that is done is re-placed like tt_env_reset (its obs row is then the
 * fresh episode's first observation; reward/done/info still describe the finished step).  The
 * reference never resets by itself (trainv2.py:489); auto_reset = 0 reproduces that. */
/* Optional device-side count of vector steps: every tt_env_step / tt_env_step_random launch adds 1 to *counter
 * (device int64, caller-owned; NULL detaches).  The trajectory ring's sampler (tt_ring_sample: k_dev) reads it, so a
 * vector step needs no separate launch to advance the ring. */
int tt_env_set_step_counter(tt_env *env, int64_t *counter);

int tt_env_step(tt_env *env, const float *action, float *obs, float *reward, uint8_t *done, const tt_info *info,
                int auto_reset, tt_stream_t stream);

/* Ring addressing: the trajectory ring of a rollout loop (obs [slots,N,23], act / rew [slots,N] f32, done [slots,N] u8) and a
 * device cursor {t, t+1, t-1, t > 0} (slot numbers of the running vector step, written by the step's opening launch:
 * tt_ring_cursor of tt_mlp_split_pack[_and_sample]).  Launches that take a view read / write the step's slots through the
 * cursor instead of through per-slot pointers, so ONE captured hipGraph serves every ring position. */
typedef struct tt_ring_view {
    int32_t *cursor;        /* [TT_CURSOR_INTS] device ([12..16]: the hand-over words, below): [4..7] / [8..11] the cursors of even / odd steps (written by the opening launch of
                               the step), [0..3] the running step's copy, left by tt_actor_act_ring for tt_env_step_ring */
    float *obs, *act, *rew;
    uint8_t *done;
    int32_t n_envs, slots;
} tt_ring_view;
typedef struct tt_ring_cursor {
    const int64_t *k_dev;   /* vector steps completed (tt_env_set_step_counter); nothing may advance it beside the launch */
    int32_t slots, reserved_;
    int32_t *cursor;        /* [TT_CURSOR_INTS] device (tt_ring_view): the launch writes the four numbers of step *k_dev at [4 + 4 (k & 1)] */
} tt_ring_cursor;
/* Image hand-over (cursor[12..15], zero-initialised by the caller; when *k_dev is set to k -- a resume -- the caller sets both
 * epoch words to the low 32 bits of k, behind the epochs k + 1 and k + 2 that the next two steps wait for, and zeroes [14..15]):
 * the words hold the low 32 bits of step numbers and are compared in wrapped 32-bit arithmetic.  A pack launch given a
 * cursor ends by publishing "cursor and image of step k = *k_dev are complete" as cursor[12 + (k & 1)] = k + 1 (release,
 * device scope), and tt_actor_act_ring begins by waiting for cursor[12 + (k & 1)] >= k + 1 with k = its *step_dev (bounded:
 * after 0.25 s it sets cursor[15] = k + 1 and goes on -- TT_CURSOR_GAVE_UP; a caller that lets the two launches run
 * unordered checks that word).  The two launches of a step therefore need NO stream / graph dependency between them; the
 * pack launch of step k + 2, which overwrites the same image, must still be ordered behind the policy launch of step k. */
#define TT_CURSOR_INTS 32
#define TT_CURSOR_GAVE_UP 15
/* cursor[18..19] (optional, 0 = none): the 64-bit address of ONE int of device-visible host memory (hipHostMalloc; a torch
 * pinned tensor) that a launch which gives up sets as well (system scope), so that the host sees a give-up by reading its own
 * memory, without a copy or a synchronize.  The caller writes the address whenever it zeroes the cursor buffer. */
#define TT_CURSOR_GAVE_UP_MIRROR 18
/* Step-chain progress (cursor[16]): tt_actor_act_ring of step k begins by storing k + 1 there (device scope).  A launch starts
 * only when everything in front of it on its stream is complete and written back, so cursor[16] >= k + 1 says: the env step of
 * step k - 1 -- and every launch before it -- is over and visible.  tt_mlp_forward_multi_sampled can wait for that word instead of
 * for a stream / graph dependency on the env step (tt_sample_args.step_progress), so that a loop's learn chain needs no edge
 * from its step chain either.  The caller sets the word to the low 32 bits of *k_dev whenever it sets *k_dev (resume). */
#define TT_CURSOR_PROGRESS 16
/* tt_env_step with obs -> ring slot t+1, reward and done -> slot t (env.step of the vector loop, trainv2.py:520-525). */
int tt_env_step_ring(tt_env *env, const float *action, const tt_ring_view *ring, int auto_reset, tt_stream_t stream);

/* tt_env_step with BASELINE.json config 2's "random policy" drawn inside the kernel:
 * action = U(-1,1) * pi/4 from Philox keyed by (policy_seed, env, step-in-episode, episode number), so no
 * host-side counter changes between launches and a captured hipGraph of K steps replays correctly.
 * action_out [N] f32 (the drawn steering, e.g. for a replay buffer) may be NULL. */
int tt_env_step_random(tt_env *env, uint64_t policy_seed, float *action_out, float *obs, float *reward,
                       uint8_t *done, const tt_info *info, int auto_reset, tt_stream_t stream);

/* Checkpoint / resume of the env batch (the reference only checkpoints networks, trainv2.py:210-244; SURVEY §8f-3
 * asks for env state too).  The blob is opaque device memory of tt_env_state_bytes(env) bytes holding every
 * per-env quantity (kinematic state, reward carry, counters, poses, goals, episode numbers); meta[4] carries the
 * handle's host-side mode {per-env-goal flag, reset seed, n_envs, version}.  Import requires the same n_envs. */
size_t tt_env_state_bytes(const tt_env *env);
int tt_env_export(tt_env *env, void *blob, uint64_t meta[4], tt_stream_t stream);
int tt_env_import(tt_env *env, const void *blob, const uint64_t meta[4], tt_stream_t stream);

/* Episode log (the per-episode record trainv2.py:488-572 keeps: score, length, success; DESIGN.md "Episode log").
 * Off by default.  tt_env_set_episode_log(env, capacity > 0) allocates and zeroes a device block (the one allocation
 * after create: call it outside a graph capture) and from then on tt_env_step, tt_env_step_ring and tt_env_step_random
 * launch the logging form of the step kernel: every lane keeps its running return (the f64 TT_I_TOTAL rewards summed in
 * step order), and every env that finishes appends one record
 *     ret f64 (the episode's return)        len i32 (env.episode_steps at the done step)
 *     flags u8 (TT_F_* bits, unmasked)      success u8 (final_success_bonus > 0: trainv2.py:541)
 *     lane i32                              end_step i64 (the logging launch it ended in, counted from 0 since enable)
 * in an order that depends on the atomics of the launch (sort by (end_step, lane) for a deterministic one).  Records past
 * `capacity` are not stored; the write index keeps counting.  Beside them, exact counters since enable
 * [TT_LOG_NCOUNTS] u64: episodes, successes, then one per TT_F_* bit (bit 0 first).  A lane starts a new episode with a
 * zero return when the step auto-resets it, on tt_env_reset (masked or full) and on tt_env_set_pose; tt_env_set_state and
 * tt_env_set_steps continue the episode.  A lane that is mid-episode when the log is enabled counts its return from
 * there.  tt_env_rollout_random refuses to run while the log is on.  capacity = 0 frees the log (the step kernel is then
 * exactly the one without it).  Enabling again starts a fresh log. */
#define TT_LOG_NCOUNTS 9
int tt_env_set_episode_log(tt_env *env, int64_t capacity, tt_stream_t stream);
/* Stream-ordered drain (follows graph replays with no host synchronisation): copies the first min(written, capacity)
 * records into the caller's [capacity] arrays (any may be NULL), writes `written` (records appended since the last
 * drain, stored or not) to *n_out (device int64) and the cumulative counters to counts_out [TT_LOG_NCOUNTS] (device u64,
 * may be NULL), then sets the write index back to 0.  TT_EINVAL when the log is off. */
int tt_env_drain_episode_log(tt_env *env, double *ret, int32_t *len, uint8_t *flags, uint8_t *success, int32_t *lane,
                             int64_t *end_step, int64_t *n_out, uint64_t *counts_out, tt_stream_t stream);
/* Checkpoint of the log: one opaque device blob of tt_env_episode_log_bytes(env) bytes (0 when off) holding the running
 * returns, the counters, the launch count and the records not yet drained; meta[2] = {capacity, n_envs}.  Import needs a
 * handle whose log is on with the same capacity and n_envs. */
size_t tt_env_episode_log_bytes(const tt_env *env);
int tt_env_export_episode_log(tt_env *env, void *blob, uint64_t meta[2], tt_stream_t stream);
int tt_env_import_episode_log(tt_env *env, const void *blob, const uint64_t meta[2], tt_stream_t stream);

/* Detailed episode log (what DDPG/viz_how_agent_learn.py and pareto_analysis.py read of every episode: its reward by term, and
 * trainv2.py's env_data start pose).  tt_env_set_episode_log2(env, capacity, flags, stream) with flags = 0 is exactly
 * tt_env_set_episode_log; with TT_LOG_DETAIL the step launches the detailed form of the logging kernel, and every record also
 * carries
 *     comp f64 [TT_LOG_NCOMP]   the episode's sum of each reward term, rows TT_I_PROGRESS .. TT_I_SMOOTH of tt_info.comp in
 *                               that order (progress, heading, orientation, staged, safety, exploration, final bonus, backward,
 *                               smoothness), each added in step order in f64 as the return is: bit for bit the host's sum
 *                               of that comp row over the episode
 *     start f64 [3]             the start pose (x, y, yaw) tt_env_get_episode reported for the lane during the episode (with
 *                               auto-reset: the finished episode's, not the one the same step places)
 * The term sums restart where the return does.  The plain records, counters and their semantics are unchanged.  Unknown
 * flag bits are TT_EINVAL.  The log's block (tt_env_episode_log_bytes) grows by 96 B per record and 72 B per env; its
 * header records the flags, and tt_env_import_episode_log refuses (TT_EINVAL) a blob of the other kind of log. */
#define TT_LOG_DETAIL 1
#define TT_LOG_NCOMP 9
int tt_env_set_episode_log2(tt_env *env, int64_t capacity, uint32_t flags, tt_stream_t stream);
/* tt_env_drain_episode_log plus the detailed columns: comp [TT_LOG_NCOMP, capacity] f64 (row = term) and start [3, capacity]
 * f64 (rows x, y, yaw), same record order as the plain columns; either may be NULL.  TT_EINVAL when comp or start is asked of
 * a plain log. */
int tt_env_drain_episode_log2(tt_env *env, double *ret, int32_t *len, uint8_t *flags, uint8_t *success, int32_t *lane,
                              int64_t *end_step, double *comp, double *start, int64_t *n_out, uint64_t *counts_out,
                              tt_stream_t stream);

/* Greedy evaluation: an env step in which a finished lane holds still (the reference evaluates with
 * evaluate=True from fixed poses: DDPG/test.py:96-115, heatmap.py:79-193).  tt_env_set_hold(env, on != 0) allocates (on = 0:
 * frees) the handle's evaluation block -- like the episode log's, an allocation: call it outside a graph capture -- with, per
 * lane,
 *     live u8      ret f64 (the f64 TT_I_TOTAL rewards summed in step order: the episode log's return)
 *     len i32      flags u8 (TT_F_* bits, unmasked)      success u8 (final_success_bonus > 0)
 *     end f64 [3]  (x2, y2, psi2 at the done step)
 * tt_env_hold_begin (after tt_env_set_pose or tt_env_reset) makes every lane live and zeroes the records.  tt_env_step_hold steps
 * every LIVE lane with the action mu[i] * action_scale (one f32 multiply; the step clips as always), without reset, adds the
 * reward to the lane's return, stores state and observation row as tt_env_step does and, where the lane is done, writes its
 * record and clears its live byte.  A lane that is not live is HELD: nothing of it changes -- state, counters, episode number,
 * observation row, record.  No reward / done arrays, no info; the step counter (tt_env_set_step_counter), the episode log and
 * the ring are not touched, and tt_env_step*, the episode log and tt_env_export ignore the block.  Every record sits in its
 * lane's slot and nothing is counted with atomics: the same poses and actions give the same bits.
 * tt_env_hold_read copies the records, stream-ordered, into the caller's device arrays of n entries (end: [3, n]; any may be
 * NULL) and writes the number of lanes still live to *live_out (device int64, may be NULL).  begin, step and read are
 * capturable into a hipGraph.  TT_EINVAL: a NULL handle, hold not enabled, NULL mu or obs, a non-finite action_scale. */
int tt_env_set_hold(tt_env *env, int on, tt_stream_t stream);
int tt_env_hold_begin(tt_env *env, tt_stream_t stream);
int tt_env_step_hold(tt_env *env, const float *mu, float action_scale, float *obs, tt_stream_t stream);
int tt_env_hold_read(tt_env *env, double *ret, int32_t *len, uint8_t *flags, uint8_t *success, double *end, int64_t *live_out,
                     tt_stream_t stream);

/* Start-pose curriculum: resets drawn by the success rate of the cell they start in.  A curriculum is a
 * grid of nx x ny x nyaw cells over the reset box reset_lo .. reset_hi, C = nx * ny * nyaw in [1, TT_CURRICULUM_MAX_CELLS], cell
 * c = (iyaw * ny + iy) * nx + ix.  Per cell, in device memory:
 *     p f64 [C]            a running success rate, 0.5 at first          seen u64 [C]      the episodes ever counted
 *     attempts u32 [C]     episodes finished since the last update       successes u32 [C] those of them that succeeded
 *     q u32 [C]            the draw weight, in [1, 65536]                cum u32 [C]       the inclusive prefix sum of q
 * and per lane cell u32 [npad] (npad: N rounded up to a multiple of 64; read and write copy the first N): the cell the lane's
 * running episode was drawn from, TT_CURRICULUM_NO_CELL when no curriculum draw made it.
 * While a curriculum is on, tt_env_reset (masked or not) and the auto-reset of tt_env_step / _step_ring / _step_random draw
 *     r = the reset's Philox words of (seed, env, episode);  t = (r[3] * cum[C - 1]) >> 32;  c = the smallest cell with cum[c] > t
 *     x = lo_x + (ix + (r[0] + 0.5) / 2^32) * ((hi_x - lo_x) / nx),   y and yaw likewise with r[1] and r[2]
 * in f64, every operation rounded on its own, and write the lane's cell.  A lane that finishes an episode in an auto-resetting
 * step adds 1 to attempts[cell] and, with final_success_bonus > 0 (the episode log's success), to successes[cell] -- integer adds:
 * the counts do not depend on the order of arrival -- before its next draw; a lane with no cell counts nothing.  tt_env_set_pose
 * and tt_env_set_state set the lanes they touch to TT_CURRICULUM_NO_CELL.  Steps with auto_reset = 0 neither count nor draw.
 * tt_env_curriculum_update (one small launch, capturable): per cell with n = attempts > 0: p <- (1 - alpha) p + alpha (successes / n),
 * seen += n, both counters 0; then for every cell f = 4 p (1 - p) (TT_CURRICULUM_FRONTIER) or 1 - p (TT_CURRICULUM_HARD),
 * w = uniform + (1 - uniform) f, q = min(65536, 1 + floor(65535 w)), cum = the inclusive scan of q.  f64 with every operation
 * rounded on its own and an integer scan: p, q and cum are a pure function of the arrays before.  With p = 0.5 everywhere every
 * cell has the same weight in both modes: a fresh curriculum draws cells uniformly.
 * tt_env_set_curriculum(env, cfg, place, stream): cfg NULL turns the curriculum off (the step and the reset are then exactly the
 * ones without it).  place NULL: the handle allocates and owns the arrays; otherwise the caller's device arrays of the extents
 * above, all seven, which must outlive their use.  An allocation and a wait for `stream`: outside a graph capture.  Starts fresh
 * (p = 0.5, nothing counted, every lane without a cell).  TT_EINVAL with a message: a bin count < 1 or C outside
 * [1, TT_CURRICULUM_MAX_CELLS]; an unknown mode; alpha outside (0, 1]; uniform outside [0, 1] or not finite; a reset pool set
 * (tt_env_set_reset_pool with m > 0 refuses likewise while a curriculum is on); the detailed episode log on
 * (tt_env_set_episode_log2 with TT_LOG_DETAIL refuses likewise); a reset box with reset_hi < reset_lo.  tt_env_rollout_random
 * refuses to run while a curriculum is on.
 * tt_env_curriculum_read / _write: stream-ordered device-to-device copies between the curriculum's arrays and the caller's
 * (members that are NULL are skipped) -- the curriculum's own export and import, beside tt_env_export, which stays as it is; also
 * how a test plants counters or weights.  A writer of q keeps cum its prefix sum; cells outside [0, C) count as no cell. */
#define TT_CURRICULUM_MAX_CELLS 4096
#define TT_CURRICULUM_NO_CELL 0xFFFFFFFFu
#define TT_CURRICULUM_FRONTIER 0
#define TT_CURRICULUM_HARD 1
typedef struct tt_curriculum {
    int32_t nx, ny, nyaw;
    int32_t mode;
    double alpha, uniform;
} tt_curriculum;
typedef struct tt_curriculum_arrays {
    double *p;
    uint64_t *seen;
    uint32_t *attempts, *successes, *q, *cum;
    uint32_t *cell;
} tt_curriculum_arrays;
int tt_env_set_curriculum(tt_env *env, const tt_curriculum *cfg, const tt_curriculum_arrays *place, tt_stream_t stream);
int tt_env_curriculum_update(tt_env *env, tt_stream_t stream);
int tt_env_curriculum_read(tt_env *env, const tt_curriculum_arrays *out, tt_stream_t stream);
int tt_env_curriculum_write(tt_env *env, const tt_curriculum_arrays *in, tt_stream_t stream);

/* Episode randomisation: the TASK is drawn per episode.  While it is on, every reset of a lane -- tt_env_reset
 * (masked or not) and the auto-reset of tt_env_step / _step_ring / _step_random -- draws the new episode's goal and trailer length
 *     r = philox4x32(env, episode, 1, 0x7452, seed_lo, seed_hi)     the reset's Philox domain with third counter word 1
 *     u_k = (r[k] + 0.5) / 2^32
 *     goal x = goal_lo[0] + (goal_hi[0] - goal_lo[0]) * u_0,  goal y and goal yaw likewise with u_1 and u_2
 *     L2 = L2_lo + (L2_hi - L2_lo) * u_3
 * in f64, every operation rounded on its own (the widths hi - lo are formed once, on the host): a pure function of (reset seed,
 * lane, episode number), and a range of width 0 gives its bound exactly.  The start pose is drawn as without the option (third
 * counter word 0; the box or the reset pool): a randomised env starts where a plain env with the same seed starts, bit for bit.
 * The lane is then placed as tt_env_set_pose(start, goal, L2) places it: the start distance and max_episode_steps come from the drawn
 * goal, the per-env rows hold goal and length (tt_env_get_episode reads them), and observation columns 12-15 carry the goal.
 * Steps with auto_reset = 0 draw nothing.  tt_env_set_pose / _set_attrs still write a lane; its next reset draws again.
 * tt_env_set_randomization(env, cfg, stream): cfg NULL turns it off -- the lanes' attributes stay as they are and the resets are the
 * ones without the option from then on (goal back to the parameters', the lane's L2 kept).  Turning it on makes the handle a per-env
 * handle (as tt_env_set_pose with a goal does); lanes change at their next reset.  An allocation and a wait for `stream`: outside a
 * graph capture.  The state blob (tt_env_export) is unchanged: goal and length are in it already.
 * TT_EINVAL with a message, before the handle is read: a bound that is not finite; lo > hi; L2_lo <= 0.  Reading the handle: a goal
 * x / y range outside the map; an L2_lo for which dt * |v| / L2 exceeds the integrator's 0.25 rad per step (tt_env_create's test);
 * a curriculum on (tt_env_set_curriculum refuses likewise while randomisation is on); the detailed episode log on
 * (tt_env_set_episode_log2 with TT_LOG_DETAIL refuses likewise).  tt_env_rollout_random refuses to run while it is on.  The MPC
 * launches only read the lanes' attributes and run as before.
 * tt_env_randomization(env, out): 1 if on (and *out, when not NULL, receives the ranges), 0 if off, TT_EINVAL for a NULL handle. */
typedef struct tt_randomization {
    double goal_lo[3], goal_hi[3];      /* x, y, yaw */
    double L2_lo, L2_hi;
} tt_randomization;
int tt_env_set_randomization(tt_env *env, const tt_randomization *cfg /* NULL: off */, tt_stream_t stream);
int tt_env_randomization(const tt_env *env, tt_randomization *out);

/* Task curriculum: the task drawn by success.  On only while episode randomisation is on: a grid of
 * bins = (ngx, ngy, ngyaw, nl2) cells over its ranges of goal x, goal y, goal yaw and L2, C = ngx * ngy * ngyaw * nl2 in
 * [1, TT_CURRICULUM_MAX_CELLS], cell c = ((il2 * ngyaw + igyaw) * ngy + igy) * ngx + igx, with the start-pose curriculum's state per
 * cell (p, seen, attempts, successes, q, cum: tt_curriculum_arrays) and per lane cell u32 [npad], the cell the lane's running episode
 * was drawn in, TT_CURRICULUM_NO_CELL when no task-curriculum draw made it.  While it is on, every reset of a lane draws
 *     r = philox4x32(env, episode, 1, 0x7452, seed_lo, seed_hi)     the task's words, as plain randomisation's
 *     s = philox4x32(env, episode, 2, 0x7452, seed_lo, seed_hi)     the cell pick
 *     t = (s[0] * cum[C - 1]) >> 32;  c = the smallest cell with cum[c] > t
 *     goal x = goal_lo[0] + (igx + u_0) * ((goal_hi[0] - goal_lo[0]) / ngx),  goal y and goal yaw likewise;  L2 from il2, u_3, nl2
 * with u_k = (r[k] + 0.5) / 2^32, in f64, every operation rounded on its own (the cell widths are formed once, on the host), and
 * writes the lane's cell.  The start pose keeps its words (third counter word 0; the box or the reset pool).  With bins (1, 1, 1, 1)
 * the draw is plain randomisation's, bit for bit.  The lane is then placed as plain randomisation places it.  A lane that finishes an
 * episode in an auto-resetting step adds 1 to attempts[cell] and, with final_success_bonus > 0, to successes[cell] before its next
 * draw, as the start-pose curriculum counts; a lane with no cell counts nothing; tt_env_set_pose and tt_env_set_state set the lanes
 * they touch to TT_CURRICULUM_NO_CELL.  Steps with auto_reset = 0 neither count nor draw.
 * tt_env_task_curriculum_update (one small launch, capturable): tt_env_curriculum_update's rule on these arrays.
 * tt_env_set_task_curriculum(env, cfg, place, stream): cfg NULL turns it off (step and reset are then plain randomisation's).  place
 * as tt_env_set_curriculum's.  An allocation and a wait for `stream`: outside a graph capture.  Starts fresh.  TT_EINVAL with a
 * message, before the handle is read: a bin count < 1 or C outside [1, TT_CURRICULUM_MAX_CELLS]; an unknown mode; alpha outside
 * (0, 1]; uniform outside [0, 1] or not finite.  Reading the handle: episode randomisation not on; more than one bin on a range of
 * width 0.  While it is on tt_env_set_randomization refuses (new ranges or NULL): "turn the task curriculum off first".  A reset
 * pool may be set or cleared while it is on.  TT_VERSION and the state blob do not change: the arrays travel by
 * tt_env_task_curriculum_read / _write, which are tt_env_curriculum_read / _write on these arrays.
 * tt_env_task_curriculum(env, out): 1 if on (and *out, when not NULL, receives the option), 0 if off, TT_EINVAL for a NULL handle. */
typedef struct tt_task_curriculum {
    int32_t bins[4];    /* ngx, ngy, ngyaw, nl2 */
    int32_t mode;
    double alpha, uniform;
} tt_task_curriculum;
int tt_env_set_task_curriculum(tt_env *env, const tt_task_curriculum *cfg /* NULL: off */, const tt_curriculum_arrays *place,
                               tt_stream_t stream);
int tt_env_task_curriculum_update(tt_env *env, tt_stream_t stream);
int tt_env_task_curriculum_read(tt_env *env, const tt_curriculum_arrays *out, tt_stream_t stream);
int tt_env_task_curriculum_write(tt_env *env, const tt_curriculum_arrays *in, tt_stream_t stream);
int tt_env_task_curriculum(const tt_env *env, tt_task_curriculum *out);

/* Success replay (csrc/ttenv_harvest.h): the transitions of the successful episodes the episode log names
 * are copied from the trajectory ring into a region of the ring's side buffer (tt_side_buffer) before the ring overwrites them.
 * A harvest runs while no step and no learn() launch is in flight.  With k = *k_dev (vector steps completed) and
 * W = min(k, slots - 1) (intact transitions per lane), it looks at the records [mark, m), m = min(*written_dev, record_capacity);
 * s = end_step + step_base is the absolute ring step of a record's done transition:
 *   - a record with success != 0 and s >= k - W is eligible; one with success != 0 and s < k - W is expired (counted).  A record
 *     that cannot be one of this ring's (lane outside [0, n_envs), len < 1, s >= k) is neither;
 *   - want = len (tail == 0) or min(len, tail); first = max(s - want + 1, k - W); rows = s - first + 1; want - rows joins rows_cut;
 *   - eligible records are taken in ascending (s, lane) order (pairs are unique in a log), each episode's rows oldest first; R is
 *     the sum of rows.  Row r of the harvest has the global number g = written_rows + r, is stored iff r >= R - capacity, and goes
 *     to row g % capacity of the region: a bit copy of the ring's transition (t = j % slots, lane) of absolute step j -- obs, act,
 *     rew, done of slot t and obs2 = obs of slot (j + 1) % slots;
 *   - then written_rows += R, episodes += the eligible records, mark = m.
 * state is int64 [8] in device memory: {mark, written_rows, episodes, rows_cut, expired, 0, 0, 0}; word 7 counts the plan
 * launch's workgroups while it runs and is 0 again when it ends.  Two launches on `stream`, no allocation, wait or host read, all
 * counts read on the device, integer arithmetic only: a plan launch (each record's rows from its first one to the harvest's end
 * into work[], by counting against every other record of the window through LDS tiles -- (m - mark)^2 / 256 tile passes of 256
 * compares; its last workgroup moves the state on) and a copy launch (one wave per eligible record at a time; lanes 0..22 move
 * obs, 32..54 obs2, 63 the scalars).  tt_ring_harvest takes the record columns from anywhere; tt_env_harvest reads the env's own
 * episode log in place and leaves it untouched (tt_env_drain_episode_log is unaffected).  ring->cursor is not read.
 * TT_EINVAL with a message that names the entry point, before any HIP call: a NULL pointer; capacity < 1 or tail < 0;
 * record_capacity < 1 or record_capacity * (slots - 1) past 2^31 - 1 (work[] holds 32-bit row counts); slots < 3 or n_envs < 1; for
 * tt_env_harvest a ring view of another number of envs, or an episode log that is off. */
typedef struct tt_harvest {
    int64_t *state;                 /* [8] device */
    float *obs, *act, *rew, *obs2;  /* the region's rows [0, capacity): obs / obs2 [capacity, 23], act / rew [capacity] */
    uint8_t *done;                  /* [capacity] */
    int32_t capacity, tail;
    int64_t step_base;              /* ring step of the log's launch 0 */
    int32_t *work;                  /* [record_capacity] scratch */
} tt_harvest;
int tt_ring_harvest(const tt_harvest *h, const tt_ring_view *ring, const int64_t *k_dev, const int32_t *lane, const int64_t *end_step,
                    const int32_t *len, const uint8_t *success, const uint64_t *written_dev, int64_t record_capacity,
                    tt_stream_t stream);
int tt_env_harvest(tt_env *env, const tt_harvest *h, const tt_ring_view *ring, const int64_t *k_dev, tt_stream_t stream);

/* K vector steps of the random policy in ONE launch (SURVEY.md §8d iii): each env stays in registers for
 * k_steps steps with in-kernel auto-reset; only the last observation is stored.  obs_out [N,23], reward_sum [N]
 * f32 (sum of the k_steps rewards) and episodes_done [N] i32 may each be NULL. */
int tt_env_rollout_random(tt_env *env, int k_steps, uint64_t policy_seed, float *obs_out, float *reward_sum,
                          int32_t *episodes_done, tt_stream_t stream);

/* Sampling MPC expert (MPPI, Williams et al. 2017; the reference's demonstrations come from a CasADi / IPOPT
 * NMPC, DDPG/exp_gen.py, npc_solver.py).  One launch makes ONE DECISION for every lane: it rolls S perturbed steering sequences
 * H steps forward from the lane's state through the step kernel's own env step, weights them by their return and writes the
 * first action of the weighted mean.  The env is only read: no state, counter, episode number, cold attribute, ring, step
 * counter or episode log changes.  For lane i, with H = horizon, S = samples, every f32 field of tt_mpc_args taken to f64:
 *   plan     plan[i, 0..H-1] f32, normalised units in [-1, 1].  When the lane's step-in-episode is 0 the plan READ is all zeros
 *            (after a reset or tt_env_set_pose no host call is needed, and a captured graph stays valid).
 *   noise    z[s, t] = sqrt(-2 ln u1) cos(2 pi u2), u = ((r >> 8) + 0.5) 2^-24 in f32 from the first two words r of
 *            Philox4x32-10 with counter (lane i, episode number, step-in-episode | t << 12 | s << 18, the domain tag 0x4D50) and
 *            key (seed low, seed high); the angle is the f32 product 2 pi u2; log, sqrt and cos in f64 (the recipe of
 *            tt_td3_agent's noise).  No other stream of the library uses the tag (0x7452 reset poses, 0xAC71 random actions,
 *            0x0A5E OU noise, 0x5A3D replay draws, 0x7D3E TD3 smoothing).
 *            eps[s, 0] = sigma z[s, 0];  eps[s, t] = rho eps[s, t-1] + sqrt(1 - rho^2) sigma z[s, t]  (f64; the factor
 *            sqrt(1 - rho^2) sigma is formed once).  Sample 0 is the noise-free nominal: eps[0, .] = 0.
 *   sample   u[s, t] = (float) clip(plan_t + eps[s, t], -1, 1); the steering is u * action_scale, ONE f32 multiply (the product
 *            tt_env_step_hold forms); the step clips it as always.
 *   return   G_s = sum_{t < T_s} gamma^t total_t in f64, in step order (gamma^t by repeated multiplication), total_t the
 *            TT_I_TOTAL of the step; T_s = the step at which done first holds, inclusive, or H.  A sample that did not terminate
 *            adds gamma^H (-(k_lat lat^2 + k_yaw dyaw^2)), lat = -(x2 - gx) sin(gyaw) + (y2 - gy) cos(gyaw) the trailer's offset
 *            from the goal axis, dyaw = wrap(gyaw - psi2).
 *   update   w_s = exp((G_s - max_s G) / lambda) in f64 (the exponent is clamped at -100), 0 for a return that is not finite (the
 *            maximum is over the finite ones);  U'_t = sum_s w_s u[s, t] / sum_s w_s, both sums in f64 IN SAMPLE ORDER, stored as
 *            f32: the same inputs give the same bits whatever the launch.  mu_out[i] = U'_0, and the plan is stored shifted:
 *            (U'_1, ..., U'_{H-1}, U'_{H-1}).  With no finite sample mu_out[i] = plan_0 and the plan read shifts unchanged.
 *   live     device u8 [N] or NULL; a lane with live[i] == 0 is skipped: its plan row, mu_out[i] and returns_out row keep their bits.
 *   returns_out   f64 [N, S] or NULL: every G_s.
 * Capturable into a hipGraph: no allocation, no host read; the noise keys are read from the device.
 * TT_EINVAL with a message that names the entry point, before any HIP call: a NULL handle, args, plan or mu_out; horizon outside
 * [1, TT_MPC_MAX_HORIZON]; samples outside [1, TT_MPC_MAX_SAMPLES]; sigma, k_lat or k_yaw negative or not finite; rho outside
 * [0, 1); lambda not finite or <= 0; gamma outside (0, 1]; action_scale not finite or <= 0. */
#define TT_MPC_MAX_HORIZON 64
#define TT_MPC_MAX_SAMPLES 1024
typedef struct tt_mpc_args {
    int32_t horizon, samples;
    float sigma, rho, lambda, gamma, k_lat, k_yaw, action_scale;
    uint64_t seed;
} tt_mpc_args;
int tt_env_mpc_plan(tt_env *env, const tt_mpc_args *args, float *plan /* [N, H] in / out */, float *mu_out /* [N] */,
                    const uint8_t *live, double *returns_out, tt_stream_t stream);

/* Expert lanes of a rollout loop: lanes [0, lanes) of the env make ONE tt_env_mpc_plan DECISION each -- the
 * same noise keys, the plan read as zeros at step-in-episode 0, the same f64 sample-ordered update and shifted plan; plan is
 * [lanes, H] -- and the decision replaces what the step's policy launch wrote for the lane:
 *     ring->act[t][i] = U'_0              (the normalised action, what a demonstration file stores)
 *     act_scaled[i]   = U'_0 * high       (ONE f32 product: the env step's input)
 * with t = ring->cursor[0], the running step's slot as tt_actor_act_ring left it for tt_env_step_ring: launch it between the two,
 * on their stream.  Lanes >= `lanes` keep every bit in ring->act and act_scaled; the env is only read; no other ring row, no
 * counter and no noise state changes.  Capturable into a hipGraph: no allocation, no host read.
 * TT_EINVAL with a message that names the entry point, before any HIP call: a NULL handle, args, plan, ring, ring->cursor,
 * ring->act or act_scaled; ring->slots < 1; lanes outside [1, ring->n_envs]; high not finite or <= 0; everything tt_env_mpc_plan
 * refuses of args; a ring view of another number of envs than the handle's. */
int tt_env_mpc_act_ring(tt_env *env, const tt_mpc_args *args, float *plan /* [lanes, H] in / out */, int32_t lanes,
                        const tt_ring_view *ring, float high, float *act_scaled /* [N] */, tt_stream_t stream);

/* Expert labels of a rollout loop: with expert_lanes = M >= 0 and label_lanes = L >= 1, M + L <= n_envs, lanes
 * [M, M + L) are LABELLED LANES.  Each of them makes ONE tt_env_mpc_plan DECISION per launch, exactly as defined above -- the same
 * noise keys, the plan read as zeros at step-in-episode 0, the f64 sample-ordered update, the plan stored shifted -- and the
 * decision goes to the ring's label array and nowhere else:
 *     label[t][i] = U'_0                  t = ring->cursor[0], label is f32 [slots, n_envs], i in [M, M + L)
 * Nothing of the decision's definition changes because the lane then executes the POLICY's action and not U'_0: the shifted plan is
 * only the next decision's warm start, not a record of what the lane did.  ring->act[t][i], act_scaled[i], the policy's noise state
 * and the env of a labelled lane keep every bit.  In the same launch lanes [0, M) do what tt_env_mpc_act_ring does, bit for bit, and
 * store no label (their stored action is their label).  plan is [M + L, H], row i the plan of lane i.  A cursor outside [0, slots)
 * stores no label (and no ring->act value, as above).  Launch it where tt_env_mpc_act_ring goes, in its place: between
 * tt_actor_act_ring and tt_env_step_ring, on their stream.  tt_ring_view keeps its layout: the label array is an argument.
 * Capturable into a hipGraph: no allocation, no host read.
 * TT_EINVAL with a message that names the entry point, before any HIP call: a NULL handle, args, plan, ring, ring->cursor or label;
 * expert_lanes < 0; label_lanes < 1; with expert_lanes > 0 a NULL ring->act or act_scaled (unused, and may be NULL, with 0);
 * ring->slots < 1; expert_lanes + label_lanes > ring->n_envs; high not finite or <= 0; everything tt_env_mpc_plan refuses of args; a
 * ring view of another number of envs than the handle's. */
int tt_env_mpc_label_ring(tt_env *env, const tt_mpc_args *args, float *plan /* [M + L, H] in / out */, int32_t expert_lanes /* M >= 0 */,
                          int32_t label_lanes /* L >= 1 */, const tt_ring_view *ring, float *label /* [slots, N] */, float high,
                          float *act_scaled /* [N]; may be NULL when M == 0 */, tt_stream_t stream);

/* Measurement hook (no reference counterpart): time each of the next `max_launches` step-kernel dispatches
 * with a HIP event pair bound to the dispatch itself (hipExtLaunchKernelGGL), on the stream they are launched
 * on; max_launches = 0 switches it off.  tt_env_profile_read waits for the recorded launches, adds them to the
 * running totals and returns sum of kernel durations [ms] and their count.  Not capturable into a hipGraph. */
int tt_env_profile(tt_env *env, int max_launches);
int tt_env_profile_read(tt_env *env, double *total_ms, int64_t *launches);

/* "random policy" of BASELINE.json config 2 as a stand-alone action generator: out[i] = U(-1,1) * pi/4 from Philox(seed, step). */
int tt_random_actions(int n, uint64_t seed, uint64_t step, float *out, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Fused inference of the reference's networks (shapes of trainv2.py:404-407: 23 -> 400 -> 300 -> 1, LayerNorm
 * eps 1e-5) at f32 accuracy.  Pointers are torch parameter storages (row-major [out,in]):
 *   w1 [400,23] b1 g1 be1 [400] = fc1, bn1;  w2 [300,400] b2 g2 be2 [300] = fc2, bn2;  w3 [300] b3 [1] = mu / q;
 *   wa [300] ba [300] = action_value (critic only).  Other shapes return TT_EINVAL (callers fall back to torch).
 * Two kernels serve a forward: the exact-f32 MFMA kernel (csrc/ttnet.hip), and for n >= 1024 rows the split-f16
 * kernel (csrc/ttnet_split.hip: every f32 operand is, to within its own rounding, the sum of two round-to-nearest f16
 * pieces; three f16 MFMAs with f32 accumulation per product block) when split_ws is set: a caller-owned
 * device workspace of tt_mlp_split_ws_bytes() bytes, one per network and per stream that may run it concurrently,
 * into which each call re-packs fc2 before it runs (never stale; the contents are private to the library).
 * split_ws = NULL always selects the exact-f32 kernel.  Structs of gradients (tt_mlp_backward_weights) ignore it. */
typedef struct tt_mlp_weights {
    const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3, *wa, *ba;
    int32_t in_dim, fc1_dims, fc2_dims;
    int32_t capped_grids;   /* with max_workgroups > 0: > 0 = only the first capped_grids grids are capped, the remaining tiles go
                               out in ONE grid over the whole chip (large n: the launches on other streams that the cap makes room
                               for are over after a few grids); 0 = every grid is capped */
    void *split_ws;
    int32_t ws_packed;      /* != 0: split_ws already holds the image of these weights (tt_mlp_split_pack): forwards do not
                               re-pack and read nothing but the image, so the weights may be updated beside them */
    int32_t max_workgroups; /* > 0: the split kernel's workgroups (one per CU is resident) go out in consecutive grids of at most
                               this many, leaving the other CUs to launches on other streams; 0 = one grid */
    void *split_ws_alt;     /* optional second image (ring addressing only): tt_mlp_split_pack[_and_sample] with a cursor then writes the
                               image of the parity of the step it opens (split_ws: even steps, split_ws_alt: odd steps) and
                               tt_actor_act_ring reads the one of the running step's parity -- so the opening launch of step
                               t+1 may run beside the policy launches of step t */
    void *fc2_img;          /* learn() kernels (tt_mlp_forward_save / _multi, tt_mlp_backward_rows_pair): NULL = fc2 products on the exact-f32
                               MFMA straight from w2; else a caller-owned device buffer of tt_mlp_fc2_image_bytes() bytes (zeroed
                               once, then tt_mlp_fc2_image_pack) that holds w2 as pre-split f16 pieces in both orientations, and
                               the products run on the f16 MFMA at f32 accuracy (three per block, as in the split-f16 forward).
                               The CALLER keeps it equal to w2: optimizer steps through tt_mlp_backward_weights /
                               tt_adam_soft_update with `images` rewrite every element they update; after any other change of
                               w2 call tt_mlp_fc2_image_pack again. */
} tt_mlp_weights;
/* fc2 as pre-split f16 pieces (x64, h = rn16, m = rn16 of the remainder) in MFMA-fragment order (1 KB = 64 lanes x 8 halves =
 * one coalesced 16-byte load per lane): a forward half [20 neuron tiles][13 k32 steps] and a backward half (dH1 = dX2 * W2)
 * [28 column tiles][10 k32 steps], an h and an m plane of each; zero padding (layout private to csrc/ttlearn.hip). */
uint64_t tt_mlp_fc2_image_bytes(void);
int tt_mlp_fc2_image_pack(const tt_mlp_weights *w, tt_stream_t stream);   /* w->fc2_img <- pieces of w->w2 */
/* images an optimizer step keeps current (either may be NULL): the updated network's and its target's fc2_img */
typedef struct tt_fc2_images {
    void *net, *target;
} tt_fc2_images;
uint64_t tt_mlp_split_ws_bytes(void);
/* Write the split kernel's image of `w` (fc2 and fc1 as pre-split f16 fragments, per-neuron vectors, head bias) into ws
 * (tt_mlp_split_ws_bytes() bytes).  bump (may be NULL): a device int64 that this launch increments by one -- the step
 * counter of a pipelined loop whose learn() chain ends with this pack. */
int tt_mlp_split_pack(const tt_mlp_weights *w, int critic, void *ws, int64_t *bump, const tt_ring_cursor *cursor,
                      tt_stream_t stream);   /* cursor (may be NULL): also writes the ring cursor of the step this launch opens */

/* ActorNetwork.forward (DDPG/networks.py:138-147) for n rows: mu_out [n] = tanh(mu(...)). */
int tt_actor_forward(int n, const float *obs /*[n,23]*/, const tt_mlp_weights *w, float *mu_out, tt_stream_t stream);

/* Agent.choose_action for n envs (DDPG_agent.py:36-49) + OUActionNoise.__call__ (noise.py:13-17) + the caller's
 * scaling (trainv2.py:516) in one launch: ou_state [n] is advanced in place (x <- x*(1-theta_dt) + sigma_sqrt_dt*N(0,1),
 * N from Philox(seed, env, step [+ *step_dev]) + Box-Muller; restarted at 0 where done_prev[i] != 0, trainv2.py:492),
 * act_raw_out [n] = mu + x (the action the replay stores, trainv2.py:525), act_scaled_out [n] = clip(.,-1,1)*high
 * (what env.step gets).  mu_out and done_prev may be NULL.  step_dev (device int64) may be NULL. */
int tt_actor_act(int n, const float *obs, const tt_mlp_weights *w, float *ou_state, const uint8_t *done_prev,
                 uint64_t seed, uint64_t step, const int64_t *step_dev, float theta_dt, float sigma_sqrt_dt, float high,
                 float *mu_out, float *act_raw_out, float *act_scaled_out, tt_stream_t stream);

/* tt_actor_act on ring slot t (observations in, stored actions out, done flags of slot t-1 restart the noise): `w` must carry a
 * caller-kept image (ws_packed).  step_dev (required) is the ring's step counter -- the one tt_env_step_ring's launch
 * advances: besides keying the noise, its parity picks the cursor pair and (split_ws_alt) the image of the running step, and
 * the launch copies that cursor to cursor[0..3] for the env step that follows it on the same stream. */
int tt_actor_act_ring(int n, const tt_ring_view *ring, const tt_mlp_weights *w, float *ou_state, uint64_t seed, uint64_t step,
                      const int64_t *step_dev, float theta_dt, float sigma_sqrt_dt, float high, float *act_scaled_out,
                      tt_stream_t stream);

/* ReplayBuffer.sample_buffer (DDPG/replay_buffer.py:23-34: uniform WITH replacement) on the device trajectory ring
 * obs [slots,N,23] f32, act/rew [slots,N] f32, done [slots,N] u8 (transition (t,e) = obs[t][e], act[t][e], rew[t][e],
 * obs[t+1][e], done[t][e]); *k_dev = vector steps completed, read on the device, so a captured hipGraph draws new
 * indices at every replay.  Outputs: s_out, s2_out [batch,23], a_out, r_out [batch] f32, d_out [batch] u8,
 * idx_out [batch,2] i32 (slot, env) or NULL.
 * reserve: 0, or the number of most recent ring slots a CONCURRENT env step may be writing (a pipelined loop samples
 * beside the step launch: then *k_dev counts the steps completed before that launch and reserve = 1 keeps the draw off the
 * observation row it overwrites; two env steps may be under way beside a draw that runs ahead of them: reserve = 2); the window is min(*k_dev - lag, slots - 1 - reserve) steps ending lag steps before *k_dev
 * (lag: steps counted by *k_dev that may still be under way on another stream -- a loop whose learn() chain runs ahead of its
 * env steps: DDPGRollout's pipelined order uses lag = 1, reserve = 2).
 * side (may be NULL): stand-alone transitions that are not part of any env's trajectory -- the expert tuples
 * `(obs, action / radians(45), reward, obs_next, done)` that trainv2.py:457-466 re-inserts with agent.remember
 * (produced by exp_gen.py:77-110).  They take part in the same uniform draw: with `count` side transitions and R
 * intact ring transitions every one of the count + R has probability 1/(count + R); a side draw reports
 * idx_out = (-1, j). */
typedef struct tt_side_buffer {
    const float *obs, *act, *rew, *obs2; /* [count,23], [count], [count], [count,23] f32 */
    const uint8_t *done;                 /* [count] */
    int32_t count, reserved_;
} tt_side_buffer;
int tt_ring_sample(int batch, int n_envs, int slots, const int64_t *k_dev, const float *obs, const float *act,
                   const float *rew, const uint8_t *done, uint64_t seed, int reserve, int lag, const tt_side_buffer *side,
                   float *s_out, float *a_out, float *r_out, float *s2_out, uint8_t *d_out, int32_t *idx_out,
                   tt_stream_t stream);

/* tt_mlp_split_pack + tt_ring_sample in ONE launch: what opens a vector step of a pipelined loop (the policy's image from
 * the actor's current weights; the first batch of the step's learn()).  The members of tt_sample_args are tt_ring_sample's
 * arguments. */
typedef struct tt_sample_args {
    int32_t batch, n_envs, slots, reserve;      /* (lag: last member) */
    const int64_t *k_dev;
    const float *obs, *act, *rew;
    const uint8_t *done;
    uint64_t seed;
    const tt_side_buffer *side;
    float *s_out, *a_out, *r_out, *s2_out;
    uint8_t *d_out;
    int32_t *idx_out;
    int32_t lag;             /* the newest `lag` steps counted by *k_dev may still be under way (tt_ring_sample) */
    int32_t draws;           /* tt_mlp_split_pack_and_sample: 0 or 1 = one draw; d > 1 = d draws of `batch` rows each from the SAME
                              * window in the one launch -- draw u uses seed + u * seed_stride and fills rows [u * batch, (u + 1) *
                              * batch) of the output buffers (sized for d * batch rows): the batches of all the learn() calls of one
                              * vector step (each of them exactly what its own tt_ring_sample with that seed would draw), so that
                              * none of them has the ring's latency on its chain.  Other entry points take one draw and ignore it */
    uint64_t seed_stride;
    const int32_t *step_progress; /* tt_mlp_forward_multi_sampled only; NULL or the ring's cursor + TT_CURSOR_PROGRESS: the launch then first
                              * waits until *step_progress >= *k_dev -- the env step whose transitions close the draw's window is over
                              * (k_dev must then be a counter that runs `lag` ahead of the steps completed, as a pipelined loop's does);
                              * bounded like the image hand-over, same give-up word (cursor[TT_CURSOR_GAVE_UP]) */
} tt_sample_args;
int tt_mlp_split_pack_and_sample(const tt_mlp_weights *w, int critic, void *ws, const tt_sample_args *sample,
                                 const tt_ring_cursor *cursor, tt_stream_t stream);

/* CriticNetwork.forward (DDPG/networks.py:55-68) for n rows: q_out [n]. */
int tt_critic_forward(int n, const float *obs /*[n,23]*/, const float *action /*[n]*/, const tt_mlp_weights *w,
                      float *q_out, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Hand-fused learn() (csrc/ttlearn.hip) for the same network shapes: Agent.learn (DDPG/DDPG_agent.py:72-106) as a
 * dozen launches.  All buffers are caller-owned device memory, row-major f32. */
typedef struct tt_mlp_saved {   /* what a forward keeps for its backward */
    float *xh1, *h1;            /* [B,400] LayerNorm1-normalised fc1 output (before gamma/beta); post-ReLU activation */
    float *xh2, *h2;            /* [B,300] same for fc2 (critic: h2 after adding action_value(a)) */
    float *rstd1, *rstd2;       /* [B] 1/sqrt(var + eps) of the two LayerNorms */
} tt_mlp_saved;

/* Forward of the actor (critic = 0: out = tanh(mu(.))) or the critic (critic = 1: out = Q(s,a)) on a small batch,
 * 16 rows per workgroup with the columns split over its 4 waves.  saved may be NULL (inference only); dq_da [B]
 * (critic only, may be NULL) receives dQ/da. */
int tt_mlp_forward_save(int n, int critic, const float *obs, const float *action, const tt_mlp_weights *w, float *out,
                        const tt_mlp_saved *saved, float *dq_da, tt_stream_t stream);

/* Up to four forwards on n rows each in ONE launch (learn()'s first phase: target actor on s', target critic's state branch
 * on s', Q(s,a), mu(s)).  critic = 0: actor (action, dq_da, z_state ignored); critic = 1 with z_state set: the target
 * critic's state branch only, z_state [n,300] = bn2(fc2(relu(bn1(fc1(s))))) (networks.py:55-61, before the action enters;
 * action and out may be NULL) -- the TD prologue of tt_mlp_backward_rows_pair (tt_td_input) finishes it once the target
 * actor's action is known; otherwise as tt_mlp_forward_save.  saved / dq_da may be NULL. */
typedef struct tt_fwd_job {
    int32_t critic, reserved_;
    const float *obs, *action;
    const tt_mlp_weights *w;
    float *out;
    const tt_mlp_saved *saved;
    float *dq_da, *z_state;
} tt_fwd_job;
int tt_mlp_forward_multi(int n, int count, const tt_fwd_job *jobs, tt_stream_t stream);
/* The same with the replay draw of ReplayBuffer.sample_buffer (DDPG/replay_buffer.py:23-34) made BY this launch: `sample`
 * are tt_ring_sample's arguments (batch = n); every job's obs must be sample->s_out or sample->s2_out and a critic job's
 * action sample->a_out -- the workgroups read those rows straight from the ring, and the five batch buffers are filled on
 * the way for the launches that follow (at least one job on s and one on s').  One launch and one dependent launch boundary
 * less per learn() than tt_ring_sample followed by tt_mlp_forward_multi; the same draw, bit for bit. */
/* k_snapshot (may be NULL): *sample->k_dev as this launch saw it, left for a LATER launch that must use the same step number
 * although the counter moves in between (tt_image_job below). */
int tt_mlp_forward_multi_sampled(int n, int count, const tt_fwd_job *jobs, const tt_sample_args *sample, int64_t *k_snapshot,
                                 tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * N-step returns in the replay draw (csrc/ttnstep.hip).  The ring is time-major, so the steps of an env after a stored
 * transition are next to it; the draw can hand learn() the n-step tuple
 *     (s_t, a_t, R = r_t + gamma r_(t+1) + ... + gamma^(m-1) r_(t+m-1), s_(t+m), D)
 * for the target y = R + gamma^m q'(s_(t+m)) (1 - D).  Semantics, beyond tt_ring_sample's (n_step in 1 .. TT_NSTEP_MAX, gamma
 * f32 in (0, 1)): with k = max(*k_dev - lag, 0), avail = min(k, slots - 1 - reserve), avail_n = avail - (n_step - 1):
 *   - Philox call, key and counter of tt_ring_sample; back = (n_step - 1) + ((u64)r[0] * avail_n >> 32),
 *     e = (u64)r[1] * n_envs >> 32, base step t0 = k - 1 - back -- only positions whose n steps lie inside the intact window; all
 *     slots are taken mod `slots`.  n_step = 1 is tt_ring_sample's draw bit for bit.
 *   - the walk j = 0 .. n_step - 1 over step t0 + j of env e: R = fmaf(g_j, rew, R) in f32, g_0 = 1, g_(j+1) = g_j * gamma in f32;
 *     it stops after the first j with done != 0 (m = j + 1, D = 1); else m = n_step, D = 0.
 *   - the batch row: s_out = obs[t0], a_out = act[t0], r_out = R, s2_out = obs[t0 + m], d_out = D, idx_out = {t0 mod slots, e}.
 *     (For D = 1, s2 is the first observation of the next episode and never enters the target, as in tt_ring_sample.)
 *   - avail_n < 1 counts as 1: an early launch reads in-bounds, meaningless rows, as tt_ring_sample does at *k_dev = 0.
 * So a row either has no done among its n steps -- discount gamma^n, THE SAME FOR EVERY SUCH ROW: pass
 * tt_td_input.gamma = (float)pow((double)gamma, n_step) -- or D = 1, and the TD prologue of tt_mlp_backward_rows_pair ignores q' and
 * the discount for it: every launch of learn() behind the draw is the one-step learn()'s.
 * TT_EINVAL with a message (tt_last_error(NULL)), before any HIP call: n_step outside 1 .. TT_NSTEP_MAX, gamma outside (0, 1),
 * slots < 3 + reserve + (n_step - 1), a side buffer with count > 0 when n_step > 1 (side tuples are single steps: their rows
 * would need a discount of their own), draws > 1, and whatever tt_ring_sample / tt_mlp_forward_multi_sampled refuse. */
#define TT_NSTEP_MAX 16
/* the lone draw into sample's batch buffers (sample->step_progress is not waited for) */
int tt_ring_sample_nstep(const tt_sample_args *sample, int n_step, float gamma, tt_stream_t stream);
/* tt_mlp_forward_multi_sampled with that draw made by the launch: the jobs on s read the rows at t0, the jobs on s' at t0 + m;
 * step_progress and k_snapshot as there. */
int tt_mlp_forward_multi_sampled_nstep(int n, int count, const tt_fwd_job *jobs, const tt_sample_args *sample, int n_step,
                                       float gamma, int64_t *k_snapshot, tt_stream_t stream);

/* learn()'s backward and optimizer step (autograd of networks.py:55-68 / 138-147, DDPG_agent.py:95-106), in the sequence
 *   tt_mlp_forward_multi[_sampled]  target actor and target critic's state branch on s', Q(s,a) and mu(s) with saved activations
 *   tt_mlp_backward_rows_pair       per-row backward of the critic (with the TD target in its prologue) and the actor
 *   tt_mlp_backward_weights(critic) the critic's gradients (+ Adam and soft update on one rank)
 *   tt_mlp_forward_save(critic on (s, mu(s)), dq_da) or, for both this and the next, tt_mlp_actor_tail
 *   tt_mlp_backward_weights(actor)  the actor's gradients (+ Adam and soft update on one rank)
 * and, with data-parallel ranks, each network's gradients all-reduced before tt_adam_soft_update[_p2p].
 * Workspace ws holds a net's per-row gradients (dpre [B], dz, dx2 [B,300], dy1, dx1 [B,400]). */
typedef struct tt_mlp_bwd_ws {
    float *dpre, *dz, *dx2, *dy1, *dx1;
} tt_mlp_bwd_ws;
/* The TD prologue of tt_mlp_backward_rows_pair (the rest of the target critic and the TD target, for the rows each
 * workgroup of the critic's backward owns): q' = q(relu(z_state + action_value(mu_target))) (networks.py:62-68) from the
 * target critic's state branch z_state [n,300] and the target actor's action mu_target [n]; y_out [n] = r + gamma q'
 * (1 - done) (DDPG_agent.py:89-93), the critic's regression target; q_out [n] (q') or NULL; *step_dev advanced by 1 (may be
 * NULL). */
typedef struct tt_td_input {
    const float *z_state, *mu_target;
    const tt_mlp_weights *target_critic;
    const float *reward;
    const uint8_t *done;
    float gamma, reserved_;
    float *y_out, *q_out;
    int64_t *step_dev;
    int64_t *window_dev;   /* optional: a second device counter advanced by 1 -- the sampling-window counter of a pipelined
                              loop (tt_ring_sample's k_dev), moved on by the last learn() of a vector step */
    /* optional: the launch that advances *step_dev also leaves Adam's bias corrections of
     * the NEW step t for the pair (adam_beta1, adam_beta2) in bias_corr_out[0..4] = {t (int32 bits), beta1, beta2,
     * 1 - beta1^t, 1 - beta2^t}, evaluated once in f64 on a workgroup of its own; the optimizer launches given the same
     * buffer (tt_mlp_backward_weights / tt_adam_soft_update: bias_corr) use it when step and betas match and otherwise
     * evaluate the two pow() themselves, in every thread: ~1.1 us per launch (DDPG/networks.py:49-50,133: torch.optim.Adam) */
    float *bias_corr_out;
    float adam_beta1, adam_beta2;
} tt_td_input;
#define TT_BIAS_CORR_FLOATS 8

/* The actor's per-row backward is linear in the row's d(loss)/d(pre-tanh) = -(1/B) dQ/da (1 - mu^2), and only dQ/da needs
 * the UPDATED critic (DDPG_agent.py:100-103): so
 *   tt_mlp_backward_rows_pair   runs the critic's per-row backward for loss = mse_loss(y, q) (d(loss)/dq = scale_critic *
 *                               (q - y), scale_critic = 2/B; DDPG_agent.py:96-97; y from the TD prologue td, required;
 *                               q_out = the critic's forward output) and, on other workgroups of the SAME launch, the
 *                               actor's per-row backward for a unit gradient (ws_actor receives d(.)/d(pre-tanh) = 1 per
 *                               row; ws_critic != ws_actor);
 *   tt_mlp_backward_weights     is the weight-gradient launch: grads (the layout of tt_mlp_weights) receives d(loss)/d(parameter)
 *                               for every parameter (overwritten, not accumulated) from saved + ws, with row b of ws counted
 *                               row_scale * row_dq_da[b] * (1 - row_mu[b]^2) times when row_dq_da / row_mu are given (both or
 *                               neither; n <= 1024).  count = 0: gradients only.  Else count = 10 (actor) / 12 (critic)
 *                               tensors in tt_mlp_weights order (HOST arrays of device pointers, as tt_adam_soft_update):
 *                               the optimizer step of tt_adam_soft_update applied in the same launch (each gradient element
 *                               is finished by exactly one workgroup, which then updates that parameter, its Adam moments and
 *                               its target); grads still receives the gradients.  For one rank: data-parallel ranks run
 *                               count = 0, all-reduce the gradients, then tt_adam_soft_update.
 * Single-rank learn(): tt_mlp_forward_multi, tt_mlp_backward_rows_pair, tt_mlp_backward_weights(critic), tt_mlp_forward_save
 * (critic on (s, mu(s)) with dq_da), tt_mlp_backward_weights(actor, row_dq_da = dq_da, row_mu = mu, row_scale = -1/B). */
/* image (may be NULL): the pack of a vector step's policy image (tt_mlp_split_pack with a cursor: image of the step's parity,
 * ring cursor, image epoch) carried by THIS launch on workgroups of its own -- the actor's weights are not written before
 * the launch after the next, the pack needs ~5 us of the launch's ~14, and a loop's learn chain is one launch and one dependent
 * boundary shorter than with an opening pack launch.  image->cursor->k_dev must be a word no launch writes meanwhile
 * (tt_mlp_forward_multi_sampled: k_snapshot): this launch also advances the step / window counters. */
typedef struct tt_image_job {
    const tt_mlp_weights *actor;        /* its split_ws / split_ws_alt are the image buffers (as for tt_mlp_split_pack) */
    const tt_ring_cursor *cursor;
} tt_image_job;
int tt_mlp_backward_rows_pair(int n, float scale_critic, const float *q_out, const tt_mlp_weights *critic,
                              const tt_mlp_saved *saved_critic, const tt_mlp_bwd_ws *ws_critic, const tt_td_input *td,
                              const float *mu_out, const tt_mlp_weights *actor, const tt_mlp_saved *saved_actor,
                              const tt_mlp_bwd_ws *ws_actor, const tt_image_job *image, tt_stream_t stream);
int tt_mlp_backward_weights(int n, int critic, const float *obs, const float *action, const tt_mlp_saved *saved,
                            const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, const float *row_dq_da, const float *row_mu,
                            float row_scale, int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                            float *const *targets, const int64_t *step_dev, float lr, float beta1, float beta2, float eps,
                            float weight_decay, float tau, const tt_fc2_images *images /* may be NULL */,
                            const float *bias_corr /* tt_td_input.bias_corr_out or NULL */, tt_stream_t stream);

/* The last two launches of the single-rank sequence above in ONE grid: tt_mlp_forward_save(critic on (s, mu), dq_da) and
 * tt_mlp_backward_weights(actor, row_dq_da = dq_da, row_mu = mu, row_scale, Adam + soft update + images).  The weight-gradient
 * workgroups request everything else they read, then wait IN DEVICE MEMORY for the row workgroups' dQ/da instead of behind a launch
 * boundary.  tail_words: 64 + 2 n device ints, set to -1 by the caller at creation and whenever it sets *step_dev back: [0, 64) one
 * hint word per row workgroup, [64, 64 + 2 n) per ROW one 8-byte word {learn step *step_dev, float bits of dQ/da} written by ONE
 * agent-scope atomic store -- a reader that finds the step it waits for holds the value of that step, so the hand-over needs no
 * ordering between two locations and no cache maintenance.  The wait is bounded (0.25 s): a thread that gives up stores the step
 * into *gave_up_host (one int of device-visible host memory, may be NULL) and goes on -- the caller must treat that learn() as
 * failed.  Same results as the two launches, bit for bit (dq_da [n] is written as well).  n <= 1024 rows. */
int tt_mlp_actor_tail(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                      const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale, int count,
                      float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                      const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                      const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host,
                      tt_stream_t stream);

/* optimizer.step() of torch.optim.Adam (weight decay folded into the gradient; networks.py:49-50,133) for `count`
 * (<= 12) parameter tensors in one launch, then the soft update of the matching target tensors
 * (Agent.update_network_parameters, DDPG_agent.py:108-131; targets NULL = none).  The arrays are HOST arrays of device
 * pointers; *step_dev (device) is the 1-based count of this step. */
int tt_adam_soft_update(int count, float *const *params, const float *const *grads, float *const *exp_avg,
                        float *const *exp_avg_sq, float *const *targets, const int32_t *numel, const int64_t *step_dev,
                        float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                        const tt_fc2_images *images /* may be NULL; tensors in tt_mlp_weights order (w2 = index 4) */,
                        const float *bias_corr /* tt_td_input.bias_corr_out or NULL */, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Population learn(): the learn() of K independent agents (K <= TT_POP_MAX_AGENTS, one batch size B <= 1024 for all, the
 * reference-shaped networks) in the four launches of ONE agent's learn() with the tail in one grid -- tt_mlp_forward_multi_sampled,
 * tt_mlp_backward_rows_pair, tt_mlp_backward_weights(critic, Adam), tt_mlp_actor_tail -- each launch running every agent's
 * workgroups.  Agent a's results are the bits of those four lone launches made with agent a's arguments.  An agent is described by
 * what its lone launches take; the library copies it into device memory at creation (every pointer must stay valid and fixed for the
 * handle's life: rebuild the handle when a buffer moves), so tt_pop_learn makes no host work per call and can be captured.
 *   sample      the agent's replay draw (batch == B, no side buffer, draws <= 1, no step_progress); update u draws with the key
 *               seed + u * seed_stride (mod 2^64): a loop's update u of a vector step
 *   jobs        [4] learn()'s forwards in the lone order: target actor on s', the target critic's state branch on s' (z_state),
 *               the critic on (s, a) with saved activations, the actor on s with saved activations
 *   td          the TD prologue; step_dev required (the agent's Adam step and its tail epoch), window_dev NULL
 *   critic / actor  the per-row workspace, the flat gradient and the optimizer step (tt_mlp_backward_weights' count .. images;
 *               the HOST arrays of device pointers are copied) of each network; the bias corrections come from td->bias_corr_out
 *   q_pi, dq_da, tail_words, gave_up_host   as tt_mlp_actor_tail's q_out, dq_da, tail_words (64 + 2 B ints, -1 at creation and
 *               whenever *step_dev is set back) and gave_up_host; the tail's row scale is -1/B, the critic's loss scale 2/B.
 * Bad arguments return TT_EINVAL with a message in tt_last_error(NULL), before any HIP call.  The tail launch dispatches the row
 * workgroups of ALL agents before any weight workgroup that waits for them (each agent's hand-over words are its own). */
#define TT_POP_MAX_AGENTS 16
typedef struct tt_population tt_population;
typedef struct tt_pop_net {
    const tt_mlp_bwd_ws *ws;
    const tt_mlp_weights *grads;
    int32_t count, reserved_;           /* 12 tensors (critic) / 10 (actor) */
    float *const *params, *const *exp_avg, *const *exp_avg_sq, *const *targets;
    float lr, beta1, beta2, eps, weight_decay, tau;
    const tt_fc2_images *images;        /* may be NULL */
} tt_pop_net;
typedef struct tt_pop_agent {
    const tt_sample_args *sample;
    const tt_fwd_job *jobs;
    const tt_td_input *td;
    tt_pop_net critic, actor;
    float *q_pi, *dq_da;
    int32_t *tail_words, *gave_up_host;
} tt_pop_agent;
int tt_pop_learn_create(int count, int batch, const tt_pop_agent *agents /*[count]*/, tt_population **out);
int tt_pop_learn(tt_population *pop, int update, tt_stream_t stream);      /* one update of every agent, enqueued on stream */
int tt_pop_learn_destroy(tt_population *pop);                                /* the caller's stream work with it must be done */

/* Population-based training's exploit/explore step (Jaderberg et al., 2017) on a live population: ONE launch for a list of pairs.
 * For each pair with dst != src, dst's learning state becomes src's: the parameters of its four networks (actor, critic and both
 * targets), both networks' Adam moments m and v, and -- when the optimizer steps keep fc2 images -- the four fc2 images.  For every
 * pair (dst == src: hyperparameters only) dst's actor learning rate becomes alpha, its critic's beta, both soft updates' tau, and
 * its TD discount gamma.  Nothing else of dst moves: its ring, env, noise and episode log are the caller's, and its step counter,
 * bias corrections and tail words stay (all agents of a population take their Adam steps in lockstep, so the step counts agree).
 * The new values live in the descriptors tt_pop_learn reads, in place: launches captured before stay valid and see them.
 * Enqueued on `stream`, ordered before the next tt_pop_learn on it.  list is a HOST array, copied into the launch's arguments.
 * TT_EINVAL with a message, before any HIP call: a NULL handle or list, pairs outside [1, K], an agent index out of range, two
 * pairs with the same dst, a dst that is the src of another pair, a non-finite value, alpha, beta or tau outside (0, 1], gamma
 * outside (0, 1).  tt_pop_hyper reads agent a's {alpha, beta, tau, gamma} back from the device (synchronous). */
typedef struct tt_pop_exploit_pair {
    int32_t dst, src;
    float alpha, beta, tau, gamma;
} tt_pop_exploit_pair;
int tt_pop_exploit(tt_population *pop, int pairs, const tt_pop_exploit_pair *list /*[pairs], host*/, tt_stream_t stream);
int tt_pop_hyper(tt_population *pop, int agent, float out[4]);

/* N-step returns in a population: each agent draws n-step tuples (tt_ring_sample_nstep's semantics) with ITS OWN n_step and gamma
 * inside the shared first launch (csrc/ttpop_nstep.hip: k_pop_fwd_multi_nstep, k_pop_fwd_multi's grid and per-update key).  The
 * library keeps a per-agent table {n_step, gamma} in device memory; an agent's TD discount gamma ** n_step takes the place of
 * gamma in its tt_td_input, so the three launches behind the draw are unchanged.
 *   discount    gamma ** n_step AS THE CALLER ROUNDS IT TO f32: it travels by value and the library never recomputes it, so an
 *               agent's bits do not depend on any pow() here.  n_step == 1: discount == gamma.
 * tt_pop_learn_set_nstep (synchronous: it waits for the device; call it before any capture) makes the table on first use, writes
 * every agent's entry and stores discount into its TD input.  FROM THEN ON tt_pop_learn's first launch is the n-step kernel, also
 * when every n_step is 1 (bit for bit the one-step draw): a later change of an agent's n_step changes no launch, so a captured
 * graph stays valid.  A population on which it was never called launches exactly the four one-step kernels.
 * tt_pop_exploit_nstep is tt_pop_exploit (its checks, its copy, alpha, beta and tau) followed on `stream` by the table writes:
 * dst of pair i takes ns[i].n_step, draws with ns[i].gamma (which must equal list[i].gamma) and discounts with ns[i].discount.
 * Plain tt_pop_exploit on a population with a table is TT_EINVAL: it would store gamma where gamma ** n_step belongs.
 * tt_pop_hyper reports gamma from the table when there is one.  tt_pop_nstep reads agent a's {n_step, gamma, discount} back from
 * the device (synchronous; without a table {1, gamma, gamma}).
 * TT_EINVAL with a message naming the entry point and the agent or pair, before any HIP call: a NULL handle or array; n_step outside
 * 1 .. TT_NSTEP_MAX; gamma outside (0, 1); discount != gamma when n_step == 1; discount outside (0, gamma) when n_step > 1; an agent
 * whose ring has fewer than 3 + reserve + (n_step - 1) slots; tt_pop_exploit_nstep without a table; whatever tt_pop_exploit refuses.
 * Not supported: side buffers (tt_pop_learn_create refuses them for every population). */
struct tt_pop_nstep {        /* (a tag without a typedef: the read-back function below has the same name) */
    int32_t n_step;
    float gamma, discount;
};
int tt_pop_learn_set_nstep(tt_population *pop, const struct tt_pop_nstep *per_agent /*[K], host*/);
int tt_pop_exploit_nstep(tt_population *pop, int pairs, const tt_pop_exploit_pair *list /*[pairs], host*/,
                         const struct tt_pop_nstep *ns /*[pairs], host*/, tt_stream_t stream);
int tt_pop_nstep(tt_population *pop, int agent, struct tt_pop_nstep *out);

/* Gradient-norm clipping in a population: each agent clips each of its two networks with ITS OWN max_norm (tt_grad_clip's formula:
 * norm = sqrt(sum of squares over the network's gradient), coef = max_norm / (norm + 1e-6), 1 where that is greater; the optimizer
 * sees coef * grad), in shared launches (csrc/ttclip.hip: k_pop_grad_sqnorm, K x TT_GRAD_CLIP_PARTIALS workgroups, and
 * k_pop_adam_soft_clip, K x the workgroups of tt_adam_soft_update).  The library keeps a per-agent table {max_norm critic, max_norm
 * actor} in device memory, with the norms' partial sums, out = {norm, coef} and counts = {updates, updates with coef < 1} per agent
 * and network.
 *   max_norm    a finite number > 0, or 0: this agent does not clip this network -- coef is 1 by definition, whatever the norm (a
 *               NaN norm does not reach it); the norm is still reported
 * tt_pop_learn_set_clip (synchronous: it waits for the device; call it before any capture) makes the table and the buffers on
 * first use, writes every agent's entry and switches the optimizer step off inside the weight-gradient launches.  FROM THEN ON
 * tt_pop_learn is eight launches, also when every value is 0: the draw and the forwards, the rows, the critic's weight gradients,
 * the critic's norm, the critic's clipped step, the actor tail (gradients only), the actor's norm, the actor's clipped step.  A
 * later change of a value changes no launch, so a captured graph stays valid.  A population on which it was never called launches
 * exactly its four kernels.  It composes with tt_pop_learn_set_nstep in either order.
 * Agent a's results, on the same draw: with a non-zero value, the bits of the lone separate-optimizer chain with
 * tt_adam_soft_update_clipped at the clipped network(s); with {0, 0}, the bits of that chain with tt_adam_soft_update at both.
 * The step sizes, tau, the step count and the fc2 images are read from the descriptors, so tt_pop_exploit's writes take effect.
 * tt_pop_clip_write enqueues ONE small launch on `stream` that writes values[i] into agents[i]'s entry (capturable; after
 * tt_pop_exploit on the same stream, the clip travels with the weights it was tuned on).  tt_pop_clip reads agent a's entry,
 * out[4] = {norm, coef} of the critic then the actor and counts[4] = {updates, clipped} likewise back from the device (synchronous).
 * TT_EINVAL with a message naming the entry point and the agent or entry, before any HIP call: a NULL handle or array; a negative,
 * NaN or infinite value; count outside [1, K]; an agent out of range or listed twice; tt_pop_clip_write / tt_pop_clip without a
 * table.  Not supported: TD3 populations (tt_pop_td3_*). */
struct tt_pop_clip {         /* (a tag without a typedef: the read-back function below has the same name) */
    float max_norm_critic, max_norm_actor;
};
int tt_pop_learn_set_clip(tt_population *pop, const struct tt_pop_clip *per_agent /*[K], host*/);
int tt_pop_clip_write(tt_population *pop, int count, const int32_t *agents /*[count], host*/,
                      const struct tt_pop_clip *values /*[count], host*/, tt_stream_t stream);
int tt_pop_clip(tt_population *pop, int agent, struct tt_pop_clip *value, float out[4], int64_t counts[4]);

/* ------------------------------------------------------------------------------------------------------
 * Learn log: one record per learn() update and agent -- the losses, the Q / TD-target / dQ/da / mu statistics and the two gradient
 * norms of that update -- reduced ON THE DEVICE by one launch (csrc/ttlearnlog.hip: k_learn_log) from the buffers learn() leaves
 * behind, so that replayed graphs keep a history of what the learner did (the episode log's counterpart on the learner's side).
 * A handle serves `agents` agents with one batch size: a lone learner is one agent, a population K.  The job descriptors are copied
 * into device memory at creation (every pointer must stay valid and fixed for the handle's life: rebuild the handle when a buffer
 * moves), so tt_learn_log_append is one launch with no host work and can be captured.  Enqueue it behind the update's last launch.
 *   step        *step_dev as the launch reads it: the Adam step t of the update just made (learn()'s second launch advances it)
 *   slot        (step / every) % capacity of the agent's ring of `capacity` records: derived from step alone -- no write index, no
 *               atomics -- so a replayed graph lands right and the ring holds the latest `capacity` records.  A launch whose
 *               step % every != 0 returns at once.
 * The values of a record, all arithmetic in f64 from the f32 inputs, in the order of tt_learn_log_drain's `values` rows:
 *    0 critic_loss      mean (q - y)^2, q from the critic BEFORE its step (DDPG_agent.py:96)
 *    1 actor_loss       -mean q_pi, the UPDATED critic on (s, mu(s)) (DDPG_agent.py:101-102)
 *    2..4  q_mean, q_min, q_max            5..7  y_mean, y_min, y_max
 *    8, 9  td_abs_mean, td_abs_max         over |y - q|
 *   10, 11 dq_da_abs_mean, dq_da_abs_max   over |dq_da|
 *   12 mu_abs_mean      mean |mu|          13 gate_mean   mean (1 - mu^2), the factor every actor row gradient carries
 *   14 grad_norm_critic, 15 grad_norm_actor   the L2 norm of each flat gradient as the optimizer launch saw it (no weight decay)
 * and nonfinite, the number of non-finite values among the 5 B row values and both gradients.  A record with nonfinite > 0 has
 * only step and nonfinite specified.  Every sum is taken in one fixed order that depends on batch and numel alone (no float atomics):
 * the same inputs give the same bits eagerly, replayed, alone or as agent a of a population.  No workgroup waits for or reads
 * another's result: each gradient is cut into TT_LEARN_LOG_CHUNKS fixed chunks whose workgroups leave an f64 sum of squares each,
 * and tt_learn_log_drain adds them in index order on the host and takes the root.
 * tt_learn_log_drain is synchronous (it waits for the device): agent `agent`'s complete records with step > after_step, oldest
 * first, at most `max` of them (the oldest); it does not modify the device block.  step_out [max], values_out
 * [TT_LEARN_LOG_NVALUES][max] (value v of record i at v * max + i), nonfinite_out [max], all host memory.  tt_learn_log_clear
 * invalidates every slot (step = -1), enqueued on `stream`: call it when *step_dev is set back, so that a step count does not meet
 * records from its future.
 * TT_EINVAL with a message naming the entry point, before any HIP call: a NULL handle, array or pointer; agents outside
 * 1 .. TT_POP_MAX_AGENTS; batch outside 1 .. 1024; capacity outside 1 .. TT_LEARN_LOG_MAX_CAPACITY; every < 1; numel <= 0; a
 * gradient that is not 16-byte aligned; an agent outside [0, agents); max < 0.
 * Not supported: data-parallel ranks (a rank's own gradient buffer is not what its optimizer applies). */
#define TT_LEARN_LOG_NVALUES 16
#define TT_LEARN_LOG_CHUNKS 16
#define TT_LEARN_LOG_MAX_CAPACITY (1 << 22)
typedef struct tt_learn_log tt_learn_log;
typedef struct tt_learn_log_job {          /* one agent; every pointer fixed for the handle's life */
    const float *y, *q, *q_pi, *dq_da, *mu;            /* [batch] */
    const float *grad_critic, *grad_actor;            /* flat, tt_mlp_weights order */
    int32_t numel_critic, numel_actor;
    const int64_t *step_dev;
} tt_learn_log_job;
int tt_learn_log_create(int agents, int batch, const tt_learn_log_job *jobs /*[agents], host*/, int64_t capacity, int32_t every,
                        tt_learn_log **out);
int tt_learn_log_append(tt_learn_log *log, tt_stream_t stream);               /* the one launch; capturable */
int tt_learn_log_drain(tt_learn_log *log, int agent, int64_t after_step, int64_t max, int64_t *step_out, double *values_out,
                       int32_t *nonfinite_out, int64_t *count);
int tt_learn_log_clear(tt_learn_log *log, tt_stream_t stream);
int tt_learn_log_destroy(tt_learn_log *log);                                 /* the caller's stream work with it must be done */

/* ------------------------------------------------------------------------------------------------------
 * Peer-to-peer gradient exchange of data-parallel ranks (one process per GPU of one node): the mean over the ranks of the
 * critic's / the actor's gradient at the reference's two optimizer sites (DDPG/DDPG_agent.py:95-104) WITHOUT a collective
 * launch on learn()'s chain.  Every rank owns two blocks of device memory -- per site a flat f32 gradient buffer
 * (tt_mlp_weights order: what tt_mlp_backward_weights writes when `grads` points into it), and, in fine-grained memory, one
 * arrival word per site and rank -- that its peers open through hipIpcMemHandles; tt_adam_soft_update_p2p is
 * tt_adam_soft_update whose gradient is
 *      g[i] = (G_0[i] + G_1[i] + ... + G_{world-1}[i]) / world        (summed in rank order: the same bits on every rank)
 * read straight from the ranks' buffers (xGMI loads at system scope).  Hand-over, per site and learn step t = *step_dev:
 * the first workgroup of rank r's launch -- which starts only when the launch that wrote G_r (same stream) is complete and
 * written back -- stores t into word [site][r] of EVERY rank's block (system scope, after a system-scope release); every
 * workgroup waits until its own block holds t in the words of all ranks, then acquires.  A rank overwrites G_r[site] only
 * in its next backward launch of that site, which lies behind its update of the OTHER site, whose wait saw every peer past
 * its reads of this one: two sites used in alternation (critic, actor, critic, ...) need no second barrier.  The wait is
 * bounded (tt_p2p_set_timeout, default 2 s): a launch that gives up marks a host-visible word (tt_p2p_gave_up) and goes on
 * with whatever the buffers hold -- the caller must treat the ranks as diverged.  Nothing here needs a process group; the
 * caller moves the TT_P2P_HANDLE_BYTES of tt_p2p_export between the processes (e.g. torch.distributed.all_gather_object on any backend). */
typedef struct tt_p2p tt_p2p;
#define TT_P2P_MAX_RANKS 8
#define TT_P2P_MAX_SITES 4
#define TT_P2P_HANDLE_BYTES 128      /* two hipIpcMemHandle_t: the flag block, the gradient block */
int tt_p2p_create(int device, int rank, int world, int sites, const int32_t *numel /*[sites] floats per site*/, tt_p2p **out);
int tt_p2p_destroy(tt_p2p *x);                               /* closes the peers' blocks, frees its own (peers must be done with it) */
int tt_p2p_export(const tt_p2p *x, void *handle_out /*[TT_P2P_HANDLE_BYTES]*/);
int tt_p2p_attach(tt_p2p *x, int peer, const void *handle /*[TT_P2P_HANDLE_BYTES] of rank `peer`*/);
float *tt_p2p_grad(const tt_p2p *x, int site);                /* this rank's gradient buffer of `site` (device memory), or NULL */
int tt_p2p_reset(tt_p2p *x, tt_stream_t stream);              /* tt_p2p_reset_at(x, 0, stream) */
/* Own arrival words to the low 32 bits of `step`, the value *step_dev was set to (resume): the words are compared with the
 * 32-bit epoch (int)(step + 1) of the next update in wrapped arithmetic, so they must lie BEHIND it -- a zero counts as arrived
 * for every step in [2^31 - 1, 2^32 - 2] mod 2^32.  The caller keeps every rank out of the exchange meanwhile. */
int tt_p2p_reset_at(tt_p2p *x, int64_t step, tt_stream_t stream);
int tt_p2p_set_timeout(tt_p2p *x, double seconds);
int tt_p2p_gave_up(const tt_p2p *x);                          /* 0, or the step whose wait was abandoned; reads host memory only */
const char *tt_p2p_last_error(const tt_p2p *x);
/* tt_adam_soft_update with the gradient taken from the exchange (above).  numel[0..count) must add up to the site's size;
 * every rank of the exchange must launch it for the same site with the same *step_dev. */
int tt_adam_soft_update_p2p(tt_p2p *x, int site, int count, float *const *params, float *const *exp_avg,
                            float *const *exp_avg_sq, float *const *targets, const int32_t *numel, const int64_t *step_dev,
                            float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                            const tt_fc2_images *images, const float *bias_corr, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * TD3 (Fujimoto, van Hoof, Meger 2018) in the fused learner (csrc/tttd3.hip, csrc/tttd3.h): twin critics, target-policy smoothing, delayed
 * actor and target updates, for one agent with the reference-shaped networks and a batch B <= 1024 drawn from its ring.
 * One update, with t = the critic updates done before it (*td->step_dev when the update starts):
 *   mu' = target_actor(s');  eps_b = clip(target_noise * N_b, -noise_clip, noise_clip), N_b standard normal from Philox4x32-10 and
 *   Box-Muller (the recipe of the OU noise) keyed by (row b, t, the domain tag 0x7D3E, noise_seed);  a'_b = clip(mu'_b + eps_b, -1, 1)
 *   (the actor's normalised action units);  y_b = r_b + gamma min(q1'(s', a'), q2'(s', a')), y_b = r_b exactly where done_b;
 *   both critics take an MSE step (scale 2/B) towards y with their own Adam moments and the shared step count t + 1;
 *   full != 0: then the actor's step on -mean Q1(s, mu(s)) through the updated critic 1, counted by the actor's OWN step counter
 *   (actor_step_dev, as torch.optim.Adam counts when step() is called every d-th time), and the soft update of all three targets;
 *   full == 0: nothing but the two critics, their moments and *td->step_dev changes -- the actor, its moments and step count, the
 *   three targets and their fc2 images keep their bits.
 * The agent is described by what the launches take (as tt_pop_agent; the library copies it into device memory at creation, every
 * pointer must stay valid and fixed for the handle's life), so tt_td3_learn makes no host work per call and can be captured:
 *   sample      the replay draw (batch == B, no side buffer, draws <= 1, no step_progress); update u draws with seed + u * seed_stride
 *   jobs        [6] target actor on s', the state branches (z_state) of target critic 1 and of target critic 2 on s', critic 1 and
 *               critic 2 on (s, a) with saved activations, the actor on s with saved activations (not run when full == 0)
 *   td          critic 1's side of the prologue: z_state, mu_target, target_critic (1), reward, done, gamma, y_out (y of critic 1's
 *               workgroups), q_out (q1', required), step_dev and bias_corr_out (both required; shared by the critics), window_dev NULL
 *   z_state_2, target_critic_2, y2_out, q2t_out   the second target head, y as critic 2's workgroups formed it (the same bits), q2'
 *   eps_out     [B] the smoothing noise of the update, always written
 *   step_snapshot   one int64 of device memory: t as the first launch saw it (the second launch advances *step_dev)
 *   actor_step_dev, actor_bias_corr_out   the actor's step count (int64) and its 8 floats of bias corrections, advanced by full updates
 *   critic, critic_2, actor   as tt_pop_agent's networks; the critics' tau applies on full updates only
 *   q_pi, dq_da, tail_words, gave_up_host   as tt_mlp_actor_tail's (the hand-over's epoch is *actor_step_dev)
 * (full == 0 rewrites every target element t as fmaf(0, p - t, t): t itself for every finite p - t, with -0.0 becoming +0.0.)
 * TT_EINVAL with a message in tt_last_error(NULL), before any HIP call: batch outside 1 .. 1024; target_noise or noise_clip
 * negative or not finite; a missing pointer; a side buffer, draws > 1 or step_progress in the sample; window_dev set; two networks
 * that share a per-row workspace, or the two critics a gradient buffer; td / z_state_2 / target_critic_2 that are not the outputs
 * and networks of jobs 0 .. 2, or td->reward / td->done that are not the draw's r_out / d_out.
 * tt_td3_update checks a new description of the same agent as tt_td3_create does and copies it over the handle's descriptor IN
 * PLACE (it waits for the device first): a parameter storage moved, or another seed.  Launches captured before stay valid and
 * read the new description. */
typedef struct tt_td3 tt_td3;
typedef struct tt_td3_agent {
    const tt_sample_args *sample;
    const tt_fwd_job *jobs;              /* [6] */
    const tt_td_input *td;
    tt_pop_net critic, critic_2, actor;
    const float *z_state_2;
    const tt_mlp_weights *target_critic_2;
    float target_noise, noise_clip;
    uint64_t noise_seed;
    float *eps_out, *y2_out, *q2t_out;
    int64_t *step_snapshot, *actor_step_dev;
    float *actor_bias_corr_out;
    float *q_pi, *dq_da;
    int32_t *tail_words, *gave_up_host;
} tt_td3_agent;
int tt_td3_create(int batch, const tt_td3_agent *agent, tt_td3 **out);
int tt_td3_update(tt_td3 *h, const tt_td3_agent *agent);
int tt_td3_learn(tt_td3 *h, int update, int full, tt_stream_t stream);       /* one update, enqueued on stream */
int tt_td3_destroy(tt_td3 *h);                                               /* the caller's stream work with it must be done */

/* ------------------------------------------------------------------------------------------------------
 * TD3 for a population (csrc/ttpop_td3.hip): the TD3 updates of K independent agents (K <= TT_POP_MAX_AGENTS, one batch size
 * B <= 1024 for all) in the launches of ONE agent's tt_td3_learn -- three on a critic-only update, four on a full one -- each
 * launch running every agent's workgroups.  Agent a's results are the bits of tt_td3_learn made with agent a's description.
 * agents[a] is a tt_td3_agent as tt_td3_create takes it, and every check of tt_td3_create is made per agent; the library copies the
 * descriptions into device memory (every pointer must stay valid and fixed for the handle's life), so tt_pop_td3_learn makes no
 * host work per call and can be captured.  `full` is an argument of the launches: the delay is one value for the whole population.
 * target_noise, noise_clip, the learning rates, tau and gamma are each agent's own.  The tail launch of a full update dispatches the
 * row workgroups of ALL agents before any weight workgroup that waits for them; each agent's hand-over words and gave_up_host are
 * its own, and its epoch is its own *actor_step_dev.
 * tt_pop_td3_exploit is tt_pop_exploit for six networks, ONE launch for a list of pairs.  dst != src: dst's six networks, the three
 * Adam moment pairs (critic 1, critic 2, actor) and every fc2 image the descriptions hold become src's.  Every dst then takes the
 * pair's six hyperparameters: alpha (the actor's learning rate), beta (both critics'), tau (all three soft updates; the tau = 0 of
 * critic-only updates stays 0), gamma, target_noise and noise_clip.  Nothing else of dst moves: both step counts, both
 * bias-correction buffers, step_snapshot, tail words, batch buffers, ring, env and noise seed stay its own.  The new values live in
 * the descriptors tt_pop_td3_learn reads, in place: launches captured before stay valid and see them.  list is a HOST array, copied
 * into the launch's arguments.  tt_pop_td3_hyper reads agent a's {alpha, beta, tau, gamma, target_noise, noise_clip} back from
 * the device (synchronous).
 * TT_EINVAL with a message that names the entry point and the agent or pair, before any HIP call: a NULL handle, array or out;
 * count outside 1 .. TT_POP_MAX_AGENTS; batch outside 1 .. 1024; whatever tt_td3_create refuses in an agent; two agents that share
 * a step counter, their tail words, a per-row workspace or a gradient buffer; update < 0; pairs outside [1, K]; an agent index out
 * of range; two pairs with the same dst; a dst that is the src of another pair; a non-finite value; alpha, beta or tau outside
 * (0, 1]; gamma outside (0, 1); a negative target_noise or noise_clip. */
typedef struct tt_pop_td3 tt_pop_td3;
typedef struct tt_pop_td3_pair {
    int32_t dst, src;
    float alpha, beta, tau, gamma, target_noise, noise_clip;
} tt_pop_td3_pair;
int tt_pop_td3_create(int count, int batch, const tt_td3_agent *agents /*[count]*/, tt_pop_td3 **out);
int tt_pop_td3_learn(tt_pop_td3 *pop, int update, int full, tt_stream_t stream);   /* one update of every agent, enqueued on stream */
int tt_pop_td3_exploit(tt_pop_td3 *pop, int pairs, const tt_pop_td3_pair *list /*[pairs], host*/, tt_stream_t stream);
int tt_pop_td3_hyper(tt_pop_td3 *pop, int agent, float out[6]);
int tt_pop_td3_destroy(tt_pop_td3 *pop);                                     /* the caller's stream work with it must be done */

/* ------------------------------------------------------------------------------------------------------
 * Loss shape of the lone learn() (csrc/ttshape.hip): a Huber critic loss and a pre-activation penalty on the actor, inside the
 * launches learn() makes anyway -- the three entry points below stand in for tt_mlp_backward_rows_pair, the ACTOR's
 * tt_mlp_backward_weights and tt_mlp_actor_tail, with the same grids, the same dispatch order and the same hand-over in device
 * memory (no wait added, the bounded one unchanged).
 *   critic   huber_delta = d > 0: loss = huber_loss(q, y, delta = d), mean over the rows (torch.nn.functional.huber_loss), so
 *            d(loss)/dq[b] = scale_critic * clamp(q[b] - y[b], -d, d) with the caller's scale_critic = 1/B.  Inside the
 *            quadratic zone that is HALF the gradient of mse_loss (torch's definition of the Huber loss: 0.5 e^2).
 *            huber_delta = 0: no clamp -- d(loss)/dq[b] = scale_critic * (q[b] - y[b]), the MSE launch with scale_critic = 2/B.
 *   actor    loss = -mean Q(s, mu(s)) + c mean(pre^2), pre [n] = the head's value before tanh, pre[b] = b3 + sum_j h2[b][j] w3[j]:
 *            recomputed in f32 from the saved h2 by the actor's row workgroups of tt_mlp_backward_rows_pair_shaped (the TD
 *            prologue's fma order and wave sum; accurate to f32 against f64, NOT the forward's bits, which are not kept) and
 *            written to shape->pre.  Row b of the weight launch then counts
 *                fmaf(pre_scale, pre[b], row_scale * dq_da[b] * (1 - mu[b]^2))        pre_scale = (float)(2 c / B), formed in f64
 *            times: the penalty's gradient 2 c pre / B does not vanish where tanh saturates.
 * With huber_delta = 0 and pre_scale = 0 the three give the bits of the entry points they stand in for: fmaf(0, pre, f) is f for
 * every finite pre -- except that a factor f = -0.0 can come back as +0.0 (equal as a number) and a non-finite pre makes it NaN.
 * shape->pre may be NULL when pre_scale = 0 (the row launch then stores no pre; the weight launches read none).
 * The learn log (tt_learn_log_*) is unchanged by a loss shape: its critic loss stays the mean square of the TD error and its actor
 * loss stays -mean q_pi, whatever loss the gradients came from.
 * TT_EINVAL with a message that names the entry point, before any HIP call: a NULL shape; huber_delta or pre_scale negative or not
 * finite; pre NULL with pre_scale > 0; the critic (or no row_dq_da / row_mu) passed to tt_mlp_backward_weights_shaped; count other
 * than 0 or 10 there; and whatever the entry point it stands in for refuses. */
typedef struct tt_loss_shape {
    float huber_delta;   /* 0 = MSE with the caller's scale */
    float pre_scale;     /* k = 2c/B, >= 0 */
    float *pre;          /* [n], required when pre_scale > 0 */
} tt_loss_shape;
int tt_mlp_backward_rows_pair_shaped(int n, float scale_critic, const float *q_out, const tt_mlp_weights *critic,
                                     const tt_mlp_saved *saved_critic, const tt_mlp_bwd_ws *ws_critic, const tt_td_input *td,
                                     const float *mu_out, const tt_mlp_weights *actor, const tt_mlp_saved *saved_actor,
                                     const tt_mlp_bwd_ws *ws_actor, const tt_image_job *image, const tt_loss_shape *shape,
                                     tt_stream_t stream);
int tt_mlp_backward_weights_shaped(int n, int critic /* must be 0 */, const float *obs, const float *action, const tt_mlp_saved *saved,
                                   const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, const float *row_dq_da, const float *row_mu,
                                   float row_scale, int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                                   float *const *targets, const int64_t *step_dev, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, float tau, const tt_fc2_images *images, const float *bias_corr,
                                   const tt_loss_shape *shape, tt_stream_t stream);
int tt_mlp_actor_tail_shaped(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                             const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                             int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                             const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                             const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host,
                             const tt_loss_shape *shape, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Demonstration loss of the lone learn() (csrc/ttdemo.hip): a behaviour-cloning term on the batch rows that came from the replay
 * side buffer, gated by a Q-filter (Nair et al. 2018), inside the launches learn() makes anyway.  For a batch of B rows the actor
 * loss is
 *     -mean_b Q(s_b, mu(s_b)) + lambda (1/B) sum_b m_b (mu_b - a_b)^2
 * a_b = the row's stored action; demo_b = idx[2 b] < 0, the mark the replay draw leaves for a side-buffer row (tt_sample_args.idx_out);
 * m_b = demo_b, and with q_filter also q_b > q_pi_b (strict; a NaN on either side leaves m_b = 0).
 * THE TWO SIDES OF THE FILTER ARE ONE CRITIC ADAM STEP APART:
 *   q_b    = Q(s_b, a_b) as learn()'s FIRST launch computed it, with the critic BEFORE this update -- the q the TD error uses;
 *   q_pi_b = Q(s_b, mu(s_b)) through the UPDATED critic -- the q_out of these launches, the number the actor loss is built from.
 * Both numbers exist anyway; a second critic forward on (s, a) would lengthen the launch the learn chain waits on longest.
 * The actor's row factor row_scale dQ/da (1 - mu^2), row_scale = -1/B, is linear in dQ/da, so the whole term is an EFFECTIVE
 *     dq_eff[b] = m_b ? fmaf(-k, mu_b - a_b, dQ/da_b) : dQ/da_b            k = (float)(2 lambda), formed in f64 by the caller
 * (a row with m_b = 0 keeps the bits of dQ/da_b).  Lane 0 of a row of the critic's pass on (s, mu(s)) writes the TRUE derivative to
 * dq_da[b], dq_eff[b], and code[b] = 0 (a ring row), 1 (a demonstration row the filter left out) or 2 (a demonstration row applied).
 *   tt_mlp_forward_save_demo   tt_mlp_forward_save(critic on (s, mu(s)), dq_da) of the five-launch chain; the actor's weight launch
 *                              that follows is tt_mlp_backward_weights[_shaped] with row_dq_da = demo->dq_eff.
 *   tt_mlp_actor_tail_demo     tt_mlp_actor_tail_shaped: the same grid, dispatch order and hand-over (the 8-byte word of a row carries
 *                              dq_eff; no wait, flag or atomic added).  shape may be NULL: then tt_mlp_actor_tail.
 * With no demonstration row in the batch both leave the bits of the entry points they stand in for.
 * TT_EINVAL with a message that names the entry point, before any HIP call: a NULL demo; k negative or not finite; a, idx, dq_eff or
 * code NULL; q NULL with q_filter; dq_eff equal to dq_da; no dq_da; critic = 0 in tt_mlp_forward_save_demo; and whatever the entry
 * point it stands in for refuses. */
typedef struct tt_demo_loss {
    const float *a;       /* [n] the batch's stored actions */
    const int32_t *idx;   /* [n][2] the draw's index buffer: idx[2 b] < 0 = a side-buffer row */
    const float *q;       /* [n] Q(s, a) with the critic before this update; read with q_filter only */
    float k;              /* 2 lambda, >= 0 */
    int32_t q_filter;     /* 0 = every demonstration row is applied */
    float *dq_eff;        /* [n] out */
    int32_t *code;        /* [n] out: 0, 1 or 2 */
} tt_demo_loss;
int tt_mlp_forward_save_demo(int n, int critic /* must be 1 */, const float *obs, const float *action, const tt_mlp_weights *w,
                             float *out, const tt_mlp_saved *saved, float *dq_da, const tt_demo_loss *demo, tt_stream_t stream);
int tt_mlp_actor_tail_demo(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                           const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale, int count,
                           float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                           const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                           const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host,
                           const tt_loss_shape *shape /* may be NULL */, const tt_demo_loss *demo, tt_stream_t stream);
/* Ring rows of EXPERT LANES as demonstration rows (tt_env_mpc_act_ring): with expert_lanes = M >= 0
 *     demo_b = idx[2 b] < 0  or  idx[2 b + 1] < M
 * -- a ring row's idx pair is (slot, lane), and lanes [0, M) of the loop's env are driven by the expert.  q, q_pi, the strict
 * comparison, dq_eff and the code values are unchanged (code 1 / 2 for a ring row of an expert lane as well).  The count travels
 * by value so that tt_demo_loss keeps its layout; the entry points above are these with expert_lanes = 0, bit for bit.
 * TT_EINVAL in the entry point's own name, before any HIP call: expert_lanes < 0, and everything the entry point above refuses. */
int tt_mlp_forward_save_demo_lanes(int n, int critic /* must be 1 */, const float *obs, const float *action, const tt_mlp_weights *w,
                                   float *out, const tt_mlp_saved *saved, float *dq_da, const tt_demo_loss *demo, int32_t expert_lanes,
                                   tt_stream_t stream);
int tt_mlp_actor_tail_demo_lanes(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                                 const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                                 int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                                 float *const *targets, const int64_t *step_dev, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, float tau, const tt_fc2_images *images, const float *bias_corr,
                                 int32_t *tail_words, int32_t *gave_up_host, const tt_loss_shape *shape /* may be NULL */,
                                 const tt_demo_loss *demo, int32_t expert_lanes, tt_stream_t stream);
/* EXPERT LABELS in the demonstration term (tt_env_mpc_label_ring).  A ring row of batch row b, idx[2 b] >= 0,
 * with first <= idx[2 b + 1] < first + count is a LABELLED ROW:
 *     a*_b   = label[idx[2 b] * n_envs + idx[2 b + 1]]      the expert's decision on the state the policy acted in
 *     m_b    = 1                                            never filtered, whatever q_filter says: q rates the STORED action, and
 *                                                           no launch computes Q(s, a*)
 *     dq_eff = fmaf(-k, mu_b - a*_b, dQ/da_b)
 *     code   = 3
 * (idx[2 b] is taken to be < slots, as the draw leaves it; a row with a slot past the array is not labelled.)  Every other row is
 * as in the _lanes form: a side row or a ring row of a lane < expert_lanes has the target demo->a[b], the filter, code 1 or 2; any
 * other ring row code 0 and the bits of dQ/da.  labels == NULL is the _lanes form, the same launches and bits.
 * TT_EINVAL in the entry point's own name, before any HIP call: everything the _lanes form refuses; with labels, label NULL,
 * n_envs < 1, slots < 1, first < 0, count < 1, first + count > n_envs, first < expert_lanes (an overlap). */
typedef struct tt_demo_labels {
    const float *label;            /* [slots, n_envs] the ring's label array */
    int32_t n_envs, slots;
    int32_t first, count;          /* labelled lanes [first, first + count) */
} tt_demo_labels;
int tt_mlp_forward_save_demo_labels(int n, int critic /* must be 1 */, const float *obs, const float *action, const tt_mlp_weights *w,
                                    float *out, const tt_mlp_saved *saved, float *dq_da, const tt_demo_loss *demo, int32_t expert_lanes,
                                    const tt_demo_labels *labels /* may be NULL */, tt_stream_t stream);
int tt_mlp_actor_tail_demo_labels(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                                  const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                                  int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                                  float *const *targets, const int64_t *step_dev, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, float tau, const tt_fc2_images *images, const float *bias_corr,
                                  int32_t *tail_words, int32_t *gave_up_host, const tt_loss_shape *shape /* may be NULL */,
                                  const tt_demo_loss *demo, int32_t expert_lanes, const tt_demo_labels *labels /* may be NULL */,
                                  tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Gradient-norm clipping of the lone learn() (csrc/ttclip.hip): torch.nn.utils.clip_grad_norm_(parameters,
 * max_norm) in front of optimizer.step(), as the optimizer launch of one network.  Clipping by the GLOBAL norm depends on every
 * element of the network's gradient, so it cannot ride in the weight-gradient launch (tt_mlp_backward_weights with count = 0 leaves
 * the gradients in memory); tt_adam_soft_update_clipped is tt_adam_soft_update with two launches on `stream`:
 *   1. the sum of squares of the `count` gradient tensors in f64 (the square of an f32 is exact there), over a fixed partition of
 *      the tensors laid end to end into TT_GRAD_CLIP_PARTIALS workgroups, each in a fixed order, each storing one partial into
 *      clip->partials[w] -- no atomics, no wait between workgroups: the same inputs give the same bits, eager or replayed.  Ragged
 *      numel are served by 16-byte loads between scalar heads and tails; nothing outside the tensors is read.
 *   2. tt_adam_soft_update's launch, in which every workgroup adds the partials in index order in f64 (the same bits in each) and
 *          norm = sqrt(sum)        coef = (float)(max_norm / (norm + 1e-6)), 1 where that is greater than 1
 *      (clip_grad_norm_'s formula), and the gradient that enters Adam is g = fmaf(weight_decay, p, coef * grad) with the product
 *      rounded on its own; moments, bias corrections, parameter, soft target update and fc2 images as tt_adam_soft_update.  With
 *      coef == 1 the product is exact and the launch leaves tt_adam_soft_update's bits.
 * out[0] = (float)norm, out[1] = coef.  counts (may be NULL): counts[0] += 1, counts[1] += (coef < 1), by plain loads and stores of
 * one thread -- one launch at a time may touch them.  The gradient buffers are NOT rewritten: they keep the unclipped gradient (so
 * the learn log's norms, tt_learn_log_*, stay those of the unclipped gradient).  A non-finite norm gets no special case (torch's
 * error_if_nonfinite=False): norm = inf gives coef = 0, a NaN stays a NaN in coef and in everything it multiplies.
 * TT_EINVAL with a message that names the entry point, before any HIP call: a NULL clip, partials or out; max_norm not finite or
 * not > 0; count outside 1..12; a NULL array or tensor; a negative (or, as tt_adam_soft_update, zero) numel. */
#define TT_GRAD_CLIP_PARTIALS 64
typedef struct tt_grad_clip {
    float max_norm;      /* finite, > 0 */
    double *partials;    /* [TT_GRAD_CLIP_PARTIALS] workspace the caller owns, one per clipped network */
    float *out;          /* [2]: the norm, the coefficient */
    int64_t *counts;     /* [2] or NULL: updates, updates with coef < 1 */
} tt_grad_clip;
int tt_adam_soft_update_clipped(int count, float *const *params, const float *const *grads, float *const *exp_avg,
                                float *const *exp_avg_sq, float *const *targets, const int32_t *numel, const int64_t *step_dev,
                                float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                                const tt_fc2_images *images, const float *bias_corr, const tt_grad_clip *clip, tt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TTENV_H */
