/*
 * rrl_hip.h -- C ABI of librrl_hip.so, the MI355X (gfx950) hot path of Recovery RL.
 *
 * Drop-in boundary.  The reference has no FFI layer; its operator
 * boundary for this path is the gym env protocol (env/navigation1.py:55-97), the replay
 * protocol (recovery_rl/replay_memory.py:11-75) and the CEM optimiser
 * (recovery_rl/optimizers.py:73-124).  Every entry point below names the reference
 * interface it replaces.  INTEGRATION.md shows the ctypes stub a reference maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensor.data_ptr());
 *     the library allocates nothing and keeps no global state; all calls are re-entrant;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued asynchronously on it
 *     (NULL = the default stream) and is safe to capture in a hipGraph;
 *   - return value: 0 on success, a negative RRL_E* code on error; nothing throws;
 *   - random draws come from Philox4x32-10 keyed by `seed`, counter words
 *     (row index, stream id, counter lo, counter hi).  `counter_dev` (nullable) points to
 *     device uint64[2] = {tick, ticket(internal, keep 0)}: tick is ADDED to `counter`, and
 *     where a function takes `counter_inc` the last workgroup to finish does
 *     tick += counter_inc, so a captured hipGraph advances its own RNG counter on replay;
 *   - env kinds: 0 navigation1, 1 navigation2, 2 maze.
 */
#ifndef RRL_HIP_H
#define RRL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRL_OK 0
#define RRL_EINVAL (-1)   /* bad argument (unknown env kind, negative size, null pointer) */
#define RRL_ELAUNCH (-2)  /* hipLaunchKernel failed; see rrl_last_hip_error() */
#define RRL_ECAPTURE (-5) /* a packed launch (rrl_*_packed) met an argument block it has not seen before while the stream was
                           * capturing: building its device copy (hipMalloc + copy) inside the capture would invalidate the
                           * graph.  Launch the same arguments once before the capture (the warm-up iterations do). */
#define RRL_EPLANS (-6)   /* more than 8192 distinct argument blocks of packed launches alive: rrl_pack_clear() */
#define RRL_ERANGE (-3)   /* size outside what the kernel supports (e.g. batch > 1024) */

enum { RRL_ENV_NAV1 = 0, RRL_ENV_NAV2 = 1, RRL_ENV_MAZE = 2 };

enum {
    RRL_STREAM_STEP = 0,       /* env transition noise           */
    RRL_STREAM_RESET = 1,      /* env reset noise                */
    RRL_STREAM_OFFLINE = 2,    /* offline constraint data        */
    RRL_STREAM_SAMPLE = 3,     /* replay sampling (positives)    */
    RRL_STREAM_SAMPLE_NEG = 4, /* replay sampling (negatives)    */
    RRL_STREAM_CEM = 5,        /* CEM truncated-normal samples   */
    RRL_STREAM_ACTION = 6,     /* uniform random actions         */
    RRL_STREAM_PLAN = 7,       /* planner particle noise         */
    RRL_STREAM_NOISE = 8       /* policy noise (rrl_normal_fill) */
};

/* ABI version, bumped on any signature change. */
int rrl_abi_version(void);
/* hipGetLastError() of the calling thread's last failed launch, as an int (0 = none). */
int rrl_last_hip_error(void);
/* *ctr += inc on the stream (one thread).  Lets a captured graph advance its RNG counter. */
int rrl_counter_add(uint64_t* ctr, uint64_t inc, void* stream);

/* --------------------------------------------------------------------------------------------
 * Environments.  Replaces Navigation1.step / Navigation2.step (env/navigation1.py:71-89,
 * env/navigation2.py:70-88) + the horizon rule of the driver (recovery_rl/experiment.py:434-435)
 * for n independent envs in lock-step.
 *   pos        [n,2] f64  in/out  env state (the reference keeps float64 state)
 *   action     [n,2] f32  in      raw action; clipped to [-1,1] inside (process_action :50-51)
 *   noise      [n,2] f64  in      N(0,1) draws to use instead of Philox, or NULL
 *   next_obs   [n,2] f32  out     s' BEFORE any auto-reset (what replay / info["next_state"] get)
 *   obs        [n,2] f32  out     observation for the next policy call (post-reset), nullable
 *   reward     [n]   f32  out     -||s|| of the OLD state (step_cost :106-110)
 *   done       [n]   u8   out     reward > -4 or obstacle(s')            (:80)
 *   constraint [n]   u8   out     obstacle(s')                           (:82)
 *   success    [n]   u8   out     reward > -4                            (:88)
 *   ep_done    [n]   u8   out     done or t == horizon (experiment.py:435), nullable
 *   t          [n]   i32  in/out  per-env step count (self.time :78)
 *   auto_reset != 0: where ep_done, pos <- [-50,0] + N(0,I) (reset :91-97) and t <- 0.
 * ------------------------------------------------------------------------------------------ */
int rrl_nav_step(int env_kind, int64_t n, double* pos, const float* action, const double* noise,
                 uint64_t seed, uint64_t counter, uint64_t* counter_dev, uint64_t counter_inc,
                 float* next_obs, float* obs, float* reward, uint8_t* done, uint8_t* constraint,
                 uint8_t* success, uint8_t* ep_done, int32_t* t, int32_t horizon, int auto_reset,
                 void* stream);

/* The same step in the compact layout of the bandwidth regime (56 B moved per env-step instead of 72; same
 * arithmetic, same bits).  The step count and the four flags of rrl_nav_step share ONE u16 status word per env:
 *   status     [n]   u16  in/out  bits 0-11 steps taken in the running episode (in: before, out: after; 0 after an
 *                                 auto-reset), bit 12 done, 13 constraint, 14 success, 15 ep_done (out; ignored on input)
 *   reset_obs  [n,2] f32  out     written ONLY at rows with ep_done when auto_reset != 0: the observation after the
 *                                 reset (= float(pos) of that row).  Everywhere else the next policy input is next_obs
 *                                 itself.  Nullable, and NULL is the fast form in the bandwidth regime: ~200 k
 *                                 scattered 8-byte stores cost as much as a dense 8 B/env array (+45 us at 2^24 envs).
 * horizon <= 4095 (RRL_ERANGE otherwise).  pos / action / noise / next_obs / reward 16-byte aligned, status and
 * reset_obs 8-byte aligned (RRL_EINVAL otherwise). */
#define RRL_STATUS_STEPS 0x0fffu
#define RRL_STATUS_DONE 0x1000u
#define RRL_STATUS_CONSTRAINT 0x2000u
#define RRL_STATUS_SUCCESS 0x4000u
#define RRL_STATUS_EP_DONE 0x8000u
int rrl_nav_step_compact(int env_kind, int64_t n, double* pos, const float* action, const double* noise,
                         uint64_t seed, uint64_t counter, uint64_t* counter_dev, uint64_t counter_inc,
                         float* next_obs, float* reset_obs, float* reward, uint16_t* status, int32_t horizon,
                         int auto_reset, void* stream);

/* Replaces Navigation*.reset (env/navigation1.py:91-97) for n envs. `mask` (nullable, u8[n])
 * restricts the reset to rows with mask != 0.  obs / t nullable. */
int rrl_nav_reset(int env_kind, int64_t n, double* pos, float* obs, int32_t* t,
                  const uint8_t* mask, const double* noise, uint64_t seed, uint64_t counter,
                  const uint64_t* counter_dev, void* stream);

/* T open-loop steps with the state held in registers (no auto-reset, no horizon):
 * actions [T,n,2]; outputs [T,n,...] (each nullable).  The CEM ground-truth-dynamics mode
 * and the roofline sweep use it. Step k uses counter + k. */
int rrl_nav_rollout(int env_kind, int64_t n, int32_t T, double* pos, const float* actions,
                    uint64_t seed, uint64_t counter, const uint64_t* counter_dev,
                    float* obs_seq, float* reward_seq, uint8_t* constraint_seq, uint8_t* done_seq,
                    void* stream);

/* Replaces get_offline_data (env/navigation1.py:133-164, env/navigation2.py:133-243): one
 * scripted <=10-step rollout per thread, stream-compacted in rollout order into replay-row
 * arrays (s,a,constraint,s',mask) of `capacity` rows.  *count_dev (device int64) receives the
 * number of rows written.  scratch: device int32[n_rollouts + 1]. Use rrl_nav_offline_rollouts()
 * for n_rollouts. */
int64_t rrl_nav_offline_rollouts(int env_kind, int64_t num_transitions);
int rrl_nav_offline(int env_kind, int64_t num_transitions, uint64_t seed, float* s, float* a,
                    float* c, float* s2, float* m, int64_t capacity, int64_t* count_dev,
                    int32_t* scratch, void* stream);

/* --------------------------------------------------------------------------------------------
 * Maze.  Replaces MazeNavigation.step / reset / get_offline_data (env/maze.py:139-213, 34-107).
 * The reference steps MuJoCo 1.50 (third-party, absent); these kernels run the kinematic
 * surrogate of DESIGN.md section 6 -- same control flow, reward, termination and geometry.
 * Buffers as rrl_nav_step; `done` already contains the env's own horizon (env/maze.py:153).
 * Reset modes: 0 'h' (default), 1 'e', 2 'm', 3 None (env/maze.py:187-196).
 * ------------------------------------------------------------------------------------------ */
int rrl_maze_step(int64_t n, double* pos, const float* action, uint64_t seed, uint64_t counter,
                  uint64_t* counter_dev, uint64_t counter_inc, float* next_obs, float* obs,
                  float* reward, uint8_t* done, uint8_t* constraint, uint8_t* success,
                  uint8_t* ep_done, int32_t* t, int32_t horizon, int auto_reset, void* stream);
int rrl_maze_reset(int64_t n, double* pos, float* obs, int32_t* t, const uint8_t* mask, int mode,
                   int check_constraint, uint64_t seed, uint64_t counter,
                   const uint64_t* counter_dev, void* stream);
/* writes exactly 2 * (num_transitions / 2) rows (half random, half expert actions) */
int rrl_maze_offline(int64_t num_transitions, uint64_t seed, float* s, float* a, float* c,
                     float* s2, float* m, int64_t capacity, void* stream);

/* --------------------------------------------------------------------------------------------
 * Replay.  Replaces ReplayMemory / ConstraintReplayMemory (recovery_rl/replay_memory.py).
 * Layout: structure-of-arrays ring, f32: s[cap,2] a[cap,2] r[cap] s2[cap,2] m[cap] = 32 B/row.
 *   state   device int64[4]: {position, size, ticket(internal, keep 0), error flag}
 *   pos_cnt device int32[RRL_POS_CNT_LEN(cap)] (zero-initialised) or NULL: number of rows with r != 0 per 64-slot chunk,
 *           then (from the next multiple of 4) per 1024-slot super-chunk, then (from the next multiple of 2) one
 *           64-bit mask per chunk (bit b = slot 64 c + b holds such a row; 8-byte aligned: keep pos_cnt 8-byte
 *           aligned); maintained by push, consumed by the stratified sampler (replay_memory.py:50,58-66), which scans
 *           the second level only (cap / 1024 entries), one super-chunk's 16 first-level counts and one mask per
 *           drawn row.
 * ------------------------------------------------------------------------------------------ */
#define RRL_POS_CNT_LEN(cap) \
    ((((((((cap) + 63) / 64 + 3) / 4) * 4 + ((cap) + 1023) / 1024) + 1) / 2) * 2 + 2 * (((cap) + 63) / 64))
typedef struct {
    float* s;
    float* a;
    float* r;
    float* s2;
    float* m;
    int64_t cap;
    int64_t* state;
    int32_t* pos_cnt;
    int32_t flags;       /* RRL_REPLAY_* bits */
    int64_t pinned;      /* rows [0, pinned) are never overwritten: after slot cap - 1 the ring continues at slot `pinned`
                          * (0 = the reference's plain ring, replay_memory.py:21-25).  The lock-step loop pins the offline
                          * constraint demonstrations: N envs fill a 1e6-row ring in 1e6 / N iterations, whereas the one-env
                          * reference never wraps within a run (4e4 env-steps), i.e. never loses them. */
} rrl_replay_t;

/* Stratified draws (RRL_DRAW_STRATIFIED) that ask for more positives (or negatives) than the ring holds: the
 * reference aborts (random.sample raises ValueError, replay_memory.py:61-66) and so does the default here (error flag
 * state[3] = 1, outputs untouched).  With this bit the draw takes every row of the short class and fills the batch
 * from the other one: n_pos' = min(n_pos, positives), n_neg' = B - n_pos' (and the other way round).  The lock-step
 * loop sets it: thousands of envs overwrite a 1e6-row ring in a few hundred iterations, so a policy that has learned
 * to avoid violations starves the positive class -- a state the one-env reference cannot reach within its runs. */
#define RRL_REPLAY_CLAMP_STRATIFIED 1

/* push (replay_memory.py:21-25,47-52) of n rows in row order; `valid` (nullable u8[n]) drops
 * rows with valid == 0 (used for add_both_transitions, experiment.py:446-448).
 * scratch: device int32[ceil(n/1024) + 1], only read when valid != NULL. */
int rrl_replay_push(const rrl_replay_t* rb, int64_t n, const float* s, const float* a,
                    const float* r, const float* s2, const float* m, const uint8_t* valid,
                    int32_t* scratch, void* stream);

/* One policy-head evaluation: the sampling step behind a policy stack's last linear layer.  Used by
 * rrl_policy_heads_fwd_multi (a launch of up to four), by the input head of rrl_stack_t (in_head) and by the recovery
 * action of the fused env step (rrl_step_push_t.sel_rec_head); the same formulas and the same bits in all three.
 *   kind         RRL_HEAD_GAUSS: GaussianPolicy.sample (recovery_rl/model.py:324-340).  head[b] = (mean0, mean1, log_std0,
 *                  log_std1); log_std is clamped to [-20, 2] (model.py:14-16); y = tanh(mean + exp(log_std) eps),
 *                  action = y scale + bias, mean_out = tanh(mean) scale + bias,
 *                  logp = sum_j -eps_j^2 / 2 - log_std_j - log(2 pi) / 2 - log(scale_j (1 - y_j^2) + 1e-6).
 *                RRL_HEAD_STOCH: StochasticPolicy.sample (model.py:511-525).  head[b] = the two raw outputs;
 *                  mean = tanh(raw) scale + bias, action = mean + exp(max(log_std, min_log_std)) eps, mean_out = mean.
 *                Anything else: RRL_EINVAL.
 *   B            rows, >= 1 (RRL_EINVAL); any size: one thread per row, 256 rows per workgroup
 *   head         [B,4] (Gaussian) / [B,2] (stochastic) f32, required: the stack's output, as n_part partial sums
 *   n_part,      part_stride floats apart (element i = p[i] + p[part_stride + i] + ..., fixed order: the partial last-layer
 *   part_stride  sums of rrl_mlp3_forward(scratch, finalize = 0)); n_part = 1: a plain tensor.  1 <= n_part <= 4 (RRL_EINVAL)
 *   eps          [B,2] N(0,1) draws.  Gaussian: required.  Stochastic: nullable, NULL = no noise (action = mean)
 *   scale, bias  [2] action_scale / action_bias of the policy, required
 *   action       out, required: row b at action + b * ld_action (2 floats); ld_action = 2 for a plain [B,2] tensor, 4 to
 *   ld_action    write columns 2..3 of a [B,4] critic input in place
 *   logp         [B] out, nullable.  Gaussian only (the stochastic head has no log-probability and ignores the field)
 *   mean_out     [B,2] out, nullable: the deterministic action (the reference's third return value), both kinds
 *   obs_in,      Gaussian only, nullable: obs_in [B,2] is copied to obs_out + b * ld_action (2 floats), which assembles the
 *   obs_out      [s | a] critic input in place when obs_out is the [B,4] buffer and action its column 2.  obs_in without
 *                obs_out: RRL_EINVAL.  The stochastic head ignores both
 *   log_std,     stochastic only: the policy's log_std parameter [2] (required) and its lower clamp
 *   min_log_std
 * A lone head is rrl_policy_heads_fwd_multi(1, ...). */
enum { RRL_HEAD_GAUSS = 0, RRL_HEAD_STOCH = 1 };
typedef struct {
    int kind, B;
    const float* head;
    int n_part;
    long long part_stride;
    const float *eps, *scale, *bias;
    float* action;
    int ld_action;
    float *logp, *mean_out;
    const float* obs_in;
    float* obs_out;
    const float* log_std;
    float min_log_std;
} rrl_policy_head_t;

/* One replay draw: B = n_pos + n_neg distinct rows of a ring, gathered into five batch tensors (row i of the batch is
 * drawn by lane i of ONE workgroup).  Replaces ReplayMemory.sample / ConstraintReplayMemory.sample
 * (replay_memory.py:27-30,54-72).  Three modes (`stratified`); 1 <= B <= 1024 and n_pos, n_neg >= 0 in all of them:
 *   RRL_DRAW_UNIFORM     sample (replay_memory.py:27-30): B distinct uniform rows among the `size` filled ones; only the
 *                        sum n_pos + n_neg is used.  cap < 2^31.  B > size: error flag 1 (the reference raises ValueError;
 *                        callers guard, experiment.py:397,403).
 *   RRL_DRAW_STRATIFIED  stratified sample (replay_memory.py:54-72): first n_pos rows uniform among the slots with r != 0,
 *                        then n_neg rows uniform among the filled slots with r == 0.  Needs rb->pos_cnt (RRL_EINVAL
 *                        without) and cap <= 2^21.  A class with fewer rows than asked: error flag 1, or the clamped draw
 *                        with RRL_REPLAY_CLAMP_STRATIFIED in rb->flags (then only B > size is an error).
 *   RRL_DRAW_DEMO_SHARE  a vectorisation rule, not a reference function: first n_pos (= n_demo) distinct uniform rows of the
 *                        pinned range [0, rb->pinned) (the offline constraint demonstrations, experiment.py:278-286), then
 *                        n_neg (= n_online) distinct uniform rows of the online range [rb->pinned, size).  In a one-env
 *                        reference run the 20 000 demonstrations stay about half of recovery_memory from the first to the
 *                        last episode (uniform draw, replay_memory.py:54-72, qrisk.py:100-105); N lock-step envs push N
 *                        rows per iteration, so a uniform draw over the ring would show the safety critic the
 *                        demonstrations -- the only violations a safe policy ever produces -- in 2 % of its batch rows.
 *                        This draw keeps their share fixed.  A range with fewer rows than asked gives every row it has and
 *                        the other range fills the batch (n_online' = min(n_online, size - pinned), n_demo' = B - n_online',
 *                        and the other way round); B > size: error flag 1.  cap < 2^31, 0 <= pinned < cap.
 * Checked before anything is launched, in this order: the ring (rb, its five arrays and state non-NULL, cap > 0) and the
 * five outputs, else RRL_EINVAL; n_pos, n_neg and B, else RRL_ERANGE; then the mode's own bounds (capacity, pinned:
 * RRL_ERANGE; an unknown mode or a stratified draw without pos_cnt: RRL_EINVAL).
 *   seed, counter      lane i of the first group (uniform: every lane; the positives; the demonstrations) draws from Philox
 *   counter_dev        stream RRL_STREAM_SAMPLE at row i, lane j of the second group (negatives; online rows) from
 *   counter_inc        RRL_STREAM_SAMPLE_NEG at row j, at counter + tick (see the conventions above).  A draw that passes
 *                      its population check does tick += counter_inc; one that raises error flag 1 leaves the tick alone.
 *   s, a, r, s2, m     out, required: [B,2] [B,2] [B] [B,2] [B] f32
 *   idx_out            out, nullable: int64[B], the chosen slots
 *   xu, x2u, xpu       out, nullable: f32 [B,4] rows pre-assembled for the networks, xu = (s, a), x2u = (s', -, -),
 *                      xpu = (s, -, -) (columns 2..3 of the latter two are written later by the policy heads)
 * Error flags (rb->state[3], outputs untouched; ReplayMemory.check_error): 1 population too small (above); 2 the
 * rejection rounds did not end (after the tick advanced); 3 pos_cnt disagrees with the rows (stratified); 4 see
 * rrl_draw_ahead_t. */
enum { RRL_DRAW_UNIFORM = 0, RRL_DRAW_STRATIFIED = 1, RRL_DRAW_DEMO_SHARE = 2 };
typedef struct {
    const rrl_replay_t* rb;
    int stratified;
    int32_t n_pos, n_neg;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    uint64_t counter_inc;
    float *s, *a, *r, *s2, *m;
    int64_t* idx_out;
    float *xu, *x2u, *xpu;
} rrl_draw_t;
/* The two draws of one lock-step iteration (task buffer -> SAC update, safety buffer -> Q_risk update,
 * experiment.py:397-416) and the iteration's policy noise (rrl_normal_fill: noise_pairs pairs into noise_out, its own
 * seed and tick) in ONE launch: they do not depend on each other.  `second` and the noise part (noise_pairs = 0) are
 * optional; a lone draw is rrl_sample_multi(first, NULL, 0, ...).  first == NULL, noise_pairs < 0 or >= 2^32, or
 * noise_pairs > 0 without noise_out: RRL_EINVAL, before the draws are looked at.  Every member runs on its own
 * workgroups, so rows, indices and normals do not depend on what else is in the launch. */
int rrl_sample_multi(const rrl_draw_t* first, const rrl_draw_t* second, long long noise_pairs, uint64_t noise_seed,
                     uint64_t noise_counter, uint64_t* noise_counter_dev, uint64_t noise_counter_inc, float* noise_out,
                     void* stream);

/* Draw-ahead: the uniform draw in two halves.  SELECT picks the B keys of `draw` for the ring as it will be `rows_ahead`
 * pushed rows from now (size' = min(cap, size + rows_ahead); 0 = the ring as it is) at the tick as it is, and leaves them in
 * `keys` [B + RRL_AHEAD_META] (keys, then tick, size' and the error code of the selection); it changes nothing else -- the
 * tick is not advanced and no flag raised.  GATHER (a rider of rrl_mlp3_forward_riders) does, after those rows were pushed,
 * what the draw does around its selection: flags rb.state[3] = 1 (B > size') before, = 2 (round cap) after advancing the
 * tick, gathers the rows of the keys into the draw's outputs.  Select + pushes + gather leave exactly what the pushes + the
 * whole draw leave; keys drawn for another tick or size are refused (rb.state[3] = 4).  Another mode: RRL_EINVAL. */
#define RRL_AHEAD_META 8
typedef struct {
    const rrl_draw_t* draw;      /* RRL_DRAW_UNIFORM */
    int64_t rows_ahead;          /* select only */
    uint32_t* keys;
} rrl_draw_ahead_t;
int rrl_draw_select(const rrl_draw_ahead_t* sel, void* stream);

/* Fused lock-step iteration tail: env step + reward penalty + bootstrap mask + memory.push + recovery_memory.push +
 * episode counters in ONE launch (the body of recovery_rl/experiment.py:420-461 for n envs in lock-step; Maze:
 * env/maze.py:139-213), optionally with the recovery gate of Experiment.get_action (experiment.py:546-577) in front and
 * the per-episode log behind.  Rows stored: memory <- (state, task_action or the executed action if push_real_action,
 * reward - reward_penalty * constraint, next_obs, 1 - done); recovery_memory (nullable) <- (state, executed action,
 * constraint, next_obs, 1 - done).  Every field is described here once; a zero-initialised struct has every option off. */
typedef struct {
    int64_t n;
    double* pos;             /* [n,2] in/out  env state (as rrl_nav_step / rrl_maze_step) */
    int32_t* t;              /* [n]   in/out  per-env step count; may be NULL when `status` is given */
    uint16_t* status;        /* [n]   in/out  nullable: the COMPACT per-env state, one u16 word per env (RRL_STATUS_*: step
                              * count in bits 0-11, so 1 <= horizon <= 4095, done / constraint / success / ep_done of the last
                              * step in bits 12-15).  It replaces `t` and the four u8 flag arrays, and with it the stored
                              * `state` of the replay rows is float(pos), so `obs` is written only (8 B less read, 8 + 4 B
                              * less written per env-step than t + flags).  Rows, counters and env state are the same bits. */
    float* obs;              /* [n,2] in/out  the current observation on entry (the stored `state`), the next one on return */
    const float* task_action;/* [n,2] in      the task policy's action; rows are ld_task floats apart (even, >= 2: the
                              * [s | a] input of the safety critic, ld_task = 4, can be passed as it is) */
    int32_t ld_task;
    const float* real_action;/* [n,2] in      the executed action, and (nullable) whether it is a recovery action: */
    const uint8_t* recovery; /* [n]   in      both read when sel_z == NULL, ignored otherwise */
    /* sel_z != NULL: the recovery gate is evaluated in the kernel, one launch less per lock-step iteration.
     * recovery[i] = max(sigmoid(z[i]), sigmoid(z[n + i])) > sel_eps_safe; executed action = recovery ? rec : task. */
    const float* sel_z;      /* [2,n] pre-sigmoid twin Q_risk(s, a_task), given as sel_n_part (1..4) partial sums */
    int32_t sel_n_part;      /* sel_part_stride floats apart, like every stack output (rrl_mlp3_forward with scratch) */
    long long sel_part_stride;
    float sel_eps_safe;
    const float* sel_rec_action;            /* [n,2] the recovery action, or NULL: it is evaluated in the kernel from */
    const rrl_policy_head_t* sel_rec_head;  /* this RRL_HEAD_STOCH description (its formula on the recovery policy's
                                             * stack output) */
    float* real_action_out;  /* [n,2] out     with the gate: the executed action and the flag, */
    uint8_t* recovery_out;   /* [n]   out     what rrl_recovery_select would have written */
    uint64_t seed, counter;  /* Philox stream position, as rrl_nav_step */
    uint64_t* counter_dev;
    uint64_t counter_inc;
    int32_t horizon, auto_reset;
    float reward_penalty;
    int32_t push_real_action;                       /* disable_action_relabeling (experiment.py:437-441) */
    const rrl_replay_t *memory, *recovery_memory;   /* n <= cap - pinned of each; recovery_memory nullable */
    /* per-env outputs of the step for callers that read them (the `info` fields of env.step: episode log, online model
     * re-fit): each may be NULL = not written (17 of the 171 B the kernel moves per env-step are theirs) */
    float *next_obs, *reward;
    uint8_t *done, *constraint, *success, *ep_done;
    uint64_t* stats;         /* uint64[8] += {env_steps, episodes, num_viols, viol_and_recovery, viol_and_no_recovery,
                              * num_successes, recovery_steps, constraint_steps} */
    double* reward_sums;     /* double[2] += {sum of rewards, sum of finished-episode returns} */
    float* ep_reward;        /* [n]   in/out  running episode return */
    /* log_state != NULL: the per-episode log (rrl_episode_log_append) is advanced by this launch as well, from the values
     * the step holds in registers -- the same records and accumulator values as the stand-alone launch fed with this
     * step's per-env outputs, without writing those outputs.  The other log_* fields are then required. */
    int32_t* log_rec_i32;    /* rrl_episode_log_t.rec_i32 / rec_f64 / cap / state */
    double* log_rec_f64;
    int64_t log_cap;
    int64_t* log_state;
    int32_t* log_len;        /* per-env accumulators [n]: ep_len, ep_ret, ep_viol, ep_rec of rrl_episode_log_append */
    double* log_ret;
    int32_t *log_viol, *log_rec;
} rrl_step_push_t;
/* RRL_EINVAL / RRL_ERANGE before any launch when a required field is missing or a size is out of range; n == 0: RRL_OK. */
int rrl_nav_step_push_x(int env_kind, const rrl_step_push_t* a, void* stream);
int rrl_maze_step_push_x(const rrl_step_push_t* a, void* stream);

/* --------------------------------------------------------------------------------------------
 * CEM.  Replaces the bookkeeping of CEMOptimizer.obtain_solution (recovery_rl/optimizers.py:73-124)
 * for M independent planning problems (one per env that needs a recovery action); the cost
 * function in between stays with the caller (MPC._compile_cost, recovery_rl/MPC.py:374-416).
 *   mean, var [M,dim] f64 in/out; lb, ub [dim] f64; samples [M,pop,dim] f32; costs [M,pop] f32;
 *   active [M] u8.
 * rrl_cem_sample : active[m] = max(var[m]) > epsilon (the while-condition, :94; an env that went
 *                  inactive stays inactive if `sticky` != 0); for active envs
 *                  constrained_var = min(((mean-lb)/2)^2, ((ub-mean)/2)^2, var)   (:95-99)
 *                  samples = truncnorm(-2,2) * sqrt(constrained_var) + mean -> f32 (:100-102)
 * rrl_cem_update : for active envs: elites = the num_elites lowest-cost samples (NaN cost -> 1e6,
 *                  MPC.py:415; ties broken by sample index), mean <- alpha*mean + (1-alpha)*mean(elites),
 *                  var <- alpha*var + (1-alpha)*var(elites)                        (:111-117)
 * pop <= 1024, dim <= 64.  Missing pointers: RRL_EINVAL (active may be NULL for the update: every problem is updated);
 * sizes out of range, M * pop > 0xffffffff for the sample: RRL_ERANGE; then num_elites outside 1..pop: RRL_EINVAL;
 * M == 0: RRL_OK without a launch.  Each entry checks the fields it reads.
 * ------------------------------------------------------------------------------------------ */
typedef struct {             /* one CEM iteration's two launches on the same buffers */
    int64_t M;               /* planning problems; with m_dev: the launch bound the buffers are sized for */
    const int32_t* m_dev;    /* nullable: the live count M = m_dev[0] <= M, read by the kernels (rrl_cem_begin): same Philox
                              * rows, same bits as the host count; an empty set leaves counter_dev alone */
    int32_t pop, dim;
    double *mean, *var;
    const double *lb, *ub;
    double epsilon;
    int sticky;
    uint8_t* active;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    uint64_t counter_inc;
    float* samples;
    int32_t num_elites;      /* update only, like alpha and costs */
    double alpha;
    const float* costs;
} rrl_cem_t;
int rrl_cem_sample(const rrl_cem_t* c, void* stream);
int rrl_cem_update(const rrl_cem_t* c, void* stream);

/* A planning set whose size is decided ON THE DEVICE (no host round trip in MPC.act, recovery_rl/MPC.py:322-347; the
 * reference plans for its one env only when Q_risk > eps_safe, experiment.py:568-571): compaction in front of the CEM
 * iterations (which take count as rrl_cem_t.m_dev), scatter behind them.
 *   rrl_cem_begin   ONE launch: idx[0..count) = rows with mask != 0 in ascending order, count[0] = their number, and the
 *                   planner's inputs of the compacted problems: mean[j] = prev_sol[idx[j]] (prev_sol [n,dim] f64),
 *                   var[j] = init_var [dim], cur_obs[j] = obs[idx[j]] (f32 [n,2]), active[j] = 1      (MPC.py:336-341)
 *   rrl_cem_finish  action[i, 0..du) = float(mean[j, 0..du)) for i = idx[j], 0 for rows that did not plan;
 *                   prev_sol[i] = mean[j] shifted left by du, zero-filled                              (MPC.py:342-344)
 * Missing pointers of the fields an entry reads: RRL_EINVAL; n outside 1..2^31-1, dim outside 1..64, du outside 1..dim
 * (finish): RRL_ERANGE. */
typedef struct {
    int64_t n;
    const uint8_t* mask;
    int32_t dim, du;         /* du: finish only, like action */
    double* prev_sol;
    const double* init_var;  /* begin only, like obs, var, cur_obs, active */
    const float* obs;
    int32_t *idx, *count;
    double *mean, *var;
    float* cur_obs;
    uint8_t* active;
    float* action;
} rrl_cem_set_t;
int rrl_cem_begin(const rrl_cem_set_t* s, void* stream);
int rrl_cem_finish(const rrl_cem_set_t* s, void* stream);

/* --------------------------------------------------------------------------------------------
 * MLP building block.  Replaces the nn.Linear forward/backward of the SAC / Q_risk networks
 * (recovery_rl/model.py:49-76,172-199,295-343,489-530) for G heads in one launch; exact f32
 * (v_mfma_f32_32x32x2_f32), one wavefront per 32x32 output tile.  Row-major, leading dimensions
 * in elements, per-head strides s*.
 *   mode 0 (NT): C[g] = A[g] . B[g]^T (+ bias[g][n]) (relu)          A [M,K], B [N,K]
 *   mode 1 (NN): C[g] = A[g] . B[g]   (zeroed where mask[g] <= 0)    A [M,K], B [K,N], mask like C
 *   mode 2 (TN): C[g] = A[g]^T . B[g] ; colsum[g][m] = sum_k A[k][m] A [K,M], B [K,N]
 *   accumulate != 0: C += result.
 * ------------------------------------------------------------------------------------------ */
int rrl_gemm_f32(int mode, int G, int M, int N, int K, const float* A, int lda, long long sA,
                 const float* B, int ldb, long long sB, float* C, int ldc, long long sC,
                 const float* bias, long long sBias, int relu, const float* mask, int ldmask,
                 long long sMask, float* colsum, long long sColsum, int accumulate, void* stream);

/* Whole 2-hidden-layer stack forward in one launch (QNetwork / QNetworkConstraint heads,
 * GaussianPolicy / StochasticPolicy trunks + last linear; model.py:66-76,188-199,317-323,511-515):
 *   out[g] = W3[g] relu(W2[g] relu(W1[g] x + b1[g]) + b2[g]) + b3[g],  x [M,din] (leading dim ldx)
 * shared by the G heads.  W1 [G,H,din], W2 [G,H,H], W3 [G,dout,H]; h1/h2 [G,M,H] receive the hidden
 * activations when non-null (needed by the backward pass).  H % 16 == 0, H <= 256, din, dout <= 4.
 * scratch (nullable, f32 [4*G*M*dout]): when given and M <= 1024, H % 64 == 0 the hidden-2 columns are
 * split over 4 workgroups per row tile (small batches are bound by streaming W2 through one CU) and their
 * partial last-layer sums [4,G,M,dout] are either added in a fixed order by a second tiny kernel
 * (finalize != 0 -> out) or left in scratch for a consumer that sums them itself (finalize == 0). */
int rrl_mlp3_forward(int G, int M, int H, int din, int dout, const float* x, int ldx, const float* W1,
                     const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                     float* h1, float* h2, float* out, float* scratch, int finalize, void* stream);
/* number of partial sums (4) if rrl_mlp3_forward(M, H, scratch != NULL) takes the split path (so finalize == 0
 * leaves that many partials in scratch), 0 otherwise */
int rrl_mlp3_is_split(int M, int H);

/* Loss description of a stack backward (rrl_head_bwd_t.loss): where the last layer's backward takes dOut [G,B,dout], the
 * gradient w.r.t. the stack's output, from.
 *   kind = -1: `out` IS dOut, a plain contiguous tensor; no other field is read.
 *   kind >= 0: dOut is produced in the kernel from the operands named below instead of read from memory, which saves
 *              the stand-alone rrl_loss_dout launch in front of every stack backward (same formulas,
 *              bit-identical dOut).  kind selects the formula and the meaning of the fields:
 *   RRL_LOSS_SAC_CRITIC   (G=2,dout=1) out=q, out_t=qt, v0=logp2, v1=r, v2=m, v3=penalty (nullable), alpha,
 *                         f0=gamma; loss[2] = the two MSEs                              (sac.py:192-214)
 *   RRL_LOSS_SAC_POLICY   (G=2,dout=1) out=qp, v0=logp, alpha; loss[1]                  (sac.py:216-231)
 *   RRL_LOSS_QRISK_CRITIC (G=2,dout=1) out=z, out_t=zt, v0=c, v1=m, f0=gamma_safe; loss[2]   (qrisk.py:118-148)
 *   RRL_LOSS_QRISK_POLICY (G=2,dout=1) out=zp; loss[1]                                  (qrisk.py:150-154)
 *   RRL_LOSS_GAUSS_HEAD   (G=1,dout=4) out=head, v0=eps, v1=scale, f0=dlogp, d_action/ld/n_heads/head_stride
 *                         (the backward of GaussianPolicy.sample, model.py:324-340)
 *   RRL_LOSS_STOCH_HEAD   (G=1,dout=2) out=raw, v0=eps, v1=log_std, v2=scale, f0=min_log_std, d_action...;
 *                         loss[2] = dlog_std                                            (model.py:511-525)
 *   RRL_LOSS_DGD_QRISK    (G=2,dout=1) out=zp (Q_risk at (s, pi)), f0=nu; loss[1] = mean max sigmoid(zp): the Q_risk half of
 *                         the Lagrangian policy loss nu (max sigmoid(zp) - eps_safe) of --DGD_constraints (sac.py:221-228),
 *                         dOut = nu w_g / B q_g (1 - q_g) -- RRL_LOSS_QRISK_POLICY scaled by nu, a critic-loss kind
 *                         wherever those are accepted (the paired launch included)
 * out / out_t take (n_part, part_stride) like the stand-alone kernels: 1 <= n_part <= 4.  G and dout of the stack must be
 * the kind's (else RRL_EINVAL); an unknown kind, n_part, da_parts or da_group out of range: RRL_ERANGE. */
enum { RRL_LOSS_SAC_CRITIC = 0, RRL_LOSS_SAC_POLICY = 1, RRL_LOSS_QRISK_CRITIC = 2, RRL_LOSS_QRISK_POLICY = 3,
       RRL_LOSS_GAUSS_HEAD = 4, RRL_LOSS_STOCH_HEAD = 5, RRL_LOSS_DGD_QRISK = 6 };
typedef struct {
    int kind;
    int n_part;
    long long part_stride;
    const float *out, *out_t;
    const float *v0, *v1, *v2, *v3;
    const float* alpha;
    float f0;
    int ld, n_heads;
    long long head_stride;
    const float* d_action;
    float* loss;
    int da_parts;                /* 0/1: d_action is a plain tensor; k: the sum of k partials da_part_stride apart */
    long long da_part_stride;    /* (the dx_part of rrl_first_layer_t: k = H/16 <= 16, or H/64 when the producer folded) */
    int da_group;                /* 0/1: the partials are added one after the other; 4: they are column-TILE partials and every
                                  * four consecutive ones are summed first ((p0 + p1) + p2) + p3, then the group sums one
                                  * after the other -- the value a producer that folds (rrl_first_layer_t.dx_fold) stores */
} rrl_loss_t;

/* --------------------------------------------------------------------------------------------
 * Grouped launches.  One SAC / Q_risk update is a chain of ~40 tiny DEPENDENT kernels whose cost is the launch
 * boundary and a few memory round trips each, not their arithmetic; kernels that do not depend on each other
 * (the three critic forwards of sac.py:192-218 once both actions are sampled; the critic's backward for the
 * critic loss and for the policy loss; the task policy and the recovery policy of the acting pass) share ONE
 * launch here, so the chain is as long as its dependency depth.  Every member runs on its own workgroups: a launch of
 * n members gives the bits of n launches of one member each.  1 <= n <= 4.  The three stages of a stack backward exist as
 * descriptors only (one stack: n = 1); every descriptor is validated before anything is launched.
 *   rrl_mlp3_forward_multi        members = rrl_mlp3_forward calls; all members must take the same path (all with
 *                                 scratch on the split path -- partial sums stay in scratch, finalize = 0 -- or all
 *                                 on the same plain tiling), else RRL_EINVAL.  Split-path members of hidden width 256
 *                                 may differ in size (round 6: a 4096-row acting forward riding with an update's 256-row
 *                                 forwards): they then run on a flat grid of exactly the workgroups each member needs,
 *                                 every member on the tiles of its stand-alone launch -- list the large member first
 *   rrl_mlp_head_backward_multi   members = rrl_head_bwd_t: the last layer's backward of one stack each
 *   rrl_mlp_hidden_backward_multi members = rrl_hidden_bwd_t: the two H x H products of one stack each (+ its first layer)
 *   rrl_mlp_input_backward_multi  members = rrl_input_bwd_t: the first layer's backward of one stack each
 *   rrl_mlp_backward_pair_multi   = rrl_mlp_head_backward_multi(n, heads) followed by rrl_mlp_hidden_backward_multi(n, hidden),
 *                                 stack k's two stages linked by heads[k].dh2 == hidden[k].dh2.  When every member is a
 *                                 critic-loss kind (RRL_LOSS_SAC_CRITIC .. RRL_LOSS_QRISK_POLICY, one output) with full
 *                                 aligned tiles, both stages go out as ONE launch: the hidden-backward tiles derive dh2
 *                                 from the saved activation h2, the loss description and W3 themselves, and dh2 is then
 *                                 NOT written (it is scratch between the two stages, sac.py:216-239 / qrisk.py:150-182
 *                                 as autograd would hold it).  Anything else: the two launches.  Same gradients, bit for bit.
 * ------------------------------------------------------------------------------------------ */
/* use_in_head != 0 (din = 4, column-split path only): columns 2..3 of the stack's input are not read from x but computed
 * -- the action in_head yields for the same row (in_head.B is ignored: the stack's M rows) -- so the policy head needs no
 * launch of its own between the policy stack and the critic stack that consumes its action.  Columns 0..1 come from
 * in_head.obs_in (rows 2 floats apart) when given, else from x.  in_head.action / logp / obs_out, when non-null,
 * receive what the head as a launch of its own would have written (same formulas, same bits). */
typedef struct {
    int G, M, H, din, dout, ldx;
    const float *x, *W1, *b1, *W2, *b2, *W3, *b3;
    float *h1, *h2, *out, *scratch;
    rrl_policy_head_t in_head;
    int use_in_head;
    /* nullable (H = 256, column-split path): the same W2 a second time in MFMA fragment order (rrl_w2_pack; kept in step by
     * rrl_adam_step_multi through rrl_adam_seg_t.w2p).  A wave then fetches its 16 x 256 slice as 16 whole-KB loads instead of
     * 16 x 16 half-used 128-byte lines: -15 % on every forward launch (profiles/round5_fwd_packed/).  Same values, same bits. */
    const float* W2p;
} rrl_stack_t;
/* Last layer of a stack backward (one side 1..4 wide, so no MFMA tile), given dOut [G,B,dout] as `loss` describes it:
 *   dW3[g] = dOut[g]^T h2[g], db3[g] = sum_b dOut[g]      and      dh2[g] = [h2[g] > 0] (dOut[g] W3[g])
 * Limits: B <= 1024, dout <= 4 (RRL_ERANGE). */
typedef struct {
    rrl_loss_t loss;          /* loss.out required (RRL_EINVAL) */
    int G, B, H, dout;        /* heads, batch rows, hidden width, outputs per head */
    const float *h2, *W3;     /* required: h2 [G,B,H] the saved activation, W3 [G,dout,H] */
    float *dW3, *db3;         /* [G,dout,H], [G,dout]; nullable: no weight gradient unless both are given */
    float* dh2;               /* [G,B,H]; nullable: weight gradients and loss scalars only.  In rrl_mlp_backward_pair_multi it
                               * is the link to hidden[k].dh2 and is NOT written when the two stages go out as one launch */
} rrl_head_bwd_t;
/* First layer of the stack backward done by the hidden-layer launch itself (instead of an rrl_input_bwd_t in a
 * dependent launch): every 16 x 16 tile of dh1 = (dh2 W2) * [h1 > 0] also emits its share of
 *   dW1 = dh1^T x, db1 = column sums of dh1   -> first_part [B/16][first_stride]: row-tile t's partial of dW1[g][h][d] at
 *                                                 t*first_stride + (g*H + h)*din + d, of db1[g][h] at ... + G*H*din + g*H + h
 *                                                 (the layout of the head of a flat [W1 | b1 | ...] gradient buffer);
 *   dx  = dh1 W1                              -> dx_part [H/16][G][B][din]: column-tile partials; with dx_fold = 1
 *                                                 [H/64][G][B][din]: the sums ((p0 + p1) + p2) + p3 of four consecutive
 *                                                 column tiles, folded inside the workgroup that holds them (the paired
 *                                                 launches of rrl_mlp_backward_pair_multi and the block form of the packed
 *                                                 hidden backward; the one-tile-per-workgroup launches return RRL_ERANGE).
 * Consumers add the partials in a fixed order: rrl_adam_step_multi (g_part fields of the segment) and the policy-head
 * backward (da_parts / da_group of rrl_loss_t: 16 tile partials with da_group = 4 give the bits of 4 folded ones).
 * x = NULL: no first-layer work (then dh1 must be given).  With x: W1 and one of first_part / dx_part required, din <= 4
 * (RRL_EINVAL); B, H % 128 == 0 and 16-byte aligned dh2, h1, W2 (RRL_ERANGE). */
typedef struct {
    const float *x, *W1;
    int ldx, din;
    float* first_part;
    long long first_stride;
    float* dx_part;
    int dx_fold;
} rrl_first_layer_t;
/* Hidden layer of a stack backward: both products read dh2 and are independent, one launch on the MFMA tiles
 *   dW2[g] = dh2[g]^T h1[g], db2[g] = column sums of dh2[g]      and      dh1[g] = (dh2[g] W2[g]) * [h1[g] > 0]
 * Any B, H (ragged tiles are bounds-checked); G <= 65535. */
typedef struct {
    int G, B, H;
    const float *dh2, *h1, *W2;   /* required: dh2, h1 [G,B,H]; W2 [G,H,H] */
    float *dW2, *db2;             /* [G,H,H], [G,H]; both or neither (RRL_EINVAL); both NULL: the input gradient dh1 only */
    float* dh1;                   /* [G,B,H]; nullable when `first` consumes it, else required (RRL_EINVAL) */
    rrl_first_layer_t first;
} rrl_hidden_bwd_t;
/* First layer of a stack backward as a launch of its own (one side 1..4 wide), dh1 [G,B,H] already masked by relu':
 *   dW1[g] = dh1[g]^T x, db1[g] = sum_b dh1[g]      and      dx[g] = dh1[g] W1[g]
 * din <= 4 (RRL_ERANGE). */
typedef struct {
    int G, B, H, din, ldx;        /* ldx: floats between rows of x */
    const float *dh1, *x, *W1;    /* required: x [B,din] shared by the heads, W1 [G,H,din] */
    float *dW1, *db1;             /* [G,H,din], [G,H]; nullable: no weight gradient unless both are given */
    float* dx;                    /* [G,B,din]; nullable: no input gradient.  Neither wanted: the member is skipped */
} rrl_input_bwd_t;
int rrl_mlp3_forward_multi(int n, const rrl_stack_t* stacks, void* stream);
/* ONE column-split stack (H = 256) with rider workgroups in front of its tiles: launches that nothing in this launch waits
 * for, each the body of the launch it replaces on a workgroup of its own (batches of at most 256 rows).  All optional:
 *   select   the select half of a draw (rrl_draw_ahead_t)
 *   gather   the gather half for keys selected ahead; the stack must be the 2B-row forward over the batch's s' (rows
 *            [0, B)) and s (rows [B, 2B)), din = 2: its rows are then read from the ring through the keys instead of from
 *            `x` -- the values the gather writes -- so the forward does not wait for the gather
 *   second   a whole draw (any mode), as rrl_sample_multi's member
 *   noise_*  the noise fill of rrl_sample_multi
 * Outputs equal the separate launches' bit for bit. */
typedef struct {
    const rrl_draw_ahead_t* select;
    const rrl_draw_ahead_t* gather;
    const rrl_draw_t* second;
    long long noise_pairs;
    uint64_t noise_seed, noise_counter;
    uint64_t* noise_counter_dev;
    uint64_t noise_counter_inc;
    float* noise_out;
} rrl_fwd_riders_t;
int rrl_mlp3_forward_riders(const rrl_stack_t* stack, const rrl_fwd_riders_t* riders, void* stream);
int rrl_mlp_head_backward_multi(int n, const rrl_head_bwd_t* members, void* stream);
int rrl_mlp_hidden_backward_multi(int n, const rrl_hidden_bwd_t* members, void* stream);
int rrl_mlp_input_backward_multi(int n, const rrl_input_bwd_t* members, void* stream);
int rrl_mlp_backward_pair_multi(int n, const rrl_head_bwd_t* heads, const rrl_hidden_bwd_t* hidden, void* stream);

/* --------------------------------------------------------------------------------------------
 * Fused element-wise pieces of the updates (one launch each instead of a chain of PyTorch ops).
 *   rrl_policy_heads_fwd_multi  1 <= n <= 4 policy heads (rrl_policy_head_t, either kind) that do not depend on each
 *                            other in ONE launch: a' = pi(s') and pi(s) of one SAC step (sac.py:192-218), the task action
 *                            and the recovery action of the acting pass (experiment.py:546-577).  Every member is validated
 *                            before anything is launched and runs on its own workgroups
 *   rrl_loss_dout            dOut [G,B,dout] of the loss `loss` describes (rrl_loss_t: the formulas and the operand fields of
 *                            the seven kinds), by the stand-alone kernel of its kind -- the launch a loss description in
 *                            rrl_head_bwd_t saves, and the reference its fused form is compared against.  RRL_EINVAL: an
 *                            operand of the kind missing, B <= 0, n_part outside 1..4, n_heads <= 0 or da_parts > 1 (the
 *                            stand-alone head kernels read a plain d_action) for the head kinds, kind == -1 (nothing to
 *                            compute); an unknown kind: RRL_ERANGE
 *   rrl_rcpo_penalty         penalty[b] = lambda[0] max sigmoid(z[.][b]) for RRL_LOSS_SAC_CRITIC's `penalty` (--RCPO,
 *                            sac.py:202-205; lambda read from device memory) and mean[0] = the batch mean of max sigmoid(z)
 *                            (penalty = NULL: the mean only -- the nu step of --update_nu at (s, pi))
 *   rrl_recovery_select      recovery gate max sigmoid(z) > eps_safe and action select
 *                            (recovery_rl/experiment.py:546-577)
 * Operands that are stack outputs (rrl_loss_t.out / out_t, the penalty's z) take (n_part, part_stride): the value of
 * element i is p[i] + p[part_stride + i] + ... (n_part terms, fixed order) -- the partial last-layer sums of
 * rrl_mlp3_forward(scratch, finalize = 0); n_part = 1 for a plain tensor.
 * ------------------------------------------------------------------------------------------ */
int rrl_loss_dout(const rrl_loss_t* loss, int B, float* dout, void* stream);
/* The arguments of rrl_rcpo_penalty (one seed's in rrl_rcpo_penalty_packed: same meaning, same checks). */
typedef struct {
    int B;
    const float* z;
    int n_part;
    long long part_stride;
    const float* lambda;  /* read from device memory by the kernel: the dual step of the same iteration writes it */
    float* penalty;       /* nullable: the mean only */
    float* mean;
} rrl_penalty_args_t;
int rrl_rcpo_penalty(const rrl_penalty_args_t* a, void* stream);
int rrl_policy_heads_fwd_multi(int n, const rrl_policy_head_t* heads, void* stream);
/* The optimiser step: torch.optim.Adam over up to RRL_ADAM_MAX_SEGS flat f32 buffers in one launch (e.g. critic + policy
 * of one update; lr, betas and eps of the launch), every segment with its own step counter and optional Polyak target.
 * Per element, with t = step_dev[0] + 1 and the bias corrections 1 - beta^t evaluated in double:
 *   m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;  p <- p - lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   target <- (1 - tau) target + tau p     (soft_update, recovery_rl/utils.py:46-49, on the UPDATED p; target = NULL: none)
 * and the segment's last workgroup stores t. */
#define RRL_ADAM_MAX_SEGS 12
typedef struct {
    long long n;          /* elements, > 0 */
    float* p;             /* required, like g, m (exp_avg), v (exp_avg_sq): n floats each */
    const float* g;
    float* m;
    float* v;
    uint64_t* step_dev;   /* required: uint64[2] {t, ticket}; t is incremented by the kernel, the ticket is left at 0 */
    float* target;        /* nullable: Polyak target, n floats */
    float tau;
    float weight_decay;   /* g <- g + weight_decay * p before the moment updates (torch.optim.Adam weight_decay) */
    const float* g2;      /* nullable: second partial gradient, g <- g + g2 (rrl_ens_train_grad) */
    const float* g_part;  /* nullable: the first part_elems gradients are the sum of n_part partials part_stride apart */
    int n_part;           /* (first_part of rrl_first_layer_t; added in a fixed order; 1 <= n_part <= 64, 0 < part_elems <= n,
                           * part_elems % 4 == 0, part_stride % 4 == 0, g_part 16-byte aligned: else RRL_EINVAL) */
    long long part_stride, part_elems;
    /* nullable: fragment-order copies (rrl_w2_pack layout, hidden width 256) of the w2_heads [256, 256] matrices that start at
     * element w2_off of p (w2_off % 4 == 0, 16-byte aligned pointers): every updated parameter of that range is stored there
     * too -- and the Polyak target's into target_w2p -- so that the forward kernels' rrl_stack_t.W2p stays current.  A captured
     * iteration re-makes nothing between its launches: this is the only step that keeps the copies of a replayed forward current */
    float* w2p;
    float* target_w2p;
    long long w2_off;
    int w2_heads;
} rrl_adam_seg_t;
int rrl_adam_step_multi(int n_seg, const rrl_adam_seg_t* segs, float lr, float beta1, float beta2, float eps,
                        void* stream);
/* The dual variables of the comparison algorithms (sac.py:256-271: log_nu of --update_nu, log_lambda of --RCPO) as members
 * of the same launch: one torch.optim.Adam step (capturable; beta1, beta2, eps of the launch, lr of the member) of the 0-dim
 * parameter log_p on the optimiser's own state tensors, gradient eps_safe - stat[0] (stat = the batch mean of max sigmoid(z)),
 * then value[0] = exp(log_p) (SAC._set_dual).  log_p = NULL: no step.  loss_out (nullable): loss_out[0] = loss_in[0] +
 * f_loss (stat[0] - eps_safe) -- the Lagrangian policy loss statistic of --DGD_constraints from its two halves, read from
 * stat BEFORE anything of the launch writes.  n_dual <= RRL_ADAM_MAX_DUALS; n_seg may be 0. */
#define RRL_ADAM_MAX_DUALS 4
typedef struct {
    float *log_p, *exp_avg, *exp_avg_sq, *step;
    float* value;
    const float* stat;
    float eps_safe;
    float lr;
    const float* loss_in;
    float* loss_out;
    float f_loss;
} rrl_dual_t;
int rrl_adam_step_multi_duals(int n_seg, const rrl_adam_seg_t* segs, int n_dual, const rrl_dual_t* duals, float lr,
                              float beta1, float beta2, float eps, void* stream);
/* W2p = the G row-major [H, H] matrices W2 (out, in -- model.py's nn.Linear weights) in the order the forward kernels' MFMA B
 * operands consume them: W2p[g][n][j][q][i][c] = W2[g][16 n + i][16 j + 4 q + c] (n, j < H / 16; q, c < 4; i < 16), i.e. the float4
 * lane (i, q) of the wave that owns output columns 16 n .. 16 n + 15 needs for K chunk j sits at float4 index
 * (n H / 16 + j) 64 + 16 q + i.  H % 16 == 0.  Pure permutation: layout only. */
int rrl_w2_pack(int G, int H, const float* W2, float* W2p, void* stream);
/* out[2i], out[2i+1] = N(0,1) pair i of Philox stream RRL_STREAM_NOISE at counter (+ device tick): replaces
 * torch.randn for the policy noise of recovery_rl/model.py:324-340,511-525 (x_t = mean + std * eps). */
int rrl_normal_fill(long long n_pairs, uint64_t seed, uint64_t counter, uint64_t* counter_dev, uint64_t counter_inc,
                    float* out, void* stream);
int rrl_recovery_select(int N, const float* z, float eps_safe, const float* task_action, int ld_task,
                        const float* rec_action, float* real_action, uint8_t* recovery, float* task_out,
                        void* stream);

/* --------------------------------------------------------------------------------------------
 * Episode log.  The reference appends one info dict per env-step to run_stats.pkl and rewrites the whole
 * file after every episode (recovery_rl/experiment.py:421,456-461,540-543, dump_logs :540-543); its plotting
 * code reduces them per episode to: length, sum of rewards, last reward, any(constraint)
 * (plotting/plot_runs.py:194-235).  This entry keeps exactly those per-episode quantities on the device:
 * per-env accumulators (ep_len i32[n], ep_ret f64[n] summed in step order, ep_viol i32[n], ep_rec i32[n]) are
 * advanced every step, and where ep_done[i] != 0 one record is appended and the accumulators are cleared.
 *   rec_i32 [cap, RRL_EPLOG_I32] = {env, iteration, length, constraint steps, recovery steps,
 *                                   flags (1 = success, 2 = constraint, 4 = recovery, all of the LAST step)}
 *   rec_f64 [cap, 2]             = {episode return, last reward}
 *   state   int64[3]             = {count, iteration, ticket}; count keeps growing past cap (overflow is
 *                                  visible to the host; records beyond cap are dropped), iteration is
 *                                  incremented by the kernel (hipGraph replay safe).
 * Records land in completion order; (iteration, env) is unique, hosts sort by it.
 * ------------------------------------------------------------------------------------------ */
#define RRL_EPLOG_I32 6
typedef struct {
    int32_t* rec_i32;
    double* rec_f64;
    int64_t cap;
    int64_t* state;
} rrl_episode_log_t;

int rrl_episode_log_append(int64_t n, const float* reward, const uint8_t* constraint, const uint8_t* success,
                           const uint8_t* ep_done, const uint8_t* recovery, int32_t* ep_len, double* ep_ret,
                           int32_t* ep_viol, int32_t* ep_rec, const rrl_episode_log_t* log, void* stream);

/* --------------------------------------------------------------------------------------------
 * Planner candidate evaluation.  Replaces MPC._compile_cost (recovery_rl/MPC.py:374-416) with
 * _predict_next_obs (:421-439), the ensemble forward (config/navigation1.py:71-96) and
 * QRiskWrapper.get_value (recovery_rl/qrisk.py:184-196) for M planning problems at once:
 *   costs[m, c] = mean over npart particles of sum_{t < plan_hor} max(Q_risk1, Q_risk2)(obs_t, ac_seqs[m, c, t]),
 *   obs_{t+1} = obs_t + mean_e(obs_t, ac_t) + z * sqrt(var_e(obs_t, ac_t)),  particle p uses member p / (npart / n_nets),
 * NaN particle costs -> 1e6.  One MFMA kernel; activations never leave the chip.
 *   rrl_plan_pack      re-packs the live weights into MFMA fragment order (call after every change of the
 *                      safety critic or the ensemble).  Q_risk tensors are the stacked twin heads W1 [2,hq,4],
 *                      b1 [2,hq], W2 [2,hq,hq], b2 [2,hq], W3 [2,1,hq], b3 [2,1] (nn.Linear layout, out x in);
 *                      ensemble tensors are lin0_w [E,4,he], lin0_b [E,1,he], lin1_w/lin2_w [E,he,he],
 *                      lin3_w [E,he,4], lin3_b [E,1,4] (in x out), inputs_mu/sigma [4], max/min_logvar [2].
 *   rrl_plan_cost      cur_obs [M,2], ac_seqs [M,pop,plan_hor*2] f32; noise nullable f32 [plan_hor, M*pop*npart, 2]
 *                      (row = (m*pop + c)*npart + p); when NULL the kernel draws Philox normals (stream
 *                      RRL_STREAM_PLAN, row, counter*16 + t).  scratch: f32 [rrl_plan_scratch_floats(n_nets, M, pop)]
 *                      (first-step values per candidate / per (candidate, member) + per-member cost sums); costs [M,pop].
 *                      Two launches + the finish: the first step once per DISTINCT row (the particles of a candidate share
 *                      (cur_obs, ac_0): MPC.py:393-402), then steps 1..plan_hor-1 per particle without the last step's
 *                      unread prediction (MPC.py:406-412) -- bit-identical to the literal loop, 74.9 % of its FLOPs.
 * Supported shape (rrl_plan_supported): hq = 256, he = 200, npart = 4 n_nets, 2-D obs and actions.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int hq, he, n_nets;
    const float *q_w1, *q_b1, *q_w2, *q_b2, *q_w3, *q_b3;
    const float *e_w0, *e_b0, *e_w1, *e_b1, *e_w2, *e_b2, *e_w3, *e_b3;
    const float *inputs_mu, *inputs_sigma, *max_logvar, *min_logvar;
} rrl_plan_weights_t;

int rrl_plan_supported(int hq, int he, int n_nets, int npart, int d_obs, int d_act);
long long rrl_plan_pack_floats(int hq, int he, int n_nets);
long long rrl_plan_scratch_floats(int n_nets, long long M, int pop);     /* M * pop * (5 n_nets + 1) */
/* f16x3 != 0 (opt-in): the three hidden-layer products (Q_risk 256 x 256, ensemble 200 x 200 twice) run on the f16 matrix
 * pipe: every f32 activation and weight is split as hi + lo (two f16 carrying 22 bits of the value) and the product is
 * hi*hi + hi*lo + lo*hi with f32 accumulation -- one v_mfma_f32_16x16x16_f16 (16 cycles) three times instead of four
 * v_mfma_f32_16x16x4_f32 (32 cycles each) per 16-wide k chunk.  Input layers, biases, activations, epilogues and the
 * rollout state stay f32.  The packed buffer has the same size for both but is NOT interchangeable.  Results agree with
 * the f32 kernels to ~1e-6 relative (tests: the same 2e-4 bound as the f32 kernel against the PyTorch path); values
 * beyond +-65504 in a hidden layer saturate. */
int rrl_plan_pack(const rrl_plan_weights_t* w, int f16x3, float* packed, void* stream);
typedef struct {
    const float* packed;
    int hq, he, n_nets, npart;
    int f16x3;               /* 0: f32 MFMA kernels, else the hi/lo f16 ones (packed by rrl_plan_pack with the same flag) */
    long long M;             /* planning problems; with m_dev: the launch bound the buffers are sized for */
    const int32_t* m_dev;    /* nullable: the live count M = m_dev[0], read by the kernels (rrl_cem_begin); workgroups past
                              * the live problems exit at once, results for the live ones equal the host count's bit for bit */
    int pop, plan_hor;
    const float *cur_obs, *ac_seqs, *noise;
    uint64_t seed, counter;
    uint64_t* counter_dev;
    uint64_t counter_inc;
    float *scratch, *costs;
} rrl_plan_cost_t;
/* Every failed check is RRL_EINVAL, before anything is launched. */
int rrl_plan_cost(const rrl_plan_cost_t* a, void* stream);

/* --------------------------------------------------------------------------------------------
 * Ensemble fitting.  One optimiser step of MPC.train (recovery_rl/MPC.py:266-292) for the PETS ensemble
 * (PtModel, config/navigation1.py:23-96): gather of the bootstrap rows idx[e, 0..batch), forward, loss
 *   sum_e mean((mean_e - y)^2 exp(-logvar_e) + logvar_e) + 0.01 (sum max_logvar - sum min_logvar) + decays (:52-59)
 * and its gradient w.r.t. every parameter EXCEPT the decay terms (pass them as the segments' weight_decay:
 * 0.00025 / 0.0005 / 0.0005 / 0.00075 for w0..w3) in ONE launch (+ a 4-thread reduction for the shared logvar bounds);
 * the update itself is rrl_adam_step_multi over the same buffers (torch.optim.Adam, lr 1e-3).
 *   parameters  w0 [E,4,H] b0 [E,1,H] w1,w2 [E,H,H] b1,b2 [E,1,H] w3 [E,H,4] b3 [E,1,4] (in x out), max/min_logvar [2],
 *               mu/sigma [4] (input standardisation, not trained); g_* = gradients, same shapes;
 *               g_logvar_part: scratch [2E,4].  A member's 32 rows are processed by two workgroups of 16 rows:
 *               rows 0..15 write g_*, rows 16..31 write g2_* (same shapes); pass g2 as the Adam segment's second
 *               gradient so that the update uses g + g2
 *   idx         int64 [E, >= batch] with row stride idx_stride (elements): rows of train_in [N,4] / train_targ [N,2]
 *   scratch     float [rrl_ens_scratch_floats(E)]; loss_out (nullable) [E] = the per-net NLL term
 * Supported shape (rrl_ens_train_supported): 4 inputs, H = 200, 4 outputs, batch 1..32 (the mean runs over the
 * real rows, as for the shorter last batch of an epoch).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int n_nets, d_in, hidden, d_out;
    float *w0, *b0, *w1, *b1, *w2, *b2, *w3, *b3, *max_logvar, *min_logvar;
    const float *mu, *sigma;
    float *g_w0, *g_b0, *g_w1, *g_b1, *g_w2, *g_b2, *g_w3, *g_b3, *g_max_logvar, *g_min_logvar, *g_logvar_part;
    float *g2_w0, *g2_b0, *g2_w1, *g2_b1, *g2_w2, *g2_b2, *g2_w3, *g2_b3;   /* second half of the batch (see above) */
    float* loss_part;                                                       /* scratch [2 E] */
} rrl_ens_t;
int rrl_ens_train_supported(int d_in, int hidden, int d_out, int batch);
long long rrl_ens_scratch_floats(int n_nets);
/* one epoch = ceil(n_rows / batch) steps {rrl_ens_train_grad on idx[:, lo:lo+batch], rrl_adam_step_multi(segs)} issued
 * from C (the batch loop of MPC.py:266-292); segs = the Adam segments of the ten parameter tensors */
int rrl_ens_train_epoch(const rrl_ens_t* m, int n_seg, const rrl_adam_seg_t* segs, float lr, float beta1, float beta2,
                        float eps, const float* train_in, const float* train_targ, const int64_t* idx,
                        long long idx_stride, long long n_rows, int batch, float* scratch, float* loss_out,
                        void* stream);
int rrl_ens_train_grad(const rrl_ens_t* m, int batch, const float* train_in, const float* train_targ,
                       const int64_t* idx, long long idx_stride, float* scratch, float* loss_out, void* stream);

/* The same optimiser step at LARGE batch (the lock-step loop's online re-fit trains on 32 x num_envs rows per member per
 * step, experiment.py:464-480 scaled by the number of envs; any batch >= 1 is accepted): same loss, same gradients
 * (to f32 summation order), same rrl_ens_t, gradients land in g_* only (g2_*, g_logvar_part, loss_part are not used: pass
 * Adam segments without g2).  Three launches: forward + backward per 64-row tile with the activations in LDS (f32 MFMA),
 * split-K weight-gradient products, fixed-order reduction of the partials (deterministic).
 *   scratch     float [rrl_ens_big_scratch_floats(E, batch)]  (6 activation-sized buffers [E][ceil64(batch)][200] + partials)
 *   idx         int64, member e's rows at idx[e * idx_stride + 0 .. batch) */
int rrl_ens_train_big_supported(int d_in, int hidden, int d_out);
long long rrl_ens_big_scratch_floats(int n_nets, long long batch);
int rrl_ens_train_grad_big(const rrl_ens_t* m, long long batch, const float* train_in, const float* train_targ,
                           const int64_t* idx, long long idx_stride, float* scratch, float* loss_out, void* stream);
int rrl_ens_train_epoch_big(const rrl_ens_t* m, int n_seg, const rrl_adam_seg_t* segs, float lr, float beta1, float beta2,
                            float eps, const float* train_in, const float* train_targ, const int64_t* idx,
                            long long idx_stride, long long n_rows, long long batch, float* scratch, float* loss_out,
                            void* stream);

/* --------------------------------------------------------------------------------------------
 * Packed launches: S independent learners ("seeds" -- own envs, replay rings, networks, Philox keys; the reference's unit
 * of parallelism is the seed loop, scripts/navigation1.sh:4-8) share every launch of the lock-step iteration.  Each entry is
 * its stand-alone counterpart for S argument sets at once: seed s runs exactly the stand-alone code on its own workgroups,
 * so every seed's results equal its solo run bit for bit.  The S argument blocks live in device memory (content-addressed
 * cache inside the library: blocks that do not change from call to call are uploaded once).  S <= 16.
 * Launch structure (round 5): as in the solo group launches the member of a seed's group is blockIdx.y, and the seed follows
 * from blockIdx.x by arithmetic (XCD-aware placement), so a workgroup's argument block arrives in one batch of scalar loads.
 *   rrl_sample_multi_packed                rrl_sample_multi            (args[s])
 *   rrl_mlp3_forward_multi_packed          rrl_mlp3_forward_multi      (n[s] stacks members[s][0..n[s]); column-split path)
 *   rrl_mlp_head_backward_multi_packed     rrl_mlp_head_backward_multi
 *   rrl_mlp_hidden_backward_multi_packed   rrl_mlp_hidden_backward_multi
 *   rrl_mlp_backward_pair_multi_packed     rrl_mlp_backward_pair_multi (heads[s], hidden[s]: one launch when every member of
 *                                          every seed qualifies for the paired form, the two packed launches otherwise)
 *   rrl_adam_step_multi_packed             rrl_adam_step_multi         (lr[s])
 *   rrl_nav_step_push_packed / rrl_maze_step_push_packed    rrl_*_step_push_x (a[s]; one env kind, sizes on one side of 16384)
 * The launches of the comparison algorithms' iterations (LR, RSPO, RCPO, SAC without a recovery policy) that the list above
 * does not cover:
 *   rrl_adam_step_multi_duals_packed       rrl_adam_step_multi_duals   (n_seg[s] may be 0, 1 <= n_dual[s] <= RRL_ADAM_MAX_DUALS;
 *                                          a kernel of its own: seed s's dual row is its row n_seg[s], as in the solo launch)
 *   rrl_rcpo_penalty_packed                rrl_rcpo_penalty            (args[s]; one workgroup per seed; seeds may differ in
 *                                          penalty == NULL, i.e. the mean-only form)
 *   rrl_policy_heads_fwd_multi_packed      rrl_policy_heads_fwd_multi  (n[s] heads heads[s][0..n[s]), either kind; flat grid
 *                                          over (seed, member, row block))
 * SQRL's constraint-sampling acting pass (declared with its descriptor below):
 *   rrl_sqrl_act_packed                    rrl_sqrl_act                (args[s]: seed s's stand-alone descriptor; n[s] workgroups
 *                                          per seed, its tick advanced by the last of them; ONE k for all seeds of a call --
 *                                          the row tiles ceil(k / 16) are a template parameter of the kernel -- else RRL_EINVAL;
 *                                          n, weights, eps_safe, seed, tick, n_part, injected draws and the diagnostics that are
 *                                          asked for may differ by seed)
 *   rrl_sqrl_act_f16x3_packed              rrl_sqrl_act_f16x3          (the same rules on the f16x3 kernels; every seed's W2p is its
 *                                          rrl_w2_pack_f16x3 stream)
 * The Q-sampling recovery acting call (declared with its descriptors below):
 *   rrl_qsample_act_packed                 rrl_qsample_act / rrl_qsample_act_gated   (args[s], gates[s] or gates == NULL; the
 *                                          score kernel gives seed s its n[s] ceil(k[s] / 128) workgroups, the fold kernel one
 *                                          thread per env; the tick of seed s is advanced by the fold thread of ITS env 0; the
 *                                          chunk count is not a template parameter, so k may differ by seed, as may n, weights,
 *                                          eps_safe, seed, tick, injected candidates and the diagnostics that are asked for)
 *   rrl_qsample_act_f16x3_packed           rrl_qsample_act_f16x3 / rrl_qsample_act_gated_f16x3   (the same rules on the f16x3 score
 *                                          kernels; every seed's W2p is its rrl_w2_pack_f16x3 stream)
 * The evaluation rollout (declared with its descriptor below; outside the iteration, at the seeds' evaluation points):
 *   rrl_eval_rollout_packed                rrl_eval_rollout            (args[s]; seed s gets its ceil(n[s] / 16) workgroups and
 *                                          its tick is advanced by the last of them; n, T, env kind, weights, groups, seed, tick
 *                                          and traces may differ by seed)
 *   rrl_eval_rollout_maze_packed           rrl_eval_rollout_maze       (args[s], horizon[s]; the same mapping on the Maze kernel)
 *   rrl_eval_rollout_qs_packed             rrl_eval_rollout_qs         (args[s]; the same mapping on the Q-sampling kernels; n, T,
 *                                          k, env seed, tick, weights, box and traces may differ by seed, and the kind within
 *                                          Navigation or the horizon within Maze; Navigation and Maze seeds in one call:
 *                                          RRL_EINVAL)
 *   rrl_eval_rollout_sqrl_packed           rrl_eval_rollout_sqrl       (args[s]; the same mapping on the SQRL kernels; n, T, k,
 *                                          env seed, tick, reset, weights and traces may differ by seed, and the kind within
 *                                          Navigation or the horizon within Maze; a Navigation + Maze mix: RRL_EINVAL)
 *   rrl_eval_rollout_qs_f16x3_packed       rrl_eval_rollout_qs_f16x3   (args[s], qW2h[s]; the rules of rrl_eval_rollout_qs_packed
 *                                          on the f16x3 kernels; the streams are part of the plan key)
 *   rrl_eval_rollout_sqrl_f16x3_packed     rrl_eval_rollout_sqrl_f16x3 (args[s], qW2h[s]; the rules of
 *                                          rrl_eval_rollout_sqrl_packed on the f16x3 kernels)
 * Every seed's arguments are checked before anything is stored or launched (the stand-alone entry's codes); a NULL array:
 * RRL_EINVAL; S outside 1 .. 16: RRL_EINVAL, except from rrl_eval_rollout[_maze|_qs|_sqrl][_f16x3]_packed, which return RRL_ERANGE
 * for it.
 * S == 1 is the stand-alone launch.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const rrl_draw_t *first, *second;
    long long noise_pairs;
    uint64_t noise_seed, noise_counter;
    uint64_t* noise_counter_dev;
    uint64_t noise_counter_inc;
    float* noise_out;
} rrl_sample_args_t;
int rrl_sample_multi_packed(int S, const rrl_sample_args_t* args, void* stream);
/* Free the cached argument blocks of every packed launch (host and device copies); returns their number.  Call only when no
 * captured graph that contains a packed launch is alive (the graphs hold the blocks' device addresses as kernel arguments). */
int rrl_pack_clear(void);
int rrl_mlp3_forward_multi_packed(int S, const int* n, const rrl_stack_t* const* members, void* stream);
int rrl_mlp_head_backward_multi_packed(int S, const int* n, const rrl_head_bwd_t* const* members, void* stream);
int rrl_mlp_hidden_backward_multi_packed(int S, const int* n, const rrl_hidden_bwd_t* const* members, void* stream);
int rrl_mlp_backward_pair_multi_packed(int S, const int* n, const rrl_head_bwd_t* const* heads,
                                       const rrl_hidden_bwd_t* const* hidden, void* stream);
int rrl_adam_step_multi_packed(int S, const int* n_seg, const rrl_adam_seg_t* const* segs, const float* lr, float beta1,
                               float beta2, float eps, void* stream);
int rrl_nav_step_push_packed(int S, int env_kind, const rrl_step_push_t* a, void* stream);
int rrl_maze_step_push_packed(int S, const rrl_step_push_t* a, void* stream);
int rrl_adam_step_multi_duals_packed(int S, const int* n_seg, const rrl_adam_seg_t* const* segs, const int* n_dual,
                                     const rrl_dual_t* const* duals, const float* lr, float beta1, float beta2, float eps,
                                     void* stream);
int rrl_rcpo_penalty_packed(int S, const rrl_penalty_args_t* args, void* stream);
int rrl_policy_heads_fwd_multi_packed(int S, const int* n, const rrl_policy_head_t* const* heads, void* stream);

/* --------------------------------------------------------------------------------------------
 * SQRL constraint-sampling acting.  Replaces SAC.select_action with --use_constraint_sampling (recovery_rl/sac.py:139-161)
 * for n envs at once: per env e, k candidate actions of the task policy, the twin Q_risk on each, one pick.  One MFMA
 * kernel, one workgroup per env; nothing but action[n, 2] (and the diagnostics that are asked for) leaves the chip.
 *   candidate  eps[e, c] = the normal pair of Philox (seed, row e k + c, RRL_STREAM_SQRL, counter + tick) rounded to f32
 *              (as rrl_normal_fill rounds), or eps_in[e, c];  a[e, c], logp[e, c] = the tanh-Gaussian head on
 *              head[e] = (mean0, mean1, log_std0, log_std1) -- RRL_HEAD_GAUSS of rrl_policy_head_t, same arithmetic
 *   score      z_h = head h of Q_risk (4 -> 256 relu -> 256 relu -> 1) on [obs_e | a_ec], exact-f32 MFMA;
 *              q = max(sigmoid z_0, sigmoid z_1) (NaN propagates); safe = q <= eps_safe
 *   pick       no safe candidate: argmin q (lowest index on ties).  Otherwise u = the open-unit double of the low 64 bits
 *              of Philox (seed, row e, RRL_STREAM_SQRL_PICK, counter + tick), or u_in[e]; weights in double
 *              w_c = safe ? exp(logp_c - max safe logp) : 0, T = their sum in ascending c, c* = the first safe c whose
 *              running sum exceeds u T (none: the last safe c); pick = (safe candidates with index <= c*) - 1 -- the
 *              position in the SAFE list applied to the FULL list, as the reference does (sac.py:157-158).
 *   action[e] = a[e, pick]
 * Weights: the stacked twin heads W1 [2,256,4], b1 [2,256], b2 [2,256], W3 [2,1,256], b3 [2,1] (nn.Linear layout) and W2 as
 * its fragment-order copy W2p (rrl_w2_pack, 16-byte aligned).
 * Checks before any launch: a required pointer NULL, n <= 0, H != 256, d_obs or d_act != 2, n_part outside 1..4,
 * misaligned W2p: RRL_EINVAL; k outside 1..128 or n k >= 2^32: RRL_ERANGE.
 * rrl_sqrl_scratch_floats(n, k): floats of `scratch` this form of the kernel needs (0: the candidates' q, logp and actions stay
 * in LDS; `scratch` may be NULL); the same range checks.
 * ------------------------------------------------------------------------------------------ */
enum { RRL_STREAM_SQRL = 9,       /* SQRL candidate noise           */
       RRL_STREAM_SQRL_PICK = 10  /* SQRL categorical draw          */ };
typedef struct {
    int n, k;                     /* envs, candidates per env */
    int H, d_obs, d_act;          /* 256, 2, 2 */
    const float* obs;             /* [n, 2] */
    const float* head;            /* [n, 4] last-layer output of the task policy, as n_part partial sums part_stride floats */
    int n_part;                   /* apart (added in the fixed order ((p0 + p1) + p2) + p3) */
    long long part_stride;
    const float *scale, *bias;    /* [2] action scale / bias */
    const float *W1, *b1, *W2p, *b2, *W3, *b3;
    float eps_safe;
    uint64_t seed, counter;
    uint64_t* counter_dev;        /* nullable {tick, ticket}: tick read by every workgroup, += counter_inc by the last one */
    uint64_t counter_inc;
    const float* eps_in;          /* nullable [n, k, 2]: replaces the candidate noise */
    const double* u_in;           /* nullable [n]: replaces the pick's uniform */
    float* scratch;               /* [rrl_sqrl_scratch_floats(n, k)]; nullable when that is 0 */
    float* action;                /* [n, 2] */
    float *q, *logp, *cand, *z;   /* nullable diagnostics: [n, k], [n, k], [n, k, 2], [2, n, k] (pre-activations) */
    int32_t *pick, *cstar, *n_safe;   /* nullable diagnostics [n]; cstar = -1 on the argmin branch */
} rrl_sqrl_act_t;
long long rrl_sqrl_scratch_floats(long long n, int k);
int rrl_sqrl_act(const rrl_sqrl_act_t* a, void* stream);
/* ... for S seeds in one launch (the packed-launch table above): args[s] is checked as rrl_sqrl_act checks it (same codes), all
 * seeds before anything is stored or launched; S outside 1 .. 16, args == NULL or seeds that differ in k: RRL_EINVAL; S == 1 is
 * rrl_sqrl_act(args). */
int rrl_sqrl_act_packed(int S, const rrl_sqrl_act_t* args, void* stream);

/* The same pass with layer 2 of the twin Q_risk in f16x3 (the planner's arithmetic, rrl_plan_cost_t.f16x3): the descriptor, the
 * checks, their order and their codes are rrl_sqrl_act's; a->W2p names the rrl_w2_pack_f16x3 stream of the two heads instead of
 * the rrl_w2_pack one.
 * W2h = the G row-major [H, H] matrices W2 (out, in -- model.py's nn.Linear weights) in the order the K = 32 f16 MFMA's B operands
 * consume them, every value w as hi = f16(w), lo = f16(w - hi) (lo unscaled; |w| > 65504 clamped first, as rrl_plan_pack does):
 * per matrix g, column tile n and 32-wide block jp (n < H / 16, jp < H / 32) two float4 slots of 8 halves per lane,
 * slot (n, 2 jp, lane) = hi[0..7] and slot (n, 2 jp + 1, lane) = lo[0..7] of W2[g][16 n + lane % 16][32 jp + 8 (lane / 16) + 0..7],
 * i.e. the float4 lane `lane` of the wave that owns output columns 16 n .. 16 n + 15 needs sits at float4 index
 * g H H / 4 + (n H / 16 + 2 jp + {0: hi, 1: lo}) 64 + lane.  G H H floats of storage, 16-byte aligned.  NULL pointer, misaligned W2h,
 * G <= 0 or H not a positive multiple of 32: RRL_EINVAL.
 * Precision contract of rrl_sqrl_act_f16x3 against rrl_sqrl_act on the same descriptor (W2p apart):
 *   cand, logp, the candidate noise, the pick's uniform and the tick advance are rrl_sqrl_act's bits.
 *   score: layer 1 (K = 4) is the exact f32 MFMA.  Its relu output v is held as hi = f16(v), lo = f16(v - hi); layer 2 sums, per
 *          32-wide k block in ascending order, hi*lo, hi*hi, lo*hi on v_mfma_f32_16x16x32_f16 with f32 accumulators (lo*lo, 2^-22
 *          of a product, is dropped); the folded last layer, z, q and the pick are rrl_sqrl_act's expressions.  z and q, and so
 *          n_safe, cstar, pick and action where a decision is within that error of its threshold, differ from rrl_sqrl_act's:
 *          |z - float64| stays within 4 x the error of the same chain evaluated in f32 (tests/test_sqrl_f16x3_gpu.py).
 *   Activations above 65504 saturate to 65504; NaN stays NaN.
 *   A candidate's z does not depend on k, on its row tile or on the pass it falls in. */
int rrl_w2_pack_f16x3(int G, int H, const float* W2, float* W2h, void* stream);
int rrl_sqrl_act_f16x3(const rrl_sqrl_act_t* a, void* stream);
/* ... packed, by the rules of rrl_sqrl_act_packed (a launch site of its own: its plans are not rrl_sqrl_act_packed's) */
int rrl_sqrl_act_f16x3_packed(int S, const rrl_sqrl_act_t* args, void* stream);

/* --------------------------------------------------------------------------------------------
 * Q-sampling recovery.  Replaces QRiskWrapper.select_action (recovery_rl/qrisk.py:214-225: --Q_sampling_recovery draws 1000
 * uniform actions and executes the one with the smallest Q_risk) for the envs whose recovery gate fired.  Per env e with
 * mask == NULL || mask[e] != 0:
 *   candidate  b = Philox (seed, row e k + c, RRL_STREAM_QSAMPLE, counter + tick); u_0, u_1 = the open-unit doubles of its low
 *              and high 64 bits (the pairing of the maze reset); a_j = float(double(lo_j) + (double(hi_j) - double(lo_j)) u_j):
 *              double arithmetic without contraction, rounded once.  With cand_in the candidate is cand_in[e, c].
 *   score      as rrl_sqrl_act: z_h = head h of Q_risk on [obs_e | a_ec], exact-f32 MFMA; q = max(sigmoid z_0, sigmoid z_1),
 *              NaN propagates
 *   pick       argmin_c q: the lowest index wins ties and NaN counts as the smallest (torch.argmin); action[e] = a[e, pick]
 * Nothing of an env whose gate did not fire is written (no action, no diagnostic), and its workgroups leave before they read
 * a weight.  Two kernels: n x ceil(k / 128) workgroups score up to 128 candidates each (two 64-row passes, the tile of
 * rrl_sqrl_act) and leave a partial (smallest q, its index, that candidate) in `scratch`; a small second kernel folds an env's
 * partials in ascending chunk order with a strict <, writes action / pick, and does tick += counter_inc -- once per call,
 * whatever the mask holds; the score kernel only reads the tick (the ticket word of counter_dev is not used).
 * Weights as rrl_sqrl_act_t.  Checks before any launch: NULL descriptor or required pointer (obs, lo, hi, W1 .. b3, scratch,
 * action), n <= 0, H != 256, d_obs or d_act != 2, misaligned W2p: RRL_EINVAL; k outside 1..1024 or n k >= 2^32: RRL_ERANGE
 * (an invalid field wins).  rrl_qsample_scratch_floats(n, k) = 4 n ceil(k / 128), with the same range checks.
 * ------------------------------------------------------------------------------------------ */
enum { RRL_STREAM_QSAMPLE = 11 };   /* Q-sampling recovery candidates */
typedef struct {
    int n, k;                       /* envs; candidates per env, 1..1024 (the reference: 1000) */
    int H, d_obs, d_act;            /* 256, 2, 2 */
    const float* obs;               /* [n, 2] */
    const uint8_t* mask;            /* nullable [n]: the recovery gate; NULL = every env */
    const float *lo, *hi;           /* [2] action box on the device */
    const float *W1, *b1, *W2p, *b2, *W3, *b3;   /* as rrl_sqrl_act_t */
    uint64_t seed, counter;
    uint64_t* counter_dev;          /* nullable {tick, unused} */
    uint64_t counter_inc;
    const float* cand_in;           /* nullable [n, k, 2]: replaces the draws */
    float* scratch;                 /* [rrl_qsample_scratch_floats(n, k)] */
    float* action;                  /* [n, 2]: written for gated envs only */
    float *q, *z, *cand;            /* nullable diagnostics [n,k], [2,n,k], [n,k,2]; gated envs only */
    int32_t* pick;                  /* nullable diagnostic [n]; gated envs only */
} rrl_qsample_act_t;
long long rrl_qsample_scratch_floats(long long n, int k);
int rrl_qsample_act(const rrl_qsample_act_t* a, void* stream);

/* The same call with the recovery gate evaluated inside it, from Q_risk(s, a_task) as a stack forward left it: the launches of
 * rrl_recovery_select (and of the sum of the partials before it) disappear, and the acting pass is made of launches that have
 * packed forms.  a->mask must be NULL.  recovery[e] = max(sigmoid z0, sigmoid z1) > eps_safe with z_h the f32 sum of the n_part
 * partials in order -- the device helper of rrl_recovery_select and of rrl_step_push_t.sel_*, same bits, NaN included.  Every
 * workgroup of the score kernel evaluates its env's gate first (the 2 n_part partials, requested as 8 loads: partial 0 stands
 * in for an absent one) and leaves if it did not fire; the fold kernel
 * writes, for EVERY env, recovery_out[e], task_out[e] (if asked) and action[e] = the pick of a gated env, else the env's task
 * action: together what rrl_recovery_select followed by rrl_qsample_act leave.  Diagnostics for gated envs only; the tick
 * advances once per call.  Checks, before any launch: the descriptor's (same codes); g, g->z, g->task_action or
 * g->recovery_out NULL, n_part outside 1..4, ld_task < 2 or odd, a->mask given: RRL_EINVAL (wins over RRL_ERANGE). */
typedef struct {
    const float* z;           /* [2, n] pre-sigmoid twin Q_risk(s, a_task): n_part partial sums part_stride floats apart */
    int n_part;               /* 1..4, summed in the fixed order every consumer of a stack output uses */
    long long part_stride;
    float eps_safe;
    const float* task_action; /* row e at task_action + e * ld_task; ld_task >= 2 and even */
    int ld_task;
    float* task_out;          /* nullable [n, 2]: the task action, as rrl_recovery_select's task_out */
    uint8_t* recovery_out;    /* [n]: the gate, as rrl_recovery_select writes it */
} rrl_qsample_gate_t;
int rrl_qsample_act_gated(const rrl_qsample_act_t* a, const rrl_qsample_gate_t* g, void* stream);
/* ... and for S seeds in two launches (the packed-launch table above).  gates == NULL: every seed uses its own mask, as
 * rrl_qsample_act; otherwise gates[s] is seed s's gate.  Every seed is checked as the stand-alone entry checks it (same
 * codes), all before anything is stored or launched; S outside 1 .. 16 or args == NULL: RRL_EINVAL; a seed with more than
 * INT32_MAX / 16 score workgroups: RRL_ERANGE; S == 1 is the stand-alone (or gated) call. */
int rrl_qsample_act_packed(int S, const rrl_qsample_act_t* args, const rrl_qsample_gate_t* gates, void* stream);

/* The same three calls with layer 2 of the twin Q_risk in f16x3 (the arithmetic of rrl_sqrl_act_f16x3 above): the descriptors,
 * the checks, their order, their codes and the scratch size (rrl_qsample_scratch_floats) are rrl_qsample_act's; a->W2p names
 * the stream rrl_w2_pack_f16x3(2, 256, W2, W2h) writes of the two heads' hidden weights instead of the rrl_w2_pack one, exactly
 * as rrl_sqrl_act_f16x3 reads it.  Nothing keeps that stream current but the caller: the scores follow the stream, not W2.
 * Precision contract against rrl_qsample_act / rrl_qsample_act_gated on the same descriptor (W2p apart):
 *   cand, the candidate draws, the gate, recovery_out, task_out, the partials' layout, the fold and the tick advance are the
 *   f32 call's bits; pick is the lowest-index argmin of the call's OWN q (NaN smallest) and action = cand[pick], by the f32
 *   call's text.
 *   score: layer 1 (K = 4) is the exact f32 MFMA.  Its relu output v is clamped at 65504 and held as hi = f16(v),
 *          lo = f16(v - hi), lo unscaled; layer 2 sums, per 32-wide k block in ascending order, hi*lo, hi*hi, lo*hi
 *          (activation * weight) on v_mfma_f32_16x16x32_f16 with f32 accumulators; lo*lo (2^-22 of a product) is dropped; the
 *          folded last layer, z and q are rrl_qsample_act's expressions.  |z - float64| stays within 4 x the error of the same
 *          chain evaluated in f32, so the picked candidate's float64 q is within half that bound of the float64 minimum
 *          (sigmoid is 1/4-Lipschitz; tests/test_qsample_f16x3_gpu.py).
 *   Activations above 65504 saturate to 65504; NaN stays NaN.
 *   A candidate's z does not depend on k, on its chunk, its row tile or the pass it falls in. */
int rrl_qsample_act_f16x3(const rrl_qsample_act_t* a, void* stream);
int rrl_qsample_act_gated_f16x3(const rrl_qsample_act_t* a, const rrl_qsample_gate_t* g, void* stream);
/* ... packed, by the rules of rrl_qsample_act_packed (a launch site of its own: its plans are not rrl_qsample_act_packed's) */
int rrl_qsample_act_f16x3_packed(int S, const rrl_qsample_act_t* args, const rrl_qsample_gate_t* gates, void* stream);

/* --------------------------------------------------------------------------------------------
 * Policy evaluation as ONE launch.  Replaces Experiment.get_test_rollout (recovery_rl/experiment.py:493-538: one
 * deterministic-policy episode per env) for n Navigation 1 / 2 envs: reset, then T x (task policy -> Q_risk gate -> recovery
 * policy -> transition) with the per-env return and flags, no launch boundary inside.  A workgroup owns a tile of 16 envs for
 * the whole rollout; the networks run on one row tile of the tile of rrl_qsample_act (activations in LDS, W2 in rrl_w2_pack
 * order, exact-f32 MFMA, k ascending), the env state stays in registers.
 *   start      reset != 0: pos_i = START + N(0, I), the normal pair of Philox (seed, i, RRL_STREAM_RESET, tick);
 *              reset == 0: pos_i = pos[i] (read, never written).  tick = counter + counter_dev[0].
 *   step j     (j = 0 .. T - 1, rows still alive) obs = float(pos);
 *              task = tanh(mean(obs)) * scale + bias (the Gaussian policy's mean rows, W3 rows 0 .. 1);
 *              with the Q_risk group: gate = max(sigmoid z0, sigmoid z1) > eps_safe on Q_risk(obs, task), the device helper
 *              of rrl_recovery_select (same bits); with the recovery group as well: rec = tanh(mean_r(obs)) * rscale + rbias +
 *              exp(max(rlog_std, min_log_std)) * eps, eps = float of the normal pair of Philox (seed, i, RRL_STREAM_EVAL,
 *              tick + reset + j), and executed = gate ? rec : task; without it executed = task;
 *              transition of rrl_nav_step on double(executed) with the noise of (seed, i, RRL_STREAM_STEP, tick + reset + j).
 *   results    ret[i] = f32 sum in step order of the rewards of the steps taken while alive, success[i] / violation[i] = OR
 *              over those steps, steps[i] = their number; a row dies after a step whose done (success | constraint) is set.
 *   tick       counter_dev[0] += T + reset by the last workgroup (counter_dev = {tick, ticket}), what reset() and T step()
 *              calls of the eager env advance it by.
 * A workgroup without a live row leaves the step loop, the recovery policy's forward is skipped while no row of the tile is
 * gated, rows >= n write nothing: none of this changes a bit of any output.  Trace buffers (each nullable) are written at
 * step j for the rows alive before it and left untouched otherwise.
 * Checks before any launch, without a device: NULL descriptor or required pointer (the task policy's eight, ret, success,
 * violation, steps), H != 256, d_obs or d_act != 2, n <= 0, unknown env_kind, a Q_risk group or a recovery group given in
 * part, a recovery group without the Q_risk group, a W2p not 16-byte aligned, reset == 0 without pos: RRL_EINVAL; T outside
 * 1..4096 or n > 2^22: RRL_ERANGE (an invalid field wins).
 * ------------------------------------------------------------------------------------------ */
enum { RRL_STREAM_EVAL = 12 };      /* recovery-policy noise of the evaluation rollout */
typedef struct {
    int n, T;                       /* envs; steps, 1..4096 (the reference: horizon + 1) */
    int H, d_obs, d_act;            /* 256, 2, 2 */
    int env_kind;                   /* RRL_ENV_NAV1 or RRL_ENV_NAV2 */
    int reset;                      /* != 0: start states drawn here; 0: taken from pos */
    const double* pos;              /* [n, 2], required with reset == 0; never written */
    const float *pW1, *pb1, *pW2p, *pb2, *pW3, *pb3;   /* task policy: [256,2], [256], fragment order, [256], [>= 2,256], [>= 2] */
    const float *scale, *bias;      /* [2] action box of the task policy */
    const float *qW1, *qb1, *qW2p, *qb2, *qW3, *qb3;   /* Q_risk group, all or none: as rrl_sqrl_act_t's W1 .. b3 */
    float eps_safe;
    const float *rW1, *rb1, *rW2p, *rb2, *rW3, *rb3;   /* recovery group, all or none (with rscale, rbias, rlog_std) */
    const float *rscale, *rbias, *rlog_std;            /* [2] each */
    float min_log_std;
    uint64_t seed, counter;         /* the env's Philox seed; tick = counter + counter_dev[0] */
    uint64_t* counter_dev;          /* nullable {tick, ticket}: += T + reset by the last workgroup */
    float* ret;                     /* [n] */
    uint8_t *success, *violation;   /* [n] */
    int32_t* steps;                 /* [n] */
    double* tr_pos;                 /* nullable trace [T, n, 2]: state before step j */
    float *tr_task, *tr_real;       /* nullable traces [T, n, 2]: task and executed action before clipping */
    float* tr_z;                    /* nullable trace [T, 2, n]: pre-sigmoid Q_risk (Q_risk group only) */
    float* tr_eps;                  /* nullable trace [T, n, 2]: the recovery noise (recovery group only) */
    float* tr_reward;               /* nullable trace [T, n] */
    uint8_t* tr_flags;              /* nullable trace [T, n]: bit 0 alive before the step, 1 done, 2 constraint, 3 success, 4 recovery */
} rrl_eval_rollout_t;
int rrl_eval_rollout(const rrl_eval_rollout_t* a, void* stream);
/* ... and for S seeds side by side (the packed-launch table above): each seed with its own n, T, weights, env seed and tick,
 * its outputs the bits of its stand-alone launch.  Every seed is checked as the stand-alone entry checks it, all before
 * anything is stored or launched; args == NULL: RRL_EINVAL; S outside 1 .. 16: RRL_ERANGE; S == 1 is rrl_eval_rollout(args). */
int rrl_eval_rollout_packed(int S, const rrl_eval_rollout_t* args, void* stream);

/* The same rollout for n Maze envs (MazeVecEnv(auto_reset = False)): the SAME descriptor on kernels of their own, so the
 * Navigation kernels carry no Maze branch.  Networks, gate, recovery noise, results, traces and the tile are those above;
 * the env part is rrl_maze_step / rrl_maze_reset's device code (maze_device.hpp), bit for bit:
 *   start      reset != 0: pos_i = the draw of rrl_maze_reset(mode 0, check_constraint 1) at the tick, rejection loop
 *              included; reset == 0: pos_i = pos[i].  The episode clock starts at 0 either way.
 *   step j     obs, task, gate and recovery action as above (noise: RRL_STREAM_EVAL at tick + reset + j);
 *              new = move(pos, double(executed)) -- the move clamps to +-0.1 itself, the traces hold the unclipped action;
 *              d = goal distance of new, reward = float(-d), constraint = contact at new, success = -d > -0.03:
 *              all judged at the NEW state (Navigation's cost is judged at the old one);
 *              done = (j + 1 >= horizon) | constraint | (d < 0.03): a row that reaches the horizon is done with neither flag.
 *   tick       counter_dev[0] += T + reset: the Maze step draws nothing, but the eager step() advances the tick by 1 as well.
 * Checks: the descriptor's, except that env_kind must be RRL_ENV_MAZE (a Navigation kind is RRL_EINVAL here, as Maze is
 * there); horizon outside 1 .. 2^30: RRL_ERANGE (an invalid field wins). */
int rrl_eval_rollout_maze(const rrl_eval_rollout_t* a, int horizon, void* stream);
/* ... and for S seeds side by side, horizon[s] seed s's (part of the plan key).  args or horizon NULL: RRL_EINVAL; S outside
 * 1 .. 16: RRL_ERANGE; every seed is checked before anything is stored or launched; S == 1 is
 * rrl_eval_rollout_maze(args, horizon[0]). */
int rrl_eval_rollout_maze_packed(int S, const rrl_eval_rollout_t* args, const int* horizon, void* stream);

/* The same rollout for Q-sampling recovery (--use_recovery --Q_sampling_recovery: QRiskWrapper.select_action,
 * recovery_rl/qrisk.py:214-225, inside get_test_rollout): in the place of a recovery policy, a row whose gate fired while
 * alive executes the best of k uniform candidates -- rrl_qsample_act's three steps inside the rollout launch, on kernels of
 * their own (Navigation 1 / 2 and Maze, by base.env_kind), so the kernels above keep their code.  Start, task policy, gate,
 * transition, results, tick and the base's traces are those above; for a gated live row i at step j:
 *   candidate  b = Philox (seed, row i k + c, RRL_STREAM_EVAL_QSAMPLE, tick + reset + j), c = 0 .. k - 1; u_0, u_1 = the
 *              open-unit doubles of its low and high 64 bits; a_j = float(double(lo_j) + (double(hi_j) - double(lo_j)) u_j):
 *              double arithmetic without contraction, rounded once (rrl_qsample_act's).  The draws are keyed by (env row,
 *              step) alone: they do not depend on which other rows are gated or alive, nor on n.
 *   score      z_h = head h of Q_risk on [float(pos_i) | a_c], q = max(sigmoid z_0, sigmoid z_1), NaN propagates: the 64-row
 *              tile of rrl_qsample_act in passes of up to four row tiles -- the bits rrl_qsample_act gives for the same
 *              obs and candidate
 *   pick       argmin_c q: the lowest index wins ties and NaN counts as the smallest (torch.argmin); executed = a_pick
 * A workgroup serves the gated live rows of its 16 one after another in ascending row order, so k up to 1024 fits its LDS
 * (82.4 KB: one workgroup per CU).  Rows that are not gated, dead rows and rows >= n draw and score nothing, a tile with no
 * gated live row in a step skips the phase, a workgroup without a live row leaves the step loop: none of this changes a bit
 * of any output.  tr_real of a gated row holds the picked candidate; tr_eps is never written; tr_pick / tr_q are written for
 * gated live rows only.  The time follows the gated share: with every row gated on every step at k = 1000 and T = 101 a
 * workgroup runs 16 rows x 16 passes x 2 heads per step, about 110 TFLOP for 4096 envs -- on the order of a second, the
 * FLOPs the module path spends on every evaluation whatever the gate says.
 * Checks before any launch, without a device: everything rrl_eval_rollout (rrl_eval_rollout_maze for RRL_ENV_MAZE) checks
 * on base, with the same codes; NULL lo or hi, no Q_risk group, any pointer of the recovery group given: RRL_EINVAL; k outside
 * 1..1024, n k >= 2^32, a Maze horizon outside 1 .. 2^30: RRL_ERANGE (an invalid field wins). */
enum { RRL_STREAM_EVAL_QSAMPLE = 13 };   /* Q-sampling candidates of the evaluation rollout */
typedef struct {
    rrl_eval_rollout_t base;   /* recovery group (rW1 ..) must be all NULL; Q_risk group required */
    int k;                     /* candidates per gated row, 1..1024 (the reference: 1000) */
    int horizon;               /* Maze only (1 .. 2^30); ignored for Navigation */
    const float *lo, *hi;      /* [2] action box on the device */
    int32_t* tr_pick;          /* nullable trace [T, n]: the pick of a gated live row, else untouched */
    float*   tr_q;             /* nullable trace [T, n]: its q, else untouched */
} rrl_eval_rollout_qs_t;
int rrl_eval_rollout_qs(const rrl_eval_rollout_qs_t* a, void* stream);
/* ... and for S seeds side by side (the packed-launch table above): all Navigation (either kind) or all Maze (any horizons),
 * a mix is RRL_EINVAL; each seed's outputs, traces and tick are the bits of its stand-alone launch.  Every seed is checked as
 * the stand-alone entry checks it, all before anything is stored or launched (RRL_EINVAL of any seed wins); args == NULL:
 * RRL_EINVAL; S outside 1 .. 16: RRL_ERANGE; S == 1 is rrl_eval_rollout_qs(args). */
int rrl_eval_rollout_qs_packed(int S, const rrl_eval_rollout_qs_t* args, void* stream);

/* The same rollout for SQRL (--use_constraint_sampling without --use_recovery: SAC._sqrl_action, recovery_rl/sac.py:139-161,
 * inside get_test_rollout): EVERY live row executes, on every step, the pick among k candidates of the task policy's
 * tanh-Gaussian head -- rrl_sqrl_act's three steps inside the rollout launch, on kernels of their own (Navigation 1 / 2 and
 * Maze, by base.env_kind), so the kernels above keep their code.  Start, transition, results, tick and the base's traces are
 * those above; for a row i alive before step j, with ctr = tick + reset + j:
 *   head       the FOUR last-layer outputs (mean0, mean1, log_std0, log_std1: pW3 / pb3 hold four rows, the stacked head that
 *              rrl_sqrl_act_t.head describes) of the task policy on float(pos_i); rows 0 .. 1 are the bits of the two-output
 *              form, so tr_task = tanh(mean) * scale + bias is what the kernels above write.  Under SQRL it is not executed.
 *   candidate  eps_c = float of the normal pair of Philox (seed, row i k + c, RRL_STREAM_EVAL_SQRL, ctr), c = 0 .. k - 1;
 *              a_c, logp_c = the tanh-Gaussian head of rrl_sqrl_act (log_std clamped to [-20, 2], kEps = 1e-6, f32, the same
 *              expression order).  The draws are keyed by (env row, step) alone.
 *   score      q_c = max(sigmoid z_0, sigmoid z_1) of Q_risk on [float(pos_i) | a_c], NaN propagates: the 64-row tile of
 *              rrl_sqrl_act -- the bits rrl_sqrl_act gives for the same obs, head and eps
 *   pick       rrl_sqrl_act's, with safe = q <= base.eps_safe and u = the open-unit double of the low 64 bits of Philox (seed,
 *              row i, RRL_STREAM_EVAL_SQRL_PICK, ctr): weights in double, the position in the SAFE list applied to the FULL
 *              list; no safe candidate: argmin q, lowest index on ties, NaN counts as the smallest
 *   execute    executed = a_pick.  No gate and no recovery policy: bit 4 of tr_flags stays 0, tr_z and tr_eps are never written.
 * A workgroup flattens the candidates of the live rows of its 16 into passes of up to 64 scoring rows (every row of a pass
 * carries its own obs), keeps the candidates, logp and q of the whole tile in LDS (103.0 KB in all: one workgroup per CU), and
 * picks for different rows on different waves.  Dead rows and rows >= n draw and score nothing, a workgroup without a live row
 * leaves the step loop: none of this changes a bit of any output.  The traces of this struct are written for live rows only.
 * Checks before any launch, without a device: everything rrl_eval_rollout (rrl_eval_rollout_maze for RRL_ENV_MAZE) checks on
 * base, with the same codes; no Q_risk group, any pointer of the recovery group given: RRL_EINVAL; k outside 1..128,
 * n k >= 2^32, a Maze horizon outside 1 .. 2^30: RRL_ERANGE (an invalid field wins). */
enum { RRL_STREAM_EVAL_SQRL = 14,        /* SQRL candidate noise of the evaluation rollout */
       RRL_STREAM_EVAL_SQRL_PICK = 15 }; /* its categorical draw */
typedef struct {
    rrl_eval_rollout_t base;  /* Q_risk group required; recovery group (rW1 ..) all NULL; pW3 / pb3 hold FOUR rows:
                                 mean0, mean1, log_std0, log_std1 (the stacked head rrl_sqrl_act_t.head describes) */
    int k;                    /* candidates per live row, 1..128 (the reference: 100) */
    int horizon;              /* Maze only (1 .. 2^30); ignored for Navigation */
    float*   tr_head;         /* nullable trace [T, n, 4]: the policy's last-layer output before the clamp */
    int32_t *tr_pick, *tr_cstar, *tr_nsafe;   /* nullable traces [T, n]; cstar = -1 on the argmin branch */
    float*   tr_q;            /* nullable trace [T, n]: q of the executed candidate */
} rrl_eval_rollout_sqrl_t;
int rrl_eval_rollout_sqrl(const rrl_eval_rollout_sqrl_t* a, void* stream);
/* ... and for S seeds side by side (the packed-launch table above): all Navigation (either kind) or all Maze (any horizons),
 * a mix is RRL_EINVAL; n, T, k, reset and weights may differ by seed; each seed's outputs, traces and tick are the bits of
 * its stand-alone launch.  Every seed is checked as the stand-alone entry checks it, all before anything is stored or launched
 * (RRL_EINVAL of any seed wins); args == NULL: RRL_EINVAL; S outside 1 .. 16: RRL_ERANGE; S == 1 is
 * rrl_eval_rollout_sqrl(args). */
int rrl_eval_rollout_sqrl_packed(int S, const rrl_eval_rollout_sqrl_t* args, void* stream);

/* The two rollouts above with the candidates scored in f16x3 (the arithmetic of rrl_sqrl_act_f16x3 / rrl_qsample_act_f16x3):
 * the same descriptors on kernels of their own (Navigation 1 / 2 and Maze, solo and packed), so the kernels above keep their
 * code.  qW2h is the stream rrl_w2_pack_f16x3(2, 256, W2, qW2h) writes of Q_risk's two heads; it rides beside the descriptor,
 * as the Maze horizon does.  Nothing keeps that stream current but the caller: the scores follow the stream, not W2.
 * base.qW2p keeps its meaning and its checks: the Q-sampling kernels read it for the gate, the SQRL kernels do not read it.
 * Precision contract against the f32 entry on the same descriptor:
 *   Start, task action, tr_head, gate (tr_z, flag bit 4: exact f32 on the 16-row stack from base.qW2p), candidates, logp,
 *   draws, the results' fold and the tick are the f32 entry's expressions.
 *   score: for a given state and step, the score of a candidate is the bits rrl_qsample_act_f16x3 / rrl_sqrl_act_f16x3 give
 *          for the same obs, candidate and stream: layer 1 (K = 4) exact f32; its relu output v held as hi = f16(v),
 *          lo = f16(v - hi); layer 2 sums, per 32-wide k block in ascending order, hi*lo, hi*hi, lo*hi on
 *          v_mfma_f32_16x16x32_f16 with f32 accumulators (lo*lo dropped); the folded last layer, z and q are the f32
 *          expressions.  Those bits are independent of k, row tile, pass and which other rows are live or gated.
 *   pick:  the f32 entry's rule on those scores.  A pick that falls within the scoring error of a tie or of eps_safe may differ
 *          from the f32 entry's; from that step on the episode may differ as well.
 * LDS: the f16 planes are 1 KB larger than the f32 activations: 83.4 KB (Q-sampling) and 104.0 KB (SQRL), one workgroup per CU.
 * Checks, their order and their codes are the f32 entry's on the same descriptor; in addition qW2h NULL or not 16-byte aligned
 * is RRL_EINVAL (for the packed entries: the array, or any seed's pointer), which wins over RRL_ERANGE as every invalid field
 * does.  The packed entries follow rrl_eval_rollout_qs_packed / rrl_eval_rollout_sqrl_packed (launch sites of their own, the
 * qW2h pointers are part of the plan key, a Navigation / Maze mix is RRL_EINVAL, S == 1 is the solo entry). */
int rrl_eval_rollout_qs_f16x3(const rrl_eval_rollout_qs_t* a, const float* qW2h, void* stream);
int rrl_eval_rollout_qs_f16x3_packed(int S, const rrl_eval_rollout_qs_t* args, const float* const* qW2h, void* stream);
int rrl_eval_rollout_sqrl_f16x3(const rrl_eval_rollout_sqrl_t* a, const float* qW2h, void* stream);
int rrl_eval_rollout_sqrl_f16x3_packed(int S, const rrl_eval_rollout_sqrl_t* args, const float* const* qW2h, void* stream);

#ifdef __cplusplus
}
#endif
#endif
