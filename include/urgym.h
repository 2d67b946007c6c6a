/*
 * urgym.h — C-ABI of the MI355X-native vectorised UR5e reach environment (liburgym_hip.so).
 *
 * The reference (WanqingXia/UR-gym) is pure Python on top of pybullet and has no FFI seam of its own
 * (SURVEY.md §8b).  The drop-in boundary is the Gymnasium Env surface of RobotTaskEnv, vectorised over N
 * environments; this header is what a ctypes binding of that surface calls.  Each entry point names the
 * reference interface it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - plain C, no torch types: the caller (PyTorch-ROCm tensors in ur_gym_amd/vector_env.py) allocates and
 *     owns EVERY buffer; the library borrows the raw device pointers registered with urgym_bind() and keeps
 *     only its constant tables (hull vertices, chain constants) uploaded at urgym_create().
 *   - state is float64 like the reference's internal state, struct-of-arrays [field][N] so that one lane per
 *     environment reads/writes coalesced; observations are float32 row-major [N][dim] exactly as
 *     RobotTaskEnv._get_obs casts them (UR_gym/envs/core.py:252-261).
 *   - all launches are asynchronous on the caller-supplied HIP stream (hipStream_t passed as void*).
 *   - return value: 0 = ok, <0 = error (urgym_last_error() gives the text).  No C++ exception crosses the ABI.
 *   - one handle per (process, device); calls on one handle are not re-entrant.
 */
#ifndef URGYM_H
#define URGYM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URGYM_ABI_VERSION 4

/* env kinds = the reference's registered ids (UR_gym/__init__.py:19-42, UR_gym/envs/ur_tasks.py:37-90) */
enum {
  URGYM_ENV_ORI = 0, /* UR5OriReach-v1 : ReachOri, reach.py:141-236 */
  URGYM_ENV_OBS = 1, /* UR5ObsReach-v1 : ReachObs, reach.py:239-374 */
  URGYM_ENV_DYN = 2, /* UR5DynReach-v1 : ReachDyn, reach.py:576-785 */
  URGYM_ENV_STA = 3, /* UR5StaReach-v1 : ReachSta, reach.py:377-573 (static obstacle; moves only when obst_end != 0) */
};

/* error codes */
enum {
  URGYM_OK = 0,
  URGYM_ERR_ARG = -1,
  URGYM_ERR_HIP = -2,
  URGYM_ERR_STATE = -3,
};

/* First separating axis of the GJK closest-point queries of the links (obstacle, table, track, self pairs).
 * BULLET: the world +Y axis, as btGjkPairDetector is entered by btConvexConvexAlgorithm -- the search then visits the
 *         same simplices as the reference's Bullet build (default; what every parity test pins).
 * GUIDED: the line from the other shape's centre to the mid point of the link's bounding capsule -- about half the
 *         iterations (a few % of step rate since the hull search starts from a direction map).  NOT parity-grade: Bullet's answer is not path-independent (its
 *         degenerate-simplex / no-progress exits return the current iterate), so on these finely faceted hulls the two
 *         modes differ by > 1e-6 m on ~1.5 % and > 1e-5 m on ~0.15 % of the queries, worst seen ~1e-4 m.  Opt-in for
 *         training runs that do not need the reference's exact numbers; see DESIGN.md "GJK start". */
enum {
  URGYM_GJK_START_BULLET = 0,
  URGYM_GJK_START_GUIDED = 1,
};

/* What task.link_dist (the five "link distance" slots of the Obs/Sta/Dyn observation and the distance-change reward) measures.
 * OBSTACLE : links 2..6 vs the obstacle -- PyBullet.get_link_distances as it stands (pyb_setup.py:439-456).  Default.
 * WORKBENCH: per link the minimum over obstacle, table and track -- what the docstring of get_link_distances still says
 *            ("the distance between workbench, obstacle and UR5") and what the reference's code evidently did when its
 *            UR5ObsReach-v1 / UR5StaReach-v1 checkpoints were trained (Sep 2023): the observations stored inside
 *            Trained_Models/Trained_{Obs,Sta}/best_model.zip are reproduced to 1e-7 by this rule and not by OBSTACLE
 *            (tests/test_reference_pins.py).  Needed to replay those two checkpoints (tests/test_closed_loop.py). */
enum {
  URGYM_LINK_DIST_OBSTACLE = 0,
  URGYM_LINK_DIST_WORKBENCH = 1,
};

/* bits of the per-env status word (device-side anomalies; SURVEY.md §5 "failure detection") */
enum {
  URGYM_STATUS_NAN = 1,              /* a NaN reached the reward/obs (utils.py:65-67 prints in the reference) */
  URGYM_STATUS_RESET_EXHAUSTED = 2,  /* rejection sampling hit max_reset_tries (reach.py:668-675 loops forever) */
  URGYM_STATUS_RESET_COLLISION = 4,  /* "Collision after reset, this should not happen" (reach.py:682-683) */
  URGYM_STATUS_PENETRATION = 8,      /* informational: a link_dist that was consumed is a penetration depth (negative) */
  URGYM_STATUS_GJK_ITER = 16,        /* GJK / EPA hit its iteration cap */
  URGYM_STATUS_STALE_RECORD = 64,    /* an env finished while the episode counter the caller had edited no longer matched its
                                        prefetched episode record, and urgym_invalidate_records had not been called: the env was
                                        NOT reset */
  URGYM_STATUS_JOINT_LIMIT = 32,     /* a joint was commanded past its URDF limit (ur5e.urdf:237-277: elbow +-pi, others +-2pi).
                                        The reference teleports joints with resetJointState, which does not clamp, but Bullet's
                                        limit constraints then act during stepSimulation: from here on the kinematic model of this
                                        build is outside the regime it was checked in. */
};

/* One POD config struct: every constant the reference hard-codes in its task constructors. */
typedef struct urgym_config {
  int32_t env_kind;          /* URGYM_ENV_* */
  int32_t num_envs;          /* N */
  int32_t max_episode_steps; /* TimeLimit, UR_gym/__init__.py:41 -> 100 */
  int32_t auto_reset;        /* 1: finished envs are reset inside urgym_step (gymnasium VectorEnv semantics) */
  int32_t check_collision;   /* 1: reference behaviour; 0: BASELINE.json configs[1] "FK + reward only" */
  int32_t max_reset_tries;   /* bound on the reference's unbounded rejection loop */
  int32_t dyn_motion_steps;  /* reach.py:735 -> 25 */
  int32_t gjk_start;         /* URGYM_GJK_START_*: first separating axis of every link query (default BULLET) */
  int32_t link_dist_scope;   /* URGYM_LINK_DIST_*: what task.link_dist measures (default OBSTACLE = the reference as it stands) */
  int32_t reserved0;         /* keeps the doubles 8-byte aligned; must be 0 */
  double action_scale;       /* UR5.py:276,314: pi*0.1 is applied as two float32 products; kept for reporting */
  double dt;                 /* pyb_setup.py:40,47-50: 20 substeps / 500 Hz = 0.04 s */
  double distance_threshold; /* reach.py:148/246/590 -> 0.05 */
  double ori_threshold;      /* reach.py:149/591 -> 0.0873 */
  double w_collision;        /* -500 */
  double w_success;          /* +200 */
  double w_distance;         /* Ori/Dyn -70, Obs -100 */
  double w_orientation;      /* Ori/Dyn -30, Obs 0 */
  double w_link[5];          /* Dyn: [8,2.4,1.2,1.2,0.2]/13*50 (reach.py:596-597); Obs: 100 each (reach.py:255,371) */
  double near_threshold;     /* 0.2 (reach.py:371,783) */
  double collision_margin;   /* 0.01 (pyb_setup.py:402,411,422) */
  double target_clearance;   /* 0.1 (reach.py:322,675) */
  double min_travel;         /* Dyn: 1.0 (reach.py:675) */
  double dyn_time_duration;  /* Dyn: 2.0 (reach.py:736) */
  double goal_low[3], goal_high[3]; /* reach.py:151-152 / 248-249 / 584-585 */
  double obst_low[3], obst_high[3]; /* reach.py:250-251 / 586-587 */
  double neutral_q[6];       /* UR5.py:262 */
} urgym_config;

/* Device pointers, all owned by the caller.  SoA state: X[f][n] at X[f*N + n]. */
typedef struct urgym_buffers {
  /* ---- per-env state (float64) ---- */
  double* q;          /* [6][N] joint angles (pybullet joint state, UR5.py:346-351) */
  double* goal;       /* [6][N] goal xyz + rpy (Obs uses rows 0..2) */
  double* obst_start; /* [6][N] obstacle start xyz+rpy  (Obs: the static obstacle; reach.py:263,582) */
  double* obst_end;   /* [6][N] obstacle end xyz+rpy    (Dyn; Sta: all-zero = static obstacle, reach.py:306) */
  double* obst_pos;   /* [3][N] current obstacle position (Bullet base position) */
  double* obst_quat;  /* [4][N] current obstacle orientation xyzw */
  double* obst_vel;   /* [9][N] rows 0..5: per-episode twist (v, omega) that set_velocity (reach.py:728-753) re-applies while
                         step_count < dyn_motion_steps; rows 6..8: the base displacement that twist produces in ONE env step
                         (20 Bullet sub-steps in which the linear velocity drifts by h * omega x v) --
                         derived at reset / refresh; a caller that writes a twist of its own into rows 0..5 calls
                         urgym_derive_obstacle_motion afterwards (urgym_refresh would recompute the twist from start / end) */
  double* link_dist;  /* [5][N] task.link_dist == task.last_dist (reach.py:680-681,780-782) */
  int32_t* step_count;/* [N] ReachDyn.step_num == TimeLimit._elapsed_steps */
  int32_t* episode_id;/* [N] number of resets so far (RNG counter) */
  /* ---- outputs ---- */
  float* observation;   /* [N][obs_dim]  */
  float* achieved_goal; /* [N][goal_dim] */
  float* desired_goal;  /* [N][goal_dim] */
  float* reward;        /* [N] */
  uint8_t* terminated;  /* [N] */
  uint8_t* truncated;   /* [N] */
  uint8_t* is_success;  /* [N] info["is_success"] (core.py:272,315) */
  uint8_t* collision;   /* [N] task.collision */
  /* terminal observation of envs that were auto-reset in this step (valid where terminated|truncated) */
  float* final_observation;   /* [N][obs_dim]  */
  float* final_achieved_goal; /* [N][goal_dim] */
  float* final_desired_goal;  /* [N][goal_dim] */
  int32_t* status;      /* [N] URGYM_STATUS_* bits, sticky until cleared by the caller */
  /* ---- scratch ---- */
  int32_t* done_list;   /* [N] compacted ids of envs to reset */
  int32_t* done_count;  /* [2] ping-pong counters */
} urgym_buffers;

/* ABI version of the loaded library (== URGYM_ABI_VERSION). */
int urgym_abi_version(void);

/* Fill cfg with the reference's constants for env_kind (reach.py constructors). */
int urgym_config_default(int env_kind, int num_envs, urgym_config* cfg);

/* Observation layout: obs_dim = 18|26|35|29, goal_dim = 6|3|6|6 (core.py:241-247; reach.py:189,307,653,453-457). */
int urgym_obs_dims(int env_kind, int* obs_dim, int* goal_dim);

/* Replaces UR5*ReachEnv.__init__ (ur_tasks.py:37-90): builds the constant scene/robot tables on `device` (hull neighbour
 * records, direction maps), allocates the library's own scratch (link distances and set-up cache of the running step, episode
 * records) and fixes the launch geometry for cfg->num_envs.  Environment variables read here, all optional and none of them
 * changes a result (scheduling / tuning / tests): URGYM_STEP_ENVS (envs per workgroup of the step kernel, 1..128),
 * URGYM_STEP_TIERS="E1,B,E2" (B workgroups of E1 envs, then workgroups of E2), URGYM_RESET_ENVS (envs per workgroup of the
 * auto-reset kernel, 1..64), URGYM_PREFETCH (0: reset finished envs with a kernel after each step instead of inline from
 * prefetched episode records), URGYM_STEP_TIERS=0 (uniform workgroups where the default would be two-tier),
 * URGYM_REFILL_BLOCKS (refill workgroups per step launch of the obstacle envs, >= 1; default: a policy that widens the grid in
 * the steps where many envs finish), URGYM_VERBOSE (print the chosen geometry to stderr). */
int urgym_create(const urgym_config* cfg, int device, void** handle);
int urgym_destroy(void* handle);

/* Register the caller-owned device buffers (all pointers must stay valid until the next bind/destroy). */
int urgym_bind(void* handle, const urgym_buffers* bufs);

/* Replaces RobotTaskEnv.reset (core.py:263-273) for every env whose mask byte is non-zero (NULL = all).
 * `seed` re-keys the counter-based RNG; pass UINT64_MAX to keep the current key. */
int urgym_reset(void* handle, const uint8_t* mask_dev, uint64_t seed, void* stream);

/* Replaces RobotTaskEnv.step (core.py:303-317) + TimeLimit (UR_gym/__init__.py:41) for all N envs.
 * actions_dev: float32 [N][6] row-major, clipped to [-1,1] inside (UR5.py:274-275). */
int urgym_step(void* handle, const float* actions_dev, void* stream);

/* K consecutive urgym_step calls enqueued back to back: actions_dev is [K][N][6]. */
int urgym_rollout(void* handle, const float* actions_dev, int num_steps, void* stream);

/* ---- ABI v4: a policy in the loop (the reference's model_test.py:26-61 evaluates a stable-baselines3 SAC checkpoint with
 * model.predict(obs, deterministic=True) between env.step calls; here actor and environment stay on the device) ---- */

/* The deterministic SAC actor of SB3's MultiInputPolicy as model_test.py:21 loads it (SAC.load): features = the Dict observation
 * concatenated in sorted key order achieved_goal | desired_goal | observation, latent_pi = Linear-ReLU-Linear-ReLU, mu = Linear,
 * action = tanh(mu).  All six arrays are HOST pointers, float32, torch's [out][in] row-major layout; they are copied (re-packed for
 * the kernel) by urgym_actor_create and not kept.  Supported: hidden_width a multiple of 32, at most 512; in_features = obs_dim +
 * 2 * goal_dim of the handle's env kind; action_dim = 6. */
typedef struct urgym_actor_desc {
  int32_t in_features;  /* 30 | 32 | 41 | 47 (Ori | Obs | Sta | Dyn) */
  int32_t hidden_width; /* width of both hidden layers (256 in the shipped checkpoints) */
  int32_t action_dim;   /* 6 (UR5.py:251) */
  int32_t reserved0;    /* must be 0 */
  const float* w0;      /* latent_pi.0.weight [hidden_width][in_features] */
  const float* b0;      /* latent_pi.0.bias   [hidden_width] */
  const float* w1;      /* latent_pi.2.weight [hidden_width][hidden_width] */
  const float* b1;      /* latent_pi.2.bias   [hidden_width] */
  const float* w_mu;    /* mu.weight [action_dim][hidden_width] */
  const float* b_mu;    /* mu.bias   [action_dim] */
} urgym_actor_desc;

/* What urgym_rollout_actor records: DEVICE pointers owned by the caller, each may be NULL (= not recorded).  K = num_steps.
 * Step k's row of the first four is what the actor saw before step k and what it answered; of the next six, what step k returned
 * (RobotTaskEnv.step, core.py:303-317; the replay buffer rows train.py's SAC collects).  The episode summary is the bookkeeping
 * of model_test.py:38-50 for the FIRST episode of every env within the call. */
typedef struct urgym_trajectory {
  float* observation;       /* [K][N][obs_dim]  */
  float* achieved_goal;     /* [K][N][goal_dim] */
  float* desired_goal;      /* [K][N][goal_dim] */
  float* action;            /* [K][N][6] */
  float* reward;            /* [K][N] */
  uint8_t* terminated;      /* [K][N] */
  uint8_t* truncated;       /* [K][N] */
  uint8_t* is_success;      /* [K][N] */
  uint8_t* collision;       /* [K][N] */
  float* final_observation; /* [K][N][obs_dim]: rows written where terminated | truncated, only with auto_reset */
  double* episode_return;   /* [N] sum of the rewards up to and including the env's first terminated step, or step K - 1 */
  int32_t* episode_last_step; /* [N] index of that step (model_test.py:46-49) */
  uint8_t* episode_success; /* [N] info["is_success"] of that step */
  uint8_t* episode_done;    /* [N] 1 once the three above are final (every env after a complete call) */
} urgym_trajectory;

/* Replaces SAC.load (model_test.py:21) for the actor: checks the shape, uploads the weights.  The actor belongs to the handle
 * (urgym_destroy releases the ones still alive) and may be used with it until urgym_actor_destroy. */
int urgym_actor_create(void* handle, const urgym_actor_desc* desc, void** actor);
int urgym_actor_destroy(void* handle, void* actor);

/* Replaces model.predict(observation, deterministic=True) (model_test.py:41) for all N envs: one forward pass from the bound
 * observation / achieved_goal / desired_goal buffers into actions_dev, float32 [N][6]. */
int urgym_actor_forward(void* handle, void* actor, float* actions_dev, void* stream);

/* Replaces the loop of model_test.py:38-50 (predict, step, bookkeeping): enqueues num_steps x (forward pass + records, step) and a
 * last record pass on `stream`.  No host synchronisation and no allocation; everything is validated before the first launch.
 * Afterwards the bound buffers hold what num_steps calls of urgym_step would have left.  traj may be NULL.  Needs observations:
 * urgym_reset or urgym_refresh must have run on this binding. */
int urgym_rollout_actor(void* handle, void* actor, int num_steps, const urgym_trajectory* traj, void* stream);

/* ---- the stochastic half of the SAC policy (train.py: SAC("MultiInputPolicy", env, ...).learn collects experience with sampled
 * actions, SB3's SquashedDiagGaussianDistribution; before learning_starts with uniform ones).  Added WITHIN ABI version 4: no
 * struct above changed and URGYM_ABI_VERSION did not move, so a caller that may meet an older version-4 library finds
 * urgym_actor_set_log_std / urgym_actor_sample / urgym_rollout_sampled by symbol lookup (dlsym) and does without them if absent.
 *
 * With h = latent_pi(x) of one env:
 *   mu = W_mu h + b_mu,  log_std = min(max(W_ls h + b_ls, -20), 2)  (SB3's LOG_STD_MIN / LOG_STD_MAX),
 *   pre = mu + exp(log_std) eps,  action = tanh(pre),
 *   log_prob = sum_j [-eps_j^2 / 2 - log_std_j - log(2 pi) / 2] - sum_j log(1 - action_j^2 + 1e-6),
 * the second sum being SB3's squash correction (epsilon = 1e-6) of the float32 action.  Everything is float32.
 *
 * The noise is a pure function of (seed, draw, env, component); the library keeps no random-number state.
 *   Philox4x32-10 (Salmon et al., SC'11; the generator of the reset sampler), key = (seed & 0xFFFFFFFF, seed >> 32),
 *   counter = (env, draw & 0xFFFFFFFF, draw >> 32, 0x504F4C00 | block), block = 0, 1.  The reset sampler's counters end in a block
 *   number 0..4, so the two never meet, whatever the seeds.  Block 0 gives the words w0 w1 w2 w3, block 1 gives w4 w5 w6 w7
 *   (w6, w7 are not used).  For a word w, m(w) = w >> 8 is a 24-bit integer and converts to float32 exactly.
 *   UNIFORM   u_j = m(w_j) * 2^-24 in [0, 1), j = 0..5;  action_j = 2 u_j - 1 (exact in float32);  log_prob = -6 log 2, the density
 *             of the uniform distribution on [-1, 1]^6.  There is no forward pass: mean_action and log_std are not written.
 *   GAUSSIAN  Box-Muller on the pairs p = 0, 1, 2:  u1 = (m(w_2p) + 1) * 2^-24 in (0, 1],  u2 = m(w_2p+1) * 2^-24 in [0, 1),
 *             r = sqrt(-2 ln u1),  eps_2p = r cos(2 pi u2),  eps_2p+1 = r sin(2 pi u2).  u1 and u2 are exact; ln, sqrt, cos and sin
 *             are the float32 functions of whoever evaluates them, so two implementations agree to their rounding, not bitwise.
 *   MEAN      eps = 0: action = tanh(mu), bitwise what urgym_actor_forward / urgym_rollout_actor give; log_prob is the formula
 *             above at eps = 0.
 * Pass k of a rollout uses draw = first_draw + k: K steps in one call and the same K steps in two calls (the second with
 * first_draw advanced) draw the same noise, and the noise depends neither on N nor on the launch geometry. */
enum { URGYM_SAMPLE_MEAN = 0, URGYM_SAMPLE_GAUSSIAN = 1, URGYM_SAMPLE_UNIFORM = 2 };

typedef struct urgym_sampling {
  int32_t mode;        /* URGYM_SAMPLE_* */
  int32_t reserved0;   /* must be 0 */
  uint64_t seed;       /* the Philox key */
  uint64_t first_draw; /* draw index of the (first) pass */
} urgym_sampling;

/* What urgym_rollout_sampled records beyond urgym_trajectory: DEVICE pointers owned by the caller, each may be NULL.
 * K = num_steps; row k belongs to the action of step k.  MEAN and GAUSSIAN need the log_std head for any of them. */
typedef struct urgym_sample_records {
  float* log_prob;    /* [K][N] */
  float* noise;       /* [K][N][6] eps (GAUSSIAN), u (UNIFORM), 0 (MEAN) */
  float* mean_action; /* [K][N][6] tanh(mu); not written by UNIFORM */
  float* log_std;     /* [K][N][6] after the clamp; not written by UNIFORM */
} urgym_sample_records;

/* Attaches (or replaces) the log_std head of an actor: actor.log_std.weight [6][hidden_width] and actor.log_std.bias [6] of the
 * checkpoint, HOST pointers, float32, copied during the call.  Synchronises the device (launches may be reading the old head).
 * urgym_actor_load replaces the head from DEVICE pointers in stream order, without the synchronisation. */
int urgym_actor_set_log_std(void* handle, void* actor, const float* w_log_std, const float* b_log_std);

/* Replaces model.predict(observation, deterministic=False) / SAC's _sample_action for all N envs: one launch from the bound
 * observation buffers into actions_dev, float32 [N][6], with draw = how->first_draw.  log_prob_dev, float32 [N], may be NULL.
 * Refused: how == NULL, an unknown mode, reserved0 != 0, GAUSSIAN (or MEAN with log_prob_dev) on an actor without log_std head. */
int urgym_actor_sample(void* handle, void* actor, const urgym_sampling* how, float* actions_dev, float* log_prob_dev, void* stream);

/* urgym_rollout_actor with sampled actions: the same contract (no host synchronisation, no allocation, everything validated
 * before the first launch; traj and extra may be NULL) and the same refusals as urgym_actor_sample.  The sample records ride in
 * the actor launch like the others.  With mode MEAN and no sample records this IS urgym_rollout_actor: the call is forwarded after
 * the checks above, so an error met later (a HIP error of a launch) carries that name in urgym_last_error. */
int urgym_rollout_sampled(void* handle, void* actor, const urgym_sampling* how, int num_steps, const urgym_trajectory* traj,
                          const urgym_sample_records* extra, void* stream);

/* ---- the critics of the SAC agent (train.py:40-48: SAC("MultiInputPolicy", env, gamma=0.95, batch_size=256); SB3's ContinuousCritic
 * holds two Q-networks qf0, qf1, each Linear-ReLU-Linear-ReLU-Linear on cat([features, action]), features = achieved_goal |
 * desired_goal | observation as for the actor).  Added WITHIN ABI version 4 like the sampling calls: no struct above changed,
 * URGYM_ABI_VERSION did not move, the new symbols (urgym_critic_create / _destroy / _evaluate, urgym_actor_sample_rows) are found by
 * lookup.  Inference only: no gradients, no optimiser; the Polyak update of a target critic is urgym_critic_load, further down.
 *
 * For row m, with x = achieved_goal[m] | desired_goal[m] | observation[m] | action[m], everything float32:
 *   q_i     = w_q,i . relu(W1,i relu(W0,i x + b0,i) + b1,i) + b_q,i,   i = 0, 1
 *   q_min   = fminf(q_0, q_1)
 *   v       = log_prob ? q_min - (ent_coef * log_prob[m]) : q_min
 *   target  = reward[m] + ((gamma * nd) * v),   nd = (terminated && terminated[m]) ? 0.0f : 1.0f
 * -- SAC's y = r + gamma (1 - done) (min_i Q_i(s', a') - alpha log pi(a'|s')).  In q_min, v and target every operation is one float32
 * operation rounded on its own, in the association the parentheses show (no fused multiply-add), so a float32 restatement of these
 * three lines is bitwise given q_0, q_1.  The sums of q_i are float32 fused-multiply-add chains in the kernel's own order: two
 * implementations agree to rounding, and bitwise where every partial sum is exact.  A row's result depends on nothing but the row:
 * not on count, not on the row's position, not on the launch geometry. */

/* One Q-network: HOST pointers, float32, torch's [out][in] row-major layout; copied (re-packed) by urgym_critic_create, not kept. */
typedef struct urgym_q_network {
  const float* w0;  /* qf{i}.0.weight [hidden_width][in_features] */
  const float* b0;  /* qf{i}.0.bias   [hidden_width] */
  const float* w1;  /* qf{i}.2.weight [hidden_width][hidden_width] */
  const float* b1;  /* qf{i}.2.bias   [hidden_width] */
  const float* w_q; /* qf{i}.4.weight [1][hidden_width] */
  const float* b_q; /* qf{i}.4.bias   [1] */
} urgym_q_network;

/* Supported: hidden_width a multiple of 32, at most 512; in_features = obs_dim + 2 * goal_dim + 6 of the handle's env kind. */
typedef struct urgym_critic_desc {
  int32_t in_features;  /* 36 | 38 | 47 | 53 (Ori | Obs | Sta | Dyn) */
  int32_t hidden_width; /* width of both hidden layers of both networks (256 in the shipped checkpoints) */
  int32_t n_critics;    /* must be 2 */
  int32_t reserved0;    /* must be 0 */
  urgym_q_network qf[2];
} urgym_critic_desc;

/* The rows an evaluation reads: DEVICE pointers, float32 row-major, `count` rows each.  observation == NULL means the handle's bound
 * observation / achieved_goal / desired_goal buffers (then count must be num_envs, and achieved_goal / desired_goal are ignored). */
typedef struct urgym_critic_rows {
  const float* observation;   /* [count][obs_dim] or NULL */
  const float* achieved_goal; /* [count][goal_dim] */
  const float* desired_goal;  /* [count][goal_dim] */
  const float* action;        /* [count][6]; always given to urgym_critic_evaluate, ignored by urgym_actor_sample_rows */
} urgym_critic_rows;

/* The terms of the SAC target: DEVICE pointers, each may be NULL. */
typedef struct urgym_critic_terms {
  const float* reward;       /* [count]; needed for target */
  const uint8_t* terminated; /* [count]; NULL = no row is terminal */
  const float* log_prob;     /* [count]; NULL = no entropy term */
  float gamma;               /* 0.95 in the shipped checkpoints */
  float ent_coef;            /* alpha = exp(log_ent_coef) */
} urgym_critic_terms;

/* What an evaluation writes: DEVICE pointers, each may be NULL, at least one is not. */
typedef struct urgym_critic_out {
  float* q;      /* [2][count] */
  float* q_min;  /* [count] */
  float* target; /* [count] */
} urgym_critic_out;

/* Checks the shapes, uploads the weights of both networks.  The critic belongs to the handle like an actor (urgym_destroy releases
 * the ones still alive).  Refused: NULL arguments or weight pointers, n_critics != 2, reserved0 != 0, an unsupported hidden_width,
 * in_features other than the env kind's. */
int urgym_critic_create(void* handle, const urgym_critic_desc* desc, void** critic);
int urgym_critic_destroy(void* handle, void* critic);

/* Both Q-networks on `count` rows in ONE launch on `stream`; a recorded trajectory [K][N] is K * N rows.  No allocation and no host
 * synchronisation; everything is validated before the launch.  terms may be NULL when no target is asked for.  Refused
 * (URGYM_ERR_ARG): NULL handle / critic / rows / out / rows->action, a critic of another handle, count <= 0, observation == NULL with
 * count != num_envs, observation given without achieved_goal and desired_goal, out->target without terms->reward, no output at all. */
int urgym_critic_evaluate(void* handle, void* critic, const urgym_critic_rows* rows, int count, const urgym_critic_terms* terms, const urgym_critic_out* out, void* stream);

/* ---- the action gradient of the critics (SAC's actor loss, mean(alpha log pi(a|s) - min_i Q_i(s, a)), needs d min_i Q_i / d a at
 * a = the policy's action and nothing else of the critic's backward pass).  Added WITHIN ABI version 4: no struct above changed,
 * URGYM_ABI_VERSION did not move, urgym_critic_action_gradient is found by lookup.
 *
 * For row m and network i, with z1 = W0,i x + b0,i and z2 = W1,i relu(z1) + b1,i the pre-activations of urgym_critic_evaluate's q_i:
 *   dq_da[i]  = W0,i[:, action columns]^T  D1  W1,i^T  D2  w_q,i,     D = diag(z > 0),   action columns = in_features - 6 .. in_features - 1
 *   dqmin_da  = dq_da[sel],   sel = (q_1 < q_0) ? 1 : 0 by this launch's own q
 * A pre-activation of exactly 0 has derivative 0 (torch's relu).  A tie q_0 == q_1 takes qf0; torch.min halves the gradient between
 * the two on an exact tie, a set of measure zero.  q and q_min are bitwise urgym_critic_evaluate's.  The sums are float32
 * fused-multiply-add chains in the kernel's own order: two implementations agree to rounding, and bitwise where every partial sum
 * is exact.  A row's result depends on nothing but the row. */

/* What the gradient call writes: DEVICE pointers, each may be NULL, at least one of the first two is not. */
typedef struct urgym_critic_grad_out {
  float* dq_da;    /* [2][count][6]  d q_i / d action */
  float* dqmin_da; /* [count][6]     dq_da[sel] */
  float* q;        /* [2][count] */
  float* q_min;    /* [count] */
} urgym_critic_grad_out;

/* ONE launch on `stream`; no allocation and no host synchronisation; everything is validated before the launch.  Refused
 * (URGYM_ERR_ARG): what urgym_critic_evaluate refuses about handle, critic, rows and count; out == NULL; dq_da == dqmin_da == NULL;
 * a critic with hidden_width above 256 (the gradient kernel is built for widths up to 256, the shipped checkpoints'). */
int urgym_critic_action_gradient(void* handle, void* critic, const urgym_critic_rows* rows, int count, const urgym_critic_grad_out* out, void* stream);

/* urgym_actor_sample on explicit rows (SAC draws a' ~ pi(.|s') on next-observation rows, which are not the bound buffers): actions_dev
 * float32 [count][6], log_prob_dev float32 [count] or NULL, draw = how->first_draw, and the `env` word of the noise counter is the row
 * index -- on copies of the bound buffers the result is bitwise urgym_actor_sample's.  rows->observation == NULL means the bound
 * buffers as above.  The refusals of urgym_actor_sample, and those of urgym_critic_evaluate that concern rows and count. */
int urgym_actor_sample_rows(void* handle, void* actor, const urgym_sampling* how, const urgym_critic_rows* rows, int count, float* actions_dev, float* log_prob_dev, void* stream);

/* ---- the replay buffer of the SAC agent (train.py:40-48: SAC(..., buffer_size=int(1e7), batch_size=256); SB3's DictReplayBuffer):
 * the transitions of a policy rollout written into a ring on the device as they happen, and minibatches drawn from it in the row
 * layout urgym_critic_rows takes.  Added WITHIN ABI version 4 like the sampling and critic calls: no struct above changed,
 * URGYM_ABI_VERSION did not move, the new symbols (urgym_rollout_collect, urgym_replay_sample) are found by lookup.  The library
 * allocates nothing and keeps no state: the ring, its cursor and its fill level are the caller's. */

/* The ring: DEVICE pointers owned by the caller, C = capacity_steps slots of N transitions each, every array [C][N][...].  All are
 * required except truncated and is_success (NULL = not kept).
 * `terminated` is the environment's own flag, NOT terminated | truncated: an episode that ends at the time limit is bootstrapped
 * through, target = r + gamma Q(s', a'), as stable-baselines3 does with handle_timeout_termination=True (SB3
 * common/buffers.py, ReplayBuffer.add / _get_samples: dones * (1 - timeouts)). */
typedef struct urgym_replay_ring {
  int32_t capacity_steps;     /* C > 0 */
  int32_t reserved0;          /* must be 0 */
  float* observation;         /* [C][N][obs_dim]  what the actor saw before the step */
  float* achieved_goal;       /* [C][N][goal_dim] */
  float* desired_goal;        /* [C][N][goal_dim] */
  float* action;              /* [C][N][6]        what it answered */
  float* reward;              /* [C][N]           what the step returned */
  float* next_observation;    /* [C][N][obs_dim]  final_* where auto_reset && (terminated | truncated), else the live rows after the step */
  float* next_achieved_goal;  /* [C][N][goal_dim] */
  float* next_desired_goal;   /* [C][N][goal_dim] */
  uint8_t* terminated;        /* [C][N] */
  uint8_t* truncated;         /* [C][N] or NULL */
  uint8_t* is_success;        /* [C][N] or NULL */
} urgym_replay_ring;

/* A minibatch: DEVICE pointers owned by the caller, `count` rows each, each may be NULL (= not gathered), at least one is not.
 * observation / achieved_goal / desired_goal / action are a urgym_critic_rows as they stand, the three next_* fields a second one. */
typedef struct urgym_replay_batch {
  float* observation;         /* [count][obs_dim]  */
  float* achieved_goal;       /* [count][goal_dim] */
  float* desired_goal;        /* [count][goal_dim] */
  float* action;              /* [count][6] */
  float* reward;              /* [count] */
  float* next_observation;    /* [count][obs_dim]  */
  float* next_achieved_goal;  /* [count][goal_dim] */
  float* next_desired_goal;   /* [count][goal_dim] */
  uint8_t* terminated;        /* [count] */
  uint8_t* truncated;         /* [count]; only from a ring that keeps it */
  uint8_t* is_success;        /* [count]; only from a ring that keeps it */
  int64_t* index;             /* [count] the flat ring entry slot * N + env the row came from */
} urgym_replay_batch;

/* urgym_rollout_sampled (all three modes, the same refusals) that writes the transition of step k, k = 0 .. num_steps - 1, into slot
 * (first_slot + k) % C of `ring`; num_steps may exceed C (later steps overwrite earlier ones).  Afterwards the bound buffers hold
 * what num_steps calls of urgym_step would have left.  Of step k and env n the slot holds: observation / achieved_goal / desired_goal
 * = what the actor saw before step k, action = what it answered, reward / terminated / truncated / is_success = what step k returned,
 * next_* = the three final_* rows where auto_reset && (terminated | truncated), else the three live rows after the step.  A slot is
 * complete when the call returns, and no launch writes into a slot other than those of the call's own steps.  3 num_steps + 1
 * launches on `stream` (store pass, actor, step; a last store pass); the actor writes its actions straight into the slot and the
 * step reads them there.  No host synchronisation, no allocation, everything validated before the first launch.
 * Refused (URGYM_ERR_ARG) beyond urgym_rollout_sampled's: ring == NULL, a NULL required pointer, capacity_steps <= 0, first_slot
 * outside [0, C), reserved0 != 0, num_steps <= 0. */
int urgym_rollout_collect(void* handle, void* actor, const urgym_sampling* how, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream);

/* Draws `count` rows with replacement, uniformly over the size = filled_steps * N entries of the slots (oldest_slot + j) % C,
 * j < filled_steps, in ONE gather launch on `stream`.  Entry e_i of row i is a pure function of (seed, draw, i, size):
 *   Philox4x32-10 (urgym_philox.h), key = (seed & 0xFFFFFFFF, seed >> 32) as for the policy noise,
 *   counter = (i, draw & 0xFFFFFFFF, draw >> 32, 0x52504C00) -- the last word meets neither the policy noise's 0x504F4C00 | block
 *   nor the reset sampler's blocks 0..4;  w = (w0 << 32) | w1;  e = (w * size) >> 64, the high half of the 128-bit product;
 *   slot = (oldest_slot + e / N) % C,  env = e % N,  index = slot * N + env.
 * It depends on nothing else: not on count, not on the launch geometry.  ur_gym_amd.evaluation.replay_indices restates it.
 * Refused (URGYM_ERR_ARG): the ring refusals of urgym_rollout_collect, filled_steps outside [1, C], oldest_slot outside [0, C),
 * count <= 0, batch == NULL or without any output, truncated / is_success asked from a ring that does not keep it. */
int urgym_replay_sample(void* handle, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, void* stream);

/* ---- refreshing weights from the device (train.py:40-60: SAC.learn alternates collection and gradient steps; after every step the
 * actor that collects and the TARGET critic that bootstraps must follow the learner's parameters, the target by SB3's
 * polyak_update with tau = 0.005).  A learner that keeps its parameters in torch hands them over as they lie: DEVICE pointers,
 * float32, torch's [out][in] row-major layout, 4-byte aligned (nothing more is assumed: a view into a larger allocation will do).
 * Added WITHIN ABI version 4 like the sampling, critic and replay calls: no struct above changed, URGYM_ABI_VERSION did not move,
 * the new symbols (urgym_actor_load, urgym_critic_load, urgym_actor_read_packed, urgym_critic_read_packed) are found by lookup.
 *
 * Each load is ONE launch on `stream`: no allocation, no host synchronisation, everything validated before the launch.  The source
 * tensors are read when the launch RUNS, not during the call: the caller keeps them alive until then and orders whatever writes
 * them before the load on `stream`.  Launches enqueued earlier on the same stream see the old weights, later ones the new.  A load
 * rewrites every float of the object's packed buffer, padding included (as +0.0f), so the buffer's content afterwards does not
 * depend on what it held before -- except where stated below (an absent log_std head; tau < 1). */

/* The tensors of an actor (urgym_actor_desc's six, then the head urgym_actor_set_log_std takes) as DEVICE pointers. */
typedef struct urgym_actor_params_dev {
  int32_t in_features;    /* must be the actor's */
  int32_t hidden_width;   /* must be the actor's */
  int32_t reserved0;      /* must be 0 */
  const float* w0;        /* latent_pi.0.weight [hidden_width][in_features] */
  const float* b0;        /* latent_pi.0.bias   [hidden_width] */
  const float* w1;        /* latent_pi.2.weight [hidden_width][hidden_width] */
  const float* b1;        /* latent_pi.2.bias   [hidden_width] */
  const float* w_mu;      /* mu.weight [6][hidden_width] */
  const float* b_mu;      /* mu.bias   [6] */
  const float* w_log_std; /* log_std.weight [6][hidden_width], or NULL together with b_log_std */
  const float* b_log_std; /* log_std.bias   [6], or NULL together with w_log_std */
} urgym_actor_params_dev;

/* One Q-network as DEVICE pointers (urgym_q_network's six). */
typedef struct urgym_q_network_dev {
  const float* w0;  /* qf{i}.0.weight [hidden_width][in_features] */
  const float* b0;  /* qf{i}.0.bias   [hidden_width] */
  const float* w1;  /* qf{i}.2.weight [hidden_width][hidden_width] */
  const float* b1;  /* qf{i}.2.bias   [hidden_width] */
  const float* w_q; /* qf{i}.4.weight [1][hidden_width] */
  const float* b_q; /* qf{i}.4.bias   [1] */
} urgym_q_network_dev;

typedef struct urgym_critic_params_dev {
  int32_t in_features;  /* must be the critic's */
  int32_t hidden_width; /* must be the critic's */
  int32_t reserved0;    /* must be 0 */
  urgym_q_network_dev qf[2];
} urgym_critic_params_dev;

/* Reloads an actor.  With w_log_std == b_log_std == NULL the floats of the log_std head are left untouched and whether the actor
 * has a head does not change; with both given the head is written and the actor has one from this launch on (GAUSSIAN calls
 * enqueued after the load are accepted).  Refused (URGYM_ERR_ARG; handle and actor stay usable, nothing is launched): NULL handle /
 * actor / params, an actor of another handle, a NULL required pointer, only one of the two log_std pointers, in_features or
 * hidden_width other than the actor's, reserved0 != 0. */
int urgym_actor_load(void* handle, void* actor, const urgym_actor_params_dev* params, void* stream);

/* Reloads both Q-networks of a critic, blending with what it holds: with omt = 1.0f - tau formed once in float32,
 *   tau == 1:   packed = src                              (the old value is not read: a load repairs a buffer that holds NaN)
 *   otherwise:  packed = (packed * omt) + (tau * src)     (SB3 polyak_update; tau = 0.005 in train.py's SAC)
 * each of the three operations one float32 operation rounded on its own (no fused multiply-add), for every float of the buffer;
 * padding stays +0.  ur_gym_amd.evaluation.polyak restates it.  Refused: as urgym_actor_load (every pointer of both networks is
 * required), and tau outside (0, 1] or not finite. */
int urgym_critic_load(void* handle, void* critic, const urgym_critic_params_dev* params, float tau, void* stream);

/* ---- the parameter gradients of the critics (SAC's critic loss, 0.5 (mse(q_0, y) + mse(q_1, y)), needs d loss / d parameters of
 * both Q-networks).  Added WITHIN ABI version 4: no struct above changed, URGYM_ABI_VERSION did not move, the new symbols
 * (urgym_critic_parameter_gradients, urgym_critic_parameter_gradients_workspace) are found by lookup.
 *
 * Per network i, with x[m] row m of urgym_critic_rows (features | action) and dq_i[m] = d loss / d q_i[m], everything float32:
 *   z1 = W0 x + b0    h1 = relu(z1)    z2 = W1 h1 + b1    h2 = relu(z2)    q = w_q . h2 + b_q
 *   d2[m] = dq[m] * w_q   where z2 > 0, else 0        d1[m] = (W1^T d2[m])   where z1 > 0, else 0
 *   g_wq = sum_m dq[m] h2[m]      g_bq = sum_m dq[m]
 *   g_W1 = sum_m d2[m] h1[m]^T    g_b1 = sum_m d2[m]
 *   g_W0 = sum_m d1[m] x[m]^T     g_b0 = sum_m d1[m]
 * The mask convention is urgym_critic_action_gradient's (a pre-activation of exactly 0, or NaN, has derivative 0) and q is bitwise
 * urgym_critic_evaluate's.  Unlike every call above the results SUM over the rows.  The sum runs in a fixed order that depends on
 * nothing but count (ur_gym_amd/csrc/urgym_critic_backward.hip states it): rows ascending within a split of 1024 rows, then the
 * splits ascending; no floating-point atomics; two calls on the same inputs give bitwise the same tensors.  Two sums are carried in
 * float64 and rounded to float32 once: g_bq within a split (a single scalar out of up to 1024 terms) and the addition of the splits.
 *
 * The upstream gradient: exactly one of `dq` and `target` is given.
 *   dq      DEVICE [2][count], used as it is.
 *   target  DEVICE [count], with `scale` (finite): dq_i[m] = (q_i[m] - target[m]) * scale, one float32 subtraction and one float32
 *           multiplication, each rounded on its own, with this call's own q.  scale = 1 / count gives SB3's critic loss above. */

/* Where the gradients go: DEVICE pointers, float32, torch's [out][in] row-major layout, 4-byte aligned -- a torch parameter's .grad
 * as it lies.  All twelve are required.  Every float of every tensor is written by every call. */
typedef struct urgym_q_network_grad {
  float* w0;  /* [hidden_width][in_features] */
  float* b0;  /* [hidden_width] */
  float* w1;  /* [hidden_width][hidden_width] */
  float* b1;  /* [hidden_width] */
  float* w_q; /* [1][hidden_width] */
  float* b_q; /* [1] */
} urgym_q_network_grad;

typedef struct urgym_critic_param_grads {
  urgym_q_network_grad qf[2];
  float* q; /* [2][count], or NULL */
} urgym_critic_param_grads;

#define URGYM_CRITIC_GRADIENTS_MAX_COUNT 65536

/* The size of the workspace a call with this critic and count needs, in bytes: the per-row quantities h1, h2, d2, d1 of both
 * networks, x, dq, and above 1024 rows the partial sums.  For hidden_width 256, in_features 53 and count 65,536 it is 592,970,240
 * bytes.  Refused: NULL handle / critic / bytes, a critic of another handle or wider than 256, count outside
 * [1, URGYM_CRITIC_GRADIENTS_MAX_COUNT]. */
int urgym_critic_parameter_gradients_workspace(void* handle, void* critic, int count, uint64_t* bytes);

/* TWO launches on `stream` up to 1024 rows (per row; the sums), THREE above (per row; the sums per split of 1024 rows; the splits
 * added up).  The caller owns the workspace (DEVICE, 16-byte aligned, at least the queried size): the library allocates nothing and
 * keeps no state between calls, every workspace float that is read was written earlier in the same call, and what the workspace or
 * the outputs held before does not matter.  No host synchronisation; everything is validated before the first launch.  Refused
 * (URGYM_ERR_ARG, nothing is launched): what urgym_critic_evaluate refuses about handle, critic, rows and count; a critic with
 * hidden_width above 256 (like urgym_critic_action_gradient); count above URGYM_CRITIC_GRADIENTS_MAX_COUNT; both or neither of dq
 * and target; target with a scale that is not finite; out == NULL or one of its twelve tensor pointers; workspace NULL, misaligned
 * or workspace_bytes below the queried size. */
int urgym_critic_parameter_gradients(void* handle, void* critic, const urgym_critic_rows* rows, int count, const float* dq, const float* target, float scale, const urgym_critic_param_grads* out, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- the parameter gradients of the actor (SAC's policy loss, mean(alpha log pi(a|s) - min_i Q_i(s, a)) with a = the policy's
 * reparameterised action, needs d loss / d parameters of the actor).  The mirror of urgym_critic_parameter_gradients.  Added WITHIN ABI
 * version 4: no struct above changed, URGYM_ABI_VERSION did not move, the new symbols (urgym_actor_parameter_gradients,
 * urgym_actor_parameter_gradients_workspace) are found by lookup.
 *
 * Per row m, with x[m] the row's features (achieved_goal | desired_goal | observation) and eps[m] the noise of (how->seed,
 * how->first_draw, env word = m) -- zeros in mode MEAN -- everything float32:
 *   z1 = W0 x + b0          h1 = relu(z1)
 *   z2 = W1 h1 + b1         h2 = relu(z2)
 *   mu = W_mu h2 + b_mu     r  = W_ls h2 + b_ls
 *   ls = min(max(r, -20), 2)
 *   pre = mu + exp(ls) eps  a  = tanh(pre)
 *   log_prob = sum_j [-eps_j^2 / 2 - ls_j - log(2 pi) / 2 - log(1 - a_j^2 + 1e-6)]
 * as "the stochastic half" above states it: `action` and `log_prob` of this call are bitwise what urgym_actor_sample_rows gives for
 * the same `how` and rows.
 *
 * The upstream gradient: exactly one of two forms is given in urgym_actor_upstream.
 *   HEADS   d_mu and d_log_std, DEVICE [count][6] each: the gradient of a loss with respect to mu and to the clamped log_std ls, used
 *           as they are.
 *   SAMPLE  d_action DEVICE [count][6] and d_log_prob DEVICE [count] (NULL means 0): the gradient with respect to this call's action
 *           and log_prob outputs.  The noise is a constant (the reparameterised gradient).  Per component, each line one float32
 *           operation rounded on its own (no fused multiply-add), in the association shown:
 *             p = a * a
 *             t = 1 - p
 *             c = (2 a) / (t + 1e-6f)            (IEEE division)
 *             A = d_action + (d_log_prob * c)
 *             d_pre = A * t
 *             d_mu = d_pre
 *             e = exp(ls) * eps                  (exp(ls) is the forward pass's own value)
 *             d_log_std = (d_pre * e) - d_log_prob
 * The clamp:  dr = d_log_std where -20 <= r <= 2, else 0 (both edges inclusive: torch.clamp's backward; a NaN r gives 0).
 * Backward, with the mask convention of the critics' gradients (a pre-activation of exactly 0, or NaN, has derivative 0):
 *   d_h2 = W_mu^T d_mu + W_ls^T dr
 *   d2   = d_h2 where z2 > 0, else 0
 *   d1   = W1^T d2 where z1 > 0, else 0
 * The sums over the rows, eight tensors in torch's [out][in] layout:
 *   g_W0  = sum_m d1 x^T       g_b0  = sum_m d1
 *   g_W1  = sum_m d2 h1^T      g_b1  = sum_m d2
 *   g_Wmu = sum_m d_mu h2^T    g_bmu = sum_m d_mu
 *   g_Wls = sum_m dr h2^T      g_bls = sum_m dr
 * in a fixed order that depends on nothing but count (ur_gym_amd/csrc/urgym_actor_backward.hip states it): rows ascending within a
 * split of 1024 rows, then the splits ascending; no floating-point atomics; two calls on the same inputs give bitwise the same
 * tensors.  Two kinds of sums are carried in float64 and rounded to float32 once: the twelve head-bias sums g_bmu, g_bls within a split,
 * and the addition of the splits.  Near tanh saturation 1 - a^2 has no relative accuracy in float32, in this or any implementation
 * of the SAMPLE form. */

/* The upstream gradient: DEVICE pointers.  SAMPLE form: d_action given, d_log_prob given or NULL, d_mu == d_log_std == NULL.  HEADS
 * form: d_mu and d_log_std given, d_action == d_log_prob == NULL. */
typedef struct urgym_actor_upstream {
  const float* d_action;   /* [count][6] */
  const float* d_log_prob; /* [count], or NULL: 0 */
  const float* d_mu;       /* [count][6] */
  const float* d_log_std;  /* [count][6], with respect to the clamped log_std */
} urgym_actor_upstream;

/* Where the gradients go: DEVICE pointers, float32, torch's [out][in] row-major layout, 4-byte aligned -- a torch parameter's .grad
 * as it lies; the eight tensors are named like urgym_actor_params_dev's and all required; every float of every tensor is written
 * by every call.  Then the optional per-row outputs, each may be NULL: feeding d_mu and d_log_std back in the HEADS form reproduces
 * the call. */
typedef struct urgym_actor_param_grads {
  float* w0;        /* [hidden_width][in_features] */
  float* b0;        /* [hidden_width] */
  float* w1;        /* [hidden_width][hidden_width] */
  float* b1;        /* [hidden_width] */
  float* w_mu;      /* [6][hidden_width] */
  float* b_mu;      /* [6] */
  float* w_log_std; /* [6][hidden_width] */
  float* b_log_std; /* [6] */
  float* action;    /* [count][6], or NULL */
  float* log_prob;  /* [count], or NULL */
  float* noise;     /* [count][6], or NULL: eps */
  float* log_std;   /* [count][6], or NULL: after the clamp */
  float* d_mu;      /* [count][6], or NULL */
  float* d_log_std; /* [count][6], or NULL: before the clamp derivative */
  float* std;       /* [count][6], or NULL: exp(ls) as the forward pass formed it, the factor of e in the SAMPLE form (the device's expf
                       and a host's float32 exp are different functions, each good to an ulp) */
} urgym_actor_param_grads;

#define URGYM_ACTOR_GRADIENTS_MAX_COUNT 65536

/* The size of the workspace a call with this actor and count needs, in bytes: the per-row quantities h1, h2, d2, d1, x, the twelve
 * head gradients, and above 1024 rows the partial sums.  For hidden_width 256, in_features 47 and count 65,536 it is 304,942,080
 * bytes.  Refused: NULL handle / actor / bytes, an actor of another handle, without a log_std head or wider than 256, count outside
 * [1, URGYM_ACTOR_GRADIENTS_MAX_COUNT]. */
int urgym_actor_parameter_gradients_workspace(void* handle, void* actor, int count, uint64_t* bytes);

/* TWO launches on `stream` up to 1024 rows (per row; the sums), THREE above (per row; the sums per split of 1024 rows; the splits
 * added up).  how: mode GAUSSIAN or MEAN, first_draw is the draw, and the noise counter's env word is the row index, as in
 * urgym_actor_sample_rows.  rows: a urgym_critic_rows whose action member is ignored; observation == NULL means the bound buffers.
 * The caller owns the workspace (DEVICE, 16-byte aligned, at least the queried size): the library allocates nothing and keeps no
 * state between calls, every workspace float that is read was written earlier in the same call, and what the workspace or the
 * outputs held before does not matter.  No host synchronisation; everything is validated before the first launch.  Refused
 * (URGYM_ERR_ARG, nothing is launched): what urgym_actor_sample_rows refuses about handle, actor, how, rows and count; mode UNIFORM;
 * an actor without a log_std head; an actor with hidden_width above 256 (the same cap as the critic's gradients: the per-row kernel is
 * built for widths up to 256, the shipped checkpoints'); count above URGYM_ACTOR_GRADIENTS_MAX_COUNT; upstream == NULL, both forms,
 * neither, or a half-given HEADS form; out == NULL or one of its eight tensor pointers; workspace NULL, misaligned or workspace_bytes
 * below the queried size. */
int urgym_actor_parameter_gradients(void* handle, void* actor, const urgym_sampling* how, const urgym_critic_rows* rows, int count, const urgym_actor_upstream* upstream, const urgym_actor_param_grads* out, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- Adam on the device (train.py's SAC keeps SB3's optimiser: torch.optim.Adam with betas (0.9, 0.999), eps 1e-8, no weight decay,
 * no amsgrad).  After the gradient calls above have written a network's gradients, ONE launch steps its parameters in place and
 * writes the packed buffer the kernels read from the stepped values: what a learner otherwise does with optimizer.step() followed by
 * urgym_actor_load / urgym_critic_load.  Added WITHIN ABI version 4: no struct above changed, URGYM_ABI_VERSION did not move, the new
 * symbols (urgym_adam_coefficients, urgym_actor_adam_step, urgym_critic_adam_step) are found by lookup.
 *
 * The library keeps NO optimiser state: the caller owns the moment tensors and counts the steps.
 *
 * Per element, with the seven float32 coefficients of urgym_adam_coefficients, everything float32 and every line ONE operation rounded
 * on its own (no fused multiply-add; sqrt and / correctly rounded; subnormals kept):
 *   m' = (b1 * m) + (omb1 * g)
 *   gg = g * g          v' = (b2 * v) + (omb2 * gg)
 *   s  = sqrt(v')       d  = (s / bc2_sqrt) + eps
 *   u  = m' / d         p' = p - (step_size * u)
 * ur_gym_amd.evaluation.adam_step restates it.  (torch.optim.Adam computes the same quantities in another association -- lerp for m,
 * addcmul for v, addcdiv for p -- and agrees to rounding, not bitwise.) */

typedef struct urgym_adam_hyper {
  double lr;         /* finite, >= 0 */
  double beta1;      /* in [0, 1) */
  double beta2;      /* in [0, 1) */
  double eps;        /* finite, > 0 */
  int64_t step;      /* the 1-based index of THIS step, counted by the caller */
  int32_t reserved0; /* must be 0 */
} urgym_adam_hyper;

/* Host only, launches nothing: out = { b1, omb1, b2, omb2, step_size, bc2_sqrt, eps }, each computed in double and rounded to float32
 * once.  With corr1 = 1 - beta1^step and corr2 = 1 - beta2^step:
 *   b1 = beta1    omb1 = 1 - beta1    b2 = beta2    omb2 = 1 - beta2    step_size = lr / corr1    bc2_sqrt = sqrt(corr2)    eps = eps
 * The step calls below take their numbers from this function, so a restatement that calls it uses bit-identical coefficients whatever
 * pow the host's libm has.  Refused (URGYM_ERR_ARG): NULL hp or out, and what the step calls refuse about hp. */
int urgym_adam_coefficients(const urgym_adam_hyper* hp, float out[7]);

/* The eight tensors of an actor (urgym_actor_params_dev's) as DEVICE pointers that are written, and as ones that are only read. */
typedef struct urgym_actor_tensors {
  float* w0;        /* [hidden_width][in_features] */
  float* b0;        /* [hidden_width] */
  float* w1;        /* [hidden_width][hidden_width] */
  float* b1;        /* [hidden_width] */
  float* w_mu;      /* [6][hidden_width] */
  float* b_mu;      /* [6] */
  float* w_log_std; /* [6][hidden_width] */
  float* b_log_std; /* [6] */
} urgym_actor_tensors;

typedef struct urgym_actor_tensors_const {
  const float* w0;
  const float* b0;
  const float* w1;
  const float* b1;
  const float* w_mu;
  const float* b_mu;
  const float* w_log_std;
  const float* b_log_std;
} urgym_actor_tensors_const;

/* All 32 pointers are required (the learner's actor always has the log_std head): DEVICE, float32, torch's [out][in] layout, 4-byte
 * aligned.  The 32 tensors must not overlap one another: that is the caller's duty, nothing checks it. */
typedef struct urgym_actor_adam {
  int32_t in_features;  /* must be the actor's */
  int32_t hidden_width; /* must be the actor's */
  int32_t reserved0;    /* must be 0 */
  urgym_actor_tensors param;       /* read and written: p -> p' */
  urgym_actor_tensors_const grad;  /* read */
  urgym_actor_tensors exp_avg;     /* read and written: m -> m' */
  urgym_actor_tensors exp_avg_sq;  /* read and written: v -> v' */
} urgym_actor_adam;

/* The same for both Q-networks: 4 x 12 pointers, all required, none overlapping another. */
typedef struct urgym_critic_adam {
  int32_t in_features;  /* must be the critic's */
  int32_t hidden_width; /* must be the critic's */
  int32_t reserved0;    /* must be 0 */
  urgym_q_network_grad param[2];      /* read and written */
  urgym_q_network_dev grad[2];        /* read */
  urgym_q_network_grad exp_avg[2];    /* read and written */
  urgym_q_network_grad exp_avg_sq[2]; /* read and written */
} urgym_critic_adam;

/* Both calls: ONE launch on `stream`; no allocation, no host synchronisation, everything validated before the launch.  The tensors are
 * read and written when the launch RUNS: the caller keeps them alive until then and orders whatever writes the gradients before the
 * call on `stream`.  Launches enqueued earlier on the stream see the old weights, later ones the new.  Every parameter element is
 * stepped exactly once per call.  There is no width cap beyond what the objects accept (hidden_width up to 512).
 *
 * Refused by both (URGYM_ERR_ARG, nothing is launched, the objects stay usable): NULL handle / object / struct / hp; an object of
 * another handle; any NULL tensor pointer; in_features or hidden_width other than the object's; reserved0 != 0 (the struct's or hp's);
 * lr not finite or negative; beta1 or beta2 outside [0, 1); eps not finite or <= 0; step < 1. */

/* Steps the eight tensors of the actor in place (p', m', v') and writes every float of the actor's packed buffer from p': padding as
 * +0.0f, the log_std head included.  From this launch on the actor has a head, as with urgym_actor_load given both head pointers. */
int urgym_actor_adam_step(void* handle, void* actor, const urgym_actor_adam* t, const urgym_adam_hyper* hp, void* stream);

/* Steps the twelve tensors of both Q-networks in place and writes every float of `online`'s packed buffer from p'.  With target !=
 * NULL the same launch blends `target`'s packed buffer exactly as urgym_critic_load does: packed = (packed * omt) + (tau * p') with omt
 * = 1.0f - tau, three float32 operations each rounded on its own; at tau == 1 the old value is not read; padding stays +0.  `tau` is
 * ignored when target is NULL.  Refused besides the above: target == online; a target whose in_features or hidden_width differ from
 * online's; with a target, tau outside (0, 1] or not finite. */
int urgym_critic_adam_step(void* handle, void* online, void* target_or_NULL, const urgym_critic_adam* t, const urgym_adam_hyper* hp, float tau, void* stream);

/* ---- SAC's entropy coefficient on the device (SB3's ent_coef = "auto": log_ent_coef is a learned scalar, stepped by its own Adam,
 * and alpha = exp(log_ent_coef) of the value BEFORE the step is the coefficient of the whole update).  Two calls carry everything of a
 * SAC update that is neither a network pass nor a network's Adam step: alpha, the entropy term of the target, the temperature's loss
 * and step, the upstream gradients of urgym_actor_parameter_gradients, and the three loss values.  Added WITHIN ABI version 4: no
 * struct above changed, URGYM_ABI_VERSION did not move, the new symbols (urgym_sac_entropy_step, urgym_sac_policy_terms) are found by
 * lookup.  The library keeps NO state: the caller owns log_ent_coef and its two moments and counts the steps.
 *
 * Each call is ONE launch of ONE workgroup of 1024 lanes on `stream`: no allocation, no host synchronisation, everything validated
 * before the launch.  Every lane reads the scalar state before anything is written; lane t handles rows t, t + 1024, ..., reading a
 * row before it writes it.  count is at most URGYM_SAC_TERMS_MAX_COUNT (64 rows per lane).
 *
 * THE ORDERED SUM of `count` float32 terms, used by every reduction here, is carried in float64:
 *   lane t (0 <= t < 1024) starts at +0.0 and adds terms t, t + 1024, t + 2048, ... in ascending order;
 *   the 1024 partials are folded with partial[t] += partial[t + s] for s = 512, 256, ..., 1 (t < s);
 *   the result is S = partial[0].  A mean is (float)(S / (double)count), rounded once.
 * The order depends on nothing but count: two calls on the same inputs give the same bits.  There are no floating-point atomics.
 *
 * Everything else is float32 and every line below is ONE operation rounded on its own (no fused multiply-add; subnormals kept).
 * ur_gym_amd.evaluation.ordered_sum / entropy_step / policy_terms restate all of it. */
#define URGYM_SAC_TERMS_MAX_COUNT 65536

/* All pointers are DEVICE pointers, 4-byte aligned where float.  The state (log_ent_coef, exp_avg, exp_avg_sq) is stepped in place.
 * Two optional groups, each given whole or not at all:
 *   the TARGET group    target_in, next_log_prob, y_out (all three non-NULL), gamma, and terminated or NULL (= no row is terminal);
 *                       y_out == target_in is allowed
 *   the UPSTREAM group  d_log_prob_out (non-NULL) and scale */
typedef struct urgym_sac_entropy_args {
  int32_t count;         /* rows, in [1, URGYM_SAC_TERMS_MAX_COUNT] */
  int32_t reserved0;     /* must be 0 */
  float target_entropy;  /* finite */
  float gamma;           /* target group; finite */
  float scale;           /* upstream group; finite */
  const float* log_prob; /* [count], the policy's log-probability on the batch rows */
  float* log_ent_coef;   /* [1], read and written: l -> l' */
  float* exp_avg;        /* [1], read and written: m -> m' */
  float* exp_avg_sq;     /* [1], read and written: v -> v' */
  float* ent_coef_out;   /* [1], written: alpha */
  float* loss_out;       /* [1], written; or NULL */
  const float* target_in;      /* [count] */
  const float* next_log_prob;  /* [count] */
  const uint8_t* terminated;   /* [count], or NULL */
  float* y_out;                /* [count] */
  float* d_log_prob_out;       /* [count] */
} urgym_sac_entropy_args;

/* SB3's ent_coef_optimizer step plus every per-row use of alpha that is ready at that point of the update:
 *   l      = log_ent_coef[0]                      read before anything is written
 *   alpha  = expf(l)                              the device's expf (1 ulp); ent_coef_out[0] = alpha
 *   nd     = terminated && terminated[m] ? 0 : 1
 *   d      = gamma * nd      t = d * alpha      e = t * next_log_prob[m]      y_out[m] = target_in[m] - e
 *   d_log_prob_out[m] = alpha * scale
 *   s[m]   = log_prob[m] + target_entropy
 *   mean   = ordered mean of s                    float64 sum, rounded once
 *   g      = -mean                                d loss / d l
 *   loss   = -(l * mean)                          loss_out[0]
 *   (l', m', v') = the Adam element of the section above on (g, l, m, v) with urgym_adam_coefficients(hp)
 * alpha is the coefficient of the OLD l.  A NaN in one next_log_prob row reaches that row of y_out only; a NaN in log_prob reaches
 * l', m', v' and the loss, and no per-row output.  What the outputs held before the call does not matter.
 *
 * Refused (URGYM_ERR_ARG, nothing is launched, nothing is written): NULL handle or args; NULL log_prob, log_ent_coef, exp_avg,
 * exp_avg_sq or ent_coef_out; count outside [1, URGYM_SAC_TERMS_MAX_COUNT]; reserved0 != 0; target_entropy not finite; a half-given
 * target group (some but not all of target_in, next_log_prob, y_out; or terminated without them); gamma or scale not finite (also
 * where its group is absent: leave it 0); and what urgym_actor_adam_step refuses about hp. */
int urgym_sac_entropy_step(void* handle, const urgym_sac_entropy_args* args, const urgym_adam_hyper* hp, void* stream);

/* Three optional groups, each given whole (all three pointers) or not at all, at least one given:
 *   UPSTREAM     dqmin_da, d_action_out, scale     d_action_out may be dqmin_da itself
 *   CRITIC LOSS  q, y, critic_loss_out
 *   ACTOR LOSS   log_prob, q_min, actor_loss_out */
typedef struct urgym_sac_policy_args {
  int32_t count;     /* rows, in [1, URGYM_SAC_TERMS_MAX_COUNT] */
  int32_t reserved0; /* must be 0 */
  float scale;       /* upstream group; finite (a learner passes -1 / count) */
  const float* ent_coef;   /* [1], required: what urgym_sac_entropy_step wrote to ent_coef_out */
  const float* dqmin_da;   /* [count][6] */
  float* d_action_out;     /* [count][6] */
  const float* q;          /* [2][count] */
  const float* y;          /* [count] */
  float* critic_loss_out;  /* [1] */
  const float* log_prob;   /* [count] */
  const float* q_min;      /* [count] */
  float* actor_loss_out;   /* [1] */
} urgym_sac_policy_args;

/* What can only be formed after the critic's step and the action gradient:
 *   d_action_out[m][k] = dqmin_da[m][k] * scale
 *   e = q[i][m] - y[m]      sq = e * e      mean_i = ordered mean of sq      critic_loss_out[0] = 0.5f * (mean_0 + mean_1)
 *   alpha = ent_coef[0]     a = alpha * log_prob[m]      b = a - q_min[m]    actor_loss_out[0] = ordered mean of b
 *
 * Refused (URGYM_ERR_ARG, nothing is launched, nothing is written): NULL handle, args or ent_coef; count outside
 * [1, URGYM_SAC_TERMS_MAX_COUNT]; reserved0 != 0; a half-given group; no group at all; scale not finite (also where the upstream
 * group is absent: leave it 0). */
int urgym_sac_policy_terms(void* handle, const urgym_sac_policy_args* args, void* stream);

/* ---- behaviour cloning in the policy loss, with a Q-filter.  SAC's policy loss, alpha log pi - min Q, sees the
 * actions of the replay ring only through the critic; a learner fed by a planner or by demonstrations also wants a pull of the policy's
 * action towards the action the ring holds (TD3+BC, Fujimoto & Gu 2021; the Q-filter of Nair et al. 2018).  urgym_sac_policy_terms_cloned
 * is urgym_sac_policy_terms with that pull added to d_action_out: still ONE launch of ONE workgroup of 1024 lanes, in its place.  Added
 * WITHIN ABI version 4: no struct above changed, URGYM_ABI_VERSION did not move, the new symbols (urgym_sac_policy_terms_cloned,
 * urgym_sac_train_cloned) are found by lookup.  All pointers are DEVICE pointers, all required. */
typedef struct urgym_sac_clone_args {
  const float* action_pi;    /* [count][6], the policy's sampled, squashed action on the batch rows */
  const float* action_data;  /* [count][6], the action the replay ring holds for the row: the one that was executed */
  float weight;              /* finite, >= 0 */
  float bc_scale;            /* finite (a learner passes 1 / count) */
  int32_t scale_by_q;        /* 0 or 1 */
  int32_t q_filter;          /* 0 or 1 */
  float* bc_loss_out;        /* [1] */
  float* bc_weight_out;      /* [1] */
  int32_t* bc_rows_out;      /* [1] */
  int32_t reserved0;         /* must be 0 */
} urgym_sac_clone_args;

/* With q = args->q (the ONLINE critics at the REPLAYED action, [2][count]) and q_min = args->q_min (at the policy's action):
 *   phase 1, per row m (lane t takes rows t, t + 1024, ...):
 *     qd        = q[1][m] < q[0][m] ? q[1][m] : q[0][m]
 *     cloned[m] = q_filter ? (qd > q_min[m]) : true            a NaN on either side, or a tie, gives not cloned
 *     for k = 0..5 ascending:  d_k = action_pi[m][k] - action_data[m][k];  p = d_k * d_k;  s = s + p      (s starts at +0.0f)
 *     h[m]      = 0.5f * s where the row is cloned, +0.0f where it is not
 *     absq[m]   = fabsf(q_min[m])                              over ALL rows
 *     mean_abs  = ordered mean of absq      bc_loss = ordered mean of h over all count rows      rows = the number of cloned rows
 *     the three sums of urgym_sac_policy_terms are formed as there
 *   scalar:  w = scale_by_q ? weight * mean_abs : weight       one float32 product; mean_abs is a constant of the step (TD3+BC's
 *            normalisation written as a weight on the cloning term instead of 1 / lambda on Q: no division)
 *   phase 2, per element:
 *     g = dqmin_da[m][k] * scale                               urgym_sac_policy_terms' line
 *     not cloned:  d_action_out[m][k] = g                      bitwise what urgym_sac_policy_terms writes
 *     cloned:      t = d_k * w;  u = t * bc_scale;  d_action_out[m][k] = g + u
 *   The two actions are read again in phase 2; nothing per row is stored between the phases.  d_action_out may be dqmin_da itself.
 *   critic_loss_out and actor_loss_out are bitwise urgym_sac_policy_terms'; bc_loss_out[0] = bc_loss, bc_weight_out[0] = w,
 *   bc_rows_out[0] = rows.  With weight = 0 a cloned element is g + (+-0): equal to g, though a -0.0 g may become +0.0.
 * A NaN in action_pi or action_data of a cloned row reaches that row of d_action_out and bc_loss_out; a NaN in q_min reaches w only with
 * scale_by_q, and through w every cloned row; a row that is not cloned is touched by neither.
 *
 * Refused (URGYM_ERR_ARG, nothing is launched, nothing is written): everything urgym_sac_policy_terms refuses; any of its three groups
 * absent (this call needs all three); NULL clone args or any NULL pointer in them; weight not finite or < 0; bc_scale not finite;
 * scale_by_q or q_filter other than 0 or 1; reserved0 != 0; d_action_out equal to action_pi or action_data. */
int urgym_sac_policy_terms_cloned(void* handle, const urgym_sac_policy_args* args, const urgym_sac_clone_args* clone, void* stream);

/* ---- the SAC training loop in ONE call (train.py:40-60: model.learn(total_timesteps) alternates collection and gradient steps and
 * does not return to the caller in between).  urgym_sac_train enqueues num_iterations x (one collection, G updates) of the calls
 * above on `stream`: no new kernel, no new arithmetic, only the host side of the existing launches, checked once.  Added WITHIN ABI
 * version 4: no struct above changed, URGYM_ABI_VERSION did not move, urgym_sac_train is found by lookup.  The library keeps NO state:
 * the ring's cursor and fill level, the draw counters and the Adam step count are the caller's, handed in through the schedule. */

/* Where a call starts and how long it runs.  Iteration i (0 <= i < num_iterations), with K = steps_per_iteration, G =
 * updates_per_iteration and C = capacity_steps, as ur_gym_amd/csrc/urgym_sac_schedule.h derives it and
 * ur_gym_amd.evaluation.training_schedule restates it:
 *   collection   K steps from slot (first_slot + i K) % C with draws collect_first_draw + i K + k, k < K;
 *                mode URGYM_SAMPLE_UNIFORM for i < uniform_iterations, URGYM_SAMPLE_GAUSSIAN after; none where K == 0
 *   ring view    of its updates, after its collection: cursor = (first_slot + (i + 1) K) % C, filled = min(C, filled_steps + (i + 1) K),
 *                oldest_slot = (cursor - filled) mod C
 *   updates      none for i < idle_iterations, G otherwise; update u, counted over the whole call across the iterations that are not
 *                idle: gather draw = update_first_draw + u (urgym_replay_sample and a' ~ pi(.|s')), policy draw = the same | 2^63,
 *                Adam step = first_step + u, loss slot = u
 *   afterwards   the caller's cursor is (first_slot + num_iterations K) % C and its fill level min(C, filled_steps + num_iterations K)
 * Refused: num_iterations < 1; a negative count (K, G, uniform_iterations, idle_iterations); K and G both 0; capacity_steps <= 0 or
 * other than the ring's; first_slot outside [0, C); filled_steps outside [0, C] (0 is allowed: nothing collected yet); an update that
 * would see an empty ring (filled_steps == 0 with K == 0); first_step < 1, or first_step + the number of updates beyond int64;
 * update_first_draw + the number of updates > 2^63. */
typedef struct urgym_sac_schedule {
  int32_t first_slot;           /* the ring's cursor */
  int32_t filled_steps;         /* valid slots before the call */
  int32_t capacity_steps;       /* C, the ring's */
  int32_t num_iterations;       /* >= 1 */
  int32_t steps_per_iteration;  /* K >= 0 */
  int32_t updates_per_iteration; /* G >= 0 */
  int32_t uniform_iterations;   /* U: the first U iterations collect with URGYM_SAMPLE_UNIFORM */
  int32_t idle_iterations;      /* I: the first I iterations run no update */
  uint64_t collect_first_draw;  /* draw of the first collection pass */
  uint64_t update_first_draw;   /* draw of the first update */
  int64_t first_step;           /* 1-based Adam step of the first update */
} urgym_sac_schedule;

/* Everything the thirteen launches of an update and the collection take.  All pointers are DEVICE pointers owned by the caller (the
 * three objects excepted), float32 where float, `count` = M rows; all are required except batch.truncated, batch.is_success and
 * batch.index (and the three loss arrays of a call without an update).  The scratch is reused by every update of the call; no two tensors may overlap (not checked). */
typedef struct urgym_sac_learner {
  void* actor;   /* urgym_actor_create's, with its log_std head */
  void* online;  /* urgym_critic_create's: the critic that is stepped */
  void* target;  /* another critic of online's shape: bootstraps, follows by Polyak averaging */
  urgym_actor_adam actor_adam;    /* its grad tensors are the ones urgym_actor_parameter_gradients writes */
  urgym_critic_adam critic_adam;  /* its grad tensors are the ones urgym_critic_parameter_gradients writes */
  void* actor_workspace;          /* urgym_actor_parameter_gradients_workspace(actor, count) bytes at least, 16-byte aligned */
  uint64_t actor_workspace_bytes;
  void* critic_workspace;         /* urgym_critic_parameter_gradients_workspace(online, count) bytes at least, 16-byte aligned */
  uint64_t critic_workspace_bytes;
  float* log_ent_coef;            /* [1] the temperature's state, stepped in place */
  float* exp_avg;                 /* [1] */
  float* exp_avg_sq;              /* [1] */
  urgym_replay_ring ring;
  urgym_replay_batch batch;       /* [count] rows each: the minibatch */
  float* next_actions;            /* [count][6]  a' ~ pi(.|s') */
  float* next_log_prob;           /* [count] */
  float* target_value;            /* [count]     urgym_critic_evaluate's target of `target`, without the entropy term */
  float* y;                       /* [count]     urgym_sac_entropy_step's y_out */
  float* action_pi;               /* [count][6]  the policy's action on the batch rows */
  float* log_prob;                /* [count] */
  float* q;                       /* [2][count]  urgym_critic_parameter_gradients' q */
  float* q_min;                   /* [count]     urgym_critic_action_gradient's, at action_pi */
  float* dqmin_da;                /* [count][6] */
  float* d_action;                /* [count][6]  urgym_sac_policy_terms' d_action_out */
  float* d_log_prob;              /* [count]     urgym_sac_entropy_step's d_log_prob_out */
  float* ent_coef;                /* [1]         alpha of the running update */
  float* critic_loss;             /* [number of updates of the call]: update u writes slot u */
  float* actor_loss;              /* the same */
  float* ent_coef_loss;           /* the same */
  int32_t count;                  /* M, the batch size: in [1, 65536] */
  int32_t reserved0;              /* must be 0 */
  uint64_t seed;                  /* of the policy noise during collection */
  uint64_t update_seed;           /* of the gather and the two policy draws of an update */
  float gamma;                    /* finite */
  float tau;                      /* in (0, 1] */
  float target_entropy;           /* finite */
  double lr;                      /* urgym_adam_hyper without step: one set for the actor, the critics and the temperature */
  double beta1;
  double beta2;
  double eps;
} urgym_sac_learner;

/* Afterwards the bound buffers, the ring, every parameter, moment and packed buffer, the temperature state, the scratch and the loss
 * slots hold BIT FOR BIT what this sequence of the calls above would have left, per iteration:
 *   urgym_rollout_collect(actor, {mode, seed, draw}, K, ring, slot)                                       skipped where K == 0
 *   and for each update, in this order (the order of SACLearner._update_on_device), M = count:
 *     urgym_replay_sample(ring, oldest_slot, filled_steps, update_seed, gather draw, M, batch)
 *     urgym_actor_sample_rows(actor, {GAUSSIAN, update_seed, gather draw}, batch.next_*, M, next_actions, next_log_prob)
 *     urgym_critic_evaluate(target, batch.next_* with next_actions, M, {batch.reward, batch.terminated, next_log_prob, gamma,
 *                           ent_coef = 0}, {target = target_value})
 *     urgym_actor_sample_rows(actor, {GAUSSIAN, update_seed, policy draw}, the batch rows, M, action_pi, log_prob)
 *     urgym_sac_entropy_step({log_prob, the state, ent_coef, ent_coef_loss + u, target_value, next_log_prob, batch.terminated, y,
 *                            d_log_prob, scale = (float)(1.0 / M)}, hp)
 *     urgym_critic_parameter_gradients(online, the batch rows with batch.action, M, target = y, scale = (float)(1.0 / M),
 *                                      {critic_adam.grad, q}, critic_workspace)
 *     urgym_critic_adam_step(online, target, critic_adam, hp, tau)
 *     urgym_critic_action_gradient(online, the batch rows with action_pi, M, {dqmin_da, q_min})
 *     urgym_sac_policy_terms({ent_coef, dqmin_da, d_action, scale = (float)(-1.0 / M), q, y, critic_loss + u, log_prob, q_min,
 *                            actor_loss + u})
 *     urgym_actor_parameter_gradients(actor, {GAUSSIAN, update_seed, policy draw}, the batch rows, M, {d_action, d_log_prob},
 *                                     {actor_adam.grad}, actor_workspace)
 *     urgym_actor_adam_step(actor, actor_adam, hp)
 *   with hp = {lr, beta1, beta2, eps, step = the update's Adam step}; its coefficients are urgym_adam_coefficients'.
 * 3 K + 1 launches per collection and 13 per update (15 above 1024 rows), the launches of those calls and no other.
 *
 * EVERYTHING is validated before the first launch: the schedule's refusals above, every refusal of every call of the sequence, and
 * the call's own -- NULL handle, learner or schedule; a NULL required pointer; reserved0 != 0; online == target;
 * schedule->capacity_steps other than ring.capacity_steps.  The caps of the gradient kernels apply (hidden_width at most 256, count at
 * most 65536).  After a refusal (URGYM_ERR_ARG; URGYM_ERR_STATE before urgym_bind, or before the first reset where K > 0) nothing has
 * been launched and nothing written.  A call whose schedule holds no update (G == 0, or every iteration idle) composes no update call:
 * only the required pointers, the schedule and what its collections take are checked.
 * The call never allocates and never synchronises with the host.  It returns when everything is enqueued; where the stream's queue
 * is full the runtime may block the caller until launches drain.  If a launch fails midway (URGYM_ERR_HIP) the call has the semantics
 * of urgym_rollout_collect: launches already enqueued stay enqueued, and urgym_last_error names the iteration and the stage. */
int urgym_sac_train(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, void* stream);

/* ---- evaluation inside the training call (train.py:55-60 hands model.learn an EvalCallback, utils/callbackFunctions.py:429-518: at each
 * evaluation it plays the deterministic policy for whole episodes, reduces them to the mean and the standard deviation of the reward,
 * the mean episode length and the success rate, and saves best_model where the mean reward is STRICTLY above the best seen so far).
 * Here the statistics are reduced on the device in a fixed order, the decision is taken on the device, and the best actor's tensors are
 * copied on the device under that decision: a training call with evaluations never returns to the host.  Added WITHIN ABI version 4: no
 * struct above changed, URGYM_ABI_VERSION did not move, the five symbols below are found by lookup.
 *
 * THE STATISTICS of N episodes with returns r[n] (float64: urgym_trajectory.episode_return), last[n] (int32: episode_last_step) and
 * succ[n] (uint8: episode_success), every line ONE float64 operation rounded on its own (ur_gym_amd/csrc/urgym_eval.h states them,
 * ur_gym_amd.evaluation.evaluation_stats restates them):
 *   sum_r        = THE ORDERED SUM (above, "SAC's entropy coefficient on the device") of r[n]: lane t of 1024 starts at +0.0 and adds
 *                  r[t], r[t + 1024], ... in ascending order, then partial[t] += partial[t + s] for s = 512, ..., 1
 *   mean         = sum_r / (double)N
 *   d            = r[n] - mean;  term = d * d                   (the second pass, as np.std takes it; NOT E[r^2] - mean^2)
 *   sum_d2       = the ordered sum of the terms
 *   var          = sum_d2 / (double)N                           (the POPULATION variance: callbackFunctions.py:479 uses np.std's default)
 *   len_sum      = sum of (int64)last[n] + 1                    (exact; an episode's length is its step count, as SB3's evaluate_policy
 *                                                                counts it)
 *   mean_length  = (double)len_sum / (double)N
 *   successes    = the number of succ[n] != 0                   (int32)
 *   success_rate = (double)successes / (double)N
 *   improved     = mean > best_mean                             (strict, callbackFunctions.py:504; false for a NaN mean)
 *   where improved:  best_mean = mean, best_index = eval_index
 * The standard deviation is NOT computed on the device: a reader takes sqrt(var_return) on the host. */
typedef struct urgym_eval_record { /* one evaluation */
  double mean_return;
  double var_return;
  double mean_length;
  double success_rate;
  double best_mean_after; /* best_mean after the decision */
  int64_t eval_index;
  int64_t length_sum;
  int32_t successes;
  int32_t count;          /* N */
  int32_t improved;       /* 0 | 1: the flag urgym_actor_snapshot reads */
  int32_t reserved0;      /* written as 0 */
} urgym_eval_record;

/* DEVICE pointers, all required.  The best state starts where the caller puts it (-inf and -1 for "nothing seen yet"). */
typedef struct urgym_eval_stats_args {
  int32_t count;                    /* N in [1, URGYM_SAC_TERMS_MAX_COUNT] */
  int32_t reserved0;                /* must be 0 */
  int64_t eval_index;               /* >= 0 */
  const double* episode_return;     /* [N] */
  const int32_t* episode_last_step; /* [N] */
  const uint8_t* episode_success;   /* [N] */
  double* best_mean;                /* [1] read and written */
  int64_t* best_index;              /* [1] read and written */
  urgym_eval_record* record;        /* [1] written, 8-byte aligned */
} urgym_eval_stats_args;

/* ONE launch of ONE workgroup on `stream`: the record and the best state as stated above.  Needs no bound environment.  No allocation,
 * no host synchronisation, everything validated before the launch.  Refused (URGYM_ERR_ARG, nothing launched, nothing written): NULL
 * handle or args, a NULL pointer (named), reserved0 != 0, count outside [1, 65536], a negative eval_index. */
int urgym_eval_stats(void* handle, const urgym_eval_stats_args* args, void* stream);

typedef struct urgym_actor_snapshot_args {
  int32_t in_features;                /* of both sets of tensors: positive */
  int32_t hidden_width;               /* positive, at most 512 */
  urgym_actor_tensors_const source;   /* read; all eight required */
  urgym_actor_tensors destination;    /* written; all eight required; no tensor may overlap another (not checked) */
  const int32_t* when;                /* [1] DEVICE flag, or NULL = copy always */
  int32_t reserved0;                  /* must be 0 */
} urgym_actor_snapshot_args;

/* ONE launch on `stream`: destination = source, element for element, for all eight tensors -- or, where `when` is given and holds 0
 * when the launch RUNS, nothing at all.  Refused (URGYM_ERR_ARG): NULL handle or args, a NULL tensor pointer (all sixteen are
 * required), reserved0 != 0, in_features < 1, hidden_width outside [1, 512]. */
int urgym_actor_snapshot(void* handle, const urgym_actor_snapshot_args* args, void* stream);

/* One evaluation of `source` on an evaluation environment of its own.  All pointers but eval_actor are DEVICE pointers owned by the
 * caller, all required; N = the evaluation handle's num_envs. */
typedef struct urgym_policy_evaluation {
  void* eval_actor;                 /* urgym_actor_create's, of the EVALUATION handle, of the source's shape */
  int32_t in_features;              /* of the source and the best tensors */
  int32_t hidden_width;
  urgym_actor_tensors_const source; /* the parameters to evaluate, the log_std head included */
  urgym_actor_tensors best;         /* receives the source where the evaluation improved */
  double* episode_return;           /* [N] scratch: the rollout's episode summary */
  int32_t* episode_last_step;       /* [N] */
  uint8_t* episode_success;         /* [N] */
  uint8_t* episode_done;            /* [N] */
  urgym_eval_record* records;       /* [record_capacity] */
  double* best_mean;                /* [1] */
  int64_t* best_index;              /* [1] */
  uint64_t reset_seed;              /* every evaluation starts the SAME episodes: env.reset(seed=reset_seed) */
  int32_t record_capacity;          /* >= 1 */
  int32_t num_steps;                /* K >= 1 steps per evaluation */
  int32_t reserved0;                /* must be 0 */
} urgym_policy_evaluation;

/* Bit for bit this sequence on `stream`:
 *   1. urgym_actor_load(eval_handle, eval_actor, the source tensors with the head)
 *   2. env.reset(seed = reset_seed) on an environment that looks fresh: the bound episode_id and the bound observation zeroed by
 *      asynchronous memsets, then urgym_reset(eval_handle, NULL, reset_seed).  (urgym_reset leaves the velocity slot of the
 *      UR5DynReach-v1 observation as it finds it -- the reference's stale ReachDyn.velocity, reach.py:657 -- so a reset depends on
 *      the observation before it; zeroing it makes EVERY evaluation start from the observations the first one of a new handle sees, and
 *      two evaluations of the same parameters give the same record.  The other env kinds' resets overwrite the whole row.)
 *   3. urgym_rollout_actor(eval_handle, eval_actor, num_steps, {episode_return, episode_last_step, episode_success, episode_done})
 *   4. urgym_eval_stats({N, eval_index, the summary, the best state, &records[record_slot]})
 *   5. urgym_actor_snapshot({source -> best, when = &records[record_slot].improved})
 * Everything is validated before the first launch; no allocation, no host synchronisation.  Refused (URGYM_ERR_ARG; URGYM_ERR_STATE for
 * an evaluation handle without urgym_bind): every refusal of the five calls; a NULL handle, struct or pointer (named); reserved0 != 0;
 * num_steps < 1; an evaluation handle with auto_reset on (the summary is that of whole first episodes) or with more than 65536 envs; an
 * eval_actor of another handle, or of another shape than in_features -> hidden_width; record_slot outside [0, record_capacity); a
 * negative eval_index. */
int urgym_policy_evaluate(void* eval_handle, const urgym_policy_evaluation* evaluation, int64_t eval_index, int32_t record_slot, void* stream);

typedef struct urgym_sac_evaluation {
  void* eval_handle;                  /* a second handle on the training handle's device, NOT the training handle */
  urgym_policy_evaluation evaluation; /* its source tensors must be learner->actor_adam.param */
  int32_t every;                      /* E >= 1, in updates */
  int32_t first_record_slot;          /* the j-th evaluation of the call writes records[first_record_slot + j] ... */
  int64_t first_eval_index;           /* ... with eval_index = first_eval_index + j */
} urgym_sac_evaluation;

/* The launches of urgym_sac_train with evaluations between iterations.  With G = updates_per_iteration let
 *   s_i = first_step - 1 + G * (the number of iterations among 0..i that are not idle),   s_{-1} = first_step - 1
 * -- the Adam steps taken when iteration i ends.  An evaluation follows iteration i exactly where floor(s_i / E) > floor(s_{i-1} / E)
 * (ur_gym_amd/csrc/urgym_eval_schedule.h; ur_gym_amd.evaluation.evaluation_points restates it): the rule of a loop that evaluates
 * whenever the update count passes a multiple of E.  The result is bit for bit that of urgym_sac_train on the segments between the
 * evaluations plus urgym_policy_evaluate at each point; the training side is bit for bit that of urgym_sac_train alone, because an
 * evaluation writes nothing the training reads.
 * The reference hands EvalCallback the TRAINING env (train.py:55), so that each evaluation resets the env the collection runs on.  That
 * quirk is deliberately NOT reproduced: eval_handle == handle is refused.
 * EVERYTHING is validated before the first launch.  Refused, besides every refusal of urgym_sac_train and urgym_policy_evaluate: a NULL
 * evaluation or eval_handle; eval_handle == handle; the two handles on different devices; source tensors other than
 * learner->actor_adam.param; every < 1; a negative first_eval_index or first_record_slot; first_record_slot + the evaluations of the
 * call beyond record_capacity.  No allocation, no host synchronisation; a launch failure midway as in urgym_sac_train. */
int urgym_sac_train_evaluated(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_evaluation* evaluation, void* stream);

/* ---- training-episode statistics on the device (train.py:52 wraps the training env in Monitor(env, log_dir), and SB3 logs
 * rollout/ep_rew_mean, rollout/ep_len_mean and rollout/success_rate from it: the return, the length and info["is_success"] of the
 * episodes THE COLLECTING POLICY ITSELF finishes).  Every quantity is in the replay ring the collection has just written -- reward,
 * terminated, truncated, is_success -- so one launch follows the episodes of all N envs through the K slots of a collection, and one
 * launch of one workgroup reduces the finished episodes to a record; neither returns to the host.  Added WITHIN ABI version 4: no struct
 * above changed, URGYM_ABI_VERSION did not move, the three symbols below are found by lookup.  SB3 averages a window of the last 100
 * episodes; here a record covers the episodes finished since the last clear, whose number the record states.
 *
 * THE STATE: DEVICE pointers owned by the caller, [N] each, N = the handle's num_envs.  All zero is the valid initial state; the library
 * keeps none of it. */
typedef struct urgym_monitor_state {
  double* running_return;  /* [N] the episode in progress: its rewards so far */
  int32_t* running_length; /* [N] the episode in progress: its steps so far */
  double* sum_return;      /* [N] the episodes env n finished since the last clear: the sum of their returns */
  int64_t* sum_length;     /* [N] ... the sum of their lengths */
  int32_t* episodes;       /* [N] ... their number */
  int32_t* successes;      /* [N] ... those that ended with is_success != 0 */
} urgym_monitor_state;

/* THE FOLD of K = num_steps steps, per env n with the steps read IN ORDER, k = 0 .. K - 1, from slot (first_slot + k) % C of the ring --
 * the slots a urgym_rollout_collect with the same arguments has just filled.  Each line is ONE operation, in float64 where a float is
 * involved (ur_gym_amd/csrc/urgym_monitor.h states them, ur_gym_amd.evaluation.monitor_fold restates them):
 *   running_return += (double)reward
 *   running_length += 1
 *   where terminated | truncated is non-zero:
 *     sum_return += running_return;  sum_length += running_length;  episodes += 1;  successes += (is_success != 0)
 *     running_return = +0.0;  running_length = 0
 * An episode may span any number of calls: folding K steps in one call or in pieces leaves identical bits.
 * ONE launch on `stream`, one lane per env; no atomics, no allocation, no host synchronisation; everything validated before the launch.
 * Refused (URGYM_ERR_ARG, nothing launched, nothing written): NULL handle or state, a NULL state pointer (named), running_return /
 * sum_return / sum_length not 8-byte aligned; the ring refusals of urgym_rollout_collect (ring == NULL, a NULL required pointer,
 * capacity_steps <= 0, reserved0 != 0, first_slot outside [0, C)); a ring without truncated or without is_success; num_steps <= 0;
 * num_steps > C (the ring no longer holds the earlier steps); a handle with auto_reset off (its episodes do not restart). */
int urgym_monitor_fold(void* handle, const urgym_monitor_state* state, const urgym_replay_ring* ring, int first_slot, int num_steps, void* stream);

/* One record: the episodes finished since the last clear, over all N envs. */
typedef struct urgym_monitor_record {
  double mean_return;   /* rollout/ep_rew_mean */
  double mean_length;   /* rollout/ep_len_mean */
  double success_rate;  /* rollout/success_rate */
  double sum_return;    /* sum_r below */
  int64_t episodes;
  int64_t length_sum;
  int64_t successes;
  int64_t iteration;    /* the caller's tag */
  int64_t reserved0;    /* written as 0 */
} urgym_monitor_record;

/* THE RECORD, every line ONE operation (urgym_monitor.h states them, ur_gym_amd.evaluation.monitor_stats restates them):
 *   episodes, length_sum, successes = the exact int64 sums of episodes[n], sum_length[n], successes[n] over the N envs
 *   sum_r        = THE ORDERED SUM (above, "SAC's entropy coefficient on the device") of sum_return[0..N): lane t of 1024 starts at +0.0
 *                  and adds sum_return[t], sum_return[t + 1024], ... in ascending order -- ceil(N / 1024) terms per lane at the most,
 *                  whatever N the handle has -- then partial[t] += partial[t + s] for s = 512, ..., 1
 *   mean_return  = sum_r / (double)episodes
 *   mean_length  = (double)length_sum / (double)episodes
 *   success_rate = (double)successes / (double)episodes
 *   with episodes == 0 the three quotients are +0.0: no division produces a NaN, and a reader checks `episodes`.  (A NaN reward does
 *   reach sum_r and mean_return, for the interval its episode ends in.)
 * With clear != 0 each lane then zeroes the four interval entries (sum_return, sum_length, episodes, successes) it has read; an entry
 * belongs to exactly one lane.  The episode in progress (running_*) is untouched.
 * ONE launch of ONE workgroup on `stream`; no atomics, no allocation, no host synchronisation.  Refused (URGYM_ERR_ARG, nothing
 * launched, nothing written): NULL handle, state or record, a NULL state pointer (named), record / running_return / sum_return /
 * sum_length not 8-byte aligned. */
int urgym_monitor_stats(void* handle, const urgym_monitor_state* state, urgym_monitor_record* record, int64_t iteration, int clear, void* stream);

typedef struct urgym_sac_monitoring {
  urgym_monitor_state state;
  urgym_monitor_record* records; /* [record_capacity] */
  int32_t record_capacity;       /* >= 0 */
  int32_t first_record;          /* the j-th record of the call is records[first_record + j] */
  int32_t log_every;             /* E >= 1, in iterations */
  int32_t clear;                 /* urgym_monitor_stats' clear, for every record of the call */
  int64_t first_iteration;       /* >= 0: the caller's count of iterations before this call */
  int64_t reserved0;             /* must be 0 */
} urgym_sac_monitoring;

/* The launches of urgym_sac_train (evaluation == NULL) or of urgym_sac_train_evaluated (evaluation given), and added to them, with
 * K = steps_per_iteration:
 *   after the launches of each iteration i with K > 0 -- idle (warm-up) iterations like the others -- ONE urgym_monitor_fold of that
 *   iteration's K slots, first_slot = (schedule->first_slot + i K) % C;
 *   then, where (first_iteration + i + 1) % log_every == 0, ONE urgym_monitor_stats into the next record with
 *   iteration = first_iteration + i + 1 (ur_gym_amd/csrc/urgym_monitor.h; ur_gym_amd.evaluation.monitor_points restates the rule);
 *   then the evaluation that follows iteration i, if any.
 * Split calls that hand the iteration count on place records where one call would.  The training side and the evaluation are bit for bit
 * those of the call without monitoring: the two launches write the state and the records and nothing else.
 * EVERYTHING is validated before the first launch.  Refused, besides every refusal of the call without monitoring and of the two calls
 * above: NULL monitoring; K > C; more record points than record_capacity - first_record; a negative first_record; log_every < 1;
 * first_iteration < 0, or first_iteration + num_iterations beyond int64; reserved0 != 0.  After a refusal nothing has been launched or
 * written.  No allocation, no host synchronisation; a launch failure midway as in urgym_sac_train. */
int urgym_sac_train_monitored(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring, void* stream);

/* ---- multi-step (n-step) returns (stable-baselines3 offers them for SAC as n_steps=; one collection step writes N transitions that are
 * all one env step old, and a one-step target moves reward back through the ring one update per step).  The ring is [C][N][...]: an
 * env's consecutive steps sit N entries apart, and the ring keeps `truncated` and the terminal next_* rows a correct walk needs.
 * Added WITHIN ABI version 4: no struct above changed, URGYM_ABI_VERSION did not move, the new symbols (urgym_replay_sample_nstep,
 * urgym_sac_entropy_step_nstep, urgym_sac_train_nstep) are found by lookup.  n_steps = 1 is the calls above. */

#define URGYM_REPLAY_NSTEP_MAX 32

typedef struct urgym_replay_nstep {
  int32_t n_steps;     /* in [1, URGYM_REPLAY_NSTEP_MAX] */
  int32_t reserved0;   /* must be 0 */
  float gamma;         /* finite */
  float reserved1;     /* must be 0 */
  float* discount;     /* [count] required: gamma^m by repeated float32 products */
  int32_t* steps;      /* [count] or NULL: m */
  int64_t* last_index; /* [count] or NULL: the ring entry that next_* and the flags came from */
} urgym_replay_nstep;

/* urgym_replay_sample whose rows span up to n_steps consecutive steps of one env, in ONE gather launch on `stream`; no allocation, no
 * host synchronisation, everything validated before the launch.  The draw is urgym_replay_sample's, word for word: the same Philox
 * counter, the same e, and `index` bitwise the same.  For row i, with N the env count and C = capacity_steps:
 *   p = e / N (the age of the drawn slot, 0 = the oldest), env = e % N;
 *   L = min(n_steps, filled_steps - p): the window never runs past the newest valid slot;
 *   entry_k = ((oldest_slot + p + k) % C) * N + env for k < L;
 *   m = the smallest k + 1 with terminated[entry_k] | truncated[entry_k] non-zero, else L: the window never crosses an episode's end
 *   (with auto_reset the env's next slot belongs to another episode).
 * The return, in float32, each operation rounded on its own (ur_gym_amd/csrc/urgym_nstep.h; no product is fused into a sum):
 *   R = reward[entry_0], g = gamma;  for k = 1 .. m - 1:  t = g * reward[entry_k];  R = R + t;  g = g * gamma;
 *   batch.reward[i] = R, discount[i] = g (= gamma^m), steps[i] = m.
 * observation, achieved_goal, desired_goal, action and index come from entry_0; the three next_* rows, terminated, truncated,
 * is_success and last_index from entry_{m-1}.  At a truncation the next_* rows are therefore the ring's final_* rows and terminated
 * is the env's own flag, 0: the target bootstraps through, as the one-step ring does.  No entry at or past age filled_steps is read.
 * With n_steps == 1 every batch output is bitwise urgym_replay_sample's and discount[i] == gamma exactly.  A NaN reward reaches that
 * row's R and nothing else.  A row depends on (seed, draw, i) and the ring only: not on count, not on the launch geometry.
 * ur_gym_amd.evaluation.nstep_batch restates it.
 * Refused (URGYM_ERR_ARG, nothing launched, nothing written): everything urgym_replay_sample refuses; nstep == NULL; n_steps outside
 * [1, URGYM_REPLAY_NSTEP_MAX]; a non-zero reserved field; gamma not finite; discount == NULL; n_steps > 1 on a ring with
 * truncated == NULL (an episode's end at the time limit could not be seen). */
int urgym_replay_sample_nstep(void* handle, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, const urgym_replay_nstep* nstep, void* stream);

/* urgym_sac_entropy_args with the target group of a per-row discount: reward, q_min_next, discount, next_log_prob and y_out go
 * together (terminated only with them); everything else as in urgym_sac_entropy_args. */
typedef struct urgym_sac_entropy_nstep_args {
  int32_t count;              /* in [1, URGYM_SAC_TERMS_MAX_COUNT] */
  int32_t reserved0;          /* must be 0 */
  float target_entropy;       /* finite */
  float scale;                /* finite; the upstream group's factor */
  const float* log_prob;      /* [count] required */
  float* log_ent_coef;        /* [1] required, stepped in place */
  float* exp_avg;             /* [1] required */
  float* exp_avg_sq;          /* [1] required */
  float* ent_coef_out;        /* [1] required: alpha of the OLD log_ent_coef */
  float* loss_out;            /* [1] or NULL */
  const float* reward;        /* [count]: the multi-step return R */
  const float* q_min_next;    /* [count]: min_i Q_i'(s', a') on the rows of entry_{m-1} */
  const float* discount;      /* [count]: gamma^m */
  const float* next_log_prob; /* [count] */
  const uint8_t* terminated;  /* [count] or NULL (= none terminal) */
  float* y_out;               /* [count]; may be reward itself */
  float* d_log_prob_out;      /* [count] or NULL: alpha * scale */
} urgym_sac_entropy_nstep_args;

/* urgym_sac_entropy_step with another target group.  Per row m, float32, one operation per line (urgym_sac_terms.h,
 * sac_target_row_nstep):
 *   nd = terminated[m] ? 0 : 1;  d = discount[m] * nd;  a = d * q_min_next[m];  tv = reward[m] + a;  t = d * alpha;
 *   e = t * next_log_prob[m];  y_out[m] = tv - e.
 * Everything else is urgym_sac_entropy_step's: alpha = expf of the old log_ent_coef, THE ORDERED SUM in float64, the loss, the Adam
 * element, d_log_prob_out, ONE launch of one workgroup of 1024 lanes.  With discount[m] == gamma on every row, y_out is bitwise what
 * urgym_critic_evaluate(target, ent_coef = 0) followed by urgym_sac_entropy_step leave.  A non-finite next_log_prob[m] reaches y_out[m]
 * alone.  ur_gym_amd.evaluation.entropy_step_nstep restates it.  Refused: what urgym_sac_entropy_step refuses, with the new group given
 * whole or not at all. */
int urgym_sac_entropy_step_nstep(void* handle, const urgym_sac_entropy_nstep_args* args, const urgym_adam_hyper* hp, void* stream);

typedef struct urgym_sac_nstep {
  int32_t n_steps;   /* in [2, URGYM_REPLAY_NSTEP_MAX] */
  int32_t reserved0; /* must be 0 */
  float* discount;   /* [count] scratch */
  float* q_min_next; /* [count] scratch */
} urgym_sac_nstep;

/* The launches of urgym_sac_train_monitored, urgym_sac_train_evaluated or urgym_sac_train, according to which of the two arguments are
 * NULL, with two differences in each update: the gather is urgym_replay_sample_nstep(..., {n_steps, gamma = learner->gamma, discount})
 * and the third call is urgym_critic_evaluate(target, next rows) writing out.q_min = q_min_next with no terms, after which the entropy
 * step is urgym_sac_entropy_step_nstep(reward = batch.reward, q_min_next, discount, next_log_prob, terminated = batch.terminated, y).
 * Still 13 launches per update (15 above 1024 rows); learner->target_value is not written.  The schedule, the draws, the step numbers
 * and the loss slots are those of urgym_sac_train (ur_gym_amd/csrc/urgym_sac_schedule.h).  EVERYTHING is validated before the first
 * launch.  Refused besides what those calls refuse: nstep == NULL, n_steps outside [2, URGYM_REPLAY_NSTEP_MAX] (n_steps == 1 is the
 * calls above), reserved0 != 0, a NULL scratch pointer, a ring without truncated -- these also where the call holds no update. */
int urgym_sac_train_nstep(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_nstep* nstep, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- prioritized replay (Schaul et al., 2016, the proportional variant: one collection step writes N near-identical mid-episode
 * transitions, and the terminal rows that move the value function are a fraction of a percent of the ring).  A priority structure over
 * the ring's entries, the draw through it, the importance weights and the write-back of the new priorities, all on the device and all
 * deterministic: no floating-point atomics, every sum in a stated order (ur_gym_amd/csrc/urgym_per.h states every index and every
 * float operation; ur_gym_amd.evaluation.per_sums / per_descent / per_terms restate it).  Added WITHIN ABI version 4: no struct above
 * changed, URGYM_ABI_VERSION did not move, the new symbols (urgym_per_sums_count, urgym_per_rebuild, urgym_per_fill,
 * urgym_replay_sample_prioritized, urgym_per_terms, urgym_sac_train_prioritized) are found by lookup.  The library allocates nothing and keeps no state; everything
 * is validated before the first launch; no host synchronisation.  Whether prioritized replay learns a task faster is asserted nowhere.
 *
 * leaf[C N], float32, indexed by the flat ring entry slot * N + env (urgym_replay_batch.index): the priority ALREADY raised to alpha,
 * 0 = never drawn; an all-zero array is a valid empty structure.  sums: float64, fan-out URGYM_PER_FANOUT.  Entry b of level 1 is the
 * sum of leaves 256 b .. 256 b + 255 (those below C N; blocks straddle slots when N is no multiple of 256), ONE float64 addition per
 * leaf in ascending order starting from +0.0; level k + 1 is the same over level k; levels are added until one has at most 256
 * entries, and the TOTAL is the ascending sum of that level.  sums holds level 1, level 2, ..., then the total: urgym_per_sums_count
 * doubles.  max_leaf[1]: what a new transition gets; the caller sets it to 1.0f once. */

#define URGYM_PER_FANOUT 256
#define URGYM_PER_TERMS_MAX_COUNT 65536

typedef struct urgym_per_priorities {
  int32_t capacity_steps; /* C of the ring the leaves belong to */
  int32_t reserved0;      /* must be 0 */
  float* leaf;            /* [C][N] */
  double* sums;           /* [urgym_per_sums_count] */
  float* max_leaf;        /* [1] */
} urgym_per_priorities;

/* The length of `sums` for a ring of capacity_steps slots of this handle's N.  Refused: NULL handle / doubles, capacity_steps <= 0,
 * more than 2^31 - 1 level-1 entries. */
int urgym_per_sums_count(void* handle, int capacity_steps, uint64_t* doubles);

/* Forms every level and the total from the leaves as they lie.  TWO launches on `stream` (level 1: one workgroup per entry; every
 * level above and the total: one workgroup).  Refused: NULL handle / pri or one of its three pointers, capacity_steps <= 0,
 * reserved0 != 0. */
int urgym_per_rebuild(void* handle, const urgym_per_priorities* pri, void* stream);

/* The leaves of slots (first_slot + k) % C, k < num_steps, become max_leaf[0] (num_steps >= C: every leaf), and the sums are
 * repaired -- the level-1 entries that overlap those slots, then every level above -- to bitwise what urgym_per_rebuild would leave.
 * TWO launches (the first writes the leaves and forms the level-1 entries).  Refused beyond urgym_per_rebuild's: first_slot outside
 * [0, C), num_steps <= 0. */
int urgym_per_fill(void* handle, const urgym_per_priorities* pri, int first_slot, int num_steps, void* stream);

/* urgym_replay_sample with the entry of row i drawn in proportion to its leaf, in ONE launch (the descent, then the same gather):
 *   w = (w0 << 32) | w1 of Philox4x32-10 with urgym_replay_sample's key and the counter (i, draw lo, draw hi, 0x50455200) -- the last
 *   word meets none of the others (0x504F4C00 | block, 0x52504C00, the reset sampler's 0..4);
 *   u = (double)(w >> 11) * 2^-53;  t = u * total;  then from the top level down, over the children of the chosen node in ascending
 *   order with s = +0.0:  s2 = s + v[k];  if t < s2 take k and t = t - s, else s = s2;  v[k] = (double)leaf at the last level.
 *   If rounding lets no child be taken: the last child with v > 0, else the first (an all-zero structure yields entry 0).
 * A leaf of 0 is never drawn while any leaf is positive, so unfilled slots need no oldest_slot.  index[i] = the entry (batch->index
 * is REQUIRED here), leaf_out[i] = leaf[entry] (float32, [count]), total_out[0] = the total (float64); the other batch fields as
 * urgym_replay_sample gathers them.  A row depends on (seed, draw, i) and the structure only: not on count, not on the launch
 * geometry.  Refused: the ring refusals of urgym_replay_sample, count <= 0, batch == NULL, batch->index == NULL, truncated /
 * is_success asked from a ring that does not keep it, the refusals of urgym_per_rebuild about pri, pri->capacity_steps other than
 * the ring's, leaf_out or total_out NULL. */
int urgym_replay_sample_prioritized(void* handle, const urgym_replay_ring* ring, const urgym_per_priorities* pri, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, float* leaf_out, double* total_out, void* stream);

/* DEVICE pointers.  The write-back group -- index, new_leaf and the three pointers of `priorities` -- is given whole or not at all. */
typedef struct urgym_per_terms_args {
  int32_t count;          /* in [1, URGYM_PER_TERMS_MAX_COUNT] */
  int32_t reserved0;      /* must be 0 */
  float size;             /* filled_steps * N as float32; positive and finite */
  float beta;             /* in [0, 1] */
  float alpha;            /* in [0, 1] */
  float eps;              /* positive and finite */
  float scale;            /* finite; 1 / count gives SB3's critic loss */
  float reserved1;        /* must be 0 */
  const float* leaf_in;   /* [count] leaf_out of the draw */
  const double* total;    /* [1] total_out of the draw */
  const float* q;         /* [2][count] urgym_critic_evaluate's q of the batch rows */
  const float* y;         /* [count] the target */
  float* w_raw;           /* [count] */
  float* w;               /* [count] */
  float* dq;              /* [2][count] urgym_critic_parameter_gradients' dq */
  const int64_t* index;   /* [count] batch.index, or NULL */
  float* new_leaf;        /* [count], or NULL */
  urgym_per_priorities priorities; /* all three pointers NULL without the group */
} urgym_per_terms_args;

/* The importance weights, the weighted upstream gradient of the critics and the new priorities.  The per-row part is ONE launch of ONE
 * workgroup of 1024 lanes (the shape of urgym_sac_entropy_step).  Per row m, each line ONE float32 operation rounded on its own
 * unless marked:
 *   prob = (float)((double)leaf_in[m] / total[0])          (one float64 division, rounded to float32 once)
 *   x = size * prob
 *   w_raw[m] = powf(x, -beta)
 *   wmax = the maximum of 0 and every w_raw (fmaxf: order-independent; a NaN is passed over)
 *   w[m] = w_raw[m] / wmax
 *   e_i = q[i][m] - y[m];   g_i = e_i * scale;   dq[i][m] = g_i * w[m]
 *   td = fmaxf(|e_0|, |e_1|);   p = td + eps;   new_leaf[m] = powf(p, alpha)
 * A new_leaf that is not finite (a NaN q or y in the row) is replaced by max_leaf[0] as it stood before the call.  With w == 1 on
 * every row (beta = 0) dq is bitwise what urgym_critic_parameter_gradients forms from target = y and the same scale.  powf is the
 * device library's (OpenCL's table allows 16 ulp): w_raw and new_leaf are outputs, and a restatement takes them as inputs.
 * With the write-back group: leaf[index[m]] = new_leaf[m]; an entry drawn by several rows ends at the LARGEST of their values (the
 * entry is set to +0, then an integer maximum on the bit patterns of the non-negative floats: order-independent); an index outside
 * [0, C N) is passed over; max_leaf[0] = fmaxf(max_leaf[0], max_m new_leaf[m]); then the sums are repaired in TWO more launches (the
 * level-1 entries of the touched leaves -- every level-1 entry where count is at least their number --, then every level above) to
 * bitwise what urgym_per_rebuild would leave.  Without the group: one launch, nothing but w_raw, w and dq is written.
 * The critic loss urgym_sac_policy_terms reports stays the unweighted one.
 * Refused (URGYM_ERR_ARG, nothing launched, nothing written): NULL handle / args; count outside [1, URGYM_PER_TERMS_MAX_COUNT];
 * reserved0 or reserved1 != 0; a NULL required pointer; alpha or beta outside [0, 1] (NaN included); eps not positive and finite; size
 * not positive and finite; scale not finite; a half-given write-back group; with the group, priorities.capacity_steps <= 0 or its
 * reserved0 != 0. */
int urgym_per_terms(void* handle, const urgym_per_terms_args* args, void* stream);

/* The structure, the exponents, the beta schedule and the [count] scratch of urgym_sac_train_prioritized. */
typedef struct urgym_sac_prioritized {
  urgym_per_priorities priorities; /* of learner->ring: the same capacity_steps */
  double beta0;       /* in [0, 1] */
  int64_t beta_steps; /* >= 1 */
  float alpha;        /* in [0, 1] */
  float eps;          /* positive and finite */
  float* leaf;        /* [count] scratch: leaf_out of the draw */
  double* total;      /* [1] scratch: total_out of the draw */
  float* q;           /* [2][count] scratch: the online critics' q on the batch rows */
  float* w_raw;       /* [count] scratch */
  float* w;           /* [count] scratch */
  float* dq;          /* [2][count] scratch */
  float* new_leaf;    /* [count] scratch */
  int64_t reserved0;  /* must be 0 */
} urgym_sac_prioritized;

/* The launches of urgym_sac_train_monitored, urgym_sac_train_evaluated or urgym_sac_train, according to which of the two arguments are
 * NULL, with these differences.  After the collection of every iteration with steps_per_iteration > 0 (idle iterations too): ONE
 * urgym_per_fill on the slots just written.  In each update: the gather is urgym_replay_sample_prioritized (batch.index is required);
 * after the entropy step come urgym_critic_evaluate(online, the batch rows with batch.action) -> q and urgym_per_terms(leaf, total, q,
 * y, size = filled_steps * N of the iteration, beta, alpha, eps, scale = 1 / count, the write-back group); and
 * urgym_critic_parameter_gradients takes dq = instead of target =, its own q output bitwise the evaluate's.  beta of the update at Adam
 * step t is beta0 + (1 - beta0) min(1, t / beta_steps), formed in float64 and rounded to float32 once (per_beta of
 * ur_gym_amd/csrc/urgym_per.h; ur_gym_amd.evaluation.per_beta restates it).  17 launches per update (19 above 1024 rows) and 2 per
 * collection.  urgym_sac_policy_terms is unchanged: the critic loss reported is the UNWEIGHTED one.  The schedule, the draws, the
 * step numbers and the loss slots are those of urgym_sac_train.  Bit for bit that sequence of single calls.  EVERYTHING is validated
 * before the first launch.  Refused besides what those calls and the single calls refuse: prioritized == NULL, reserved0 != 0, a NULL
 * scratch pointer, beta0 outside [0, 1], beta_steps < 1, priorities.capacity_steps other than the ring's, batch.index == NULL --
 * these also where the call holds no update.  Multi-step returns together with priorities are out of scope (the multi-step gather
 * draws its own indices): there is no such call. */
int urgym_sac_train_prioritized(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_prioritized* prioritized, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- hindsight experience replay (SB3's HerReplayBuffer): a drawn transition gets, as its goal, a pose its own
 * episode reached at the same or a later step, and is re-scored against it.  The ring holds everything this needs (next_achieved_goal,
 * next_desired_goal, the three flags; consecutive steps of an env lie N entries apart), so nothing is collected differently and
 * nothing joins the ring or a checkpoint.  Added WITHIN ABI version 4: no struct above changed, URGYM_ABI_VERSION did not move, the
 * new symbols (urgym_replay_sample_hindsight, urgym_sac_train_hindsight) are found by lookup.  The rule, as
 * ur_gym_amd/csrc/urgym_her.h states it and ur_gym_amd.evaluation.hindsight_pick / hindsight_batch restate it, for row i:
 *
 * Draw.  The Philox word of urgym_replay_sample unchanged (same key, same counter, last word 0x52504C00): w[0], w[1] give e,
 * p = e / N, env and index exactly as there, batch.index is bitwise what urgym_replay_sample writes.  HER spends w[2] and w[3], which
 * that call leaves unused, and only them.
 * Relabel decision.  Relabel iff (uint64)w[2] < relabel_threshold, in [0, 2^32]; the host forms it with integers as
 * (n_sampled_goal << 32) / (n_sampled_goal + 1) (SB3's n_sampled_goal = 4: a ratio of 0.8).  A row that is not relabelled is bitwise
 * the row urgym_replay_sample gathers, in every output.
 * Episode window.  H = min(horizon, filled_steps - p), entry_k = ((oldest_slot + p + k) % C) N + env, F = the smallest k + 1 <= H with
 * terminated[entry_k] | truncated[entry_k] non-zero, else H.  No entry at or past age filled_steps is read.  An episode still in
 * progress ends, for this purpose, at the newest slot (SB3 samples finished episodes only; the multi-step window does the same as here).
 * Goal entry g = entry_j.  URGYM_HER_GOAL_FUTURE: j = ((uint64)w[3] F) >> 32 (SB3's `future`, own step included).
 * URGYM_HER_GOAL_FINAL: j = F - 1.  URGYM_HER_GOAL_OWN (a diagnostic): no entry; the "new" goal is next_desired_goal[e], so the whole
 * re-scoring path runs with the goal the row already had.  Otherwise the new goal is next_achieved_goal[g], goal_dim float32 words
 * copied bitwise.
 * Rows of a relabelled sample.  desired_goal and next_desired_goal become the new goal; observation and next_observation are the
 * ring's rows with floats [12, 12 + goal_dim) replaced by it (the goal lies there in all four env kinds); achieved_goal,
 * next_achieved_goal, action, truncated and index come from e unchanged; goal_index holds g, or -1 where the row was not relabelled or
 * the strategy is OWN.
 * Re-scoring, in float64 with every operation rounded on its own, the weights and thresholds being the handle's urgym_config:
 *   coll = terminated[e] && !is_success[e]; succ0 = is_success[e] (the stored flag); a = next_achieved_goal[e], g1 the new goal,
 *   g0 = next_desired_goal[e], each widened to double; d = distance(a, g1), th = angular_distance(a + 3, g1 + 3) for goal_dim == 6,
 *   else 0 (the step kernel's own functions); d0, th0 the same against g0; succ = d < distance_threshold, and for goal_dim == 6 also
 *   th < ori_threshold.
 *   Ori and Obs: G(s, d, th) = (((s ? w_success : 0) + (coll ? w_collision : 0)) + w_distance d) + w_orientation th, and
 *     r' = ((double)r - G(succ0, d0, th0)) + G(succ, d, th).
 *   Dyn and Sta: coll: r' = w_collision; else succ: r' = w_success; else r' = (w_distance d + w_orientation th) + S with
 *     S = ((double)r - w_distance d0) - w_orientation th0 if !succ0, else 0.
 *   batch.reward = (float)r', terminated' = succ || coll, is_success' = terminated' && !coll.
 * The bracketed remainder is the part of the stored reward that does not depend on the goal (the link-distance shaping; for Ori the
 * rounding residue of the float64 goal).  A NaN in a goal reaches that row's reward and nothing else.  pose_terms[i] = {d, th, d0,
 * th0} (zeros where the row was not relabelled): sincos and acos of the device library are restated bitwise by no host, so the
 * restatement takes them as inputs. */
#define URGYM_HER_HORIZON_MAX 256
#define URGYM_HER_GOAL_FUTURE 0
#define URGYM_HER_GOAL_FINAL 1
#define URGYM_HER_GOAL_OWN 2

typedef struct urgym_replay_hindsight {
  uint64_t relabel_threshold; /* in [0, 2^32]: 0 relabels no row, 2^32 every row */
  int32_t strategy;           /* URGYM_HER_GOAL_* */
  int32_t horizon;            /* in [1, URGYM_HER_HORIZON_MAX]: the env's max_episode_steps */
  int64_t* goal_index;        /* [count] or NULL */
  double* pose_terms;         /* [count][4] or NULL */
  int64_t reserved0;          /* must be 0 */
} urgym_replay_hindsight;

/* urgym_replay_sample with the rule above, in ONE launch on `stream`: no allocation, no host synchronisation.  Refused
 * (URGYM_ERR_ARG, nothing launched, nothing written): everything urgym_replay_sample refuses; hindsight == NULL; relabel_threshold >
 * 2^32; strategy outside 0..2; horizon outside [1, URGYM_HER_HORIZON_MAX]; a non-zero reserved field; a ring without truncated or
 * without is_success. */
int urgym_replay_sample_hindsight(void* handle, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, const urgym_replay_hindsight* hindsight, void* stream);

typedef struct urgym_sac_hindsight {
  uint64_t relabel_threshold; /* as urgym_replay_hindsight */
  int32_t strategy;           /* URGYM_HER_GOAL_FUTURE or URGYM_HER_GOAL_FINAL */
  int32_t horizon;
  int64_t reserved0;          /* must be 0 */
} urgym_sac_hindsight;

/* urgym_sac_train, urgym_sac_train_evaluated or urgym_sac_train_monitored -- by which of evaluation_or_NULL and monitoring_or_NULL is
 * given -- with the gather of each update replaced by urgym_replay_sample_hindsight(..., {relabel_threshold, strategy, horizon}):
 * still 13 launches per update (15 above 1024 rows), the same schedule, draws, step numbers and loss slots.  Everything is validated
 * before the first launch, also where the call holds no update.  Refused besides what those calls and the gather refuse: hindsight ==
 * NULL, URGYM_HER_GOAL_OWN (a diagnostic of the gather, not a way to train). */
int urgym_sac_train_hindsight(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_hindsight* hindsight, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- gradient-norm clipping on the device (torch.nn.utils.clip_grad_norm_, the usual torch idiom; SB3's SAC does NOT clip, so this
 * is an option the reference does not have).  The global norm of a network's gradient tensors is reduced on the device in a stated
 * order, the clip coefficient stays on the device, and the Adam steps apply it while they step.  Added WITHIN ABI version 4: no struct
 * above changed, URGYM_ABI_VERSION did not move, the new symbols (urgym_actor_grad_norm, urgym_critic_grad_norm,
 * urgym_actor_adam_step_scaled, urgym_critic_adam_step_scaled, urgym_sac_train_clipped) are found by lookup.
 *
 * A group is the gradient tensors of one optimiser in a FIXED order: the actor's 8 in the order of urgym_actor_tensors; or the 2 x 6
 * of both Q-networks, network 0 then network 1, each w0, b0, w1, b1, w_q, b_q (both networks are ONE group).  For tensor k:
 *   s_k    = THE ORDERED SUM (above, "SAC's entropy coefficient on the device": 1024 lanes, lane t adds elements t, t + 1024, ... in
 *            ascending order, fold 512 .. 1) over the tensor's flat elements of (double)g * (double)g -- exact in float64
 *   total  = ((s_0 + s_1) + s_2) + ...                    float64, tensor order
 *   norm64 = sqrt(total)                                  float64, correctly rounded
 *   c64    = (double)max_norm / (norm64 + 1e-6)           torch's formula
 *   scale  = c64 < 1.0 ? (float)c64 : 1.0f
 *   norm   = (float)norm64                                for the record only
 * The order depends on the tensors' shapes alone; there are no atomics.  ur_gym_amd.evaluation.grad_norm restates all of it, the
 * square root included (the device's is held bitwise to the host's correctly rounded one by the GPU tests).
 * UNLIKE torch the gradient tensors are NOT written: the scaled steps multiply each element as they read it, gs = g * scale, ONE
 * float32 multiply rounded on its own, and the element of urgym_actor_adam_step runs on gs unchanged.
 * Non-finite elements: a NaN makes c64 NaN, the comparison false and scale 1.0f -- the step is then what it is without clipping.  An
 * infinity (and no NaN) makes norm64 = +inf and scale = +0.0f: finite elements step with gs = +-0, the infinite ones with gs = NaN. */
typedef struct urgym_grad_norm {
  float max_norm;          /* finite, > 0 */
  int32_t reserved0;       /* must be 0 */
  float* norm_out;         /* [1] DEVICE */
  float* scale_out;        /* [1] DEVICE */
  double* tensor_sums_out; /* [8] (actor) or [12] (critics) DEVICE, 8-byte aligned; or NULL */
} urgym_grad_norm;

/* Both calls: ONE launch of ONE workgroup of 1024 lanes on `stream`; no allocation, no host synchronisation, everything validated
 * before the launch.  The gradient tensors (shapes: the object's) are read when the launch RUNS and are not written.  Refused
 * (URGYM_ERR_ARG, nothing launched, nothing written): NULL handle / object / grad / args; an object of another handle; a NULL tensor
 * pointer; a NULL norm_out or scale_out; tensor_sums_out not 8-byte aligned; reserved0 != 0; max_norm not finite or <= 0. */
int urgym_actor_grad_norm(void* handle, void* actor, const urgym_actor_tensors_const* grad, const urgym_grad_norm* args, void* stream);
int urgym_critic_grad_norm(void* handle, void* critic, const urgym_q_network_dev grad[2], const urgym_grad_norm* args, void* stream);

/* urgym_actor_adam_step / urgym_critic_adam_step with every gradient element multiplied by *scale_dev as it is read (see above): ONE
 * launch each, kernels of their own.  scale_dev is a DEVICE scalar read when the launch runs -- what a urgym_*_grad_norm call earlier
 * on `stream` wrote to scale_out.  With *scale_dev == 1.0f every output is bit for bit the unscaled call's.  Refused: everything the
 * unscaled step refuses, and a NULL scale_dev. */
int urgym_actor_adam_step_scaled(void* handle, void* actor, const urgym_actor_adam* t, const urgym_adam_hyper* hp, const float* scale_dev, void* stream);
int urgym_critic_adam_step_scaled(void* handle, void* online, void* target_or_NULL, const urgym_critic_adam* t, const urgym_adam_hyper* hp, float tau, const float* scale_dev, void* stream);

typedef struct urgym_sac_clipping {
  float max_grad_norm;     /* finite, > 0: of the critics' group and of the actor's group alike */
  int32_t reserved0;       /* must be 0 */
  float* scale;            /* [2] DEVICE scratch: the critics' coefficient, then the actor's, of the running update */
  float* critic_grad_norm; /* [number of updates of the call] DEVICE: update u writes slot u, like the losses */
  float* actor_grad_norm;  /* the same */
} urgym_sac_clipping;

/* urgym_sac_train -- or urgym_sac_train_evaluated / _monitored / _nstep / _prioritized / _hindsight, by which of the five optional
 * arguments are given -- with two more launches per update and the two steps replaced by their scaled forms.  Afterwards everything
 * is BIT FOR BIT what that call's sequence would have left with these substitutions, u = the update's slot:
 *     urgym_critic_parameter_gradients(...)                                                        as before
 *     urgym_critic_grad_norm(online, critic_adam.grad, {max_grad_norm, critic_grad_norm + u, scale + 0, NULL})
 *     urgym_critic_adam_step_scaled(online, target, critic_adam, hp, tau, scale + 0)               in place of urgym_critic_adam_step
 *     ...
 *     urgym_actor_parameter_gradients(...)                                                         as before
 *     urgym_actor_grad_norm(actor, actor_adam.grad, {max_grad_norm, actor_grad_norm + u, scale + 1, NULL})
 *     urgym_actor_adam_step_scaled(actor, actor_adam, hp, scale + 1)                               in place of urgym_actor_adam_step
 * 15 launches per update (17 above 1024 rows; the prioritized route's count plus two).  The temperature's scalar step is not clipped.
 * Everything is validated before the first launch.  Refused besides what the composed call refuses: clipping == NULL; reserved0 != 0;
 * max_grad_norm not finite or <= 0; a NULL scale; a NULL critic_grad_norm or actor_grad_norm in a call that holds an update; more
 * than one of nstep, prioritized and hindsight (the pairings those calls already refuse). */
int urgym_sac_train_clipped(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_clipping* clipping, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- weights back to the device tensors (a checkpoint: the reference's train.py:31-36 continues a saved run, and the TARGET critic
 * exists only as a packed buffer, blended in place by urgym_critic_load(tau < 1) and urgym_critic_adam_step(target)).  The packing
 * map of ur_gym_amd/csrc/urgym_pack_map.h run the other way, on the device: every element of every destination tensor -- DEVICE
 * pointers, float32, torch's [out][in] row-major layout, 4-byte aligned and nothing more -- is written from the one packed float that
 * holds it; padding has no destination.  Copies only: every bit pattern goes through unchanged, NaN payloads and -0.0f included.
 * Added WITHIN ABI version 4: no struct above changed, URGYM_ABI_VERSION did not move, the new symbols (urgym_actor_unpack,
 * urgym_critic_unpack) are found by lookup.
 *
 * Each unpack is ONE launch on `stream`: no allocation, no host synchronisation, everything validated before the launch.  The
 * destinations are written when the launch RUNS, not during the call.  Stream order holds against the loads, the Adam steps and the
 * urgym_sac_train* calls: an unpack sees what those enqueued before it on the same stream left in the buffer, and nothing of those
 * enqueued after it.  Every hidden width the objects accept is covered (32 to 512).
 * ROUND TRIP: urgym_*_unpack followed by urgym_*_load (tau == 1) of the same tensors leaves the packed buffer bit for bit as it was. */

/* urgym_actor_params_dev with pointers that are written. */
typedef struct urgym_actor_params_out {
  int32_t in_features;    /* must be the actor's */
  int32_t hidden_width;   /* must be the actor's */
  int32_t reserved0;      /* must be 0 */
  float* w0;        /* latent_pi.0.weight [hidden_width][in_features] */
  float* b0;        /* latent_pi.0.bias   [hidden_width] */
  float* w1;        /* latent_pi.2.weight [hidden_width][hidden_width] */
  float* b1;        /* latent_pi.2.bias   [hidden_width] */
  float* w_mu;      /* mu.weight [6][hidden_width] */
  float* b_mu;      /* mu.bias   [6] */
  float* w_log_std; /* log_std.weight [6][hidden_width], or NULL together with b_log_std: the head is skipped */
  float* b_log_std; /* log_std.bias   [6], or NULL together with w_log_std */
} urgym_actor_params_out;

/* urgym_q_network_dev with pointers that are written. */
typedef struct urgym_q_network_out {
  float* w0;  /* qf{i}.0.weight [hidden_width][in_features] */
  float* b0;  /* qf{i}.0.bias   [hidden_width] */
  float* w1;  /* qf{i}.2.weight [hidden_width][hidden_width] */
  float* b1;  /* qf{i}.2.bias   [hidden_width] */
  float* w_q; /* qf{i}.4.weight [1][hidden_width] */
  float* b_q; /* qf{i}.4.bias   [1] */
} urgym_q_network_out;

typedef struct urgym_critic_params_out {
  int32_t in_features;  /* must be the critic's */
  int32_t hidden_width; /* must be the critic's */
  int32_t reserved0;    /* must be 0 */
  urgym_q_network_out qf[2];
} urgym_critic_params_out;

/* Writes an actor's tensors.  Refused (URGYM_ERR_ARG; handle and actor stay usable, nothing is launched, nothing is written): NULL
 * handle / actor / out, an actor of another handle, a NULL required pointer (the message names it), only one of the two log_std
 * pointers, log_std pointers for an actor that has no head, in_features or hidden_width other than the actor's, reserved0 != 0. */
int urgym_actor_unpack(void* handle, void* actor, const urgym_actor_params_out* out, void* stream);

/* Writes both Q-networks of a critic.  Refused: as urgym_actor_unpack (every pointer of both networks is required). */
int urgym_critic_unpack(void* handle, void* critic, const urgym_critic_params_out* out, void* stream);

/* Verification aid, not a hot path: synchronises the device, then copies the object's packed buffer (the kernel's own layout,
 * ur_gym_amd/csrc/urgym_pack_map.h) to host_out and stores its length in floats in *count.  host_out == NULL only reports *count;
 * otherwise capacity (in floats) must be at least that.  Refused: NULL handle / object / count, an object of another handle,
 * capacity too small.  The parameters themselves, in torch's layout and without a synchronisation, are urgym_actor_unpack /
 * urgym_critic_unpack: nothing that is kept should hold this layout. */
int urgym_actor_read_packed(void* handle, void* actor, float* host_out, uint64_t capacity, uint64_t* count);
int urgym_critic_read_packed(void* handle, void* critic, float* host_out, uint64_t capacity, uint64_t* count);

/* ---- running observation and reward normalization on the device (stable-baselines3's VecNormalize, which the reference's
 * utils/callbackFunctions.py names: sync_envs_normalization, get_vec_normalize_env, save_vecnormalize).  The running mean and variance
 * of what the collecting actor saw and of the discounted return are kept in float64 on the device, folded from the replay ring a
 * collection has just written, and applied by one launch to rows (what the actor reads) or to a learner's batch.  The ring keeps the
 * RAW rows, as SB3's buffer does.  Added WITHIN ABI version 4: no struct above changed, URGYM_ABI_VERSION did not move, the new symbols
 * (urgym_norm_workspace, urgym_norm_fold, urgym_norm_rows, urgym_norm_batch, urgym_norm_snapshot, urgym_rollout_collect_normalized,
 * urgym_policy_evaluate_normalized, urgym_sac_train_normalized) are found by lookup.
 * The library keeps none of the state.  Non-finite inputs are out of scope: nothing below is stated or tested for them.
 *
 * THE STATE: DEVICE pointers owned by the caller, all float64, 8-byte aligned.  Four groups -- observation [obs_dim], achieved_goal
 * [goal_dim], desired_goal [goal_dim], ret [1] -- each mean[d], var[d] and ONE count; running_ret [N] is the discounted return of each
 * env's running episode.  The initial state is mean = 0, var = 1, count = 1e-4, running_ret = 0 (SB3's RunningMeanStd). */
typedef struct urgym_norm_state {
  double* observation_mean;    /* [obs_dim] */
  double* observation_var;     /* [obs_dim] */
  double* observation_count;   /* [1] */
  double* achieved_goal_mean;  /* [goal_dim] */
  double* achieved_goal_var;   /* [goal_dim] */
  double* achieved_goal_count; /* [1] */
  double* desired_goal_mean;   /* [goal_dim] */
  double* desired_goal_var;    /* [goal_dim] */
  double* desired_goal_count;  /* [1] */
  double* ret_mean;            /* [1] */
  double* ret_var;             /* [1] */
  double* ret_count;           /* [1] */
  double* running_ret;         /* [N] */
} urgym_norm_state;

typedef struct urgym_normalization {
  urgym_norm_state state;
  double gamma;             /* the discount of running_ret */
  double eps;               /* >= 0 */
  double clip_obs;          /* > 0, +inf allowed */
  double clip_reward;       /* > 0, +inf allowed */
  int32_t norm_obs;         /* 0: the three observation groups are neither folded nor applied */
  int32_t norm_reward;      /* 0: the return group is neither folded nor applied */
  int32_t training;         /* 0: urgym_norm_fold launches nothing and leaves the state untouched */
  float* scratch;           /* [N][obs_dim + 2 goal_dim] DEVICE: the N observation rows, then the N achieved_goal rows, then the N
                               desired_goal rows the collecting actor reads; required by urgym_rollout_collect_normalized only */
  void* workspace;          /* DEVICE, 8-byte aligned: the partial sums of urgym_norm_fold; required by urgym_norm_fold only */
  uint64_t workspace_bytes; /* at least urgym_norm_workspace(num_steps) */
  float* eval_scratch;      /* [N_eval][obs_dim + 2 goal_dim] DEVICE, laid out like scratch for the EVALUATION handle's env count;
                               required by urgym_policy_evaluate_normalized and by an evaluation inside urgym_sac_train_normalized only */
  const urgym_norm_state* best_state; /* where an evaluation that improved snapshots the statistics (running_ret is not copied and may
                               be NULL); required where eval_scratch is */
  int64_t reserved0;        /* must be 0 */
} urgym_normalization;

/* THE FOLD of one ring slot.  The inputs are the rows s of that slot -- what the actor saw, N rows per group.  Per feature j:
 *   S1 = the float64 sum of (double)x, S2 = the float64 sum of (double)x * (double)x (each product is exact), BOTH IN THIS ORDER, a
 *   function of N alone (ur_gym_amd/csrc/urgym_norm.h states it, ur_gym_amd.evaluation.norm_sums restates it):
 *     slab b holds rows 128 b .. min(128 b + 127, N - 1).  Within a slab, chain q = 0..3 starts at +0.0 and adds rows 128 b + q,
 *     128 b + q + 4, ... in ascending order (32 terms at the most);  slab = (chain0 + chain1) + (chain2 + chain3);
 *     part c = 0..15 starts at +0.0 and adds slabs c, c + 16, c + 32, ... in ascending order;
 *     part[c] += part[c + s] for s = 8, 4, 2, 1;  the sum is part[0].
 *   n = (double)N;  bm = S1 / n;  bv = max(S2 / n - bm * bm, 0.0)
 * then the merge of SB3's update_from_moments, ONE float64 operation per line in the association written:
 *   delta = bm - mean
 *   tot   = count + n
 *   mean' = mean + (delta * n) / tot
 *   M2    = (var * count + bv * n) + ((delta * delta) * count) * n / tot
 *   var'  = M2 / tot
 *   count' = tot
 * The return group, per env: running_ret = running_ret * gamma + (double)reward; then the same sums and the same merge over the N
 * values of running_ret (a group of one feature); then running_ret = +0.0 where terminated | truncated.
 * K = num_steps slots (first_slot + k) % C are folded in slot order with one merge per slot: K steps in one call and the same steps in
 * pieces leave identical bits.  norm_obs == 0 leaves the three observation groups alone, norm_reward == 0 the return group and
 * running_ret; training == 0 launches nothing.
 * TWO launches on `stream` whatever K is: many workgroups reduce slabs to partial sums in the workspace (one lane per env walks the K
 * slots for running_ret in the same launch), ONE workgroup of 1024 lanes combines them, merges slot by slot and writes the state.  No
 * atomics, nothing crosses between workgroups but through the launch boundary, no allocation, no host synchronisation, everything
 * validated before the first launch.
 * Refused (URGYM_ERR_ARG, nothing launched, nothing written): NULL handle or norm; a NULL or misaligned state pointer (named); gamma
 * outside [0, 1]; eps < 0; a clip <= 0; reserved0 != 0; a NULL or misaligned workspace or workspace_bytes too small; and
 * urgym_monitor_fold's ring refusals (ring == NULL, a NULL required pointer, capacity_steps <= 0, reserved0 != 0, first_slot outside
 * [0, C), a ring without truncated or is_success, num_steps <= 0, num_steps > C, a handle with auto_reset off). */
int urgym_norm_workspace(void* handle, int num_steps, uint64_t* bytes);
int urgym_norm_fold(void* handle, const urgym_normalization* norm, const urgym_replay_ring* ring, int first_slot, int num_steps, void* stream);

/* NORMALIZE.  Once per feature: inv_j = 1.0 / sqrt(var_j + eps), in float64 (both correctly rounded).
 *   an observation or goal element becomes (float)min(max(((double)x - mean_j) * inv_j, -clip_obs), clip_obs)
 *   a reward becomes (float)min(max((double)r * inv_ret, -clip_reward), clip_reward): no mean is subtracted, as in SB3
 * The state is read when the launch RUNS: a fold earlier on `stream` is seen, a later one is not.
 *
 * urgym_norm_rows: ONE launch maps `count` rows of the three groups, each source pointer optional (NULL = that group is skipped,
 * together with its destination), from source to destination; a destination may be its source.  With norm_obs == 0 the rows are
 * copied unchanged.  Refused: NULL handle or norm, the state and option refusals of urgym_norm_fold (not the workspace's), count <= 0,
 * no group at all, a source without its destination or the reverse. */
typedef struct urgym_norm_rows_args {
  const float* observation;   /* [count][obs_dim] or NULL */
  const float* achieved_goal; /* [count][goal_dim] or NULL */
  const float* desired_goal;  /* [count][goal_dim] or NULL */
  float* observation_out;
  float* achieved_goal_out;
  float* desired_goal_out;
} urgym_norm_rows_args;
int urgym_norm_rows(void* handle, const urgym_normalization* norm, const urgym_norm_rows_args* rows, int count, void* stream);

/* urgym_norm_batch: ONE launch normalizes a learner's batch of `count` rows IN PLACE: observation and next_observation with the
 * observation group, achieved_goal and next_achieved_goal, desired_goal and next_desired_goal likewise (norm_obs != 0), and reward
 * with the return group (norm_reward != 0).  Every pointer of the batch may be NULL (= left alone); action and the flags are not
 * touched.  With both switches off nothing is launched.  Refused: as urgym_norm_rows; NULL batch. */
int urgym_norm_batch(void* handle, const urgym_normalization* norm, const urgym_replay_batch* batch, int count, void* stream);

/* urgym_rollout_collect whose actor reads NORMALIZED rows: before the policy pass of every step ONE more launch (urgym_norm_rows of
 * the N bound rows into norm->scratch), and the actor runs on the scratch; its kernels, its noise (a function of the env index) and
 * the step are those of urgym_rollout_collect.  The store pass files the RAW rows.  4 num_steps + 1 launches.  The statistics are
 * NOT folded inside the call -- a step's action sees the statistics as of the start of the call, a stated deviation from SB3, which
 * updates them every step -- : fold afterwards with urgym_norm_fold from the slots the call wrote.  With norm_obs == 0 the call is
 * urgym_rollout_collect.  Refused: everything urgym_rollout_collect and urgym_norm_rows refuse; a NULL scratch. */
int urgym_rollout_collect_normalized(void* handle, void* actor, const urgym_sampling* how, int num_steps, const urgym_replay_ring* ring, int first_slot, const urgym_normalization* norm, void* stream);

/* THE STATE SNAPSHOT, the twin of urgym_actor_snapshot: destination = source for mean, var and count of the four groups (running_ret is
 * not copied) in ONE launch of one workgroup -- or nothing at all where `when`, a DEVICE int32, holds 0 when the launch RUNS (NULL =
 * always).  dims are the handle's.  Refused: NULL handle / source / destination, a NULL or misaligned pointer of the twelve. */
int urgym_norm_snapshot(void* handle, const urgym_norm_state* source, const urgym_norm_state* destination, const int32_t* when, void* stream);

/* urgym_policy_evaluate whose actor reads rows normalized with the statistics normalization->state points to -- the TRAINING state, read
 * through its pointers when the launches run: SB3's sync_envs_normalization.  One more launch per step before the policy pass (the N_eval
 * bound rows of the evaluation handle into normalization->eval_scratch; none with norm_obs == 0), and after urgym_actor_snapshot ONE
 * urgym_norm_snapshot of the state into normalization->best_state under the record's `improved` flag, so that the best actor is kept
 * with the statistics it was selected under.  Rewards are NOT normalized: the records hold raw returns.  Nothing is folded.  Refused:
 * everything urgym_policy_evaluate and urgym_norm_rows refuse; a NULL eval_scratch or best_state; a NULL or misaligned pointer of
 * best_state's twelve. */
int urgym_policy_evaluate_normalized(void* eval_handle, const urgym_policy_evaluation* evaluation, const urgym_normalization* normalization, int64_t eval_index, int32_t record_slot, void* stream);

/* urgym_sac_train -- or urgym_sac_train_clipped / _nstep / _prioritized / _hindsight / _monitored, by which of the optional arguments
 * are given -- with the statistics in it.  Afterwards everything is BIT FOR BIT what that call's sequence would have left with:
 *   every collection urgym_rollout_collect_normalized (one more launch per step);
 *   after each iteration's collection, idle warm-up iterations included, and before the monitor's fold, ONE urgym_norm_fold of the
 *     K slots just written (two launches; none with training == 0);
 *   right after the gather of every update, whichever gather it is, ONE urgym_norm_batch of the learner's batch: 14 launches per
 *     update instead of 13, 16 with clipping.  With n_steps > 1 the normalized reward is the row's ACCUMULATED multi-step return.
 * normalization->workspace must hold steps_per_iteration steps.  Everything is validated before the first launch.  Refused besides
 * what the composed call, urgym_norm_fold and urgym_norm_batch refuse: normalization == NULL; a NULL scratch with norm_obs != 0 in a
 * call that collects; more than one of nstep, prioritized and hindsight.  An evaluation inside the call is
 * urgym_policy_evaluate_normalized with this normalization (its refusals: a NULL eval_scratch or best_state). */
int urgym_sac_train_normalized(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_normalization* normalization, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- sampling-based MPC on the device: an MPPI planner (Williams et al., 2017) that plans with the step kernel itself (DESIGN.md
 * section 26).  Added WITHIN ABI version 4 like everything since the sampling calls: no struct above changed, the new symbols
 * (urgym_mppi_*) are found by lookup.  No existing kernel is touched: the planner's futures are ordinary environments of a second
 * handle, stepped by urgym_step's own launches.
 *
 * Notation.  E source envs ("parents"), K samples per parent in [2, URGYM_MPPI_SAMPLES_MAX], H horizon steps in
 * [1, URGYM_MPPI_HORIZON_MAX], I refinement iterations in [1, URGYM_MPPI_ITERATIONS_MAX].  The PLANNER is a handle of the same env
 * kind and config with num_envs == E * K and auto_reset == 0; its env n = p * K + j is sample j of parent p (p = n / K, j = n - p * K).
 * The SOURCE handle has num_envs == E.  Every array below is a DEVICE pointer owned by the caller; the library allocates nothing.
 *
 * THE FAN-OUT (urgym_mppi_fanout, one launch).  For every planner env n it copies parent p's column of every state field of
 * urgym_buffers from the source's bound buffers (SoA [f][E]) into the planner's ([f][E * K]): q, goal, obst_start, obst_end, obst_pos,
 * obst_quat, obst_vel (all 9 rows), link_dist, step_count, episode_id; and the rows of observation, achieved_goal, desired_goal (a Dyn
 * step may read the row it finds).  Bytes only.  The planner's status is zeroed.  The planner thus inherits the parent's step_count:
 * a time limit that falls inside the horizon truncates the sample there.
 *
 * THE SAMPLE (urgym_mppi_sample, one launch) writes actions[h][n][c] and eps[h][n][c], float32 [H][E * K][6].  Sample j = 0 is the
 * nominal sequence: eps = 0.  Otherwise eps is Box-Muller exactly as the GAUSSIAN policy noise above states it (u1, u2, r, cos, sin;
 * pairs p = 0, 1, 2 from the words w0 .. w5) on the words of Philox4x32-10 with key = (seed & 0xFFFFFFFF, seed >> 32) and
 *   counter = (p, (i << 24) | (h << 16) | j, (uint32)draw, URGYM_MPPI_TAG | block),  block = 0, 1,
 * i the refinement iteration.  URGYM_MPPI_TAG = 0x4D505000 meets none of 0x504F4C00 | b (policy noise), 0x52504C00 (replay),
 * 0x50455200 (prioritized replay) or the reset sampler's 0 .. 4.  draw >= 2^32 is refused.  The action line, float32, one operation per
 * line:
 *   s = sigma * eps;  a = mean[h][p][c] + s;  action = fminf(fmaxf(a, -1), 1).
 * The noise is a function of (seed, draw, i, p, j, h, c) only -- not of E, K or the launch geometry.
 *
 * THE SCORE (urgym_mppi_score, one launch after planner step h, one lane per planner env n, float64, one operation per line):
 *   at h == 0 first:  ret = 0;  g = 1;  alive = 1;  end_step = H - 1;  success = 0;  collided = 0
 *   where alive:      t = g * (double)reward[n];  ret = ret + t;  g = g * gamma;
 *                     if (terminated[n] | truncated[n]) { alive = 0;  end_step = h;  success = is_success[n];  collided = collision[n]; }
 * reward .. collision being the planner's bound outputs.  A NaN reward reaches that env's ret only.
 *
 * THE UPDATE (urgym_mppi_update, one launch: one workgroup of 1024 lanes per parent, lane j < K, float64, no atomics).  r_j = ret[pK + j].
 *   rmax = the fmax over the FINITE r_j (a NaN or an infinity is passed over; -inf when none is finite)
 *   none finite:  w_0 = 1, w_j = 0 otherwise.   else:  d = r_j - rmax;  x = d / lambda;  w_j = finite(r_j) ? exp(x) : 0
 *   Z = THE ORDERED SUM (above, "SAC's entropy coefficient on the device") of w_j over j < K, float64 terms
 *   for each (h, c):  S = the ordered sum of w_j * (double)actions[h][pK + j][c];  m = S / Z;  new_mean[h][p][c] = (float)m
 *   Q = the ordered sum of w_j * w_j;  zz = Z * Z;  ess[p] = zz / Q
 *   action_out[p][c] = new_mean[0][p][c];  best_return[p] = rmax;  nominal_return[p] = r_0;  w[p][j] = w_j (w may be NULL)
 *   then mean = new_mean; with shift != 0 instead mean[h] = new_mean[h + 1] for h < H - 1 and mean[H - 1] = new_mean[H - 1].
 * exp is the device library's: w is an output, and a restatement takes it as an input (as powf is treated by urgym_per_terms).
 *
 * THE RECORD (urgym_mppi_record, one launch) is pass k of urgym_rollout_actor's records, restated for the closed loop: pass k in
 * [0, num_steps] copies the source's observation rows into row k of the trajectory (k < num_steps), initialises the episode summary
 * (k == 0), and for k > 0 files what source step k - 1 returned (reward .. final_observation rows k - 1, action row k - 1 =
 * action_out) and the episode summary exactly as urgym_trajectory states it.  For k > 0 it also zeroes mean[:, p, :] where source env
 * p has just finished (terminated | truncated), so that a new episode does not start from the old plan.  traj may be NULL (only the
 * zeroing is left); episode_done is required when any of the three other summary arrays is given. */
#define URGYM_MPPI_TAG 0x4D505000u
/* Blocks 0 and 1 under the tag are THE SAMPLE's.  Blocks 2 and 3 are the exploration noise of urgym_mppi_execute (below, "planner-
 * collected experience"): counter = (p, 0, (uint32)draw, URGYM_MPPI_TAG | block), block = URGYM_MPPI_EXPLORE_BLOCK, + 1. */
#define URGYM_MPPI_EXPLORE_BLOCK 2
#define URGYM_MPPI_SAMPLES_MAX 1024
#define URGYM_MPPI_HORIZON_MAX 64
#define URGYM_MPPI_ITERATIONS_MAX 8

typedef struct urgym_mppi {
  int32_t num_parents;   /* E */
  int32_t samples;       /* K in [2, 1024] */
  int32_t horizon;       /* H in [1, 64] */
  int32_t iterations;    /* I in [1, 8] (urgym_mppi_plan / _control only) */
  int32_t shift;         /* != 0: the update (of the LAST iteration, in a plan) leaves mean advanced by one step */
  int32_t reserved0;     /* must be 0 */
  float sigma;           /* finite, >= 0 */
  int32_t reserved1;     /* must be 0 */
  double lam;            /* lambda, the temperature: finite, > 0 */
  double gamma;          /* finite */
  uint64_t seed;         /* the Philox key */
  float* mean;           /* [H][E][6] the nominal sequence: in (sample) and out (update, record) */
  float* new_mean;       /* [H][E][6] */
  float* actions;        /* [H][E*K][6] */
  float* eps;            /* [H][E*K][6] */
  double* ret;           /* [E*K] */
  double* g;             /* [E*K] */
  uint8_t* alive;        /* [E*K] */
  int32_t* end_step;     /* [E*K] */
  uint8_t* success;      /* [E*K] */
  uint8_t* collided;     /* [E*K] */
  float* action_out;     /* [E][6] */
  double* best_return;   /* [E] */
  double* nominal_return;/* [E] */
  double* ess;           /* [E] */
  double* w;             /* [E][K], may be NULL */
} urgym_mppi;

/* The five single launches.  Everything is validated before the launch; no allocation, no host synchronisation.  Refused by all
 * (the message names the entry point and the argument): a NULL handle; a NULL m; a NULL pointer of m other than w; K, H or
 * iterations out of range; num_parents < 1; sigma not finite or < 0; lam not finite or <= 0; gamma not finite; a non-zero reserved
 * field.  urgym_mppi_sample and urgym_mppi_update need no bound environment (the handle names the device).  Refused besides:
 *   _fanout  an unbound handle; handles on different devices; a planner with auto_reset != 0 (its episodes must not restart); planner
 *            num_envs != E * K; source num_envs != E; any urgym_config field other than num_envs and auto_reset differing between
 *            the two handles
 *   _sample  draw >= 2^32; iteration outside [0, 8)
 *   _score   an unbound planner; planner num_envs != E * K; h outside [0, H)
 *   _record  an unbound source; source num_envs != E; num_steps < 1; k outside [0, num_steps]; a summary array without episode_done */
int urgym_mppi_fanout(void* source_handle, void* planner_handle, const urgym_mppi* m, void* stream);
int urgym_mppi_sample(void* handle, const urgym_mppi* m, uint64_t draw, int iteration, void* stream);
int urgym_mppi_score(void* planner_handle, const urgym_mppi* m, int h, void* stream);
int urgym_mppi_update(void* handle, const urgym_mppi* m, void* stream);
int urgym_mppi_record(void* source_handle, const urgym_mppi* m, int k, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream);

/* ONE PLAN: I x (fanout, sample with iteration i, H x (urgym_step(planner, actions[h]), score h), update), the shift applied by the
 * update of the last iteration only: 3 + 2 H launches per iteration besides what a step itself launches.  Bit for bit that sequence of
 * single calls and urgym_steps.  Afterwards action_out holds the first action of the refined nominal sequence of every parent.
 * Refused: everything urgym_mppi_fanout and urgym_mppi_sample refuse. */
int urgym_mppi_plan(void* source_handle, void* planner_handle, const urgym_mppi* m, uint64_t draw, void* stream);

/* THE CLOSED LOOP: record pass 0, then for t < num_steps: urgym_mppi_plan with draw = first_draw + t; urgym_step(source, action_out);
 * record pass t + 1.  Bit for bit that sequence.  A source env that finishes inside the call has its mean zeroed by the record pass and,
 * with the source's auto_reset, plans its new episode from the next step.  Refused: everything urgym_mppi_plan and urgym_mppi_record
 * refuse; num_steps < 1; first_draw + num_steps > 2^32. */
int urgym_mppi_control(void* source_handle, void* planner_handle, const urgym_mppi* m, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream);

/* ---- MPPI with the learner in the loop: the critic values the state a plan stops in, the actor proposes samples, and a future that
 * ends without success costs a scalar.  Added WITHIN ABI version 4: no struct above changed, the four new
 * symbols are found by lookup, and urgym_mppi_plan / urgym_mppi_control and the five single launches are what they were.  The actor and
 * the critic are ordinary ones (urgym_actor_create, urgym_critic_create) of the PLANNER handle: they read its bound rows, [E * K] of
 * them, raw -- a policy trained on normalized observations is not served.
 *
 * THE GUIDE (urgym_mppi_guide_actions, one launch before planner step h, one lane per (n, c), float32, one operation per line) rewrites
 * the action rows of samples 1 .. P of every parent, planner envs n = p K + j with 1 <= j <= P:
 *   s = policy_sigma * eps[h][n][c];  a = policy_action[n][c] + s;  actions[h][n][c] = fminf(fmaxf(a, -1), 1)
 * eps being what the sample launch drew for (h, n, c) -- no new Philox words -- and policy_action what urgym_actor_forward wrote for
 * the planner's bound observation before planner step h.  Sample 0 (the nominal) and samples j > P are not written.  actions then
 * holds what every future executed, which is what the update's weighted mean reads.
 *
 * THE TERMINAL STEP (urgym_mppi_terminal, one launch after the score of step H - 1, one lane per planner env n, float64):
 *   alive:                  v = terminal_value ? (double)value[n] : 0
 *   not alive, success:     v = 0
 *   not alive, no success:  v = -fail_cost
 *   terminal[n] = v;   if (v != 0) { t = g * v;  ret = ret + t; }
 * alive, success, g and ret as the score left them: g is gamma^H for a live future and gamma^(end_step + 1) for an ended one.  The
 * choice of the case is a selection: value[n] of an ended future is not read, so a NaN there reaches nothing; a NaN value of a live
 * future reaches that future's ret only, and the update gives a return that is not finite the weight 0.  value[n] is
 * min(q0, q1)(s_H, actor(s_H)), urgym_critic_evaluate's q_min.  The shipped critics were trained with gamma = 0.95: a plan that credits
 * their value should discount with it. */
typedef struct urgym_mppi_guide {
  void* actor;             /* an actor of the PLANNER handle, or NULL */
  void* critic;            /* a critic of the PLANNER handle, or NULL */
  int32_t policy_samples;  /* P in [0, K - 1]: samples 1 .. P follow the actor */
  int32_t terminal_value;  /* != 0: a future alive after H steps is credited min Q(s_H, actor(s_H)) */
  float policy_sigma;      /* finite, >= 0 */
  int32_t reserved0;       /* must be 0 */
  double fail_cost;        /* finite, >= 0 */
  float* policy_action;    /* [E*K][6]; needed when the actor is used (P > 0 or terminal_value) */
  float* value;            /* [E*K]; needed with terminal_value */
  double* terminal;        /* [E*K]; needed when the terminal launch is made (terminal_value or fail_cost > 0) */
} urgym_mppi_guide;

/* The two single launches.  Everything is validated before the launch; no allocation, no host synchronisation.  Refused by both and
 * by the two composed calls below (the message names the entry point and the argument): what urgym_mppi_score refuses about handle, m
 * and the planner; a NULL g; a non-zero reserved0; P outside [0, K - 1]; P > 0 without an actor; terminal_value without an actor or
 * without a critic; an actor or critic that is not the planner handle's (the source handle's in particular) or does not take its env
 * kind's features; policy_sigma not finite or < 0; fail_cost not finite or < 0; a NULL policy_action, value or terminal that the chosen
 * options need.  Refused besides: _guide_actions  h outside [0, H);  _terminal  neither terminal_value nor fail_cost > 0 (there is no
 * terminal launch then).  With P == 0 no sample follows the actor and urgym_mppi_guide_actions launches nothing. */
int urgym_mppi_guide_actions(void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* g, int h, void* stream);
int urgym_mppi_terminal(void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* g, void* stream);

/* ONE GUIDED PLAN, per iteration: fanout; sample; for each h: with P > 0 urgym_actor_forward(planner, actor, policy_action) and the
 * guide launch h, then urgym_step(planner, actions[h]) and score h; with terminal_value urgym_actor_forward(planner, actor,
 * policy_action) and urgym_critic_evaluate(planner, critic, the bound rows with action = policy_action, E * K, out.q_min = value); with
 * terminal_value or fail_cost > 0 the terminal launch; update (the shift on the last iteration only).  That is up to 2 H + 3 launches
 * per iteration more than a plain plan.  Bit for bit that sequence of single calls; with P == 0, terminal_value == 0 and fail_cost == 0
 * it launches, and leaves, what urgym_mppi_plan does.  The actor reads the rows the fan-out and the planner's steps wrote: the planner
 * needs no urgym_reset of its own.  Refused: everything urgym_mppi_plan and the two launches above refuse. */
int urgym_mppi_plan_guided(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* g, uint64_t draw, void* stream);

/* THE GUIDED CLOSED LOOP: urgym_mppi_control with urgym_mppi_plan_guided in place of urgym_mppi_plan, bit for bit.  Refused:
 * everything urgym_mppi_plan_guided and urgym_mppi_control refuse. */
int urgym_mppi_control_guided(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* g, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream);

/* ---- planner-collected experience: MPPI files its transitions into the ring.  urgym_mppi_control(_guided)
 * writes a urgym_trajectory, an evaluation record; urgym_rollout_collect fills the replay ring but takes an actor.  The two calls below
 * are a collection whose policy is the planner, so that an off-policy learner can train on what the planner did.  Added WITHIN ABI
 * version 4: no struct above changed, the two new symbols are found by lookup, and urgym_mppi_plan, urgym_mppi_control, their guided
 * forms and urgym_rollout_collect are what they were.  The ring is filled by urgym_rollout_collect's own store pass, so every gather
 * (one-step, multi-step, prioritized, hindsight), urgym_monitor_fold and urgym_norm_fold read the slots as they read a policy's.
 *
 * THE EXPLORATION NOISE.  For source env (parent) p and draw d, six normals e[p][0 .. 5]: Box-Muller exactly as THE SAMPLE above forms
 * its own (u1, u2, r, cos, sin; pairs 0, 1, 2 from the words w0 .. w5) on the words of Philox4x32-10 with the planner's key,
 * (m->seed & 0xFFFFFFFF, m->seed >> 32), and
 *   counter = (p, 0, (uint32)d, URGYM_MPPI_TAG | block),  block = 2, 3
 * (w0 .. w3 from block 2, w4 and w5 from block 3).  THE SAMPLE's counters carry block 0 or 1 in the same word, so no exploration
 * counter meets a sample counter, whatever (i, h, j) are; the other tags are those THE SAMPLE lists.  The noise is a function of
 * (seed, d, p, c) only -- not of E or the launch geometry.
 *
 * THE EXECUTE LINE (urgym_mppi_execute, one launch, one lane per (p, c), float32, one operation per line):
 *   s = explore_sigma * e[p][c];  a = action_out[p][c] + s;  executed[p][c] = fminf(fmaxf(a, -1), 1)
 * With explore_sigma == 0 no Philox word is drawn and executed[p][c] is the 32 bits of action_out[p][c] (a -0.0 stays -0.0).
 * explore_eps[p][c], where given, receives e[p][c], or 0 with explore_sigma == 0.  A NaN in action_out reaches its own element only.
 * The launch has no LDS and no atomics, one writer per output, and writes executed and explore_eps only. */
typedef struct urgym_mppi_explore {
  float explore_sigma;   /* finite, >= 0 */
  int32_t reserved0;     /* must be 0 */
  float* explore_eps;    /* [E][6] or NULL */
} urgym_mppi_explore;

/* The single launch.  Refused (the source keeps the message): a NULL handle; everything urgym_mppi_record refuses about m and the source
 * (an unbound source, source num_envs != E); a NULL x; a non-zero reserved0; explore_sigma not finite or < 0; a NULL executed;
 * draw >= 2^32. */
int urgym_mppi_execute(void* source_handle, const urgym_mppi* m, const urgym_mppi_explore* x, uint64_t draw, float* executed /* [E][6] */, void* stream);

/* THE COLLECTION.  With C = ring->capacity_steps and slot(t) = (first_slot + t) % C, for t < num_steps:
 *   1. store pass t: urgym_rollout_collect's store launch, sequenced as there -- the source's live rows are at once the s of step t
 *      (into slot(t)) and, for t > 0, the s' of step t - 1 (into slot(t - 1), with its reward and flags; the final_* rows in place of the
 *      live ones for an env that finished under auto_reset);
 *   2. for t > 0, record pass t with a NULL trajectory (THE RECORD above): it zeroes mean[:, p, :] of every source env p that has just
 *      finished, as urgym_mppi_control does;
 *   3. the plan: urgym_mppi_plan, or urgym_mppi_plan_guided where a guide is given, with draw = first_draw + t;
 *   4. the execute launch with draw = first_draw + t and executed = the action rows of slot(t): the planner's action is written straight
 *      into the ring, as the actor's is in urgym_rollout_collect;
 *   5. urgym_step(source, those rows).
 * After the loop: store pass num_steps (the outcome of the last step into slot(num_steps - 1)) and record pass num_steps.
 * Launches: per step one store pass, one record pass (none at t == 0) and one execute launch besides the plan's and the step's own,
 * and one store pass and one record pass after the loop: 3 num_steps + 1 in all besides num_steps plans and num_steps steps.
 *
 * A slot is complete when the call returns.  num_steps may exceed C (the ring wraps; later steps overwrite earlier ones of the same
 * call).  No launch writes a slot other than those of the call's own steps.  No allocation, no host synchronisation; everything is
 * validated before the first launch.  Afterwards the source's bound buffers hold what num_steps calls of urgym_step with those actions
 * would have left, and mean is carried to the next call: two calls of a and b steps, the second with first_draw + a and the slot after
 * the first's last, leave the bits of one call of a + b steps.  With explore_sigma == 0 the ring's action, reward and flags are, bit for
 * bit, what urgym_mppi_control(_guided) with the same arguments records in its trajectory.  x->explore_eps, where given, holds the
 * noise of the LAST step.  The planner's actor and critic read raw rows: a policy trained on normalized observations is not served.
 * Refused, each launching and writing nothing: everything urgym_mppi_control (guide_or_NULL == NULL) or urgym_mppi_control_guided
 * refuses about its arguments; everything urgym_rollout_collect refuses about the ring, first_slot, num_steps and a source that has
 * observed nothing; a NULL x; a non-zero reserved0; explore_sigma not finite or < 0. */
int urgym_mppi_collect(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_guide* guide_or_NULL, const urgym_mppi_explore* x, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream);

/* ---- elite samples and an adaptive std: the update TD-MPC's planner runs.  THE UPDATE above weighs every
 * finite sample under one temperature, and every refinement iteration samples with the one scalar sigma.  The calls below rank the K
 * returns of a parent, keep the M best as elites, weigh those as THE UPDATE does, and form, beside the mean, a standard deviation per
 * (horizon step, joint) with which the next iteration of the same plan samples.  Opt-in and WITHIN ABI version 4: no struct above
 * changed, the five new symbols are found by lookup, and every call above launches and leaves what it did.
 *
 * THE RANK of sample j of parent p (float64's own comparisons, so -0.0 == 0.0):
 *   key_j  = finite(r_j) ? r_j : -inf                          (the term of rmax; no key is a NaN)
 *   rank_j = #{ i < K : key_i > key_j, or key_i == key_j and i < j }      a permutation of 0 .. K - 1 whatever the returns are
 *   elite_j = rank_j < M && finite(r_j)
 *   elite_count[p] = the number of elites = min(M, the number of finite returns)
 *   threshold[p]   = r_j of the elite with rank elite_count[p] - 1, the smallest elite return; -inf with no elite
 *
 * THE ELITE WEIGHT.  rmax as in THE UPDATE (the best finite return has rank 0 and is an elite).
 *   none finite:  w_0 = 1, w_j = 0 otherwise.   else:  d = r_j - rmax;  x = d / lambda;  w_j = elite_j ? exp(x) : 0
 * With M == K elite_j is finite(r_j): the weight is THE UPDATE's.
 *
 * Z, S, new_mean, Q, ess, action_out, best_return, nominal_return, w and the shift of mean are THE UPDATE's lines over all j < K, in its
 * order; a sample that is no elite contributes a zero term.  With M == K each of them is, bit for bit, what urgym_mppi_update writes.
 *
 * THE STD, for each (h, c), float64, one operation per line, after S and Z of THE UPDATE:
 *   m = S / Z                                                   (the mean before it is rounded to float32)
 *   per j:  a = (double)actions[h][pK + j][c];  d = a - m;  dd = d * d;  t = w_j * dd
 *   V = the ordered sum of t;  v = V / Z;  sd = sqrt(v)          (the correctly rounded square root)
 *   lo = fmax(sd, (double)std_min);  hi = fmin(lo, (double)std_max);  new_std[h][p][c] = (float)hi
 * A NaN v (a NaN action, even one that weighs nothing) ends at std_min, by fmax.  new_std is not shifted, and it is not carried from one
 * plan to the next: every plan starts at sigma.
 *
 * THE ADAPTIVE SAMPLE (urgym_mppi_sample_adaptive, one launch, THE SAMPLE's geometry).  Counters, words, Box-Muller and eps are THE
 * SAMPLE's, bit for bit; sample 0 is the nominal with eps = 0.  The action line reads its width per element:
 *   s = std[h][p][c] * eps;  a = mean[h][p][c] + s;  action = fminf(fmaxf(a, -1), 1).
 * With every element of std equal to sigma, actions and eps are bitwise urgym_mppi_sample's.
 *
 * THE ELITE UPDATE (urgym_mppi_update_elite, one launch: one workgroup of 1024 lanes per parent, lane j < K, no atomics, one writer per
 * output).  It writes what THE UPDATE writes and new_std, rank, elite (each may be NULL), elite_count and threshold.  It does not
 * write std. */
typedef struct urgym_mppi_adapt {
  int32_t elites;        /* M in [1, K] */
  int32_t adapt_std;     /* != 0: iterations >= 1 of a plan sample with new_std of the iteration before */
  float std_min, std_max;/* finite, 0 <= std_min <= std_max */
  float* std;            /* [H][E][6] what urgym_mppi_sample_adaptive reads */
  float* new_std;        /* [H][E][6] what the elite update writes */
  int32_t* rank;         /* [E][K], may be NULL */
  uint8_t* elite;        /* [E][K], may be NULL */
  int32_t* elite_count;  /* [E] */
  double* threshold;     /* [E] */
} urgym_mppi_adapt;

/* The two single launches.  Like urgym_mppi_sample and urgym_mppi_update they need no bound environment.  Refused, each launching and
 * writing nothing (the message names the entry point and the argument): everything urgym_mppi_sample (_sample_adaptive) or
 * urgym_mppi_update (_update_elite) refuses; a NULL a; elites outside [1, K]; std_min or std_max not finite or negative;
 * std_min > std_max; a NULL std, new_std, elite_count or threshold. */
int urgym_mppi_sample_adaptive(void* handle, const urgym_mppi* m, const urgym_mppi_adapt* a, uint64_t draw, int iteration, void* stream);
int urgym_mppi_update_elite(void* handle, const urgym_mppi* m, const urgym_mppi_adapt* a, void* stream);

/* ONE ADAPTIVE PLAN.  Per iteration i it runs what urgym_mppi_plan runs, or urgym_mppi_plan_guided where a guide is given, with the
 * elite update in place of the update.  Iteration 0 samples with urgym_mppi_sample and m->sigma.  With adapt_std, an iteration i >= 1
 * first copies new_std (of iteration i - 1) into std, device to device on the stream, and samples with urgym_mppi_sample_adaptive;
 * without adapt_std every iteration samples with urgym_mppi_sample.  The launches are a plain plan's and at most that copy per
 * iteration.  Bit for bit that sequence of single calls and urgym_steps.  With M == K and adapt_std == 0 it leaves every buffer of
 * urgym_mppi and of the planner as urgym_mppi_plan(_guided) leaves it.  Refused: everything urgym_mppi_plan (guide_or_NULL == NULL) or
 * urgym_mppi_plan_guided refuses, and what the two launches above refuse about a. */
int urgym_mppi_plan_adaptive(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_adapt* a, const urgym_mppi_guide* guide_or_NULL, uint64_t draw, void* stream);

/* THE CLOSED LOOP and THE COLLECTION with the adaptive plan inside: urgym_mppi_control(_guided) and urgym_mppi_collect with
 * urgym_mppi_plan_adaptive in place of the plan, bit for bit.  Refused: everything those calls refuse, and what the two launches above
 * refuse about a. */
int urgym_mppi_control_adaptive(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_adapt* a, const urgym_mppi_guide* guide_or_NULL, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream);
int urgym_mppi_collect_adaptive(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_adapt* a, const urgym_mppi_guide* guide_or_NULL, const urgym_mppi_explore* x, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream);

/* ---- the planner inside the training call, with plan statistics.  urgym_mppi_collect(_adaptive) is a collection
 * whose policy is the planner, but a run that trains on it went back to the host between every collection, its updates and the reload
 * of the planner's actor and critic.  urgym_sac_train_planned is urgym_sac_train and its kin with that collection inside, and
 * urgym_mppi_stats reduces what a plan left in best_return, nominal_return, ess (and elite_count, threshold) to one record on the device,
 * at the points where the call writes the monitor's records.  Added WITHIN ABI version 4: no struct above changed, the two new symbols
 * are found by lookup, and every call above launches and leaves what it did.
 *
 * THE PLAN STATISTICS (urgym_mppi_stats: ONE launch of ONE workgroup of 1024 lanes, float64, no atomics, one writer per output; it
 * reads the [E] diagnostics and writes the record, nothing else).  "finite" is r - r == 0 (false for a NaN and either infinity).  Every
 * sum is THE ORDERED SUM ("SAC's entropy coefficient on the device") over ALL parents p < E: a parent that is passed over contributes
 * the term +0.0, so the order depends on E alone.  Every mean is one float64 division of the sum by (double)count, and +0.0 where the
 * count is 0.
 *   planned          = #{p : best_return[p] finite}      (the update writes -inf where no sample's return was finite)
 *   mean_best_return = (the sum of best_return[p] over those p) / planned
 *   nominal_finite   = #{p : nominal_return[p] finite};  mean_nominal_return likewise
 *   gain_count       = #{p : both finite};  mean_gain = (the sum of best_return[p] - nominal_return[p], one subtraction, over those p) / gain_count
 *   mean_ess         = (the sum of ess[p] over all p) / E: a NaN in one parent's ess reaches mean_ess of that record, and nothing else
 *   min_ess          = fmin over all p, with what fmin leaves open fixed: f(a, b) = a is NaN ? b : b is NaN ? a : b < a ? b : a.  Lane t
 *                      starts at NaN and takes p = t, t + 1024, ... ascending as m = f(m, ess[p]); the 1024 results are folded by THE
 *                      ORDERED SUM's levels, level[t] = f(level[t], level[t + s]), s = 512 .. 1.  NaN only where every ess is NaN.
 *   with a:  mean_elite_count = (the sum of (double)elite_count[p] over all p) / E;  threshold_count = #{p : threshold[p] finite},
 *            mean_threshold = (the sum of threshold[p] over those p) / threshold_count.  Without a the three fields are 0.
 * The record is 88 bytes, 8-byte aligned; an array of records is contiguous. */
typedef struct urgym_mppi_stats_record {
  double mean_best_return;
  double mean_nominal_return;
  double mean_gain;
  double mean_ess;
  double min_ess;
  double mean_elite_count;      /* 0 without urgym_mppi_adapt */
  double mean_threshold;        /* 0 without urgym_mppi_adapt */
  int64_t iteration;            /* the caller's tag */
  int32_t num_parents;          /* E */
  int32_t planned;
  int32_t nominal_finite;
  int32_t gain_count;
  int32_t threshold_count;      /* 0 without urgym_mppi_adapt */
  int32_t reserved0;            /* written as 0 */
} urgym_mppi_stats_record;

/* What urgym_sac_train_planned takes beyond the learner, the schedule and the options of urgym_sac_train_clipped: the planner that
 * collects.  The training handle is the planner's source. */
typedef struct urgym_sac_planning {
  void* planner_handle;
  const urgym_mppi* mppi;
  const urgym_mppi_adapt* adapt_or_NULL;
  const urgym_mppi_guide* guide_or_NULL;
  urgym_mppi_explore explore;
  int32_t sync;                       /* != 0: after the updates of every non-idle iteration the guide's actor and critic are reloaded */
  int32_t record_capacity;            /* >= 0 */
  urgym_mppi_stats_record* records;   /* [record_capacity] or NULL: no plan statistics */
  int64_t reserved0;                  /* must be 0 */
} urgym_sac_planning;

/* The single launch; it needs no bound environment.  record_dev is a DEVICE pointer.  Refused, launching and writing nothing: a NULL
 * handle, m or record_dev; num_parents < 1 or above 65,536; a NULL best_return, nominal_return or ess; with a, a NULL elite_count or
 * threshold; a record_dev that is not 8-byte aligned. */
int urgym_mppi_stats(void* handle, const urgym_mppi* m, const urgym_mppi_adapt* a_or_NULL, urgym_mppi_stats_record* record_dev, int64_t iteration, void* stream);

/* THE PLANNED TRAINING CALL.  With K = steps_per_iteration and G = updates_per_iteration, iteration i enqueues
 *   1. the launches of urgym_mppi_collect, or of urgym_mppi_collect_adaptive where adapt_or_NULL is given, with the planning's mppi,
 *      guide and explore, first_draw = the iteration's collect_first_draw (the field the sampled collection draws with), num_steps = K and
 *      first_slot = the iteration's collect_first_slot; with priorities, urgym_per_fill on those slots.  Every step is planned:
 *      schedule->uniform_iterations has no meaning and must be 0;
 *   2. for an iteration that is not idle, the G updates exactly as urgym_sac_train_clipped with the same options launches them
 *      (clipping_or_NULL == NULL: as urgym_sac_train_nstep, _prioritized, _hindsight or urgym_sac_train do);
 *   3. where sync != 0, the iteration is not idle and G > 0: the launch of urgym_actor_load on the planner handle, guide->actor from
 *      learner->actor_adam.param, then the launch of urgym_critic_load on the planner handle, guide->critic from
 *      learner->critic_adam.param (the ONLINE critics) with tau = 1.  One launch each on the call's stream; a part the guide does not
 *      use is skipped (an actor given with policy_samples == 0 and no terminal_value, a critic given without terminal_value); without a
 *      guide nothing is launched;
 *   4. what urgym_sac_train_monitored runs after an iteration (the monitor's fold, its record, the evaluation), and, where
 *      planning->records is given, directly after every urgym_monitor_stats launch that writes monitor record r one urgym_mppi_stats
 *      launch into planning->records[r], with iteration = monitoring->first_iteration + i + 1: the index is the monitor's own
 *      (first_record + the records of the call so far).  The record describes the LAST plan of iteration i: neither the updates nor the
 *      reload touch the buffers it reads.
 * Bit for bit that sequence of single calls.  Two calls of a and b iterations whose counters are handed on leave the bits of one call
 * of a + b iterations; mean is carried between calls.  There is no normalization argument: the planner's actor and critic read raw
 * rows.  No allocation, no host synchronisation; everything is validated before the first launch.
 * Refused, each launching and writing nothing (the message names urgym_sac_train_planned): a NULL handle; everything
 * urgym_sac_train_clipped refuses about the learner, the schedule and the options given; a NULL planning, planner_handle or mppi; a
 * non-zero reserved0; steps_per_iteration == 0 (there is nothing to plan); uniform_iterations != 0; everything
 * urgym_mppi_collect(_adaptive) refuses about the two handles, mppi, adapt, guide, explore, the ring and the draws
 * (collect_first_draw + num_iterations * K > 2^32); planner_handle equal to the training handle or to the evaluation's eval_handle;
 * with sync != 0, a guide's actor whose in_features / hidden_width are not learner->actor_adam's, or a guide's critic whose shape is
 * not learner->critic_adam's; a negative record_capacity; records without monitoring; records with fewer than monitoring->first_record
 * + the record points of the call entries; records not 8-byte aligned. */
int urgym_sac_train_planned(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_planning* planning, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- the temperature from a target effective sample size.  urgym_mppi.lam is one scalar for a whole run and
 * every env, while the scale of the returns moves by orders of magnitude with the critic's terminal value, with the distance to the
 * goal and with fail_cost: a fixed lambda leaves the weights of many parents on a single sample.  The tempered update solves the
 * temperature per parent, at every update, so that the weights have a chosen effective sample size (the temperature of REPS; TD-MPC
 * and MPPI-Generic normalise their scores to the same end).  Added WITHIN ABI version 4: no struct above changed, URGYM_ABI_VERSION did
 * not move, no kernel of the calls above changed, the five symbols below are found by lookup.  A planner that does not use them makes
 * the calls it made and leaves the bits it left.
 *
 * THE EXPONENTIAL.  The weights of THE UPDATE and THE ELITE UPDATE come from the device library's exp, which no host restates bitwise;
 * that is why w is an output a host restatement is given.  A search that compares an effective sample size with a target cannot be
 * handed its exponentials, so the tempered update has its own, texp, float64, for x <= 0, one rounding per operation:
 *     x < -708.0 gives +0.0; otherwise
 *     y = x * LOG2E (1.4426950408889634);  kf = rint(y), to nearest, ties to even;
 *     hi = kf * LN2_HI;  r1 = x - hi;  lo = kf * LN2_LO;  r = r1 - lo     (fdlibm's split: LN2_HI = 6.93147180369123816490e-01,
 *                                                                            LN2_LO = 1.90821492927058770002e-10; hi is exact)
 *     p = c13;  then for n = 12 .. 0:  t = p * r;  p = t + cn             (Horner; cn = 1 / n!, the correctly rounded float64)
 *     scale = the double whose bits are (1023 + (int64) kf) << 52;  texp = p * scale.
 * texp(0) = texp(-0.0) = 1 exactly; kf >= -1021 on the accepted range, so scale and the result are normal.  Within 2 ulp of exp.
 *
 * THE ESS AT A TEMPERATURE.  For parent p, rmax is THE UPDATE's.  sample j is COUNTED where its return is finite, and, with adapt, where
 * it is an elite of THE RANK.  At a temperature lam:  d = r_j - rmax;  x = d / lam;  w_j = texp(x) where j is counted, else +0.0;
 * Z = THE ORDERED SUM of w_j;  Q = THE ORDERED SUM of w_j * w_j;  ess(lam) = (Z * Z) / Q.  The best counted sample weighs 1, so Z >= 1
 * and Q >= 1.
 *
 * THE SEARCH, per parent, with T = ess_target and S = steps:
 *   1. no return is finite: lam = m->lam and w_0 = 1, every other 0, as THE UPDATE puts it; saturated = URGYM_MPPI_TEMPER_NO_RETURN;
 *   2. else if ess(lam_max) < T: lam = lam_max, the target cannot be met; saturated = URGYM_MPPI_TEMPER_AT_MAX;
 *   3. else if ess(lam_min) >= T: lam = lam_min; saturated = URGYM_MPPI_TEMPER_AT_MIN;
 *   4. else lo = lam_min, hi = lam_max, and S times:  q = lo * hi;  mid = sqrt(q), correctly rounded;  e = ess(mid);  e >= T ? hi = mid
 *      : lo = mid.  Then lam = hi; saturated = URGYM_MPPI_TEMPER_SOLVED.  S is fixed and there is no early exit.
 * The weights are w_j at lam.  Everything after them is THE UPDATE's lines, or with adapt THE ELITE UPDATE's, unchanged, on those
 * weights: Z, Q, ess, new_mean, action_out, best_return, nominal_return, w, the shift, and with adapt rank, elite, elite_count,
 * threshold and new_std.  ess[p] is the value the search last accepted.  Without adapt none of urgym_mppi_adapt's arrays is touched. */
#define URGYM_MPPI_TEMPER_SOLVED 0
#define URGYM_MPPI_TEMPER_AT_MAX 1
#define URGYM_MPPI_TEMPER_AT_MIN 2
#define URGYM_MPPI_TEMPER_NO_RETURN 3
#define URGYM_MPPI_TEMPER_STEPS_MAX 64

typedef struct urgym_mppi_temper {
  double ess_target;     /* T, finite, in [1, M] (M = adapt->elites; samples without adapt) */
  double lam_min, lam_max; /* finite, 1e-100 <= lam_min <= lam_max <= 1e100 */
  int32_t steps;         /* S in [1, URGYM_MPPI_TEMPER_STEPS_MAX] */
  int32_t reserved0;     /* must be 0 */
  double* lam_out;       /* [E] the temperature of the last update */
  uint8_t* saturated;    /* [E] URGYM_MPPI_TEMPER_*, may be NULL */
} urgym_mppi_temper;

/* The single launch: ONE workgroup of 1024 lanes per parent; it needs no bound environment.  Refused, launching and writing nothing (the
 * message names the entry point and the argument): everything urgym_mppi_update refuses, and with adapt_or_NULL everything
 * urgym_mppi_update_elite refuses; a NULL temper or lam_out; an ess_target that is not finite or outside [1, M]; bounds that are not
 * finite, outside [1e-100, 1e100] or out of order; steps outside [1, 64]; a non-zero reserved0. */
int urgym_mppi_update_tempered(void* handle, const urgym_mppi* m, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt_or_NULL, void* stream);

/* urgym_mppi_plan_adaptive, urgym_mppi_control_adaptive and urgym_mppi_collect_adaptive with the tempered update in place of the update
 * (adapt_or_NULL == NULL: urgym_mppi_plan(_guided), _control(_guided) and urgym_mppi_collect with it): bit for bit the sequence of single
 * launches.  lam_out and saturated hold what the last update of the call left.  Refused: what the untempered call refuses, and what
 * urgym_mppi_update_tempered refuses about temper. */
int urgym_mppi_plan_tempered(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, uint64_t draw, void* stream);
int urgym_mppi_control_tempered(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream);
int urgym_mppi_collect_tempered(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_temper* temper, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, const urgym_mppi_explore* x, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream);

/* THE PLANNED TRAINING CALL with step 1 the launches of urgym_mppi_collect_tempered; everything else as urgym_sac_train_planned states
 * it, urgym_sac_planning and urgym_mppi_stats_record unchanged.  Refused: what urgym_sac_train_planned refuses (the message names
 * urgym_sac_train_tempered), and what urgym_mppi_update_tempered refuses about temper. */
int urgym_sac_train_tempered(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_planning* planning, const urgym_mppi_temper* temper, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- temporally correlated sampling noise.  THE SAMPLE draws every (horizon step, sample, joint) independently:
 * a sample's net displacement over H steps grows like sigma * sqrt(H), and most of a sequence's energy is step-to-step jitter that the
 * weighted mean cancels.  The coloured sample runs a first-order autoregressive recurrence along the horizon on top of the same draws
 * (the change iCEM makes to CEM; smoothed MPPI and Ornstein-Uhlenbeck exploration do the same in their places).  Added WITHIN ABI
 * version 4: no struct above changed, URGYM_ABI_VERSION did not move, no kernel of the calls above changed, the five symbols below are
 * found by lookup.  A planner that does not use them makes the calls it made and leaves the bits it left.
 *
 * THE COLOURED SAMPLE (urgym_mppi_sample_colored, one launch).  xi[h][n][c] is THE SAMPLE's eps exactly as stated above: the same
 * counters (p, (i << 24) | (h << 16) | j, (uint32)draw, URGYM_MPPI_TAG | block) with blocks 0 and 1, the same words, the same Box-Muller
 * lines, and zero for sample j = 0.  No other Philox block is used.
 *   on the host, once per call, float64:  b = (double)beta;  bb = b * b;  d = 1.0 - bb;  r = sqrt(d), correctly rounded;
 *                                         scale = (float)r.        The kernel is handed beta and scale; the device never forms scale.
 *   the recurrence, float32, one rounding per line:
 *       eps[0][n][c] = xi[0][n][c]
 *       for h >= 1:  a = beta * eps[h - 1][n][c];  b = scale * xi[h][n][c];  eps[h][n][c] = a + b
 *   the action line is THE SAMPLE's:  s = width * eps[h][n][c];  a = mean[h][p][c] + s;  action = fminf(fmaxf(a, -1), 1),
 *       width = m->sigma, or, where an adapt struct is given, std[h][p][c], read as THE ADAPTIVE SAMPLE reads it.
 * Every step has unit marginal variance and lag-1 correlation beta.  Sample 0 stays the nominal sequence: every eps is +0.0.  beta = 0
 * gives eps = xi by value (a -0.0 of xi becomes +0.0 from step 1 on), beta = 1 gives scale = 0 and every step the value of step 0.
 * Both eps -- the coloured values -- and actions are written to urgym_mppi's arrays: THE GUIDE, which executes actor(state) +
 * policy_sigma * eps, gets correlated policy samples with no change, and THE ELITE UPDATE's std, formed from actions, is unchanged too.
 * The result is a function of (seed, draw, i, p, j, h, c, beta) only -- not of E, K or the launch geometry. */
typedef struct urgym_mppi_noise {
  float beta;        /* finite, in [0, 1] */
  int32_t reserved0; /* must be 0 */
} urgym_mppi_noise;

/* The single launch; like urgym_mppi_sample it needs no bound environment.  Refused, launching and writing nothing (the message names
 * the entry point and the argument): everything urgym_mppi_sample refuses, and with adapt_or_NULL everything urgym_mppi_sample_adaptive
 * refuses; a NULL noise; a beta that is not finite or outside [0, 1]; a non-zero reserved0. */
int urgym_mppi_sample_colored(void* handle, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_adapt* adapt_or_NULL, uint64_t draw, int iteration, void* stream);

/* urgym_mppi_plan_tempered, urgym_mppi_control_tempered and urgym_mppi_collect_tempered with the coloured sample as the sample launch of
 * every iteration (temper_or_NULL == NULL: urgym_mppi_plan_adaptive, _control_adaptive and _collect_adaptive with it; adapt_or_NULL ==
 * NULL as well: the plain or guided calls with it).  Where adapt_std is set and i >= 1 that launch follows the same copy of new_std into
 * std and runs with the adapt struct; otherwise it runs with m->sigma.  Everything else is the untouched call: bit for bit the sequence
 * of single launches.  Refused: what the call without noise refuses, and what urgym_mppi_sample_colored refuses about noise. */
int urgym_mppi_plan_colored(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, uint64_t draw, void* stream);
int urgym_mppi_control_colored(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream);
int urgym_mppi_collect_colored(void* source_handle, void* planner_handle, const urgym_mppi* m, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_adapt* adapt_or_NULL, const urgym_mppi_guide* guide_or_NULL, const urgym_mppi_explore* x, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream);

/* THE PLANNED TRAINING CALL with step 1 the launches of urgym_mppi_collect_colored; everything else as urgym_sac_train_planned (with
 * temper_or_NULL: urgym_sac_train_tempered) states it.  Refused: what that call refuses (the message names urgym_sac_train_colored), and
 * what urgym_mppi_sample_colored refuses about noise. */
int urgym_sac_train_colored(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_planning* planning, const urgym_mppi_noise* noise, const urgym_mppi_temper* temper_or_NULL, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- the training call with behaviour cloning: in every update the launch of urgym_sac_policy_terms is the one
 * of urgym_sac_policy_terms_cloned, with action_pi = learner->action_pi, action_data = learner->batch.action (the ring's action: the
 * executed one, under every gather), bc_scale = (float)(1.0 / M), and weight, scale_by_q and q_filter as given here.  Update u of the call
 * writes slot u of bc_loss, bc_weight and bc_rows.  Nothing else in the sequence moves: an update stays thirteen launches (more with
 * the other options, as they state), and the actor's backward pass, Adam, the ring and the planner are unchanged. */
typedef struct urgym_sac_cloning {
  float weight;        /* finite, >= 0 */
  int32_t scale_by_q;  /* 0 or 1 */
  int32_t q_filter;    /* 0 or 1 */
  int32_t reserved0;   /* must be 0 */
  float* bc_loss;      /* [updates of the call] */
  float* bc_weight;    /* the same */
  int32_t* bc_rows;    /* the same */
} urgym_sac_cloning;

/* Every option after `cloning` may be NULL and is then as in the call without it: planning (with temper and noise, which need it),
 * normalization, clipping, at most one of nstep, prioritized and hindsight, evaluation, monitoring.  Refused, nothing launched (the
 * message names urgym_sac_train_cloned): NULL cloning; what urgym_sac_policy_terms_cloned refuses about weight, the two flags and
 * reserved0; a NULL bc_loss, bc_weight or bc_rows where the call holds an update; temper or noise without planning; normalization
 * together with planning; and what the call with the same options and no cloning refuses. */
int urgym_sac_train_cloned(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_cloning* cloning, const urgym_sac_planning* planning_or_NULL, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_noise* noise_or_NULL, const urgym_normalization* normalization_or_NULL, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- the demonstration ring: a second replay ring that collection never overwrites, a fixed part of every
 * minibatch drawn from it, and cloning on those rows only (Nair et al. 2018 keep such a buffer and clone its rows; RLPD, Ball et al. 2023,
 * draws half of every batch from offline data; with the whole batch from it, TD3+BC).  Opt-in and added WITHIN ABI version 4: no struct
 * above changed, no symbol above changed, URGYM_ABI_VERSION did not move, the three symbols below (urgym_replay_sample_mixed,
 * urgym_sac_policy_terms_cloned_masked, urgym_sac_train_demonstrated) are found by lookup.  The library keeps no state: the
 * demonstration ring, its cursor and its fill level are the caller's, like the learner's own. */

/* The last counter word of a draw from the demonstrations.  It meets none of the tags in use: 0x504F4C00 | block (policy noise),
 * 0x52504C00 (replay), 0x50455200 (prioritized replay), 0x4D505000 | block (the planner), the reset sampler's blocks 0..4. */
#define URGYM_DEMO_TAG 0x44454D00u   /* "DEM\0" */

typedef struct urgym_replay_demonstrations {
  urgym_replay_ring ring;  /* a ring of the SAME env kind, every array [C_d][N_d][...]; truncated / is_success may be NULL */
  int32_t num_envs;        /* N_d >= 1; need not be the handle's N */
  int32_t oldest_slot;     /* in [0, C_d) */
  int32_t filled_steps;    /* in [1, C_d] */
  int32_t count;           /* D in [0, count]: rows 0 .. D-1 of the minibatch come from here */
} urgym_replay_demonstrations;

/* urgym_replay_sample whose first D = demo->count rows come from the demonstrations, in ONE gather launch on `stream`.
 * Rows i >= D are exactly urgym_replay_sample's row i: the same Philox call, counter (i, draw lo, draw hi, 0x52504C00), the same
 *   e = (w * size) >> 64 and the same slot and env arithmetic, so they are bitwise the rows that call gathers at the same (seed, draw) and
 *   position; with D == 0 every output is bitwise that call's.
 * Rows i < D draw from the demonstrations: the same key, counter (i, draw lo, draw hi, URGYM_DEMO_TAG);  w = (w0 << 32) | w1;
 *   size_d = filled_d * N_d;  e = (w * size_d) >> 64;  slot = (oldest_d + e / N_d) % C_d;  env = e % N_d;  index = slot * N_d + env,
 *   an entry of the DEMONSTRATION ring (batch->index[i] holds it).
 * The result is a function of (seed, draw, i, size, size_d) alone: not of count, not of the launch geometry.  source_out[i] is 1 for a
 * demonstration row and 0 otherwise.  The geometry is urgym_replay_sample's (64 samples per wave, 16 lanes per row, four rows per
 * round); in a wave whose samples straddle D each group of 16 lanes reads the ring of ITS sample.
 * ur_gym_amd.evaluation.mixed_indices restates the draw.
 * Refused (URGYM_ERR_ARG, nothing is launched, nothing is written): everything urgym_replay_sample refuses; demo == NULL; a NULL
 * required pointer in demo->ring or capacity_steps <= 0 there; reserved0 != 0 in demo->ring; num_envs < 1; oldest_slot outside [0, C_d);
 * filled_steps outside [1, C_d]; demo->count outside [0, count]; filled_steps * num_envs not below 2^63; truncated or is_success asked for
 * while either ring does not keep it. */
int urgym_replay_sample_mixed(void* handle, const urgym_replay_ring* ring, int oldest_slot, int filled_steps, uint64_t seed, uint64_t draw, int count, const urgym_replay_batch* batch, const urgym_replay_demonstrations* demo, uint8_t* source_out /* [count] or NULL */, void* stream);

/* urgym_sac_policy_terms_cloned with ONE change to the verdict of a row:
 *     cloned[m] = row_mask[m] != 0 && (q_filter ? qd > q_min[m] : true)
 * Everything else is that call's, line by line: absq and mean_abs stay over ALL rows; bc_loss stays the ordered mean over all count rows
 * with +0.0f for a row that is not cloned; rows counts the cloned rows; a row that is not cloned gets d_action_out bitwise
 * urgym_sac_policy_terms'.  ONE launch of ONE workgroup of 1024 lanes, like the kernel it stands in for.  A mask of all ones gives
 * urgym_sac_policy_terms_cloned's bits; a mask of all zeros gives urgym_sac_policy_terms' bits, bc_loss = +0.0, rows = 0, and bc_weight
 * still written.  action_pi and action_data of a row the mask excludes reach no output.  d_action_out may be dqmin_da itself.
 * Refused (URGYM_ERR_ARG, nothing is launched, nothing is written): what urgym_sac_policy_terms_cloned refuses, and a NULL row_mask. */
int urgym_sac_policy_terms_cloned_masked(void* handle, const urgym_sac_policy_args* args, const urgym_sac_clone_args* clone, const uint8_t* row_mask /* [count], required */, void* stream);

/* The training call with demonstrations.  In every update the gather launch is urgym_replay_sample_mixed's, at the (seed, draw) the plain
 * call would use, with source_out = source; and, with cloning and clone_demonstrations_only, the policy-terms launch is
 * urgym_sac_policy_terms_cloned_masked's with row_mask = source.  Nothing else in the sequence moves: an update stays thirteen launches
 * (more with the other options, as they state).  bc_scale stays (float)(1.0 / M), so a weight means the same at every demonstration
 * share.  urgym_norm_batch normalizes the gathered batch as it does today: demonstration rows are RAW rows like any other, and the running
 * statistics still come from the learner's own collection only (no demonstration row is ever folded).  There is no nstep, prioritized
 * or hindsight parameter: each of those has a gather of its own, and the pairs are out of scope. */
typedef struct urgym_sac_demonstrating {
  urgym_replay_demonstrations demonstrations;  /* count = D rows of each of the learner's M */
  uint8_t* source;                             /* [M] scratch: the gather's source_out */
  int32_t clone_demonstrations_only;           /* 0 or 1; 1 needs cloning */
  int32_t reserved0;                           /* must be 0 */
} urgym_sac_demonstrating;

/* Every option after `demonstrating` may be NULL and is then as in the call without it.  Refused, nothing launched (the message names
 * urgym_sac_train_demonstrated): NULL demonstrating; what urgym_replay_sample_mixed refuses; D > M; a NULL source where the call holds an
 * update; clone_demonstrations_only other than 0 or 1, or 1 without cloning; reserved0 != 0; and what the call with the same options and
 * no demonstrations refuses. */
int urgym_sac_train_demonstrated(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_demonstrating* demonstrating, const urgym_sac_cloning* cloning_or_NULL, const urgym_sac_planning* planning_or_NULL, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_noise* noise_or_NULL, const urgym_normalization* normalization_or_NULL, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- advantage-weighted cloning in the policy loss.  The Q-filter above is a hard gate: a row is cloned whole or
 * not at all, and it drops nearly every demonstration as soon as the critics rate the policy's own action marginally higher.  The soft
 * form weights each cloned row by exp(advantage / temperature), normalised over the batch: AWAC (Nair et al. 2020; rlkit's
 * softmax(A / beta) * batch_size) and the exponential variant of CRR (Wang et al. 2020), whose binary variant the Q-filter is.  Every row
 * still pulls, better rows pull harder, and one temperature moves between "every row alike" and "the best row alone".  Added WITHIN ABI
 * version 4: no struct above changed, no symbol above changed, URGYM_ABI_VERSION did not move, the two symbols below
 * (urgym_sac_policy_terms_weighted, urgym_sac_train_weighted) are found by lookup.  All pointers are DEVICE pointers. */
typedef struct urgym_sac_advantage_args {
  float temperature;         /* finite, > 0 */
  float max_weight;          /* > 0, finite or +infinity (no cap) */
  const uint8_t* row_mask;   /* [count], or NULL: every row is marked */
  float* adv_ess_out;        /* [1] */
  float* adv_max_out;        /* [1] */
  int32_t* adv_clipped_out;  /* [1] */
  int32_t reserved0;         /* must be 0 */
} urgym_sac_advantage_args;

/* urgym_sac_policy_terms_cloned (q_filter = 0) with a weight per row in the place of the verdict.  ONE launch of ONE workgroup of 1024
 * lanes, in its place, in three sweeps of the rows (lane t takes rows t, t + 1024, ...) with the folds between them; nothing per row is
 * kept between the sweeps.  With q = args->q (the ONLINE critics at the REPLAYED action) and q_min = args->q_min (at the policy's):
 *   per row m:
 *     qd      = q[1][m] < q[0][m] ? q[1][m] : q[0][m]
 *     A[m]    = qd - q_min[m]                                   one float32 subtraction
 *     elig[m] = (row_mask == NULL || row_mask[m] != 0) && isfinite(A[m])      a NaN or an infinity on either side: not eligible
 *   sweep 1:  n = the number of eligible rows;  A_max = the largest A over them (float32 comparisons of finite values: any order)
 *   sweep 2, float64:
 *     d = (double)A[m] - (double)A_max;  x = d / (double)temperature          never positive
 *     e[m] = THE EXPONENTIAL of "the temperature from a target effective sample size" at x (+0.0 below -708; exactly 1 on the A_max
 *            row), +0.0 where the row is not eligible
 *     Z = THE ORDERED SUM of e over all count rows;  Q = THE ORDERED SUM of e * e;  the four sums of urgym_sac_policy_terms_cloned
 *     (the two critic terms, the actor's, absq) are formed as there, over ALL rows
 *   scalars:  mean_e = Z / (double)n;  mean_abs and w = scale_by_q ? weight * mean_abs : weight as in urgym_sac_policy_terms_cloned
 *   sweep 3, per row (e[m] formed again):
 *     u = e[m] / mean_e;  v = u > (double)max_weight ? (double)max_weight : u;  a[m] = (float)v       +0.0f where not eligible
 *     clipped counts the rows with u > max_weight
 *     h[m] = 0.5f * s as in urgym_sac_policy_terms_cloned where the row is eligible, +0.0f where it is not
 *     bc_loss = ordered mean over all count rows of the float32 product a[m] * h[m]
 *     g = dqmin_da[m][k] * scale
 *     not eligible:  d_action_out[m][k] = g                     bitwise what urgym_sac_policy_terms writes
 *     eligible:      wr = w * a[m];  t = d_k * wr;  u = t * bc_scale;  d_action_out[m][k] = g + u
 *   critic_loss_out and actor_loss_out are bitwise urgym_sac_policy_terms'; bc_loss_out[0] = bc_loss; bc_weight_out[0] = w;
 *   bc_rows_out[0] = n; adv_ess_out[0] = (float)((Z * Z) / Q), the effective number of rows the weights spread over, in [1, n];
 *   adv_max_out[0] = a of the A_max row = (float)min(1 / mean_e, max_weight), the largest weight; adv_clipped_out[0] = clipped.
 *   With n == 0 nothing is divided: every a is +0.0f, d_action_out is urgym_sac_policy_terms' bits, bc_loss, adv_ess and adv_max are
 *   +0.0f and both counts are 0.
 * With the largest finite temperature and max_weight = +infinity every e is 1 for ordinary advantages, every a is exactly 1.0f and
 * wr = w: the bits of urgym_sac_policy_terms_cloned (with a mask, of urgym_sac_policy_terms_cloned_masked) at q_filter = 0.
 * A NaN in action_pi or action_data of an eligible row reaches that row of d_action_out and bc_loss_out only; the actions of a row that
 * is not eligible are never read.  A row's six elements are read from dqmin_da before they are written: d_action_out may be dqmin_da.
 *
 * Refused (URGYM_ERR_ARG, nothing is launched, nothing is written): what urgym_sac_policy_terms_cloned refuses; clone->q_filter != 0
 * (the two gates are alternatives); NULL advantage or a NULL output pointer in it; temperature not finite or not > 0; max_weight a NaN
 * or not > 0; reserved0 != 0. */
int urgym_sac_policy_terms_weighted(void* handle, const urgym_sac_policy_args* args, const urgym_sac_clone_args* clone, const urgym_sac_advantage_args* advantage, void* stream);

/* The training call with advantage-weighted cloning: in every update the policy-terms launch is urgym_sac_policy_terms_weighted's, with
 * the clone args urgym_sac_train_cloned forms, temperature and max_weight as given here, and row_mask = demonstrating->source where
 * demonstrating is given with clone_demonstrations_only, NULL otherwise.  Update u of the call writes slot u of adv_ess, adv_max and
 * adv_clipped beside cloning's three.  Nothing else in the sequence moves: an update stays thirteen launches. */
typedef struct urgym_sac_weighting {
  float temperature;     /* finite, > 0 */
  float max_weight;      /* > 0, finite or +infinity */
  int32_t reserved0;     /* must be 0 */
  float* adv_ess;        /* [updates of the call] */
  float* adv_max;        /* the same */
  int32_t* adv_clipped;  /* the same */
} urgym_sac_weighting;

/* `weighting` and `cloning` are required; every option after them may be NULL and is then as in the call without it.  Refused, nothing
 * launched (the message names urgym_sac_train_weighted): NULL weighting or cloning; cloning->q_filter != 0; what
 * urgym_sac_policy_terms_weighted refuses about temperature, max_weight and reserved0; a NULL adv_ess, adv_max or adv_clipped where the
 * call holds an update; what urgym_sac_train_cloned and urgym_sac_train_demonstrated refuse, demonstrating together with nstep,
 * prioritized or hindsight among it. */
int urgym_sac_train_weighted(void* handle, const urgym_sac_learner* learner, const urgym_sac_schedule* schedule, const urgym_sac_weighting* weighting, const urgym_sac_cloning* cloning, const urgym_sac_demonstrating* demonstrating_or_NULL, const urgym_sac_planning* planning_or_NULL, const urgym_mppi_temper* temper_or_NULL, const urgym_mppi_noise* noise_or_NULL, const urgym_normalization* normalization_or_NULL, const urgym_sac_clipping* clipping_or_NULL, const urgym_sac_nstep* nstep_or_NULL, const urgym_sac_prioritized* prioritized_or_NULL, const urgym_sac_hindsight* hindsight_or_NULL, const urgym_sac_evaluation* evaluation_or_NULL, const urgym_sac_monitoring* monitoring_or_NULL, void* stream);

/* ---- a scripted reach controller on the device: damped least-squares inverse kinematics.  The planner above is
 * the only demonstrator and needs a second environment of E * K envs; a resolved-rate controller -- Jacobian, damped least squares, a
 * step toward the goal pose -- is one small launch per control step.  It does not see obstacles: its failures are collisions on the way.
 * Opt-in and added WITHIN ABI version 4: no struct above changed, no symbol above changed, URGYM_ABI_VERSION did not move, the three
 * symbols below are found by lookup.  The library keeps no state for it.
 *
 * THE CHAIN WALK.  From q[0..5] of env n (the bound float64 state), with T = identity and for joint k = 0 .. 5 in turn, as the step
 * kernels walk the URDF chain (data/ur5e_model.h):  o_k = T.t + T.R xyz_k;  T.t = o_k;  G = T.R rot_k;  z_k = the third column of G;
 * T.R = G Rz(q_k).  The end-effector frame is link 6's: p = T.t, R = T.R.
 * THE JACOBIAN, geometric, 6 x 6:  J[0:3][k] = z_k x (p - o_k);  J[3:6][k] = z_k.
 * THE ERROR.  e[0:3] = goal[0:3] - p.  For the kinds whose goal has six floats: q_goal = pybullet's getQuaternionFromEuler(goal[3:6]),
 * q_ee = the quaternion of R (largest-diagonal branch), d = q_goal (x) conj(q_ee), negated where d.w < 0 (the shortest arc);
 * n = |d.xyz|;  ang = 2 atan2(n, d.w);  e[3:6] = d.xyz * (ang / n), or 2 d.xyz where n < 1e-12.  The target is the pose whose pybullet
 * Euler read-out equals the goal; the task's own angular_distance reads the same three numbers as 'ZYX' angles, a different metric with
 * the same zero.  For UR5ObsReach-v1 (a goal of three floats) rows 3..5 of e and of J are zero and goal rows 3..5 are not read.
 * THE STEP, float64, one operation per line (ur_gym_amd/csrc/urgym_ik.h):  A = J J^T + damping^2 I (its lower triangle);  A = L L^T by
 * Cholesky, no pivoting (A is symmetric positive definite by construction);  L w = e;  L^T y = w;  dq = gain * (J^T y);
 * a = dq / cfg.action_scale;  m = max_c |a_c|;  where m > 1 every component is divided by m (the direction is kept; nothing is clamped
 * per joint);  action[n][c] = (float)a_c, the one rounding to float32.  A row whose q or goal (the rows its kind reads) holds a value
 * that is not finite, or whose a does not stay finite, gets six +0.0f.
 * THE EXPLORATION NOISE is THE EXECUTE LINE of "planner-collected experience" restated on this action:  s = explore_sigma * eps[n][c];
 * a' = action[n][c] + s;  action[n][c] = fminf(fmaxf(a', -1), 1).  eps is Box-Muller with THE SAMPLE's pairing of the words (pairs 0, 1, 2
 * of w0 .. w5, m = w >> 8, u1 = (m1 + 1) 2^-24, the angle 2 pi m2 2^-24, r = sqrt(-2 ln u1), the pair (r cos, r sin)) but NOT its library
 * calls: ln, cos and sin are float64 lines of their own (ur_gym_amd/csrc/urgym_ik.h: ik_ln_unit -- frexp, then the series of 2 atanh
 * up to s^13 -- and ik_sincospi -- the angle reduced exactly to a quadrant and |x| <= pi / 4, Taylor polynomials up to x^13 and x^14),
 * good to 1e-13, and r cos and r sin are rounded once to float32.  frexp, rint, sqrt and the basic operations are exact or correctly
 * rounded everywhere, so explore_eps is, bit for bit, what ur_gym_amd.evaluation.ik_explore_noise computes on the host (logf and cospif
 * of a device library cannot be restated that way: the planner's own eps is held to a bound instead).  The words are those of
 * Philox4x32-10 with key = (seed & 0xFFFFFFFF, seed >> 32) and
 *   counter = (n, 0, (uint32)draw, URGYM_IK_TAG | block),  block = 0, 1      (w0 .. w3 from block 0, w4 and w5 from block 1).
 * URGYM_IK_TAG meets none of the tags in use: 0x504F4C00 | block (policy noise), 0x52504C00 (replay), 0x50455200 (prioritized replay),
 * 0x4D505000 | block (the planner), 0x44454D00 (demonstrations), the reset sampler's blocks 0..4.  With explore_sigma == 0 no word is
 * drawn, the action keeps the bits THE STEP gave it and explore_eps, where given, receives zeros.  The noise is a function of
 * (seed, draw, n, c) only.
 * The launch (urgym_ik.hip): one lane per env, 256 lanes a workgroup, q and goal read SoA, no LDS, no atomics, one writer per output;
 * it writes actions and explore_eps only.  Row n is a function of env n's q and goal alone -- not of N or the launch geometry.
 * ur_gym_amd.evaluation.ik_actions / ik_explore_noise restate it. */
#define URGYM_IK_TAG 0x494B5200u   /* "IKR\0" */

typedef struct urgym_reach_controller {
  double damping;        /* finite, in [1e-2, 10] */
  double gain;           /* finite, in (0, 10] */
  uint64_t seed;         /* the Philox key of the exploration noise */
  float explore_sigma;   /* finite, >= 0 */
  int32_t reserved0;     /* must be 0 */
  float* explore_eps;    /* [N][6] or NULL */
} urgym_reach_controller;

/* The single launch.  No allocation, no host synchronisation; everything is validated before the launch.  Refused (URGYM_ERR_ARG,
 * nothing is launched, nothing is written): a NULL handle; a NULL c; a handle without bound buffers; a NULL actions; a non-zero
 * reserved0; damping not finite or outside [1e-2, 10]; gain not finite or outside (0, 10]; explore_sigma not finite or < 0;
 * draw >= 2^32. */
int urgym_controller_actions(void* handle, const urgym_reach_controller* c, uint64_t draw, float* actions /* [N][6] */, void* stream);

/* THE CLOSED LOOP: record pass 0 (THE RECORD of "sampling-based MPC on the device", without a mean to zero), then for t < num_steps:
 * the action launch with draw = first_draw + t, written into row t of traj->action; urgym_step(handle, that row); record pass t + 1 --
 * 2 num_steps + 1 launches besides the steps' own.  Bit for bit that sequence of single calls.  The library allocates nothing, so the
 * action rows are the trajectory's: a call without traj->action (a NULL trajectory among them) has nowhere to put them and is refused --
 * a loop that keeps no record is urgym_controller_collect into a ring of one slot.  c->explore_eps, where given, holds the noise of the
 * LAST step.  Refused (URGYM_ERR_ARG, nothing launched): everything urgym_controller_actions refuses about handle and c; num_steps < 1;
 * first_draw + num_steps > 2^32; a summary array of traj without episode_done; a NULL traj or traj->action; (URGYM_ERR_STATE) a handle
 * that has observed nothing. */
int urgym_controller_control(void* handle, const urgym_reach_controller* c, uint64_t first_draw, int num_steps, const urgym_trajectory* traj_or_NULL, void* stream);

/* THE COLLECTION of "planner-collected experience" with the plan, the record pass and the execute launch replaced by the action launch.
 * With C = ring->capacity_steps and slot(t) = (first_slot + t) % C, for t < num_steps: store pass t (urgym_rollout_collect's store
 * launch, unchanged); the action launch with draw = first_draw + t and actions = the action rows of slot(t); urgym_step(handle, those
 * rows).  After the loop store pass num_steps.  2 num_steps + 1 launches besides the steps' own.  A slot is complete when the call
 * returns; num_steps may exceed C (the ring wraps); no launch writes a slot other than those of the call's own steps.  Two calls of a and
 * b steps, the second with first_draw + a and the slot after the first's last, leave the bits of one call of a + b steps.  With
 * explore_sigma == 0 the ring's action, reward and flags are, bit for bit, what urgym_controller_control records in its trajectory.
 * c->explore_eps, where given, holds the noise of the LAST step.  Refused (URGYM_ERR_ARG, nothing launched, nothing written):
 * everything urgym_controller_actions refuses about handle and c; everything urgym_rollout_collect refuses about the ring, first_slot and
 * num_steps; first_draw + num_steps > 2^32; (URGYM_ERR_STATE) a handle that has observed nothing. */
int urgym_controller_collect(void* handle, const urgym_reach_controller* c, uint64_t first_draw, int num_steps, const urgym_replay_ring* ring, int first_slot, void* stream);

/* Replaces Reach*.set_goal / set_goal_and_obstacle (reach.py:202-204, 328-335, 702-713): the caller has
 * overwritten goal / obst_start / obst_end (and possibly q) for the masked envs; this recomputes obstacle pose,
 * velocity, collision, link_dist and the observation for them, leaving step_count untouched. */
int urgym_refresh(void* handle, const uint8_t* mask_dev, void* stream);

/* The caller has edited episode_id (or step_count) of some envs in the bound buffers: the episode records the library keeps ready
 * for the inline auto-reset may no longer match, so the next max_episode_steps + 1 steps carry the fallback
 * launches that reset such envs with a kernel.  Every record and every pending refill entry is discarded (each env takes the
 * fallback at its first finish and leaves it with fresh records), after a device synchronisation: call it between steps, like the
 * edit itself.  Not needed after urgym_bind / urgym_reset (they do it themselves). */
int urgym_invalidate_records(void* handle);

/* The caller has written an obstacle twist of its own into rows 0..5 of obst_vel (a set_state-style harness; the reference's
 * counterpart is assigning task.velocity before sim.step, reach.py:745-747): re-derives rows 6..8 -- the base displacement of one
 * env step under that twist (pyb_setup.py:52-55, 20 sub-steps) -- for every env.  Leaves everything else alone (urgym_refresh would
 * teleport the obstacle to obst_start and recompute the twist from start / end).  No-op for UR5OriReach-v1. */
int urgym_derive_obstacle_motion(void* handle, void* stream);

/* Unit probe of the device closest-distance routine (what p.getClosestPoints computes, pyb_setup.py:401-452): one query per
 * entry, all pointers are DEVICE pointers.  type: 0 hull (par[0] = PyBullet link 1..6), 1 cylinder-Z (radius, height),
 * 2 box (half extents), 3 sphere (radius); pose = xyz + quaternion xyzw; out_dist = signed distance incl. Bullet margins.
 * Used by the parity tests to reach the hull<->box and hull<->hull paths directly. */
int urgym_probe_closest(void* handle, int count, const int* type_a, const double* par_a, const double* pose_a, const int* type_b,
                        const double* par_b, const double* pose_b, double threshold, double* out_dist, int* out_info, void* stream);

/* Unit probe of the device pose distances (utils.distance, utils.py:5-31; utils.angular_distance, utils.py:34-69 -- what
 * is_success and compute_reward call, reach.py:212-236): a6 / b6 are [count][6] float64 poses xyz + rpy (DEVICE pointers),
 * out2[count][2] = {distance, angular distance}.  Lets the fixtures generated by the reference's own utils.py reach the
 * device code directly (tests/test_gpu_parity.py). */
int urgym_probe_pose_distance(void* handle, int count, const double* a6, const double* b6, double* out2, void* stream);

/* Average device time (microseconds) of the step launch over the calls since the last query, measured with hipEvents on the
 * launch stream; returns <0 if timing was not enabled.  enable = k > 1 times every k-th step only: a pair of events costs the
 * stream about 6 us per step, i.e. measuring every launch slows the thing measured by ~3 % (bench.py samples every 8th). */
int urgym_enable_timing(void* handle, int enable);
int urgym_query_timing(void* handle, double* step_kernel_us, double* reset_kernel_us, int* launches);

/* Kept for ABI v2 callers: always reports 0.  The search for the next episodes of the envs that finished used to run as a launch
 * of its own on a side stream; it now rides in the step launch (its workgroups follow the step workgroups in one grid), so
 * urgym_query_timing()'s step figure includes it. */
int urgym_query_refill_timing(void* handle, double* refill_us);

const char* urgym_last_error(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* URGYM_H */
