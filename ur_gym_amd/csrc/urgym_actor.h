// urgym_actor.h — seam between two translation units of liburgym_hip.so: urgym_actor.hip (the actor / record kernels, compiled
// with fma contraction) offers these; urgym_policy_abi.hip (the learner's entry points) calls them.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urgym.h"

namespace urgym {

struct Actor;  // packed weights and scratch on the device (urgym_actor.hip)

// Where a pass reads the environment's outputs (the bound buffers of the handle)
struct ActorEnv {
  int N, obs_dim, goal_dim, auto_reset;
  const float *observation, *achieved_goal, *desired_goal, *reward, *final_observation;
  const uint8_t *terminated, *truncated, *is_success, *collision;
};

// The records of one pass of a rollout (every pointer may be null).  Pass k runs before step k: obs / ach / des are the rows of
// step k (what the actor sees now), reward .. final_obs the rows of step k - 1 (what that step left in the bound buffers); the
// episode arrays are per env.  k = 0 initialises the episode summary; k = num_steps is the last pass, without a forward pass.
struct ActorPass {
  float *obs, *ach, *des;
  float* reward;
  uint8_t *terminated, *truncated, *is_success, *collision;
  float* final_obs;
  double* ep_return;
  int32_t* ep_last;
  uint8_t *ep_success, *ep_done;  // ep_done: the summary's own state, never null while one of the three others is recorded
  int k, num_steps;
};

// checks desc (shape only; in_features is compared with `in_features`), uploads the packed weights; on failure writes a message
int actor_create(const urgym_actor_desc* desc, int in_features, int num_envs, Actor** out, char* err, size_t err_len);
void actor_destroy(Actor* a);
int actor_in_features(const Actor* a);
float* actor_action_scratch(Actor* a);  // [N][6], the actions of a rollout that does not record them
uint8_t* actor_done_scratch(Actor* a);  // [N], ActorPass::ep_done of a rollout that does not record it

// forward pass (actions != nullptr) and / or records (pass != nullptr) in ONE launch on `s`
void actor_launch(Actor* a, const ActorEnv& env, float* actions, const ActorPass* pass, hipStream_t s);

// How one pass samples (include/urgym.h, "the stochastic half"): the rows of this pass in the sample records, each may be null
struct ActorSample {
  int mode;  // URGYM_SAMPLE_*
  uint64_t seed, draw;
  float *log_prob, *noise, *mean_action, *log_std;
};

// attaches the log_std head ([6][hidden], [6], host pointers); the caller has made sure that no launch is reading the weights
int actor_set_log_std(Actor* a, const float* w, const float* b, char* err, size_t err_len);
bool actor_has_log_std(const Actor* a);

// The packed buffer p1 | p2 | small (device, `floats` long) and the shape it was packed for: what a reload (urgym_weights.h) writes.
struct ActorPacked {
  float* weights;
  size_t floats;
  int in_features, hidden;
};
ActorPacked actor_packed(Actor* a);
void actor_mark_log_std(Actor* a);  // a reload has filled the log_std head

// actor_launch with sampled actions (actions != nullptr).  UNIFORM runs no forward pass; MEAN and GAUSSIAN need the log_std head.
void actor_launch_sampled(Actor* a, const ActorEnv& env, float* actions, const ActorPass* pass, const ActorSample& how, hipStream_t s);

// The parameter gradients of the actor summed over M rows (urgym_actor_backward.hip; include/urgym.h, urgym_actor_parameter_gradients):
// the rows, how the pass samples (MEAN or GAUSSIAN; the noise counter's env word is the row index), the upstream gradient in one of
// its two forms (d_action, with d_log_prob or null; or d_mu and d_log_std), the eight output tensors in the order of
// urgym_actor_params_dev, the optional per-row outputs and the workspace.
struct ActorBackwardCall {
  const float *observation, *achieved_goal, *desired_goal;
  int M, obs_dim, goal_dim;
  int mode;  // URGYM_SAMPLE_MEAN or _GAUSSIAN
  uint64_t seed, draw;
  const float *d_action, *d_log_prob;  // the SAMPLE form: d_action != null
  const float *d_mu, *d_log_std;       // the HEADS form: both != null
  float* grad[8];
  float *action, *log_prob, *noise, *log_std, *out_d_mu, *out_d_log_std, *std;  // each may be null
  float* workspace;  // actor_backward_workspace_bytes(a, M), 16-byte aligned
};
// the widths the per-row kernel is built for (hidden_width <= 256)
bool actor_backward_supported(Actor* a);
uint64_t actor_backward_workspace_bytes(Actor* a, int count);
// the launches of one call: 2 up to 1024 rows, 3 above
int actor_backward_launches(int count);
// on `s`; the caller has validated `call`, actor_backward_supported(a) and the log_std head
void actor_backward_launch(Actor* a, const ActorBackwardCall& call, hipStream_t s);
constexpr int ACTOR_BACKWARD_MAX_COUNT = 65536;  // urgym_actor_backward.hip asserts it against urgym_backward_map.h

}  // namespace urgym
