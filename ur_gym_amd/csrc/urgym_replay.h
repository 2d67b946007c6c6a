// urgym_replay.h — seam between urgym_replay.hip (the store pass and the gather of the device replay ring, compiled with the flags of
// urgym_actor.hip) and urgym_policy_abi.hip (the learner's entry points), beside urgym_actor.h and urgym_critic.h.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urgym.h"

namespace urgym {

// One store pass of urgym_rollout_collect.  Pass k runs before the actor of step k: the live rows are at once the s of step k (copied
// into obs / ach / des of slot k; null in the last pass) and the s' of step k - 1, whose outcome goes into the `out` pointers of slot
// k - 1 (next_obs null in the first pass: no outcome part).  All pointers are already offset to their slot.
struct ReplayStore {
  int N, obs_dim, goal_dim, auto_reset;
  // the bound buffers
  const float *observation, *achieved_goal, *desired_goal, *reward, *final_observation, *final_achieved_goal, *final_desired_goal;
  const uint8_t *terminated, *truncated, *is_success;
  // slot k
  float *obs, *ach, *des;
  // slot k - 1
  float *reward_out, *next_obs, *next_ach, *next_des;
  uint8_t *terminated_out, *truncated_out, *is_success_out;  // the last two may be null (the ring does not keep them)
};

// ONE launch on `s`; the caller has validated `p`
void replay_store_launch(const ReplayStore& p, hipStream_t s);

// One minibatch (urgym_replay_sample): `ring` and `batch` as the caller gave them, validated
struct ReplayGather {
  int N, obs_dim, goal_dim, capacity, oldest_slot, count;
  uint64_t size;  // filled_steps * N
  uint64_t seed, draw;
  urgym_replay_ring ring;
  urgym_replay_batch batch;
};

// ONE launch on `s`
void replay_gather_launch(const ReplayGather& p, hipStream_t s);

// One minibatch of multi-step returns (urgym_replay_sample_nstep): the gather above plus the window of urgym_nstep.h, validated
struct ReplayGatherNstep {
  ReplayGather g;
  int n_steps, filled_steps;  // g.size = filled_steps * g.N
  float gamma;
  float* discount;      // [count]
  int32_t* steps;       // [count] or null
  int64_t* last_index;  // [count] or null
};

// ONE launch on `s`
void replay_gather_nstep_launch(const ReplayGatherNstep& p, hipStream_t s);

// One minibatch with relabelled goals (urgym_replay_sample_hindsight; urgym_her.hip, a unit of its own): the one-step gather's draw
// and geometry plus the rule of urgym_her.h, validated
struct ReplayGatherHindsight {
  ReplayGather g;
  int filled_steps;  // g.size = filled_steps * g.N
  int strategy, horizon;
  uint64_t relabel_threshold;
  // the re-scoring rule's numbers, from the handle's urgym_config (HerRule of urgym_her.h)
  double distance_threshold, ori_threshold, w_collision, w_success, w_distance, w_orientation;
  int additive;
  int64_t* goal_index;  // [count] or null
  double* pose_terms;   // [count][4] or null
};

// ONE launch on `s`
void replay_gather_hindsight_launch(const ReplayGatherHindsight& p, hipStream_t s);

}  // namespace urgym
