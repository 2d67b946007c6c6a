// urgym_critic.h — seam between urgym_critic.hip (the twin Q-network kernel, compiled with fma contraction like urgym_actor.hip) and
// urgym_hip.hip (handle, C-ABI), beside urgym_actor.h.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urgym.h"

namespace urgym {

struct Critic;  // the packed weights of both Q-networks on the device (urgym_critic.hip)

// One evaluation: M rows of inputs (DEVICE pointers, row-major), the optional terms of the SAC target and the optional outputs.
struct CriticCall {
  int M, obs_dim, goal_dim;
  const float *observation, *achieved_goal, *desired_goal, *action;  // [M][obs_dim], [M][goal_dim], [M][goal_dim], [M][6]
  const float* reward;        // [M], null unless target
  const uint8_t* terminated;  // [M] or null (= nowhere terminated)
  const float* log_prob;      // [M] or null (= no entropy term)
  float gamma, ent_coef;
  float *q, *q_min, *target;  // [2][M], [M], [M]; each may be null
};

// checks desc (shape only; in_features is compared with `in_features`), uploads the packed weights; on failure writes a message
int critic_create(const urgym_critic_desc* desc, int in_features, Critic** out, char* err, size_t err_len);
void critic_destroy(Critic* c);
int critic_in_features(const Critic* c);

// The packed buffer of both networks (device, `floats` long) and the shape it was packed for: what a reload (urgym_weights.h) writes.
struct CriticPacked {
  float* weights;
  size_t floats;
  int in_features, hidden;
};
CriticPacked critic_packed(Critic* c);

// ONE launch on `s`; the caller has validated `call`
void critic_launch(Critic* c, const CriticCall& call, hipStream_t s);

}  // namespace urgym
