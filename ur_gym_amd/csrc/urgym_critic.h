// urgym_critic.h — seam between urgym_critic.hip (the twin Q-network kernel, compiled with fma contraction like urgym_actor.hip) and
// urgym_policy_abi.hip (the learner's entry points), beside urgym_actor.h.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urgym.h"

namespace urgym {

// The geometry both critic units (urgym_critic.hip, urgym_critic_grad.hip) are written for; each asserts its own constants against it.
constexpr int CRITIC_GEOMETRY_THREADS = 256, CRITIC_GEOMETRY_ROWS = 128, CRITIC_GEOMETRY_CIN_PAD = 56;

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
// where the small arrays (per network b0[HP] | b1[HP] | w_q[HP] | b_q, 0, 0, 0) begin in the packed buffer, in floats
inline size_t critic_small_offset(const CriticPacked& p) { return p.floats - 2 * ((size_t)((p.hidden + 127) / 128 * 128) * 3 + 4); }

// ONE launch on `s`; the caller has validated `call`
void critic_launch(Critic* c, const CriticCall& call, hipStream_t s);

// The action gradient of both networks on M rows (urgym_critic_grad.hip): the inputs of CriticCall, the outputs of
// urgym_critic_grad_out (DEVICE pointers, each may be null).
struct CriticGradCall {
  int M, obs_dim, goal_dim;
  const float *observation, *achieved_goal, *desired_goal, *action;  // [M][obs_dim], [M][goal_dim], [M][goal_dim], [M][6]
  float *dq_da, *dqmin_da, *q, *q_min;                               // [2][M][6], [M][6], [2][M], [M]
};

// the gradient kernel is built for hidden widths up to this (urgym_critic_grad.hip says why)
constexpr int CRITIC_GRAD_MAX_HIDDEN = 256;
bool critic_grad_supported(Critic* c);
// ONE launch on `s`; the caller has validated `call` and critic_grad_supported(c)
void critic_grad_launch(Critic* c, const CriticGradCall& call, hipStream_t s);

// The parameter gradients of both networks summed over M rows (urgym_critic_backward.hip): the inputs of CriticCall, the upstream
// gradient (exactly one of dq and target), the twelve outputs in the order of urgym_q_network_dev, the optional q and the caller's
// workspace (all DEVICE pointers).
struct CriticBackwardCall {
  int M, obs_dim, goal_dim;
  const float *observation, *achieved_goal, *desired_goal, *action;  // [M][obs_dim], [M][goal_dim], [M][goal_dim], [M][6]
  const float* dq;      // [2][M] or null
  const float* target;  // [M] or null: dq = (q - target) * scale
  float scale;
  float* grad[2][6];    // per network: W0, b0, W1, b1, w_q, b_q
  float* q;             // [2][M] or null
  float* workspace;     // critic_backward_workspace_bytes(c, M), 16-byte aligned
};

// built for the widths of the action gradient (CRITIC_GRAD_MAX_HIDDEN)
bool critic_backward_supported(Critic* c);
constexpr int CRITIC_BACKWARD_MAX_COUNT = 65536;
uint64_t critic_backward_workspace_bytes(Critic* c, int count);
// the launches of one call: 2 up to 1024 rows, 3 above (urgym_critic_backward.hip)
int critic_backward_launches(int count);
// on `s`; the caller has validated `call` and critic_backward_supported(c)
void critic_backward_launch(Critic* c, const CriticBackwardCall& call, hipStream_t s);

}  // namespace urgym
