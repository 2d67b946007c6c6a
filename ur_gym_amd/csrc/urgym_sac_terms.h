// urgym_sac_terms.h — SAC's entropy coefficient on the device: the per-row arithmetic, the summation order and
// the scalar tail of urgym_sac_entropy_step / urgym_sac_policy_terms, stated once as functions the kernels of urgym_sac_terms.hip and
// tests/sac_terms_harness.cpp (a host program, built without HIP) both compile; and, for HIP units only, the seam between
// urgym_sac_terms.hip and urgym_policy_abi.hip.  Nothing here is exported.
#pragma once
#include <stdint.h>

#include "urgym_adam.h"

namespace urgym {

constexpr int SAC_TERMS_LANES = 1024;       // ONE workgroup of this many lanes runs either kernel
constexpr int SAC_TERMS_MAX_COUNT = 65536;  // 64 rows per lane at the most

// Every function below is float32 with ONE operation per line, rounded on its own: the units that compile this are built with
// -ffp-contract=off.  ur_gym_amd.evaluation.entropy_step / policy_terms restate them.

// y = target - ((gamma * nd) * alpha) * next_log_prob, the association of the learner's torch line
URGYM_HD inline float sac_target_row(float target, float next_log_prob, bool terminal, float gamma, float alpha) {
  const float nd = terminal ? 0.0f : 1.0f;
  const float d = gamma * nd;
  const float t = d * alpha;
  const float e = t * next_log_prob;
  return target - e;
}

// The same y from a per-row discount (urgym_sac_entropy_step_nstep: discount = gamma^m of a multi-step return) and the bootstrap
// value itself: y = (reward + (discount * nd) * q_min_next) - ((discount * nd) * alpha) * next_log_prob.  With discount == gamma this is
// urgym_critic_evaluate's target at ent_coef = 0 followed by sac_target_row, operation for operation.
URGYM_HD inline float sac_target_row_nstep(float reward, float q_min_next, float discount, float next_log_prob, bool terminal, float alpha) {
  const float nd = terminal ? 0.0f : 1.0f;
  const float d = discount * nd;
  const float a = d * q_min_next;
  const float tv = reward + a;
  const float t = d * alpha;
  const float e = t * next_log_prob;
  return tv - e;
}

// the term of the temperature loss: s = log_prob + target_entropy
URGYM_HD inline float sac_entropy_term(float log_prob, float target_entropy) { return log_prob + target_entropy; }

// the term of one Q-network's loss: (q - y)^2
URGYM_HD inline float sac_critic_term(float q, float y) {
  const float e = q - y;
  return e * e;
}

// the term of the actor's loss: alpha log_prob - q_min
URGYM_HD inline float sac_actor_term(float alpha, float log_prob, float q_min) {
  const float a = alpha * log_prob;
  return a - q_min;
}

// The ordered sum, first half: lane t starts at +0.0 and adds terms t, t + 1024, t + 2048, ... in ascending order, in float64.
template <class Term>
URGYM_HD inline double ordered_partial(int t, int count, Term term) {
  double s = 0.0;
  for (int m = t; m < count; m += SAC_TERMS_LANES) s += (double)term(m);
  return s;
}

// The ordered sum, second half, as a host loop: partial[t] += partial[t + s] for s = 512, 256, ..., 1; the result is partial[0].
// (The kernels run the same levels with a barrier after each.)
inline double ordered_fold(double (&partial)[SAC_TERMS_LANES]) {
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1)
    for (int t = 0; t < s; t++) partial[t] += partial[t + s];
  return partial[0];
}

template <class Term>
inline double ordered_sum(int count, Term term) {
  double partial[SAC_TERMS_LANES];
  for (int t = 0; t < SAC_TERMS_LANES; t++) partial[t] = ordered_partial(t, count, term);
  return ordered_fold(partial);
}

// a mean: the float64 sum over the float64 count, rounded to float32 once
URGYM_HD inline float ordered_mean(double sum, int count) { return (float)(sum / (double)count); }

// the scalar tail of the entropy step: g = d loss / d l, the loss, and Adam on the one element
URGYM_HD inline void sac_entropy_tail(const AdamCoef& c, float mean, float& l, float& m, float& v, float& loss) {
  const float g = -mean;
  const float lm = l * mean;
  loss = -lm;
  adam_element(c, g, l, m, v);
}

// the critic's loss from the two means
URGYM_HD inline float sac_critic_loss(float mean0, float mean1) {
  const float s = mean0 + mean1;
  return 0.5f * s;
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// include/urgym.h, urgym_sac_entropy_args, validated: DEVICE pointers; a group that is absent has its output pointer null
struct SacEntropyCall {
  int count;
  float target_entropy, gamma, scale;
  const float* log_prob;
  float *log_ent_coef, *exp_avg, *exp_avg_sq;
  float *ent_coef_out, *loss_out;  // loss_out may be null
  const float *target_in, *next_log_prob;
  const uint8_t* terminated;  // may be null with the group given
  float* y_out;               // null = no target group
  float* d_log_prob_out;      // null = no upstream group
  AdamCoef c;
};

// include/urgym.h, urgym_sac_entropy_nstep_args, validated: SacEntropyCall with the target group of a per-row discount
struct SacEntropyNstepCall {
  int count;
  float target_entropy, scale;
  const float* log_prob;
  float *log_ent_coef, *exp_avg, *exp_avg_sq;
  float *ent_coef_out, *loss_out;  // loss_out may be null
  const float *reward, *q_min_next, *discount, *next_log_prob;
  const uint8_t* terminated;  // may be null with the group given
  float* y_out;               // null = no target group
  float* d_log_prob_out;      // null = no upstream group
  AdamCoef c;
};

// include/urgym.h, urgym_sac_policy_args, validated
struct SacPolicyCall {
  int count;
  float scale;
  const float* ent_coef;
  const float* dqmin_da;
  float* d_action_out;  // null = no upstream group
  const float *q, *y;
  float* critic_loss_out;  // null = no critic-loss group
  const float *log_prob, *q_min;
  float* actor_loss_out;  // null = no actor-loss group
};

// ONE launch of ONE workgroup of SAC_TERMS_LANES lanes on `s` each.  The caller has validated everything.
void sac_entropy_launch(const SacEntropyCall& call, hipStream_t s);
void sac_entropy_nstep_launch(const SacEntropyNstepCall& call, hipStream_t s);
void sac_policy_launch(const SacPolicyCall& call, hipStream_t s);

}  // namespace urgym
#endif
