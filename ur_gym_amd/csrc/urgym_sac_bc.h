// urgym_sac_bc.h — behaviour cloning in SAC's policy loss on the device, with a Q-filter: the per-row arithmetic
// and the scalar weight of urgym_sac_policy_terms_cloned, stated once as functions the kernel of urgym_sac_bc.hip and
// tests/sac_bc_harness.cpp (a host program, built without HIP) both compile; and, for HIP units only, the seam between urgym_sac_bc.hip
// and urgym_policy_abi.hip.  The sums, the means and the three loss terms are urgym_sac_terms.h's, used as they are.  Nothing here is
// exported.
#pragma once
#include <stdint.h>

#include "urgym_mppi_temper.h"  // mppi_temper_weight / mppi_temper_exp, mppi_square_term, mppi_ess: the advantage weight's float64 (section 35)
#include "urgym_sac_terms.h"

namespace urgym {

// Every function below is float32 with ONE operation per line, rounded on its own: the units that compile this are built with
// -ffp-contract=off.  ur_gym_amd.evaluation.policy_terms_cloned restates them.

// the smaller of the two online critics at the replayed action; a NaN q1 gives q0
URGYM_HD inline float sac_bc_q_data(float q0, float q1) { return q1 < q0 ? q1 : q0; }

// THE Q-FILTER (Nair et al. 2018): a row is cloned only where the critic rates the replayed action above the policy's own.  A NaN on
// either side, or a tie, gives not cloned.  Without the filter every row is cloned.
URGYM_HD inline bool sac_bc_cloned(bool q_filter, float q_data, float q_min) { return q_filter ? (q_data > q_min) : true; }

// THE MASKED VERDICT (urgym_sac_policy_terms_cloned_masked): only a row the caller marks -- one a demonstrator
// filed -- can be cloned; a marked row is cloned as above.  ur_gym_amd.evaluation.policy_terms_cloned(row_mask=) restates it.
URGYM_HD inline bool sac_bc_cloned_masked(uint8_t mask, bool q_filter, float q_data, float q_min) {
  return mask != 0 && sac_bc_cloned(q_filter, q_data, q_min);
}

// one difference of the two actions
URGYM_HD inline float sac_bc_difference(float action_pi, float action_data) { return action_pi - action_data; }

// the term of the cloning loss of one row: half the squared distance of the six components, added in ascending order from +0.0f
URGYM_HD inline float sac_bc_term(const float* action_pi, const float* action_data) {
  float s = 0.0f;
  for (int k = 0; k < 6; k++) {
    const float d = sac_bc_difference(action_pi[k], action_data[k]);
    const float p = d * d;
    s = s + p;
  }
  return 0.5f * s;
}

// the weight of the cloning term: TD3+BC's normalisation by the mean |Q|, written as a weight on the cloning term (no division)
URGYM_HD inline float sac_bc_weight(bool scale_by_q, float weight, float mean_abs) { return scale_by_q ? weight * mean_abs : weight; }

// one element of the upstream gradient of a cloned row: g is dqmin_da * scale, the line of urgym_sac_policy_terms
URGYM_HD inline float sac_bc_upstream(float g, float d, float w, float bc_scale) {
  const float t = d * w;
  const float u = t * bc_scale;
  return g + u;
}

// ---- ADVANTAGE-WEIGHTED CLONING (urgym_sac_policy_terms_weighted): every eligible row is cloned, with a weight
// exp(A / temperature) normalised to mean 1 over the eligible rows (AWAC, Nair et al. 2020; the exponential variant of CRR, Wang et al.
// 2020), capped at max_weight.  The exponential, the square and the effective sample size are urgym_mppi_temper.h's and urgym_mppi.h's,
// used as they are.  ur_gym_amd.evaluation.policy_terms_weighted restates the lines below.

// the advantage of the replayed action over the policy's own: one float32 subtraction
URGYM_HD inline float sac_adv_advantage(float q_data, float q_min) { return q_data - q_min; }
// false for a NaN and for either infinity
URGYM_HD inline bool sac_adv_finite(float a) { return a - a == 0.0f; }
// THE ELIGIBLE ROW: marked (or no mask at all) and a finite advantage
URGYM_HD inline bool sac_adv_eligible(bool masked, uint8_t mask, float advantage) { return (!masked || mask != 0) && sac_adv_finite(advantage); }
// one term of A_max: a row that is not eligible is passed over.  Comparisons of finite float32: the order does not matter
URGYM_HD inline float sac_adv_max_term(bool eligible, float advantage) { return eligible ? advantage : -INFINITY; }
URGYM_HD inline float sac_adv_max(float a, float b) { return b > a ? b : a; }
// e = exp((A - A_max) / temperature) in float64, +0.0 for a row that is not eligible: the argument is never positive
URGYM_HD inline double sac_adv_e(float advantage, float a_max, float temperature, bool eligible) {
  return mppi_temper_weight((double)advantage, (double)a_max, (double)temperature, eligible);
}
// the mean of e over the n eligible rows (n >= 1: the A_max row has e = 1, so the mean is positive)
URGYM_HD inline double sac_adv_mean_e(double Z, int n) { return Z / (double)n; }
// the weight of a row: u = e / mean_e, capped; `over` says whether the cap held it
URGYM_HD inline float sac_adv_row_weight(double e, double mean_e, float max_weight, bool& over) {
  const double u = e / mean_e;
  over = u > (double)max_weight;
  const double v = over ? (double)max_weight : u;
  return (float)v;
}
// the term of the weighted cloning loss of one row: one float32 product
URGYM_HD inline float sac_adv_term(float a, float h) { return a * h; }
// the weight of one element of an eligible row: the scalar w times the row's a
URGYM_HD inline float sac_adv_element_weight(float w, float a) { return w * a; }
// the effective sample size of the weights, rounded to float32 once
URGYM_HD inline float sac_adv_ess(double Z, double Q) { return (float)mppi_ess(Z, Q); }

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// include/urgym.h, urgym_sac_clone_args, validated: DEVICE pointers, none null
struct SacCloneCall {
  const float *action_pi, *action_data;
  float weight, bc_scale;
  int scale_by_q, q_filter;
  float *bc_loss_out, *bc_weight_out;
  int32_t* bc_rows_out;
};

// ONE launch of ONE workgroup of SAC_TERMS_LANES lanes on `s`.  The caller has validated everything: all three groups of `call` given.
void sac_policy_bc_launch(const SacPolicyCall& call, const SacCloneCall& clone, hipStream_t s);

// The same launch with the masked verdict (urgym_sac_bc_masked.hip, a unit of its own): row_mask is a DEVICE pointer, [count], not null
void sac_policy_bc_masked_launch(const SacPolicyCall& call, const SacCloneCall& clone, const uint8_t* row_mask, hipStream_t s);

// include/urgym.h, urgym_sac_advantage_args, validated: DEVICE pointers; row_mask may be null, the outputs are not
struct SacAdvantageCall {
  float temperature, max_weight;
  const uint8_t* row_mask;
  float *adv_ess_out, *adv_max_out;
  int32_t* adv_clipped_out;
};

// The launch with the advantage weight in the place of the verdict (urgym_sac_bc_weighted.hip, a unit of its own): ONE workgroup of
// SAC_TERMS_LANES lanes, three sweeps.  clone.q_filter is 0 (the caller has refused anything else).
void sac_policy_bc_weighted_launch(const SacPolicyCall& call, const SacCloneCall& clone, const SacAdvantageCall& adv, hipStream_t s);

}  // namespace urgym
#endif
