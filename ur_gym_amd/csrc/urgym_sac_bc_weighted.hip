// urgym_sac_bc_weighted.hip — advantage-weighted cloning in SAC's policy loss (include/urgym.h, urgym_sac_policy_terms_weighted;
// DESIGN.md section 35): urgym_sac_policy_terms_cloned's outputs with a soft weight in the place of the verdict.  Every eligible row --
// marked, or no mask given, and with a finite advantage A = min(q) at the replayed action - q_min -- is cloned with the weight
// a = min(e / mean(e), max_weight), e = exp((A - A_max) / temperature) in float64 by the project's own exponential.  Everything a row
// or an element computes is a function of urgym_sac_bc.h, urgym_sac_terms.h or urgym_mppi_temper.h, the ones
// tests/sac_bc_weighted_harness.cpp compiles; what this file adds is the walk over the rows and the folds.
//
// ONE launch of ONE workgroup of 1024 lanes, because the weights need three reductions over all rows before an element can be written:
//   sweep 1   lane t walks rows t, t + 1024, ...: the largest advantage of its eligible rows and their number; folded to A_max and n.
//   sweep 2   the same rows again: the four sums of urgym_sac_policy_terms_cloned (q0's, q1's and the actor's terms, |q_min|) and Z,
//             the sum of e, folded together through the five LDS arrays; then Q, the sum of e * e, through the first of them.
//   sweep 3   the same rows a third time: a of the row, the term a * h of the weighted loss, the count of rows the cap held, and the
//             row's six elements; then the fold of the loss and the count.
// Nothing per row is kept between the sweeps: a row's advantage, eligibility and e are formed again from q, q_min and the mask, so the
// kernel's LDS is the 44 KB of the kernel it stands in for (five float64 arrays and one int32 array, each quantity folded through them in
// turn, as mppi_stats_kernel does).  Every sum is THE ORDERED SUM over ALL count rows -- a row that is not eligible adds +0.0 -- so the
// order is a function of count alone.  No atomics.
//
// The lane that writes a row's elements is the lane that read dqmin_da of that row, each element read before it is written, and no other
// lane touches the row: d_action_out may be dqmin_da.  Sweeps 1 and 2 read neither.  action_pi and action_data of a row that is not
// eligible are never read, so a NaN there reaches no output.  The mask pointer is uniform: one kernel serves both forms.
//
// A unit of its own, so that the text of urgym_sac_bc.hip's and urgym_sac_bc_masked.hip's kernels does not depend on it; built with
// -ffp-contract=off like those units.
#include <hip/hip_runtime.h>

#include "urgym_sac_bc.h"

namespace urgym {

namespace {

__global__ void __launch_bounds__(SAC_TERMS_LANES) sac_policy_bc_weighted_kernel(const SacPolicyCall P, const SacCloneCall B, const SacAdvantageCall A) {
  __shared__ double partial[5][SAC_TERMS_LANES];  // sweep 1: A_max; sweep 2: q0's, q1's and the actor's terms, |q_min|, e, then e * e; sweep 3: a * h
  __shared__ int32_t counts[SAC_TERMS_LANES];     // sweep 1: eligible rows; sweep 3: rows the cap held
  const int t = threadIdx.x;
  const int count = P.count;
  const float alpha = P.ent_coef[0];
  const bool masked = A.row_mask != nullptr;
  const float temperature = A.temperature, max_weight = A.max_weight;

  // ---- sweep 1: A_max and n
  float lane_max = -INFINITY;
  int32_t lane_n = 0;
  for (int r = t; r < count; r += SAC_TERMS_LANES) {
    const float adv = sac_adv_advantage(sac_bc_q_data(P.q[r], P.q[(size_t)count + r]), P.q_min[r]);
    const bool eligible = sac_adv_eligible(masked, masked ? A.row_mask[r] : (uint8_t)1, adv);
    lane_max = sac_adv_max(lane_max, sac_adv_max_term(eligible, adv));
    lane_n += eligible ? 1 : 0;
  }
  partial[0][t] = (double)lane_max;  // a float32 or -inf: exact in float64
  counts[t] = lane_n;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) {
      const double a = partial[0][t], b = partial[0][t + s];
      partial[0][t] = b > a ? b : a;
      counts[t] += counts[t + s];
    }
    __syncthreads();
  }
  const float a_max = (float)partial[0][0];
  const int32_t n = counts[0];
  __syncthreads();  // every lane has read both before sweep 2 writes the arrays again

  // ---- sweep 2: the four sums of the cloned call, Z and Q
  double s0 = 0.0, s1 = 0.0, sa = 0.0, sq = 0.0, sz = 0.0, sqq = 0.0;
  for (int r = t; r < count; r += SAC_TERMS_LANES) {
    const float y = P.y[r], q0 = P.q[r], q1 = P.q[(size_t)count + r], q_min = P.q_min[r];
    s0 += (double)sac_critic_term(q0, y);
    s1 += (double)sac_critic_term(q1, y);
    sa += (double)sac_actor_term(alpha, P.log_prob[r], q_min);
    sq += (double)fabsf(q_min);
    const float adv = sac_adv_advantage(sac_bc_q_data(q0, q1), q_min);
    const bool eligible = sac_adv_eligible(masked, masked ? A.row_mask[r] : (uint8_t)1, adv);
    const double e = sac_adv_e(adv, a_max, temperature, eligible);
    sz += e;
    sqq += mppi_square_term(e);
  }
  partial[0][t] = s0, partial[1][t] = s1, partial[2][t] = sa, partial[3][t] = sq, partial[4][t] = sz;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s)
      for (int j = 0; j < 5; j++) partial[j][t] += partial[j][t + s];
    __syncthreads();
  }
  const double S0 = partial[0][0], S1 = partial[1][0], SA = partial[2][0], SQ = partial[3][0], Z = partial[4][0];
  __syncthreads();
  partial[0][t] = sqq;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) partial[0][t] += partial[0][t + s];
    __syncthreads();
  }
  const double Q = partial[0][0];
  __syncthreads();

  // the same scalars in every lane: mean_abs over ALL rows whatever the mask; nothing is divided where no row is eligible
  const float mean_abs = ordered_mean(SQ, count);
  const float w = sac_bc_weight(B.scale_by_q != 0, B.weight, mean_abs);
  const double mean_e = n > 0 ? sac_adv_mean_e(Z, n) : 1.0;

  // ---- sweep 3: the weighted loss, the rows the cap held, and the elements
  double sh = 0.0;
  int32_t lane_clipped = 0;
  for (int r = t; r < count; r += SAC_TERMS_LANES) {
    const float adv = sac_adv_advantage(sac_bc_q_data(P.q[r], P.q[(size_t)count + r]), P.q_min[r]);
    const bool eligible = sac_adv_eligible(masked, masked ? A.row_mask[r] : (uint8_t)1, adv);
    const size_t base = (size_t)r * 6;
    float g[6];
    for (int k = 0; k < 6; k++) g[k] = P.dqmin_da[base + k] * P.scale;
    float term = 0.0f;
    if (eligible) {  // n >= 1 here
      bool over;
      const float a = sac_adv_row_weight(sac_adv_e(adv, a_max, temperature, true), mean_e, max_weight, over);
      lane_clipped += over ? 1 : 0;
      float a_pi[6], a_data[6];
      for (int k = 0; k < 6; k++) a_pi[k] = B.action_pi[base + k], a_data[k] = B.action_data[base + k];
      term = sac_adv_term(a, sac_bc_term(a_pi, a_data));
      const float wr = sac_adv_element_weight(w, a);
      for (int k = 0; k < 6; k++) g[k] = sac_bc_upstream(g[k], sac_bc_difference(a_pi[k], a_data[k]), wr, B.bc_scale);
    }
    for (int k = 0; k < 6; k++) P.d_action_out[base + k] = g[k];
    sh += (double)term;
  }
  partial[0][t] = sh;
  counts[t] = lane_clipped;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) {
      partial[0][t] += partial[0][t + s];
      counts[t] += counts[t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  P.critic_loss_out[0] = sac_critic_loss(ordered_mean(S0, count), ordered_mean(S1, count));
  P.actor_loss_out[0] = ordered_mean(SA, count);
  B.bc_loss_out[0] = ordered_mean(partial[0][0], count);
  B.bc_weight_out[0] = w;
  B.bc_rows_out[0] = n;
  bool over = false;
  A.adv_ess_out[0] = n > 0 ? sac_adv_ess(Z, Q) : 0.0f;
  A.adv_max_out[0] = n > 0 ? sac_adv_row_weight(1.0, mean_e, max_weight, over) : 0.0f;  // the A_max row has e = 1 exactly
  A.adv_clipped_out[0] = counts[0];
}

}  // namespace

void sac_policy_bc_weighted_launch(const SacPolicyCall& call, const SacCloneCall& clone, const SacAdvantageCall& adv, hipStream_t s) {
  hipLaunchKernelGGL(sac_policy_bc_weighted_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call, clone, adv);
}

}  // namespace urgym
