// urgym_sac_bc_masked.hip — behaviour cloning on marked rows only (include/urgym.h, urgym_sac_policy_terms_cloned_masked; DESIGN.md
// section 34): urgym_sac_policy_terms_cloned's kernel with one change to a row's verdict, cloned = row_mask != 0 && (the Q-filter's
// verdict), sac_bc_cloned_masked of urgym_sac_bc.h.  Everything a row or an element computes is a function of urgym_sac_bc.h or
// urgym_sac_terms.h, the ones urgym_sac_bc.hip compiles; what this file repeats of that unit is the walk over the rows and the fold
// (DESIGN.md section 34 says why the walk is not a shared header: it moved the existing kernel's instructions).
//
// ONE launch of ONE workgroup of 1024 lanes, the two phases urgym_sac_bc.hip states, the same sums over ALL rows.  A lane reads its
// row's mask byte in both phases, as it re-forms the filter's verdict: nothing per row is kept between them.  Phase 1 never reads
// action_pi or action_data of a row that is not cloned, and phase 2 selects g for it, so a NaN there reaches no output.  A lane reads
// dqmin_da[i] before it writes d_action_out[i], and phase 1 reads neither, so d_action_out may be dqmin_da.
//
// A unit of its own, so that the text of urgym_sac_bc.hip's kernel does not depend on it; built with -ffp-contract=off like that unit.
#include <hip/hip_runtime.h>

#include "urgym_sac_bc.h"

namespace urgym {

namespace {

__global__ void __launch_bounds__(SAC_TERMS_LANES) sac_policy_bc_masked_kernel(const SacPolicyCall P, const SacCloneCall B, const uint8_t* row_mask) {
  __shared__ double partial[5][SAC_TERMS_LANES];  // q0's, q1's and the actor's terms, |q_min|, the cloning term
  __shared__ int32_t cloned_rows[SAC_TERMS_LANES];
  const int t = threadIdx.x;
  const float alpha = P.ent_coef[0];
  const bool q_filter = B.q_filter != 0;
  double s0 = 0.0, s1 = 0.0, sa = 0.0, sq = 0.0, sh = 0.0;
  int32_t rows = 0;
  for (int r = t; r < P.count; r += SAC_TERMS_LANES) {
    const float y = P.y[r], q0 = P.q[r], q1 = P.q[(size_t)P.count + r], q_min = P.q_min[r];
    s0 += (double)sac_critic_term(q0, y);
    s1 += (double)sac_critic_term(q1, y);
    sa += (double)sac_actor_term(alpha, P.log_prob[r], q_min);
    sq += (double)fabsf(q_min);
    const bool cloned = sac_bc_cloned_masked(row_mask[r], q_filter, sac_bc_q_data(q0, q1), q_min);
    float h = 0.0f;
    if (cloned) {
      float a_pi[6], a_data[6];
      for (int k = 0; k < 6; k++) a_pi[k] = B.action_pi[(size_t)r * 6 + k], a_data[k] = B.action_data[(size_t)r * 6 + k];
      h = sac_bc_term(a_pi, a_data);
      rows++;
    }
    sh += (double)h;
  }
  partial[0][t] = s0, partial[1][t] = s1, partial[2][t] = sa, partial[3][t] = sq, partial[4][t] = sh;
  cloned_rows[t] = rows;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) {
      for (int j = 0; j < 5; j++) partial[j][t] += partial[j][t + s];
      cloned_rows[t] += cloned_rows[t + s];
    }
    __syncthreads();
  }
  // the same scalar in every lane: mean_abs is a constant of the step, over ALL rows whatever the mask
  const float mean_abs = ordered_mean(partial[3][0], P.count);
  const float w = sac_bc_weight(B.scale_by_q != 0, B.weight, mean_abs);
  const int n = P.count * 6;  // at most 393,216
  for (int i = t; i < n; i += SAC_TERMS_LANES) {
    const int r = i / 6;
    const float g = P.dqmin_da[i] * P.scale;
    const bool cloned = sac_bc_cloned_masked(row_mask[r], q_filter, sac_bc_q_data(P.q[r], P.q[(size_t)P.count + r]), P.q_min[r]);
    P.d_action_out[i] = cloned ? sac_bc_upstream(g, sac_bc_difference(B.action_pi[i], B.action_data[i]), w, B.bc_scale) : g;
  }
  if (t != 0) return;
  P.critic_loss_out[0] = sac_critic_loss(ordered_mean(partial[0][0], P.count), ordered_mean(partial[1][0], P.count));
  P.actor_loss_out[0] = ordered_mean(partial[2][0], P.count);
  B.bc_loss_out[0] = ordered_mean(partial[4][0], P.count);
  B.bc_weight_out[0] = w;
  B.bc_rows_out[0] = cloned_rows[0];
}

}  // namespace

void sac_policy_bc_masked_launch(const SacPolicyCall& call, const SacCloneCall& clone, const uint8_t* row_mask, hipStream_t s) {
  hipLaunchKernelGGL(sac_policy_bc_masked_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call, clone, row_mask);
}

}  // namespace urgym
