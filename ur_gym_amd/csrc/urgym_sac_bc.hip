// urgym_sac_bc.hip — behaviour cloning in SAC's policy loss on the device (include/urgym.h, urgym_sac_policy_terms_cloned): what
// urgym_sac_policy_terms forms -- d_action = dqmin_da * scale and the critic's and the actor's loss values -- plus a pull of the policy's
// action towards the action the replay ring holds, row by row, gated by the Q-filter and weighted by the mean |Q|.
//
// The kernel is ONE launch of ONE workgroup of 1024 lanes (16 waves), as the kernels of urgym_sac_terms.hip are and for their reasons:
// the weight w depends on a mean over ALL rows, so the rows' gradient can only be written after a reduction, and a single workgroup gets
// from one to the other with a barrier, no ordering between workgroups and no floating-point atomics.  Phase 1: lane t reads rows t,
// t + 1024, ... and adds each row's five terms (q0's, q1's, the actor's, |q_min| and the cloning term) to its float64 partials and the
// row's verdict to an int32 count; the partials are folded through LDS side by side, 40 KB + 4 KB, a barrier per level.  Every lane then
// reads the folded sum of |q_min| and forms the same w.  Phase 2 walks the [count][6] elements as urgym_sac_policy_terms does (lane t
// takes elements t, t + 1024, ...: neighbouring lanes read neighbouring floats), re-forms the verdict of the element's row from q and
// q_min and re-reads the two actions: nothing per row is kept between the phases.  A lane reads dqmin_da[i] before it writes
// d_action_out[i], and phase 1 reads neither, so d_action_out may be dqmin_da.
//
// This unit is built with -ffp-contract=off: every line of urgym_sac_bc.h and urgym_sac_terms.h is one float32 operation rounded on its
// own; subnormals are kept.
#include <hip/hip_runtime.h>

#include "urgym_sac_bc.h"

namespace urgym {

namespace {

__global__ void __launch_bounds__(SAC_TERMS_LANES) sac_policy_bc_kernel(const SacPolicyCall P, const SacCloneCall B) {
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
    const bool cloned = sac_bc_cloned(q_filter, sac_bc_q_data(q0, q1), q_min);
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
  // the same scalar in every lane: mean_abs is a constant of the step
  const float mean_abs = ordered_mean(partial[3][0], P.count);
  const float w = sac_bc_weight(B.scale_by_q != 0, B.weight, mean_abs);
  const int n = P.count * 6;  // at most 393,216
  for (int i = t; i < n; i += SAC_TERMS_LANES) {
    const int r = i / 6;
    const float g = P.dqmin_da[i] * P.scale;
    const bool cloned = sac_bc_cloned(q_filter, sac_bc_q_data(P.q[r], P.q[(size_t)P.count + r]), P.q_min[r]);
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

void sac_policy_bc_launch(const SacPolicyCall& call, const SacCloneCall& clone, hipStream_t s) {
  hipLaunchKernelGGL(sac_policy_bc_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call, clone);
}

}  // namespace urgym
