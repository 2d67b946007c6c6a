// urgym_sac_terms.hip — SAC's entropy coefficient on the device (include/urgym.h, urgym_sac_entropy_step / urgym_sac_policy_terms):
// the temperature's Adam step, alpha = exp(log_ent_coef), the entropy term of the target, the upstream gradients of the actor's
// backward pass and the three loss values -- what a learner that keeps log_ent_coef in torch does with some forty small launches.
//
// Each kernel is ONE launch of ONE workgroup of 1024 lanes (16 waves).  A single workgroup is the point: every lane reads the scalar
// state (log_ent_coef and its moments, or ent_coef) once, before the first barrier and before lane 0 overwrites it after the last, so
// no ordering between workgroups is needed; there are no floating-point atomics; and the order of every sum depends on nothing but
// count.  Lane t handles rows t, t + 1024, ... (64 at the cap of 65,536 rows): it reads a row, writes the row's outputs (so y_out ==
// target_in is allowed) and adds the row's term to its float64 partial.  The partials are folded through LDS, 8 KB per sum, with a
// barrier per level.  Results are written with ordinary stores.
//
// This unit is built with -ffp-contract=off: every line of urgym_sac_terms.h is one float32 operation rounded on its own.  expf is
// the device library's (1 ulp), division is the correctly rounded one, subnormals are kept.
#include <hip/hip_runtime.h>

#include "urgym_sac_terms.h"

namespace urgym {

namespace {

// partial[t] += partial[t + s] for s = 512, ..., 1, a barrier per level (and one before the first); the result is partial[0]
__device__ __forceinline__ void fold(double* partial, int t) {
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) partial[t] += partial[t + s];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(SAC_TERMS_LANES) sac_entropy_kernel(const SacEntropyCall P) {
  __shared__ double partial[SAC_TERMS_LANES];
  const int t = threadIdx.x;
  // read by every lane before the first barrier; lane 0 writes them after the last
  float l = P.log_ent_coef[0], m = P.exp_avg[0], v = P.exp_avg_sq[0];
  const float alpha = expf(l);
  const float up = alpha * P.scale;
  double s = 0.0;
  for (int r = t; r < P.count; r += SAC_TERMS_LANES) {
    s += (double)sac_entropy_term(P.log_prob[r], P.target_entropy);
    if (P.y_out) {
      const bool terminal = P.terminated && P.terminated[r];
      P.y_out[r] = sac_target_row(P.target_in[r], P.next_log_prob[r], terminal, P.gamma, alpha);
    }
    if (P.d_log_prob_out) P.d_log_prob_out[r] = up;
  }
  partial[t] = s;
  fold(partial, t);
  if (t != 0) return;
  const float mean = ordered_mean(partial[0], P.count);
  float loss;
  sac_entropy_tail(P.c, mean, l, m, v, loss);
  P.ent_coef_out[0] = alpha;
  if (P.loss_out) P.loss_out[0] = loss;
  P.log_ent_coef[0] = l, P.exp_avg[0] = m, P.exp_avg_sq[0] = v;
}

// sac_entropy_kernel with the target group of urgym_sac_entropy_step_nstep: a row's y comes from its own discount and the bootstrap
// value (sac_target_row_nstep); a lane reads the row before it writes it, so y_out == reward is allowed.  Everything else is the
// kernel above, line for line.
__global__ void __launch_bounds__(SAC_TERMS_LANES) sac_entropy_nstep_kernel(const SacEntropyNstepCall P) {
  __shared__ double partial[SAC_TERMS_LANES];
  const int t = threadIdx.x;
  float l = P.log_ent_coef[0], m = P.exp_avg[0], v = P.exp_avg_sq[0];
  const float alpha = expf(l);
  const float up = alpha * P.scale;
  double s = 0.0;
  for (int r = t; r < P.count; r += SAC_TERMS_LANES) {
    s += (double)sac_entropy_term(P.log_prob[r], P.target_entropy);
    if (P.y_out) {
      const bool terminal = P.terminated && P.terminated[r];
      P.y_out[r] = sac_target_row_nstep(P.reward[r], P.q_min_next[r], P.discount[r], P.next_log_prob[r], terminal, alpha);
    }
    if (P.d_log_prob_out) P.d_log_prob_out[r] = up;
  }
  partial[t] = s;
  fold(partial, t);
  if (t != 0) return;
  const float mean = ordered_mean(partial[0], P.count);
  float loss;
  sac_entropy_tail(P.c, mean, l, m, v, loss);
  P.ent_coef_out[0] = alpha;
  if (P.loss_out) P.loss_out[0] = loss;
  P.log_ent_coef[0] = l, P.exp_avg[0] = m, P.exp_avg_sq[0] = v;
}

__global__ void __launch_bounds__(SAC_TERMS_LANES) sac_policy_kernel(const SacPolicyCall P) {
  __shared__ double partial[3][SAC_TERMS_LANES];  // q0's, q1's and the actor's terms
  const int t = threadIdx.x;
  const float alpha = P.ent_coef[0];
  if (P.d_action_out) {
    const int n = P.count * 6;  // at most 393,216
    for (int i = t; i < n; i += SAC_TERMS_LANES) P.d_action_out[i] = P.dqmin_da[i] * P.scale;
  }
  double s0 = 0.0, s1 = 0.0, sa = 0.0;
  for (int r = t; r < P.count; r += SAC_TERMS_LANES) {
    if (P.critic_loss_out) {
      const float y = P.y[r];
      s0 += (double)sac_critic_term(P.q[r], y);
      s1 += (double)sac_critic_term(P.q[(size_t)P.count + r], y);
    }
    if (P.actor_loss_out) sa += (double)sac_actor_term(alpha, P.log_prob[r], P.q_min[r]);
  }
  partial[0][t] = s0, partial[1][t] = s1, partial[2][t] = sa;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) {
      partial[0][t] += partial[0][t + s];
      partial[1][t] += partial[1][t + s];
      partial[2][t] += partial[2][t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  if (P.critic_loss_out) P.critic_loss_out[0] = sac_critic_loss(ordered_mean(partial[0][0], P.count), ordered_mean(partial[1][0], P.count));
  if (P.actor_loss_out) P.actor_loss_out[0] = ordered_mean(partial[2][0], P.count);
}

}  // namespace

void sac_entropy_launch(const SacEntropyCall& call, hipStream_t s) {
  hipLaunchKernelGGL(sac_entropy_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call);
}

void sac_entropy_nstep_launch(const SacEntropyNstepCall& call, hipStream_t s) {
  hipLaunchKernelGGL(sac_entropy_nstep_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call);
}

void sac_policy_launch(const SacPolicyCall& call, hipStream_t s) {
  hipLaunchKernelGGL(sac_policy_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call);
}

}  // namespace urgym
