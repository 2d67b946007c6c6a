// urgym_grad_clip.h — gradient-norm clipping on the device: the global norm of a group of gradient tensors, the
// clip coefficient and the scaled Adam element, stated once as functions the kernel of urgym_grad_clip.hip, the scaled kernels of
// urgym_adam.hip and tests/grad_clip_harness.cpp (a host program, built without HIP) all compile; and, for HIP units only, the seam
// between urgym_grad_clip.hip and urgym_policy_abi.hip.  Nothing here is exported.
//
// A group is a list of float32 tensors in a FIXED order: the actor's eight in the order of urgym_actor_tensors, or the twelve of both
// Q-networks, network 0 then network 1, each in the order w0, b0, w1, b1, w_q, b_q (both networks are one group, as they are one
// optimiser).  For tensor k with n_k flat elements g:
//   s_k    = THE ORDERED SUM (urgym_sac_terms.h: ordered_partial / ordered_fold) of (double)g * (double)g over the n_k elements.  The
//            square of a float32 is exact in float64, so nothing is rounded before the sum.
//   total  = ((s_0 + s_1) + s_2) + ...     float64, tensor order
//   norm64 = sqrt(total)                   float64, correctly rounded
//   c64    = (double)max_norm / (norm64 + 1e-6)          torch.nn.utils.clip_grad_norm_'s formula
//   scale  = c64 < 1.0 ? (float)c64 : 1.0f
//   norm   = (float)norm64                 for the record only: nothing reads it
// The order depends on the tensors' shapes alone; there are no atomics.
//
// UNLIKE torch, the gradient tensors are NOT written: the scaled Adam step multiplies each element as it reads it, gs = g * scale, one
// float32 multiply rounded on its own, and adam_element runs on gs unchanged.  At scale == 1.0f, gs == g bit for bit (NaN payloads
// aside, which adam_element does not keep either), so the scaled step is then the unscaled one.
//
// Non-finite elements.  A NaN anywhere makes total, norm64 and c64 NaN; `c64 < 1.0` is then false and scale is 1.0f: the step is what
// it is without clipping.  A +inf or -inf (and no NaN) makes total = norm64 = +inf, c64 = +0.0 and scale = +0.0f: every finite element
// steps with gs = +-0.0f, the infinite ones with gs = NaN.  Finite float32 elements cannot overflow float64.
#pragma once
#include <math.h>
#include <stdint.h>

#include "urgym_adam.h"
#include "urgym_sac_terms.h"

namespace urgym {

constexpr int GRAD_NORM_ACTOR_TENSORS = PACK_ACTOR_TENSORS;        // 8
constexpr int GRAD_NORM_CRITIC_TENSORS = 2 * PACK_CRITIC_TENSORS;  // 12
constexpr int GRAD_NORM_MAX_TENSORS = GRAD_NORM_CRITIC_TENSORS;
constexpr double GRAD_NORM_EPS = 1e-6;

// Every function below is ONE operation per line, rounded on its own: the units that compile this are built with -ffp-contract=off;
// sqrt and / are the correctly rounded ones.  ur_gym_amd.evaluation.grad_norm restates them.

// the term of the sum: exact
URGYM_HD inline double grad_square(float g) {
  const double d = (double)g;
  return d * d;
}

// one tensor's sum on the host (the kernel runs ordered_partial per lane and the same fold levels with a barrier after each)
inline double grad_tensor_sum(const float* g, int count) {
  return ordered_sum(count, [g](int m) { return grad_square(g[m]); });
}

// total = ((s_0 + s_1) + s_2) + ...
URGYM_HD inline double grad_total(const double* sums, int tensors) {
  double total = sums[0];
  for (int k = 1; k < tensors; k++) total = total + sums[k];
  return total;
}

struct GradClip {
  double norm64;
  float norm, scale;
};

URGYM_HD inline GradClip grad_clip_tail(double total, float max_norm) {
  GradClip r;
  r.norm64 = sqrt(total);
  const double d = r.norm64 + GRAD_NORM_EPS;
  const double c64 = (double)max_norm / d;
  r.scale = c64 < 1.0 ? (float)c64 : 1.0f;  // a NaN c64 compares false
  r.norm = (float)r.norm64;
  return r;
}

// the whole thing on the host: sums_out[tensors] may be null
inline GradClip grad_norm(const float* const* grad, const int* count, int tensors, float max_norm, double* sums_out) {
  double sums[GRAD_NORM_MAX_TENSORS];
  for (int k = 0; k < tensors; k++) sums[k] = grad_tensor_sum(grad[k], count[k]);
  if (sums_out)
    for (int k = 0; k < tensors; k++) sums_out[k] = sums[k];
  return grad_clip_tail(grad_total(sums, tensors), max_norm);
}

// One element of the scaled step: the gradient is multiplied as it is read, then adam_element as it stands.
URGYM_HD inline void adam_element_scaled(const AdamCoef& c, float g, float scale, float& p, float& m, float& v) {
  const float gs = g * scale;
  adam_element(c, gs, p, m, v);
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// include/urgym.h, urgym_actor_grad_norm / urgym_critic_grad_norm, validated: DEVICE pointers; tensors is 8 or 12
struct GradNormCall {
  int tensors;
  float max_norm;
  const float* grad[GRAD_NORM_MAX_TENSORS];
  int count[GRAD_NORM_MAX_TENSORS];  // flat elements of each
  float* norm_out;
  float* scale_out;
  double* tensor_sums_out;  // [tensors], or null
};

// ONE launch of ONE workgroup of SAC_TERMS_LANES lanes on `s`.  The caller has validated everything.
void grad_norm_launch(const GradNormCall& call, hipStream_t s);

}  // namespace urgym
#endif
