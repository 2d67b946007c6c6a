// urgym_grad_clip.hip — the global gradient norm and the clip coefficient on the device (include/urgym.h, urgym_actor_grad_norm /
// urgym_critic_grad_norm; urgym_grad_clip.h states every float): what torch.nn.utils.clip_grad_norm_ does with a launch per tensor, a
// stack, a second norm and, for the coefficient, a multiply per tensor.
//
// ONE launch of ONE workgroup of 1024 lanes (16 waves) walks the tensors of the group, the layout of urgym_sac_terms.hip.  The
// definition leaves no other parallelism within a tensor: lane t's partial is a chain of float64 additions over elements t, t + 1024,
// ... in ascending order, so a tensor has exactly 1024 chains.  Lane t reads consecutive addresses with its neighbours (plain 4-byte
// loads: the tensors are only 4-byte aligned), squares in float64 (exact) and adds.  The partials of FOUR tensors are folded at once
// through LDS, 32 KB, with a barrier per level -- the levels of ordered_fold, so three rounds of ten barriers cover the critics' twelve
// tensors and two rounds the actor's eight.  Every lane keeps the sums; lane 0 adds them in tensor order, takes the square root and the
// coefficient (grad_clip_tail) and writes the results with ordinary stores.  No atomics; the gradient tensors are only read.
//
// This unit is built with -ffp-contract=off: every line of urgym_grad_clip.h is one operation rounded on its own.  The float64 sqrt
// and division are the correctly rounded ones (hipcc's default).
// It is also built with -mllvm -unroll-runtime -mllvm -unroll-count=8 (the Makefile says why): ordered_partial's loop, compiled as it
// stands, waits for every load before it issues the next; unrolled by eight, remainder trips first, a lane has eight loads in flight
// and adds in the loop's order.
#include <hip/hip_runtime.h>

#include "urgym_grad_clip.h"

namespace urgym {

namespace {

constexpr int GRAD_NORM_BATCH = 4;  // tensors folded together: 4 x 1024 doubles of LDS

template <int K>
__global__ void __launch_bounds__(SAC_TERMS_LANES) grad_norm_kernel(const GradNormCall P) {
  static_assert(K % GRAD_NORM_BATCH == 0 && K <= GRAD_NORM_MAX_TENSORS, "the rounds below");
  __shared__ double partial[GRAD_NORM_BATCH][SAC_TERMS_LANES];
  const int t = threadIdx.x;
  double sums[K];
#pragma unroll
  for (int b = 0; b < K; b += GRAD_NORM_BATCH) {
#pragma unroll
    for (int j = 0; j < GRAD_NORM_BATCH; j++) {
      const float* const g = P.grad[b + j];
      partial[j][t] = ordered_partial(t, P.count[b + j], [g](int m) { return grad_square(g[m]); });
    }
    __syncthreads();
    for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
      if (t < s) {
#pragma unroll
        for (int j = 0; j < GRAD_NORM_BATCH; j++) partial[j][t] += partial[j][t + s];
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < GRAD_NORM_BATCH; j++) sums[b + j] = partial[j][0];
    __syncthreads();  // the next round overwrites the partials
  }
  if (t != 0) return;
  const GradClip r = grad_clip_tail(grad_total(sums, K), P.max_norm);
  P.norm_out[0] = r.norm;
  P.scale_out[0] = r.scale;
  if (P.tensor_sums_out) {
#pragma unroll
    for (int k = 0; k < K; k++) P.tensor_sums_out[k] = sums[k];
  }
}

}  // namespace

void grad_norm_launch(const GradNormCall& call, hipStream_t s) {
  if (call.tensors == GRAD_NORM_ACTOR_TENSORS)
    hipLaunchKernelGGL(grad_norm_kernel<GRAD_NORM_ACTOR_TENSORS>, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call);
  else
    hipLaunchKernelGGL(grad_norm_kernel<GRAD_NORM_CRITIC_TENSORS>, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call);
}

}  // namespace urgym
