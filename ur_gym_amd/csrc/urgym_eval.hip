// urgym_eval.hip — evaluation inside the training call (include/urgym.h, urgym_eval_stats / urgym_actor_snapshot; DESIGN.md section
// 18): the statistics of N evaluation episodes, the improvement decision and the copy of the best actor, all on the device, so that a
// training call never returns to the host to decide whether a policy is the best so far.
//
// eval_stats_kernel is ONE launch of ONE workgroup of 1024 lanes, in the structure of sac_policy_kernel (urgym_sac_terms.hip): lane t
// handles episodes t, t + 1024, ... (64 at the cap of 65,536), the float64 partials are folded through LDS with a barrier per level,
// the scalar tail runs on lane 0.  Two folds follow one another -- the returns, then, after the mean has gone to every lane through
// LDS, the squared deviations from it -- and the two integer sums ride in the first.  No atomics: the order of every sum depends on
// nothing but count.  The best state is read and written by lane 0 alone.
//
// actor_snapshot_kernel copies an actor's eight tensors over a flat index, or nothing where the device flag it reads first is zero.
//
// This unit is built with -ffp-contract=off: every line of urgym_eval.h is one float64 operation rounded on its own.  Division is the
// correctly rounded one.
#include <hip/hip_runtime.h>

#include "urgym_eval.h"

namespace urgym {

namespace {

constexpr int SNAPSHOT_LANES = 256;

__global__ void __launch_bounds__(SAC_TERMS_LANES) eval_stats_kernel(const EvalStatsCall P) {
  __shared__ double partial[SAC_TERMS_LANES];
  __shared__ int64_t lengths[SAC_TERMS_LANES];
  __shared__ int32_t successes[SAC_TERMS_LANES];
  __shared__ double mean_all;
  const int t = threadIdx.x;
  const double* const r = P.episode_return;
  // first pass: the returns, the lengths and the successes
  int64_t len = 0;
  int32_t ok = 0;
  for (int n = t; n < P.count; n += SAC_TERMS_LANES) {
    len += eval_length_term(P.episode_last_step[n]);
    ok += eval_success_term(P.episode_success[n]);
  }
  partial[t] = ordered_partial(t, P.count, [r](int n) { return r[n]; });
  lengths[t] = len, successes[t] = ok;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) {
      partial[t] += partial[t + s];
      lengths[t] += lengths[t + s];
      successes[t] += successes[t + s];
    }
    __syncthreads();
  }
  if (t == 0) mean_all = eval_mean(partial[0], P.count);
  __syncthreads();  // every lane has mean_all; lane 0 has read partial[0] before any lane overwrites its partial
  const double mean = mean_all;
  // second pass: the squared deviations from the computed mean
  partial[t] = ordered_partial(t, P.count, [r, mean](int n) { return eval_deviation_term(r[n], mean); });
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) partial[t] += partial[t + s];
    __syncthreads();
  }
  if (t != 0) return;
  double best_mean = P.best_mean[0];
  int64_t best_index = P.best_index[0];
  urgym_eval_record rec;
  eval_tail(mean, partial[0], lengths[0], successes[0], P.count, P.eval_index, best_mean, best_index, rec);
  P.record[0] = rec;
  P.best_mean[0] = best_mean, P.best_index[0] = best_index;
}

__global__ void __launch_bounds__(SNAPSHOT_LANES) actor_snapshot_kernel(const ActorSnapshotCall P) {
  if (P.when && P.when[0] == 0) return;  // the decision of the evaluation before it: nothing is written
  const uint32_t i = blockIdx.x * (uint32_t)SNAPSHOT_LANES + threadIdx.x;
  if (i >= P.first[ACTOR_SNAPSHOT_TENSORS]) return;
  int k = 0;
  _Pragma("unroll") for (int j = 1; j < ACTOR_SNAPSHOT_TENSORS; j++) k += i >= P.first[j] ? 1 : 0;
  // the arrays of the kernel argument are indexed with constants only: a dynamic index would put them in scratch
  const float* src = P.src[0];
  float* dst = P.dst[0];
  uint32_t first = 0;
  _Pragma("unroll") for (int j = 1; j < ACTOR_SNAPSHOT_TENSORS; j++)
    if (k == j) src = P.src[j], dst = P.dst[j], first = P.first[j];
  dst[i - first] = src[i - first];
}

}  // namespace

void eval_stats_launch(const EvalStatsCall& call, hipStream_t s) {
  hipLaunchKernelGGL(eval_stats_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call);
}

void actor_snapshot_launch(const ActorSnapshotCall& call, hipStream_t s) {
  const uint32_t total = call.first[ACTOR_SNAPSHOT_TENSORS];
  hipLaunchKernelGGL(actor_snapshot_kernel, dim3((total + SNAPSHOT_LANES - 1) / SNAPSHOT_LANES), dim3(SNAPSHOT_LANES), 0, s, call);
}

}  // namespace urgym
