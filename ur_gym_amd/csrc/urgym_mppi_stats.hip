// urgym_mppi_stats.hip — plan statistics on the device (include/urgym.h, urgym_mppi_stats): what the last plan
// left in best_return, nominal_return and ess (and, with elites, elite_count and threshold) of E parents, reduced to one
// urgym_mppi_stats_record, so that a training call whose collecting policy is the planner reports how its plans went without a copy of
// the [E] diagnostics to the host.
//
// mppi_stats_kernel is ONE launch of ONE workgroup of 1024 lanes, in the structure of eval_stats_kernel (urgym_eval.hip) and
// monitor_stats_kernel (urgym_monitor.hip): lane t handles parents t, t + 1024, ..., each float64 partial and each count is folded
// through LDS with a barrier per level, the scalar tail runs on lane 0.  The quantities are folded one after the other through the same
// two LDS arrays.  No atomics, one writer per output: the order of every sum depends on nothing but E.  It reads the diagnostics and
// writes the record, nothing else.
//
// This unit is built with -ffp-contract=off: every line of urgym_mppi_stats.h is one operation rounded on its own.  Division is the
// correctly rounded one.
#include <hip/hip_runtime.h>

#include "urgym_mppi_stats.h"

namespace urgym {

namespace {

// the levels of ordered_fold (urgym_sac_terms.h) on every lane's `v`, with `op` in place of +=; every lane returns level[0].  The
// first barrier lets the lanes that still read level[0] of the fold before finish.
template <class T, class Op>
__device__ T fold(T* level, int t, T v, Op op) {
  __syncthreads();
  level[t] = v;
  __syncthreads();
  for (int s = SAC_TERMS_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) level[t] = op(level[t], level[t + s]);
    __syncthreads();
  }
  return level[0];
}

__global__ void __launch_bounds__(SAC_TERMS_LANES) mppi_stats_kernel(const MppiStatsCall P) {
  __shared__ double level[SAC_TERMS_LANES];
  __shared__ int32_t tally[SAC_TERMS_LANES];
  const int t = threadIdx.x, E = P.num_parents;
  const double *best = P.best_return, *nominal = P.nominal_return, *ess = P.ess, *threshold = P.threshold;
  const int32_t* elite_count = P.elite_count;
  const bool adaptive = elite_count != nullptr;
  const auto add = [](double a, double b) { return a + b; };
  const auto count = [](int32_t a, int32_t b) { return a + b; };
  const auto low = [](double a, double b) { return mppi_stats_fmin(a, b); };
  int32_t planned = 0, nominal_finite = 0, gain_count = 0, threshold_count = 0;
  for (int p = t; p < E; p += SAC_TERMS_LANES) {
    planned += mppi_finite(best[p]) ? 1 : 0;
    nominal_finite += mppi_finite(nominal[p]) ? 1 : 0;
    gain_count += mppi_stats_gain_counts(best[p], nominal[p]) ? 1 : 0;
    if (adaptive) threshold_count += mppi_finite(threshold[p]) ? 1 : 0;
  }
  MppiStatsSums s;
  s.best = fold(level, t, ordered_partial(t, E, [best](int p) { return mppi_stats_term(mppi_finite(best[p]), best[p]); }), add);
  s.nominal = fold(level, t, ordered_partial(t, E, [nominal](int p) { return mppi_stats_term(mppi_finite(nominal[p]), nominal[p]); }), add);
  s.gain = fold(level, t, ordered_partial(t, E, [best, nominal](int p) {
                  return mppi_stats_term(mppi_stats_gain_counts(best[p], nominal[p]), mppi_stats_gain(best[p], nominal[p]));
                }), add);
  s.ess = fold(level, t, ordered_partial(t, E, [ess](int p) { return ess[p]; }), add);
  s.min_ess = fold(level, t, mppi_stats_min_partial(t, E, ess), low);
  s.elite_count = 0.0, s.threshold = 0.0;
  if (adaptive) {  // uniform over the workgroup: every lane takes the same side
    s.elite_count = fold(level, t, ordered_partial(t, E, [elite_count](int p) { return (double)elite_count[p]; }), add);
    s.threshold = fold(level, t, ordered_partial(t, E, [threshold](int p) { return mppi_stats_term(mppi_finite(threshold[p]), threshold[p]); }), add);
  }
  s.planned = fold(tally, t, planned, count);
  s.nominal_finite = fold(tally, t, nominal_finite, count);
  s.gain_count = fold(tally, t, gain_count, count);
  s.threshold_count = fold(tally, t, threshold_count, count);
  if (t != 0) return;
  urgym_mppi_stats_record rec;
  mppi_stats_tail(s, E, adaptive, P.iteration, rec);
  P.record[0] = rec;
}

}  // namespace

void mppi_stats_launch(const MppiStatsCall& call, hipStream_t s) {
  hipLaunchKernelGGL(mppi_stats_kernel, dim3(1), dim3(SAC_TERMS_LANES), 0, s, call);
}

}  // namespace urgym
