// urgym_mppi_stats.h — plan statistics on the device (include/urgym.h, "the planner inside the training call"):
// the diagnostics the last plan left for E parents (best_return, nominal_return, ess and, with elites, elite_count and threshold)
// reduced to one urgym_mppi_stats_record, stated once as functions the kernel of urgym_mppi_stats.hip and tests/mppi_stats_harness.cpp
// (a host program, built without HIP) both compile; and, for HIP units only, the seam between urgym_mppi_stats.hip and
// urgym_mppi_abi.hip.  The ordered sum is urgym_sac_terms.h's (ordered_partial / ordered_fold / ordered_sum, SAC_TERMS_LANES), used as it
// is; "finite" is urgym_mppi.h's mppi_finite.  Nothing here is exported.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_mppi.h"
#include "urgym_sac_terms.h"

namespace urgym {

// Every function below is ONE operation per line, float64, rounded on its own: the units that compile this are built with
// -ffp-contract=off.  ur_gym_amd.evaluation.mppi_plan_stats restates them.

// a term of a sum over the parents that count: a parent that is passed over contributes +0.0, so the order depends on E alone
URGYM_HD inline double mppi_stats_term(bool counts, double x) { return counts ? x : 0.0; }

// the gain of a parent: counted where both returns are finite
URGYM_HD inline bool mppi_stats_gain_counts(double best, double nominal) { return mppi_finite(best) && mppi_finite(nominal); }
URGYM_HD inline double mppi_stats_gain(double best, double nominal) { return best - nominal; }

// fmin with the choice it leaves open fixed: a NaN operand gives the other one, equal operands (a zero of either sign) give a
URGYM_HD inline double mppi_stats_fmin(double a, double b) {
  if (a != a) return b;
  if (b != b) return a;
  return b < a ? b : a;
}

// lane t of the minimum: starts at NaN (no operand yet) and takes parents t, t + 1024, ... in ascending order
URGYM_HD inline double mppi_stats_min_partial(int t, int count, const double* x) {
  double m = NAN;
  for (int p = t; p < count; p += SAC_TERMS_LANES) m = mppi_stats_fmin(m, x[p]);
  return m;
}

// a mean over `count` terms: one division; +0.0 where nothing counted
URGYM_HD inline double mppi_stats_mean(double sum, int64_t count) {
  if (count == 0) return 0.0;
  return sum / (double)count;
}

// what the reduction hands to the scalar tail
struct MppiStatsSums {
  double best, nominal, gain, ess, min_ess, elite_count, threshold;
  int32_t planned, nominal_finite, gain_count, threshold_count;
};

// The scalar tail: the six quotients.  Writes every field of the record.
URGYM_HD inline void mppi_stats_tail(const MppiStatsSums& s, int num_parents, bool adaptive, int64_t iteration, urgym_mppi_stats_record& rec) {
  rec.mean_best_return = mppi_stats_mean(s.best, s.planned);
  rec.mean_nominal_return = mppi_stats_mean(s.nominal, s.nominal_finite);
  rec.mean_gain = mppi_stats_mean(s.gain, s.gain_count);
  rec.mean_ess = mppi_stats_mean(s.ess, num_parents);
  rec.min_ess = s.min_ess;
  rec.mean_elite_count = adaptive ? mppi_stats_mean(s.elite_count, num_parents) : 0.0;
  rec.mean_threshold = adaptive ? mppi_stats_mean(s.threshold, s.threshold_count) : 0.0;
  rec.iteration = iteration;
  rec.num_parents = num_parents;
  rec.planned = s.planned, rec.nominal_finite = s.nominal_finite, rec.gain_count = s.gain_count;
  rec.threshold_count = adaptive ? s.threshold_count : 0;
  rec.reserved0 = 0;
}

// The record as a host loop, in the kernel's order.  elite_count and threshold: both given or both null.
inline void mppi_stats_host(int num_parents, const double* best_return, const double* nominal_return, const double* ess, const int32_t* elite_count,
                            const double* threshold, int64_t iteration, urgym_mppi_stats_record& rec) {
  const int E = num_parents;
  const bool adaptive = elite_count != nullptr;
  MppiStatsSums s;
  s.best = ordered_sum(E, [=](int p) { return mppi_stats_term(mppi_finite(best_return[p]), best_return[p]); });
  s.nominal = ordered_sum(E, [=](int p) { return mppi_stats_term(mppi_finite(nominal_return[p]), nominal_return[p]); });
  s.gain = ordered_sum(E, [=](int p) {
    return mppi_stats_term(mppi_stats_gain_counts(best_return[p], nominal_return[p]), mppi_stats_gain(best_return[p], nominal_return[p]));
  });
  s.ess = ordered_sum(E, [=](int p) { return ess[p]; });
  s.elite_count = adaptive ? ordered_sum(E, [=](int p) { return (double)elite_count[p]; }) : 0.0;
  s.threshold = adaptive ? ordered_sum(E, [=](int p) { return mppi_stats_term(mppi_finite(threshold[p]), threshold[p]); }) : 0.0;
  s.planned = s.nominal_finite = s.gain_count = s.threshold_count = 0;
  for (int p = 0; p < E; p++) {
    s.planned += mppi_finite(best_return[p]) ? 1 : 0;
    s.nominal_finite += mppi_finite(nominal_return[p]) ? 1 : 0;
    s.gain_count += mppi_stats_gain_counts(best_return[p], nominal_return[p]) ? 1 : 0;
    if (adaptive) s.threshold_count += mppi_finite(threshold[p]) ? 1 : 0;
  }
  double low[SAC_TERMS_LANES];  // the minimum's levels, as the kernel folds them
  for (int t = 0; t < SAC_TERMS_LANES; t++) low[t] = mppi_stats_min_partial(t, E, ess);
  for (int w = SAC_TERMS_LANES / 2; w >= 1; w >>= 1)
    for (int t = 0; t < w; t++) low[t] = mppi_stats_fmin(low[t], low[t + w]);
  s.min_ess = low[0];
  mppi_stats_tail(s, E, adaptive, iteration, rec);
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// include/urgym.h, urgym_mppi_stats, validated: DEVICE pointers; elite_count and threshold both given (adaptive) or both null
struct MppiStatsCall {
  int num_parents;
  int64_t iteration;
  const double *best_return, *nominal_return, *ess;
  const int32_t* elite_count;
  const double* threshold;
  urgym_mppi_stats_record* record;
};

// ONE launch of ONE workgroup of SAC_TERMS_LANES lanes on `s`.  The caller has validated everything.
void mppi_stats_launch(const MppiStatsCall& call, hipStream_t s);

}  // namespace urgym
#endif
