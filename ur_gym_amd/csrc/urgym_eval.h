// urgym_eval.h — evaluation inside the training call: the arithmetic that reduces N evaluation episodes to one
// urgym_eval_record and takes the improvement decision, stated once as functions the kernel of urgym_eval.hip and
// tests/eval_harness.cpp (a host program, built without HIP) both compile; and, for HIP units only, the seam between urgym_eval.hip
// and urgym_policy_abi.hip.  The ordered sum is urgym_sac_terms.h's (ordered_partial / ordered_fold, SAC_TERMS_LANES), used as it is.
// Nothing here is exported.
#pragma once
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_sac_terms.h"

namespace urgym {

// Every function below is float64 with ONE operation per line, rounded on its own: the units that compile this are built with
// -ffp-contract=off.  ur_gym_amd.evaluation.evaluation_stats restates them.

// mean = sum_r / (double)N
URGYM_HD inline double eval_mean(double sum_r, int count) { return sum_r / (double)count; }

// the term of the second pass: d * d with d = r - mean (np.std's two passes, not E[r^2] - mean^2)
URGYM_HD inline double eval_deviation_term(double r, double mean) {
  const double d = r - mean;
  return d * d;
}

// an episode's length is its step count: the index of its last step + 1 (exact in int64)
URGYM_HD inline int64_t eval_length_term(int32_t last_step) { return (int64_t)last_step + 1; }

URGYM_HD inline int32_t eval_success_term(uint8_t success) { return success != 0 ? 1 : 0; }

// The scalar tail: the four quotients, the STRICT improvement decision (false for a NaN mean) and the best state.  Writes every field
// of the record.
URGYM_HD inline void eval_tail(double mean, double sum_d2, int64_t length_sum, int32_t successes, int count, int64_t eval_index, double& best_mean,
                               int64_t& best_index, urgym_eval_record& rec) {
  const double n = (double)count;
  const double var = sum_d2 / n;
  const double mean_length = (double)length_sum / n;
  const double success_rate = (double)successes / n;
  const bool improved = mean > best_mean;
  if (improved) {
    best_mean = mean;
    best_index = eval_index;
  }
  rec.mean_return = mean, rec.var_return = var, rec.mean_length = mean_length, rec.success_rate = success_rate;
  rec.best_mean_after = best_mean;
  rec.eval_index = eval_index, rec.length_sum = length_sum;
  rec.successes = successes, rec.count = count, rec.improved = improved ? 1 : 0, rec.reserved0 = 0;
}

// The whole reduction as a host loop, in the kernel's order.
inline void eval_stats_host(const double* r, const int32_t* last, const uint8_t* succ, int count, int64_t eval_index, double& best_mean, int64_t& best_index,
                            urgym_eval_record& rec) {
  const double sum_r = ordered_sum(count, [&](int n) { return r[n]; });
  const double mean = eval_mean(sum_r, count);
  const double sum_d2 = ordered_sum(count, [&](int n) { return eval_deviation_term(r[n], mean); });
  int64_t length_sum = 0;
  int32_t successes = 0;
  for (int n = 0; n < count; n++) length_sum += eval_length_term(last[n]), successes += eval_success_term(succ[n]);
  eval_tail(mean, sum_d2, length_sum, successes, count, eval_index, best_mean, best_index, rec);
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// include/urgym.h, urgym_eval_stats_args, validated: DEVICE pointers, count in [1, SAC_TERMS_MAX_COUNT]
struct EvalStatsCall {
  int count;
  int64_t eval_index;
  const double* episode_return;
  const int32_t* episode_last_step;
  const uint8_t* episode_success;
  double* best_mean;
  int64_t* best_index;
  urgym_eval_record* record;
};

constexpr int ACTOR_SNAPSHOT_TENSORS = 8;  // urgym_actor_tensors' eight, in its order

// include/urgym.h, urgym_actor_snapshot_args, validated: first[i] is the flat index of tensor i's first float, first[8] the total
struct ActorSnapshotCall {
  const float* src[ACTOR_SNAPSHOT_TENSORS];
  float* dst[ACTOR_SNAPSHOT_TENSORS];
  uint32_t first[ACTOR_SNAPSHOT_TENSORS + 1];
  const int32_t* when;  // null = copy always
};

// the sizes of an in -> H -> H -> 6 actor with its log_std head, as flat offsets (at most 512 * 47 + 512 * 512 + ... floats: fits uint32)
inline void actor_snapshot_offsets(int in_features, int hidden, uint32_t (&first)[ACTOR_SNAPSHOT_TENSORS + 1]) {
  const uint32_t n = (uint32_t)in_features, H = (uint32_t)hidden;
  const uint32_t size[ACTOR_SNAPSHOT_TENSORS] = {H * n, H, H * H, H, 6 * H, 6, 6 * H, 6};
  first[0] = 0;
  for (int i = 0; i < ACTOR_SNAPSHOT_TENSORS; i++) first[i + 1] = first[i] + size[i];
}

// ONE launch on `s` each.  The caller has validated everything.
void eval_stats_launch(const EvalStatsCall& call, hipStream_t s);     // one workgroup of SAC_TERMS_LANES lanes
void actor_snapshot_launch(const ActorSnapshotCall& call, hipStream_t s);

}  // namespace urgym
#endif
