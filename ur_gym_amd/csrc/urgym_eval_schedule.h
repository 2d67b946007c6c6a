// urgym_eval_schedule.h — where the evaluations of one urgym_sac_train_evaluated call fall (include/urgym.h) and
// nothing else: index arithmetic on the caller's urgym_sac_schedule and the evaluation interval.  Plain C++ without a HIP include, next
// to urgym_sac_schedule.h, which it uses and does not change: urgym_policy_abi.hip compiles it, and so does tests/eval_harness.cpp, a
// host program built with g++.  ur_gym_amd.evaluation.evaluation_points restates it in Python integers.  Nothing here is exported.
#pragma once
#include <stdint.h>

#include "urgym_sac_schedule.h"

namespace urgym {

// s_i: the Adam steps taken when iteration i ends (i = -1: before the call).  The schedule's own refusals keep it inside int64.
inline int64_t eval_steps_after(const urgym_sac_schedule& s, int64_t i) {
  const int64_t active = i + 1 > s.idle_iterations ? i + 1 - s.idle_iterations : 0;
  return s.first_step - 1 + active * s.updates_per_iteration;
}

// an evaluation follows iteration i where the step count passes a multiple of `every` in it (every >= 1; the counts are not negative)
inline bool eval_follows(const urgym_sac_schedule& s, int32_t every, int32_t i) {
  return eval_steps_after(s, i) / every > eval_steps_after(s, (int64_t)i - 1) / every;
}

// the evaluations of the whole call: an iteration is followed by one at the most, however many multiples its updates pass
inline int64_t eval_count(const urgym_sac_schedule& s, int32_t every) {
  if (s.updates_per_iteration >= every) return s.num_iterations > s.idle_iterations ? (int64_t)s.num_iterations - s.idle_iterations : 0;
  // fewer updates per iteration than the interval: an iteration passes one multiple at the most
  return eval_steps_after(s, (int64_t)s.num_iterations - 1) / every - eval_steps_after(s, -1) / every;
}

// what the validation refuses about the placement (include/urgym.h lists them); nullptr = accepted.  The schedule has been accepted.
inline const char* eval_schedule_refusal(const urgym_sac_schedule& s, int32_t every, int64_t first_eval_index, int32_t first_record_slot,
                                         int32_t record_capacity) {
  if (every < 1) return "evaluation->every must be at least 1 (updates between evaluations)";
  if (first_eval_index < 0) return "evaluation->first_eval_index is negative";
  if (first_record_slot < 0) return "evaluation->first_record_slot is negative";
  const int64_t count = eval_count(s, every);
  if (count > (int64_t)record_capacity - first_record_slot) return "first_record_slot + the evaluations of the call is beyond record_capacity";
  if (first_eval_index > INT64_MAX - count) return "first_eval_index + the evaluations of the call does not fit int64";
  return nullptr;
}

}  // namespace urgym
