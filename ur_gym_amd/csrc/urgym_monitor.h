// urgym_monitor.h — training-episode statistics on the device: the arithmetic that follows the episodes of N envs
// through the slots of a collection and reduces the finished ones to one urgym_monitor_record, stated once as functions the kernels of
// urgym_monitor.hip and tests/monitor_harness.cpp (a host program, built without HIP) both compile; where the records of one
// urgym_sac_train_monitored call fall, as plain C++ on the caller's schedule; and, for HIP units only, the seam between urgym_monitor.hip
// and urgym_policy_abi.hip.  The ordered sum is urgym_sac_terms.h's (ordered_partial / ordered_fold, SAC_TERMS_LANES), used as it is.
// Nothing here is exported.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_sac_schedule.h"
#include "urgym_sac_terms.h"

namespace urgym {

// Every function below is ONE operation per line, float64 where a float is involved, rounded on its own: the units that compile this
// are built with -ffp-contract=off.  ur_gym_amd.evaluation.monitor_fold / monitor_stats restate them.

// what one env carries: the episode in progress, and the episodes it finished since the last clear
struct MonitorLane {
  double running_return;
  int32_t running_length;
  double sum_return;
  int64_t sum_length;
  int32_t episodes;
  int32_t successes;
};

// one step of one env, as the ring holds it
URGYM_HD inline void monitor_step(MonitorLane& m, float reward, uint8_t terminated, uint8_t truncated, uint8_t is_success) {
  m.running_return += (double)reward;
  m.running_length += 1;
  if ((terminated | truncated) == 0) return;
  m.sum_return += m.running_return;
  m.sum_length += (int64_t)m.running_length;
  m.episodes += 1;
  m.successes += is_success != 0 ? 1 : 0;
  m.running_return = 0.0;
  m.running_length = 0;
}

// the ring entry of step k and env n of a fold that starts at first_slot: slot (first_slot + k) % C, n contiguous within a slot
URGYM_HD inline size_t monitor_entry(int first_slot, int k, int capacity, int num_envs, int n) {
  return (size_t)(((int64_t)first_slot + k) % capacity) * (size_t)num_envs + (size_t)n;
}

// The scalar tail: the three quotients, each one float64 division, +0.0 where no episode finished.  Writes every field of the record.
URGYM_HD inline void monitor_tail(double sum_r, int64_t episodes, int64_t length_sum, int64_t successes, int64_t iteration, urgym_monitor_record& rec) {
  double mean_return = 0.0, mean_length = 0.0, success_rate = 0.0;
  if (episodes != 0) {
    const double e = (double)episodes;
    mean_return = sum_r / e;
    mean_length = (double)length_sum / e;
    success_rate = (double)successes / e;
  }
  rec.mean_return = mean_return, rec.mean_length = mean_length, rec.success_rate = success_rate, rec.sum_return = sum_r;
  rec.episodes = episodes, rec.length_sum = length_sum, rec.successes = successes, rec.iteration = iteration, rec.reserved0 = 0;
}

// The fold as a host loop: the state and the four ring arrays are host arrays here.
inline void monitor_fold_host(const urgym_monitor_state& st, const float* reward, const uint8_t* terminated, const uint8_t* truncated, const uint8_t* is_success,
                              int num_envs, int capacity, int first_slot, int num_steps) {
  for (int n = 0; n < num_envs; n++) {
    MonitorLane m{st.running_return[n], st.running_length[n], st.sum_return[n], st.sum_length[n], st.episodes[n], st.successes[n]};
    for (int k = 0; k < num_steps; k++) {
      const size_t at = monitor_entry(first_slot, k, capacity, num_envs, n);
      monitor_step(m, reward[at], terminated[at], truncated[at], is_success[at]);
    }
    st.running_return[n] = m.running_return, st.running_length[n] = m.running_length, st.sum_return[n] = m.sum_return;
    st.sum_length[n] = m.sum_length, st.episodes[n] = m.episodes, st.successes[n] = m.successes;
  }
}

// The record as a host loop, in the kernel's order.
inline void monitor_stats_host(const urgym_monitor_state& st, int num_envs, int64_t iteration, int clear, urgym_monitor_record& rec) {
  const double* sum_return = st.sum_return;
  const double sum_r = ordered_sum(num_envs, [sum_return](int n) { return sum_return[n]; });
  int64_t episodes = 0, length_sum = 0, successes = 0;
  for (int n = 0; n < num_envs; n++) episodes += st.episodes[n], length_sum += st.sum_length[n], successes += st.successes[n];
  monitor_tail(sum_r, episodes, length_sum, successes, iteration, rec);
  if (!clear) return;
  for (int n = 0; n < num_envs; n++) st.sum_return[n] = 0.0, st.sum_length[n] = 0, st.episodes[n] = 0, st.successes[n] = 0;
}

// ---- where the records of one urgym_sac_train_monitored call fall (include/urgym.h): index arithmetic on the caller's count of
// iterations and nothing else.  ur_gym_amd.evaluation.monitor_points restates it in Python integers.

// a record follows iteration i where the caller's count, that iteration included, is a multiple of log_every (log_every >= 1, first_iteration >= 0)
inline bool monitor_record_follows(int64_t first_iteration, int32_t log_every, int32_t i) { return (first_iteration + i + 1) % log_every == 0; }

// the records of the whole call: the multiples of log_every in (first_iteration, first_iteration + num_iterations]
inline int64_t monitor_record_count(int64_t first_iteration, int32_t log_every, int32_t num_iterations) {
  return (first_iteration + num_iterations) / log_every - first_iteration / log_every;
}

// what the validation refuses about the placement; nullptr = accepted.  The schedule has been accepted.
inline const char* monitor_schedule_refusal(const urgym_sac_schedule& s, int32_t log_every, int64_t first_iteration, int32_t first_record, int32_t record_capacity) {
  if (log_every < 1) return "monitoring->log_every must be at least 1 (iterations between records)";
  if (first_iteration < 0) return "monitoring->first_iteration is negative";
  if (first_iteration > INT64_MAX - s.num_iterations) return "first_iteration + num_iterations does not fit int64";
  if (first_record < 0) return "monitoring->first_record is negative";
  if (s.steps_per_iteration > s.capacity_steps) return "steps_per_iteration is above capacity_steps (the ring no longer holds an iteration's earlier steps when it is folded)";
  if (monitor_record_count(first_iteration, log_every, s.num_iterations) > (int64_t)record_capacity - first_record)
    return "first_record + the records of the call is beyond record_capacity";
  return nullptr;
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// include/urgym.h, urgym_monitor_fold, validated: DEVICE pointers, 1 <= num_steps <= capacity, 0 <= first_slot < capacity
struct MonitorFoldCall {
  int num_envs, capacity, first_slot, num_steps;
  urgym_monitor_state state;
  const float* reward;
  const uint8_t *terminated, *truncated, *is_success;
};

// include/urgym.h, urgym_monitor_stats, validated
struct MonitorStatsCall {
  int num_envs, clear;
  int64_t iteration;
  urgym_monitor_state state;
  urgym_monitor_record* record;
};

// ONE launch on `s` each.  The caller has validated everything.
void monitor_fold_launch(const MonitorFoldCall& call, hipStream_t s);    // one lane per env
void monitor_stats_launch(const MonitorStatsCall& call, hipStream_t s);  // one workgroup of SAC_TERMS_LANES lanes

}  // namespace urgym
#endif
