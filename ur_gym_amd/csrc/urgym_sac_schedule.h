// urgym_sac_schedule.h — the index arithmetic of one urgym_sac_train call (include/urgym.h) and nothing else:
// which slots, draws, step numbers and ring views the iterations and updates of a call use, as functions of the caller's
// urgym_sac_schedule alone.  Plain C++ without a HIP include: urgym_policy_abi.hip compiles it, and so does
// tests/sac_schedule_harness.cpp, a host program built with g++.  ur_gym_amd.evaluation.training_schedule restates it in Python
// integers.  Nothing here is exported.
//
// The ring arithmetic is DeviceReplay's: a collection of K steps from `cursor` leaves cursor = (cursor + K) % C and
// filled = min(C, filled + K); the oldest valid slot is (cursor - filled) mod C.  Every product is taken in 64 bits: the counts are
// int32, so i * K stays below 2^62.
#pragma once
#include <stdint.h>

#include "../../include/urgym.h"

namespace urgym {

// what the validation refuses (include/urgym.h lists them); nullptr = accepted
inline const char* sac_schedule_refusal(const urgym_sac_schedule& s) {
  if (s.capacity_steps <= 0) return "schedule->capacity_steps must be positive";
  if (s.num_iterations < 1) return "schedule->num_iterations must be at least 1";
  if (s.steps_per_iteration < 0 || s.updates_per_iteration < 0 || s.uniform_iterations < 0 || s.idle_iterations < 0)
    return "a count of the schedule is negative (steps_per_iteration, updates_per_iteration, uniform_iterations, idle_iterations)";
  if (s.steps_per_iteration == 0 && s.updates_per_iteration == 0) return "steps_per_iteration and updates_per_iteration are both 0";
  if (s.first_slot < 0 || s.first_slot >= s.capacity_steps) return "schedule->first_slot outside [0, capacity_steps)";
  if (s.filled_steps < 0 || s.filled_steps > s.capacity_steps) return "schedule->filled_steps outside [0, capacity_steps]";
  const int64_t active = s.num_iterations > s.idle_iterations ? (int64_t)s.num_iterations - s.idle_iterations : 0;
  // the only way to an empty view: nothing in the ring and nothing collected before the first update
  if (active * s.updates_per_iteration > 0 && s.filled_steps == 0 && s.steps_per_iteration == 0)
    return "an update would see an empty ring (filled_steps and steps_per_iteration are both 0)";
  if (s.first_step < 1) return "first_step is the 1-based index of the first Adam step: it must be at least 1";
  const uint64_t updates = (uint64_t)(active * s.updates_per_iteration), top = (uint64_t)1 << 63;
  if (s.update_first_draw > top || updates > top - s.update_first_draw)
    return "update_first_draw + the number of updates is above 2^63 (the top bit marks the policy's own draw)";
  if ((uint64_t)s.first_step > (uint64_t)INT64_MAX - updates) return "first_step + the number of updates does not fit int64";
  return nullptr;
}

// the updates of the whole call: updates_per_iteration in every iteration that is not idle
inline int64_t sac_schedule_updates(const urgym_sac_schedule& s) {
  const int64_t active = s.num_iterations > s.idle_iterations ? (int64_t)s.num_iterations - s.idle_iterations : 0;
  return active * s.updates_per_iteration;
}

// the ring after `iterations` collections of the call
struct SacRing {
  int32_t cursor, filled, oldest;
};
inline SacRing sac_schedule_ring(const urgym_sac_schedule& s, int64_t iterations) {
  const int64_t C = s.capacity_steps, steps = iterations * s.steps_per_iteration;
  SacRing r;
  r.cursor = (int32_t)((s.first_slot + steps) % C);
  r.filled = (int32_t)(s.filled_steps + steps < C ? s.filled_steps + steps : C);
  r.oldest = (int32_t)(((int64_t)r.cursor - r.filled + C) % C);
  return r;
}

// iteration i, 0 <= i < num_iterations
struct SacIteration {
  int32_t collect_first_slot;   // where its collection starts (its steps go to (collect_first_slot + k) % C)
  uint64_t collect_first_draw;  // collect_first_draw + i * K
  int32_t collect_mode;         // URGYM_SAMPLE_UNIFORM for i < uniform_iterations, URGYM_SAMPLE_GAUSSIAN after
  int32_t idle;                 // 1 for i < idle_iterations: no update
  int32_t oldest_slot, filled_steps;  // what its updates see, after its collection
  int64_t first_update;         // the index, over the whole call, of its first update (of the next one, where it has none)
};
inline SacIteration sac_schedule_iteration(const urgym_sac_schedule& s, int32_t i) {
  SacIteration it;
  it.collect_first_slot = sac_schedule_ring(s, i).cursor;
  it.collect_first_draw = s.collect_first_draw + (uint64_t)((int64_t)i * s.steps_per_iteration);
  it.collect_mode = i < s.uniform_iterations ? URGYM_SAMPLE_UNIFORM : URGYM_SAMPLE_GAUSSIAN;
  it.idle = i < s.idle_iterations;
  const SacRing after = sac_schedule_ring(s, (int64_t)i + 1);
  it.oldest_slot = after.oldest, it.filled_steps = after.filled;
  it.first_update = (i > s.idle_iterations ? (int64_t)i - s.idle_iterations : 0) * s.updates_per_iteration;
  return it;
}

// update u, 0 <= u < sac_schedule_updates(s), counted over the whole call across the iterations that are not idle
struct SacUpdate {
  uint64_t gather_draw;  // update_first_draw + u: urgym_replay_sample's draw and that of a' ~ pi(.|s')
  uint64_t policy_draw;  // the same with bit 63 set: the policy's own draw on the batch rows
  int64_t adam_step;     // first_step + u
  int64_t loss_slot;     // u
};
inline SacUpdate sac_schedule_update(const urgym_sac_schedule& s, int64_t u) {
  SacUpdate up;
  up.gather_draw = s.update_first_draw + (uint64_t)u;
  up.policy_draw = up.gather_draw | (uint64_t)1 << 63;
  up.adam_step = s.first_step + u;
  up.loss_slot = u;
  return up;
}

}  // namespace urgym
