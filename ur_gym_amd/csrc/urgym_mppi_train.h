// urgym_mppi_train.h — the seam between the two host units for urgym_sac_train_planned (include/urgym.h, "the planner inside the
// training call"): sac_train_body of urgym_policy_abi.hip drives the call, the planner's checks, collect() and
// plan() stay in urgym_mppi_abi.hip, where the three functions below are defined.  A checking half that launches nothing and fills
// PlannedCall, and two launching halves that refuse nothing.  Host code only.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_handle.h"
#include "urgym_mppi_stats.h"

namespace urgym {

// urgym_sac_planning, validated against the training handle, the learner's ring and the schedule
struct PlannedCall {
  Handle *source, *planner;
  urgym_mppi m;
  urgym_mppi_guide guide;  // with `guided`
  urgym_mppi_adapt adapt;  // with `adaptive`
  urgym_mppi_temper temper;  // with `tempered` (urgym_sac_train_tempered)
  urgym_mppi_noise noise;    // with `colored` (urgym_sac_train_colored)
  bool guided, adaptive, tempered, colored;
  urgym_mppi_explore explore;
  urgym_replay_ring ring;
  Actor* sync_actor;    // the guide's actor where a plan launches it, else null: what planner_sync reloads
  Critic* sync_critic;  // the same for the guide's critic
  urgym_mppi_stats_record* records;  // null: no plan statistics
  int record_capacity;
  MppiStatsCall stats;               // record and iteration move per record
};

// What urgym_sac_train_planned refuses about `planning` alone and what urgym_mppi_collect(_adaptive) refuses about the handles, mppi,
// adapt, guide, explore, the ring and the draws of the whole call, and with temper_or_NULL what urgym_mppi_update_tempered refuses about
// it, and with noise_or_NULL what urgym_mppi_sample_colored refuses about it; the schedule has been accepted.  `h` keeps the message.
int planned_check(const char* who, Handle* h, const urgym_sac_planning* planning, const urgym_replay_ring* ring, const urgym_sac_schedule& schedule, PlannedCall* out,
                  const urgym_mppi_temper* temper_or_NULL = nullptr, const urgym_mppi_noise* noise_or_NULL = nullptr);
// the launches of urgym_mppi_collect(_adaptive), with a temper struct of urgym_mppi_collect_tempered, with a noise struct of
// urgym_mppi_collect_colored
int planned_collect(const PlannedCall& call, uint64_t first_draw, int num_steps, int first_slot, hipStream_t s);
// the launch of urgym_mppi_stats into `record`
void planned_stats(const PlannedCall& call, urgym_mppi_stats_record* record, int64_t iteration, hipStream_t s);

}  // namespace urgym
