// urgym_replay_gather.h — the body of the one-step gather, shared by the kernels that draw a ring entry per sample and then copy its
// row: replay_gather_kernel of urgym_replay.hip (the uniform draw) and per_gather_kernel of urgym_per.hip (the descent through the
// priority sums).  Device code only; it moves bytes (float32 rows travel as 32-bit words), so it means the same under either unit's flags.
//
// One wave takes 64 samples.  Lane l holds the ring entry of sample l (it also moves that sample's scalars: index, reward, flags --
// written coalesced), then the wave works through its samples four at a time, a group of 16 lanes per sample with the lanes along the
// row's floats.  16 lanes are one 64-byte run: a row is a few such runs (35 floats = 3 trips, a goal or an action 1), and the four
// groups of a wave write four neighbouring output rows, i.e. one contiguous stretch.
#pragma once
#include "urgym_replay.h"

namespace urgym {

constexpr int GATHER_THREADS = 64;
constexpr int GATHER_GROUP = 16;
constexpr int GATHER_ROUNDS = GATHER_THREADS / (GATHER_THREADS / GATHER_GROUP);  // 16 rounds of 4 samples

__device__ __forceinline__ void gather_row(float* __restrict__ dst, const float* __restrict__ src, int dim, size_t sample, size_t entry, int l) {
  if (!dst) return;
  for (int i = l; i < dim; i += GATHER_GROUP) dst[sample * dim + i] = src[entry * dim + i];
}

// the scalars of sample i, drawn at `entry`: by the sample's own lane
__device__ __forceinline__ void gather_scalars(const urgym_replay_ring& R, const urgym_replay_batch& B, int i, int64_t entry) {
  if (B.index) B.index[i] = entry;
  if (B.reward) B.reward[i] = R.reward[entry];
  if (B.terminated) B.terminated[i] = R.terminated[entry];
  if (B.truncated) B.truncated[i] = R.truncated[entry];
  if (B.is_success) B.is_success[i] = R.is_success[entry];
}

// the rows of the wave's samples base .. base + 63, those below P.count; `entry` is this lane's sample's.  Every lane of the wave
// calls it.
__device__ __forceinline__ void gather_rows(const ReplayGather& P, int base, int lane, int64_t entry) {
  const urgym_replay_ring& R = P.ring;
  const urgym_replay_batch& B = P.batch;
  const int group = lane / GATHER_GROUP, l = lane % GATHER_GROUP;
  const int lo = (int)(uint32_t)entry, hi = (int)(uint32_t)((uint64_t)entry >> 32);
  for (int r = 0; r < GATHER_ROUNDS; r++) {
    const int from = r * (GATHER_THREADS / GATHER_GROUP) + group;  // the lane that holds this group's sample
    const uint32_t e_lo = (uint32_t)__shfl(lo, from), e_hi = (uint32_t)__shfl(hi, from);  // every lane takes part
    const int sample = base + from;
    if (sample >= P.count) continue;
    const size_t e = (size_t)(((uint64_t)e_hi << 32) | e_lo), s = (size_t)sample;
    gather_row(B.observation, R.observation, P.obs_dim, s, e, l);
    gather_row(B.achieved_goal, R.achieved_goal, P.goal_dim, s, e, l);
    gather_row(B.desired_goal, R.desired_goal, P.goal_dim, s, e, l);
    gather_row(B.action, R.action, 6, s, e, l);
    gather_row(B.next_observation, R.next_observation, P.obs_dim, s, e, l);
    gather_row(B.next_achieved_goal, R.next_achieved_goal, P.goal_dim, s, e, l);
    gather_row(B.next_desired_goal, R.next_desired_goal, P.goal_dim, s, e, l);
  }
}

}  // namespace urgym
