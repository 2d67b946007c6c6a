// urgym_her.hip — the gather of hindsight experience replay (include/urgym.h, urgym_replay_sample_hindsight):
// replay_gather_kernel's geometry and draw, word for word, with the goal of a relabelled sample replaced by a pose its own episode
// reached later and the row re-scored against it, as urgym_her.h states.  A unit of its own, built with -ffp-contract=off: the
// re-scoring is float64 with one operation per line, and the pose distances are the step kernel's functions (urgym_device.h) under
// the step kernel's contraction setting.  The kernels of urgym_replay.hip and urgym_per.hip are not touched.
//
// One wave takes 64 samples (urgym_replay_gather.h).  The sample's lane draws, decides, walks the flag bytes of its episode window --
// the addresses follow from (age, env) alone, so the loads of HER_CHUNK steps are issued together and then scanned; steps at or past
// H are not read -- picks the goal entry, re-scores and writes the scalars.  Then the wave moves the rows by groups of 16 lanes: the
// goal entry is shuffled beside the drawn entry, and the goal slice of the two observation rows and the two desired goals are taken
// from it.
#include "urgym_replay.h"

#include "urgym_device.h"
#include "urgym_her.h"
#include "urgym_replay_gather.h"

namespace urgym {

namespace {

// a row of `dim` floats whose floats [at, at + goal_dim) come from `goal` where that is given
__device__ __forceinline__ void gather_row_goal(float* __restrict__ dst, const float* __restrict__ src, const float* __restrict__ goal, int dim, int at,
                                                int goal_dim, size_t sample, size_t entry, int l) {
  if (!dst) return;
  for (int i = l; i < dim; i += GATHER_GROUP) {
    const bool swap = goal && i >= at && i < at + goal_dim;
    dst[sample * dim + i] = swap ? goal[i - at] : src[entry * dim + i];
  }
}

__global__ void __launch_bounds__(GATHER_THREADS) replay_gather_hindsight_kernel(const ReplayGatherHindsight Q) {
  const ReplayGather& P = Q.g;
  const int lane = threadIdx.x;
  const int base = blockIdx.x * GATHER_THREADS;
  const urgym_replay_ring& R = P.ring;
  const urgym_replay_batch& B = P.batch;
  const int GD = P.goal_dim;
  int64_t entry = 0, goal = -1;  // goal: the ring entry whose row holds the new goal (the drawn entry itself with OWN), -1 = keep
  if (base + lane < P.count) {
    const int i = base + lane;
    uint32_t w[4];
    philox4x32_10((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)i, (uint32_t)P.draw, (uint32_t)(P.draw >> 32), 0x52504C00u, w);
    const uint64_t e = __umul64hi(((uint64_t)w[0] << 32) | w[1], P.size);  // uniform on [0, size)
    const uint64_t step = e / (uint64_t)P.N, env = e - step * (uint64_t)P.N;
    const int p = (int)step;  // < filled_steps
    entry = (int64_t)((uint64_t)her_slot(P.oldest_slot, p, 0, P.capacity) * (uint64_t)P.N + env);
    float reward = R.reward[entry];
    uint8_t terminated = R.terminated[entry], is_success = R.is_success[entry];
    int64_t picked = -1;
    double d = 0.0, th = 0.0, d0 = 0.0, th0 = 0.0;
    if (her_relabels(w[2], Q.relabel_threshold)) {
      goal = entry;
      if (Q.strategy != HER_GOAL_OWN) {
        const int H = her_window(Q.horizon, Q.filled_steps, p);
        HerWalk walk = her_begin();
        for (int k0 = 0; k0 < H && walk.open; k0 += HER_CHUNK) {
          uint32_t ends[HER_CHUNK];
#pragma unroll
          for (int j = 0; j < HER_CHUNK; j++) {
            // a lane whose window is shorter reads its step H - 1 again (her_chunk ignores it): no entry past the window is read
            const size_t at = (size_t)her_slot(P.oldest_slot, p, min(k0 + j, H - 1), P.capacity) * (size_t)P.N + (size_t)env;
            ends[j] = (uint32_t)R.terminated[at] | (uint32_t)R.truncated[at];
          }
          her_chunk(walk, k0, H, ends);
        }
        const int j = her_pick(Q.strategy, w[3], walk.F);
        goal = picked = (int64_t)((uint64_t)her_slot(P.oldest_slot, p, j, P.capacity) * (uint64_t)P.N + env);
      }
      const float* g1 = Q.strategy == HER_GOAL_OWN ? R.next_desired_goal + (size_t)entry * GD : R.next_achieved_goal + (size_t)goal * GD;
      const float* a = R.next_achieved_goal + (size_t)entry * GD;
      const float* g0 = R.next_desired_goal + (size_t)entry * GD;
      double a6[6] = {0, 0, 0, 0, 0, 0}, n6[6] = {0, 0, 0, 0, 0, 0}, o6[6] = {0, 0, 0, 0, 0, 0};
      for (int k = 0; k < 6; k++)
        if (k < GD) a6[k] = (double)a[k], n6[k] = (double)g1[k], o6[k] = (double)g0[k];
      d = pos_distance(a6, n6), d0 = pos_distance(a6, o6);
      if (GD == 6) th = angular_distance(a6 + 3, n6 + 3), th0 = angular_distance(a6 + 3, o6 + 3);
      const HerRule rule{Q.distance_threshold, Q.ori_threshold, Q.w_collision, Q.w_success, Q.w_distance, Q.w_orientation, Q.additive, GD};
      const HerScore s = her_rescore(rule, reward, terminated != 0, is_success != 0, d, th, d0, th0);
      reward = s.reward, terminated = s.terminated, is_success = s.is_success;
    }
    if (B.index) B.index[i] = entry;
    if (B.reward) B.reward[i] = reward;
    if (B.terminated) B.terminated[i] = terminated;
    if (B.truncated) B.truncated[i] = R.truncated[entry];
    if (B.is_success) B.is_success[i] = is_success;
    if (Q.goal_index) Q.goal_index[i] = picked;
    if (Q.pose_terms) {
      double* t = Q.pose_terms + (size_t)i * 4;
      t[0] = d, t[1] = th, t[2] = d0, t[3] = th0;
    }
  }
  const int group = lane / GATHER_GROUP, l = lane % GATHER_GROUP;
  const int lo0 = (int)(uint32_t)entry, hi0 = (int)(uint32_t)((uint64_t)entry >> 32);
  const int lo1 = (int)(uint32_t)goal, hi1 = (int)(uint32_t)((uint64_t)goal >> 32);
  const float* const goal_rows = Q.strategy == HER_GOAL_OWN ? R.next_desired_goal : R.next_achieved_goal;
  for (int r = 0; r < GATHER_ROUNDS; r++) {
    const int from = r * (GATHER_THREADS / GATHER_GROUP) + group;  // the lane that holds this group's sample
    const uint32_t a_lo = (uint32_t)__shfl(lo0, from), a_hi = (uint32_t)__shfl(hi0, from);  // every lane takes part
    const uint32_t b_lo = (uint32_t)__shfl(lo1, from), b_hi = (uint32_t)__shfl(hi1, from);
    const int sample = base + from;
    if (sample >= P.count) continue;
    const size_t e = (size_t)(((uint64_t)a_hi << 32) | a_lo), s = (size_t)sample;
    const int64_t g = (int64_t)(((uint64_t)b_hi << 32) | b_lo);
    const float* ng = g < 0 ? nullptr : goal_rows + (size_t)g * GD;  // the same for the 16 lanes of a group
    gather_row_goal(B.observation, R.observation, ng, P.obs_dim, HER_GOAL_OFFSET, GD, s, e, l);
    gather_row(B.achieved_goal, R.achieved_goal, GD, s, e, l);
    gather_row_goal(B.desired_goal, R.desired_goal, ng, GD, 0, GD, s, e, l);
    gather_row(B.action, R.action, 6, s, e, l);
    gather_row_goal(B.next_observation, R.next_observation, ng, P.obs_dim, HER_GOAL_OFFSET, GD, s, e, l);
    gather_row(B.next_achieved_goal, R.next_achieved_goal, GD, s, e, l);
    gather_row_goal(B.next_desired_goal, R.next_desired_goal, ng, GD, 0, GD, s, e, l);
  }
}

}  // namespace

void replay_gather_hindsight_launch(const ReplayGatherHindsight& p, hipStream_t s) {
  hipLaunchKernelGGL(replay_gather_hindsight_kernel, dim3((p.g.count + GATHER_THREADS - 1) / GATHER_THREADS), dim3(GATHER_THREADS), 0, s, p);
}

}  // namespace urgym
