// urgym_replay.hip — the device replay ring of the SAC agent (include/urgym.h, "the replay buffer"): the store pass that
// urgym_rollout_collect runs between the steps, and the gather of urgym_replay_sample.  Both kernels only move bytes; float32 rows
// travel as 32-bit words, so a copy is bitwise whatever the value.  The gather of urgym_replay_sample_nstep also accumulates the
// multi-step return, as urgym_nstep.h states it: this unit is built with -ffp-contract=off.
//
// Layout.  A transition row is 72 to 188 bytes of float32 per side (s and s'), far from any power of two, and a slot starts wherever
// slot * N * dim falls: no 16-byte alignment can be assumed.  Both kernels therefore lay the lanes along the FLOATS of consecutive
// rows, one dword per lane: a wave touches 256 contiguous bytes per access whatever dim is.  The flags are one byte per env.
#include "urgym_replay.h"

#include "urgym_nstep.h"
#include "urgym_replay_gather.h"
#include "urgym_philox.h"

namespace urgym {

namespace {

constexpr int STORE_THREADS = 256;
constexpr int STORE_ENVS = 64;  // envs per workgroup: 1024 workgroups at N = 65536, several per CU

// Rows [env0, env0 + cnt) of one of the three observation arrays: the live value goes to `pre` (the s of slot k) and, unless the env
// finished under auto-reset (then the final_* row), to `next` (the s' of slot k - 1).  The live row is read once for both.
__device__ __forceinline__ void store_rows(const float* __restrict__ live, const float* __restrict__ fin, float* __restrict__ pre,
                                           float* __restrict__ next, const uint8_t* done, int dim, int env0, int cnt, int tid) {
  const size_t first = (size_t)env0 * dim;
  const int total = cnt * dim;
  // env of element i = i / dim, by a float product: i < 64 * 35 and (i + 0.5) / dim is at least 0.5 / 35 away from an integer, far
  // more than the rounding of the two float operations, so the truncation is the exact quotient
  const float inv = 1.0f / (float)dim;
  for (int i = tid; i < total; i += STORE_THREADS) {
    const float v = live[first + i];
    if (pre) pre[first + i] = v;
    if (next) next[first + i] = done[(int)(((float)i + 0.5f) * inv)] ? fin[first + i] : v;
  }
}

__global__ void __launch_bounds__(STORE_THREADS) replay_store_kernel(const ReplayStore P) {
  __shared__ uint8_t done[STORE_ENVS];
  const int tid = threadIdx.x, env0 = blockIdx.x * STORE_ENVS, cnt = min(STORE_ENVS, P.N - env0);
  const bool outcome = P.next_obs != nullptr;
  if (outcome) {
    if (tid < cnt) {
      const int e = env0 + tid;
      const uint8_t term = P.terminated[e], trunc = P.truncated[e];
      done[tid] = P.auto_reset && (term | trunc);
      P.reward_out[e] = P.reward[e];
      P.terminated_out[e] = term;
      if (P.truncated_out) P.truncated_out[e] = trunc;
      if (P.is_success_out) P.is_success_out[e] = P.is_success[e];
    }
    __syncthreads();
  }
  store_rows(P.observation, P.final_observation, P.obs, P.next_obs, done, P.obs_dim, env0, cnt, tid);
  store_rows(P.achieved_goal, P.final_achieved_goal, P.ach, P.next_ach, done, P.goal_dim, env0, cnt, tid);
  store_rows(P.desired_goal, P.final_desired_goal, P.des, P.next_des, done, P.goal_dim, env0, cnt, tid);
}

// The gather (urgym_replay_gather.h states the geometry and holds the body the prioritized draw of urgym_per.hip shares): lane l
// computes the ring entry of sample l, then the wave copies its samples' rows.
__global__ void __launch_bounds__(GATHER_THREADS) replay_gather_kernel(const ReplayGather P) {
  const int lane = threadIdx.x;
  const int base = blockIdx.x * GATHER_THREADS;  // count is an int: so is every sample number
  int64_t entry = 0;
  if (base + lane < P.count) {
    const int i = base + lane;
    uint32_t w[4];
    philox4x32_10((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)i, (uint32_t)P.draw, (uint32_t)(P.draw >> 32), 0x52504C00u, w);
    const uint64_t e = __umul64hi(((uint64_t)w[0] << 32) | w[1], P.size);  // uniform on [0, size)
    const uint64_t step = e / (uint64_t)P.N, env = e - step * (uint64_t)P.N;
    uint64_t slot = (uint64_t)P.oldest_slot + step;  // < 2 C
    if (slot >= (uint64_t)P.capacity) slot -= (uint64_t)P.capacity;
    entry = (int64_t)(slot * (uint64_t)P.N + env);
    gather_scalars(P.ring, P.batch, i, entry);
  }
  gather_rows(P, base, lane, entry);
}

// The gather of multi-step returns (urgym_replay_sample_nstep): replay_gather_kernel's geometry and draw, word for word.  The sample's
// lane also walks its window (urgym_nstep.h).  The addresses of all L flag bytes and rewards follow from (age, env) alone, so the
// lane issues the loads of NSTEP_CHUNK steps together -- none depends on another's result -- and scans what came back; steps at or
// past L (the newest valid slot) are not read.  Two entry numbers per sample go to the row groups: entry_0 for s and the action,
// entry_{m-1} for s'.
__global__ void __launch_bounds__(GATHER_THREADS) replay_gather_nstep_kernel(const ReplayGatherNstep Q) {
  const ReplayGather& P = Q.g;
  const int lane = threadIdx.x;
  const int base = blockIdx.x * GATHER_THREADS;
  const urgym_replay_ring& R = P.ring;
  const urgym_replay_batch& B = P.batch;
  int64_t first = 0, last = 0;
  if (base + lane < P.count) {
    const int i = base + lane;
    uint32_t w[4];
    philox4x32_10((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)i, (uint32_t)P.draw, (uint32_t)(P.draw >> 32), 0x52504C00u, w);
    const uint64_t e = __umul64hi(((uint64_t)w[0] << 32) | w[1], P.size);  // uniform on [0, size)
    const uint64_t step = e / (uint64_t)P.N, env = e - step * (uint64_t)P.N;
    const int p = (int)step;  // < filled_steps
    const int L = nstep_window(Q.n_steps, Q.filled_steps, p);
    NstepWalk walk = nstep_begin(Q.gamma);
    for (int k0 = 0; k0 < L && walk.open; k0 += NSTEP_CHUNK) {
      uint32_t flag[NSTEP_CHUNK];
      float reward[NSTEP_CHUNK];
#pragma unroll
      for (int j = 0; j < NSTEP_CHUNK; j++) {
        flag[j] = 0u, reward[j] = 0.0f;
        if (k0 + j >= Q.n_steps) continue;  // the same for every lane: at n_steps = 1 one set of loads, as replay_gather_kernel
        // a lane whose window is shorter reads its step L - 1 again (nstep_chunk ignores it): no divergent branch, and no entry past
        // the window is read
        const size_t at = (size_t)nstep_slot(P.oldest_slot, p, min(k0 + j, L - 1), P.capacity) * (size_t)P.N + (size_t)env;
        reward[j] = R.reward[at];
        uint32_t f = R.terminated[at];
        if (R.truncated) f |= (uint32_t)R.truncated[at] << NSTEP_TRUNCATED_SHIFT;
        if (R.is_success) f |= (uint32_t)R.is_success[at] << NSTEP_SUCCESS_SHIFT;
        flag[j] = f;
      }
      nstep_chunk(walk, k0, L, flag, reward, Q.gamma);
    }
    first = (int64_t)((uint64_t)nstep_slot(P.oldest_slot, p, 0, P.capacity) * (uint64_t)P.N + env);
    last = (int64_t)((uint64_t)nstep_slot(P.oldest_slot, p, walk.m - 1, P.capacity) * (uint64_t)P.N + env);
    if (B.index) B.index[i] = first;
    if (B.reward) B.reward[i] = walk.R;
    if (B.terminated) B.terminated[i] = (uint8_t)walk.last;
    if (B.truncated) B.truncated[i] = (uint8_t)(walk.last >> NSTEP_TRUNCATED_SHIFT);
    if (B.is_success) B.is_success[i] = (uint8_t)(walk.last >> NSTEP_SUCCESS_SHIFT);
    Q.discount[i] = walk.g;
    if (Q.steps) Q.steps[i] = walk.m;
    if (Q.last_index) Q.last_index[i] = last;
  }
  const int group = lane / GATHER_GROUP, l = lane % GATHER_GROUP;
  const int lo0 = (int)(uint32_t)first, hi0 = (int)(uint32_t)((uint64_t)first >> 32);
  const int lo1 = (int)(uint32_t)last, hi1 = (int)(uint32_t)((uint64_t)last >> 32);
  for (int r = 0; r < GATHER_ROUNDS; r++) {
    const int from = r * (GATHER_THREADS / GATHER_GROUP) + group;  // the lane that holds this group's sample
    const uint32_t a_lo = (uint32_t)__shfl(lo0, from), a_hi = (uint32_t)__shfl(hi0, from);  // every lane takes part
    uint32_t b_lo = a_lo, b_hi = a_hi;  // one step: entry_{m-1} is entry_0
    if (Q.n_steps > 1) b_lo = (uint32_t)__shfl(lo1, from), b_hi = (uint32_t)__shfl(hi1, from);  // the same branch for every lane
    const int sample = base + from;
    if (sample >= P.count) continue;
    const size_t e0 = (size_t)(((uint64_t)a_hi << 32) | a_lo), e1 = (size_t)(((uint64_t)b_hi << 32) | b_lo), s = (size_t)sample;
    gather_row(B.observation, R.observation, P.obs_dim, s, e0, l);
    gather_row(B.achieved_goal, R.achieved_goal, P.goal_dim, s, e0, l);
    gather_row(B.desired_goal, R.desired_goal, P.goal_dim, s, e0, l);
    gather_row(B.action, R.action, 6, s, e0, l);
    gather_row(B.next_observation, R.next_observation, P.obs_dim, s, e1, l);
    gather_row(B.next_achieved_goal, R.next_achieved_goal, P.goal_dim, s, e1, l);
    gather_row(B.next_desired_goal, R.next_desired_goal, P.goal_dim, s, e1, l);
  }
}

}  // namespace

void replay_gather_nstep_launch(const ReplayGatherNstep& p, hipStream_t s) {
  hipLaunchKernelGGL(replay_gather_nstep_kernel, dim3((p.g.count + GATHER_THREADS - 1) / GATHER_THREADS), dim3(GATHER_THREADS), 0, s, p);
}

void replay_store_launch(const ReplayStore& p, hipStream_t s) {
  hipLaunchKernelGGL(replay_store_kernel, dim3((p.N + STORE_ENVS - 1) / STORE_ENVS), dim3(STORE_THREADS), 0, s, p);
}

void replay_gather_launch(const ReplayGather& p, hipStream_t s) {
  hipLaunchKernelGGL(replay_gather_kernel, dim3((p.count + GATHER_THREADS - 1) / GATHER_THREADS), dim3(GATHER_THREADS), 0, s, p);
}

}  // namespace urgym
