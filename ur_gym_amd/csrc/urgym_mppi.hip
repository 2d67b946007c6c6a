// urgym_mppi.hip — the kernels of the MPPI planner (include/urgym.h, "sampling-based MPC on the device"): the four
// that connect the step kernel to a plan -- fan-out, sample, score, update -- and the record pass of the closed loop.  urgym_mppi.h
// states every index and every float operation; the kernels below only decide who runs which of them.
//
// This unit is built with -ffp-contract=off.  There are no atomics: every output has ONE writer, and the sums of the update are formed
// in the order ordered_partial / ordered_fold state (urgym_sac_terms.h), which depends on nothing but K.  exp, logf, sqrtf, cospif and
// sinpif are the device library's; division is the correctly rounded one.
//
// Launches.  mppi_fanout_kernel, mppi_sample_kernel, mppi_score_kernel, mppi_record_kernel: 256 lanes a workgroup, one lane per planner
// env (fan-out, score), per (h, planner env) (sample) or per source env (record); consecutive lanes write consecutive addresses of the
// SoA state rows.  mppi_update_kernel: ONE workgroup of 1024 lanes per parent, lane j < K holds sample j; the six sums of a horizon step
// are folded side by side through LDS (6 x 1024 doubles = 48 KB), a barrier per level.
#include "urgym_mppi.h"

#include "urgym_philox.h"
#include "urgym_policy_noise.h"

namespace urgym {

namespace {

constexpr int T = 256;  // lanes of a workgroup of every kernel but the update

// rows of a float64 SoA field [rows][E] -> [rows][NK]: lane n reads its parent's column
__device__ __forceinline__ void fan_rows(double* dst, const double* src, int rows, size_t NK, size_t E, size_t n, size_t p) {
  for (int f = 0; f < rows; f++) dst[f * NK + n] = src[f * E + p];
}

// rows [env][dim] of the envs [env0, env0 + cnt): the workgroup's lanes stride over the floats
__device__ __forceinline__ void fan_obs(float* dst, const float* src, size_t dim, size_t env0, size_t cnt, int K, int tid) {
  for (size_t i = tid; i < cnt * dim; i += T) {
    const size_t n = env0 + i / dim, c = i % dim;
    dst[n * dim + c] = src[(size_t)mppi_parent((int)n, K) * dim + c];
  }
}

__global__ void __launch_bounds__(T) mppi_fanout_kernel(const MppiFanout P) {
  const int tid = threadIdx.x;
  const size_t E = (size_t)P.E, NK = E * (size_t)P.K;
  const size_t env0 = (size_t)blockIdx.x * T;
  const size_t cnt = NK - env0 < (size_t)T ? NK - env0 : (size_t)T;
  const size_t n = env0 + tid;
  if (n < NK) {
    const size_t p = (size_t)mppi_parent((int)n, P.K);
    fan_rows(P.dst.q, P.src.q, 6, NK, E, n, p);
    fan_rows(P.dst.goal, P.src.goal, 6, NK, E, n, p);
    fan_rows(P.dst.obst_start, P.src.obst_start, 6, NK, E, n, p);
    fan_rows(P.dst.obst_end, P.src.obst_end, 6, NK, E, n, p);
    fan_rows(P.dst.obst_pos, P.src.obst_pos, 3, NK, E, n, p);
    fan_rows(P.dst.obst_quat, P.src.obst_quat, 4, NK, E, n, p);
    fan_rows(P.dst.obst_vel, P.src.obst_vel, 9, NK, E, n, p);
    fan_rows(P.dst.link_dist, P.src.link_dist, 5, NK, E, n, p);
    P.dst.step_count[n] = P.src.step_count[p];
    P.dst.episode_id[n] = P.src.episode_id[p];
    P.dst.status[n] = 0;
  }
  fan_obs(P.dst.observation, P.src.observation, (size_t)P.obs_dim, env0, cnt, P.K, tid);
  fan_obs(P.dst.achieved_goal, P.src.achieved_goal, (size_t)P.goal_dim, env0, cnt, P.K, tid);
  fan_obs(P.dst.desired_goal, P.src.desired_goal, (size_t)P.goal_dim, env0, cnt, P.K, tid);
}

__global__ void __launch_bounds__(T) mppi_sample_kernel(const urgym_mppi M, const uint64_t draw, const int iteration) {
  const size_t E = (size_t)M.num_parents, NK = E * (size_t)M.samples;
  const size_t at = (size_t)blockIdx.x * T + threadIdx.x;
  if (at >= NK * (size_t)M.horizon) return;
  const int h = (int)(at / NK), n = (int)(at % NK);
  const int p = mppi_parent(n, M.samples), j = mppi_sample(n, M.samples);
  float eps[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (j != 0) {
    const uint32_t k0 = (uint32_t)M.seed, k1 = (uint32_t)(M.seed >> 32);
    const MppiCounter c0 = mppi_counter(p, iteration, h, j, draw, 0u), c1 = mppi_counter(p, iteration, h, j, draw, 1u);
    uint32_t a[4], b[4];
    philox4x32_10(k0, k1, c0.c0, c0.c1, c0.c2, c0.c3, a);
    philox4x32_10(k0, k1, c1.c0, c1.c1, c1.c2, c1.c3, b);
    const float m[6] = {(float)(a[0] >> 8), (float)(a[1] >> 8), (float)(a[2] >> 8), (float)(a[3] >> 8), (float)(b[0] >> 8), (float)(b[1] >> 8)};
#pragma unroll
    for (int q = 0; q < 3; q++) {  // Box-Muller: u1 in (0, 1], u2 in [0, 1), both exact (the GAUSSIAN policy noise's lines)
      const float r = sqrtf(-2.0f * logf((m[2 * q] + 1.0f) * TWO_M24));
      const float turn = 2.0f * (m[2 * q + 1] * TWO_M24);  // angle / pi: exact
      eps[2 * q] = r * cospif(turn);
      eps[2 * q + 1] = r * sinpif(turn);
    }
  }
  const float* mean = M.mean + ((size_t)h * E + (size_t)p) * 6;
#pragma unroll
  for (int c = 0; c < 6; c++) {
    M.eps[at * 6 + c] = eps[c];
    M.actions[at * 6 + c] = mppi_action(mean[c], eps[c], M.sigma);
  }
}

__global__ void __launch_bounds__(T) mppi_score_kernel(const urgym_mppi M, const MppiOutcome O, const int h) {
  const size_t NK = (size_t)M.num_parents * (size_t)M.samples;
  const size_t n = (size_t)blockIdx.x * T + threadIdx.x;
  if (n >= NK) return;
  MppiLane L;
  if (h > 0) L = MppiLane{M.ret[n], M.g[n], M.alive[n], M.end_step[n], M.success[n], M.collided[n]};
  mppi_score_step(L, h, M.horizon, M.gamma, O.reward[n], O.terminated[n], O.truncated[n], O.is_success[n], O.collision[n]);
  M.ret[n] = L.ret, M.g[n] = L.g, M.alive[n] = L.alive, M.end_step[n] = L.end_step, M.success[n] = L.success, M.collided[n] = L.collided;
}

// part[c][t] += part[c][t + s] for s = 512, ..., 1 and c < C: ordered_fold with a barrier per level; a barrier before the first level
template <int C>
__device__ __forceinline__ void fold(double (*part)[MPPI_LANES], int t) {
  __syncthreads();
  for (int s = MPPI_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int c = 0; c < C; c++) part[c][t] += part[c][t + s];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(MPPI_LANES) mppi_update_kernel(const urgym_mppi M) {
  __shared__ double part[6][MPPI_LANES];
  const int t = threadIdx.x, p = blockIdx.x, K = M.samples, H = M.horizon;
  const size_t E = (size_t)M.num_parents, NK = E * (size_t)K;
  const bool in = t < K;
  const size_t n = (size_t)p * K + (in ? t : 0);  // lanes past K read sample 0 and weigh nothing
  const double r = M.ret[n];
  // rmax: a maximum does not depend on the order of its operands
  part[0][t] = in ? mppi_max_term(r) : -INFINITY;
  __syncthreads();
  for (int s = MPPI_LANES / 2; s >= 1; s >>= 1) {
    if (t < s) part[0][t] = fmax(part[0][t], part[0][t + s]);
    __syncthreads();
  }
  const double rmax = part[0][0];
  __syncthreads();  // every lane has rmax before a lane overwrites part[0]
  double w = 0.0;
  if (in && !mppi_weight_fixed(r, rmax, t, w)) w = exp(mppi_exponent(r, rmax, M.lam));
  if (in && M.w) M.w[n] = w;
  // Z and Q side by side
  part[0][t] = ordered_partial(t, K, [w](int) { return w; });
  part[1][t] = ordered_partial(t, K, [w](int) { return mppi_square_term(w); });
  fold<2>(part, t);
  const double Z = part[0][0], Q = part[1][0];
  if (t == 0) {
    M.best_return[p] = rmax;
    M.nominal_return[p] = r;
    M.ess[p] = mppi_ess(Z, Q);
  }
  for (int h = 0; h < H; h++) {
    __syncthreads();  // part[..][0] of the step before (and Z, Q) have been read
    const float* a = M.actions + ((size_t)h * NK + n) * 6;
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const float ac = a[c];
      part[c][t] = ordered_partial(t, K, [w, ac](int) { return mppi_mean_term(w, ac); });
    }
    fold<6>(part, t);
    if (t < 6) {
      const float v = mppi_mean(part[t][0], Z);
      M.new_mean[((size_t)h * E + p) * 6 + t] = v;
      if (h == 0) M.action_out[(size_t)p * 6 + t] = v;
      int first, second;
      mppi_shift_rows(h, H, M.shift, first, second);
      if (first >= 0) M.mean[((size_t)first * E + p) * 6 + t] = v;
      if (second >= 0) M.mean[((size_t)second * E + p) * 6 + t] = v;
    }
  }
}

__device__ __forceinline__ void copy_rows(float* dst, const float* src, size_t first, size_t count, int tid) {
  if (!dst) return;
  for (size_t i = tid; i < count; i += T) dst[first + i] = src[first + i];
}

// record_rows of urgym_actor.hip, restated for the closed loop of the planner (the *_row pointers are the rows of this pass already),
// with the action row and the zeroing of the finished parents' mean
__global__ void __launch_bounds__(T) mppi_record_kernel(const MppiRecord R) {
  const int tid = threadIdx.x;
  const int env0 = blockIdx.x * T;
  const int cnt = min(T, R.E - env0);
  const size_t od = R.obs_dim, gd = R.goal_dim;
  if (R.k < R.num_steps) {
    copy_rows(R.obs, R.observation, env0 * od, cnt * od, tid);
    copy_rows(R.ach, R.achieved_goal, env0 * gd, cnt * gd, tid);
    copy_rows(R.des, R.desired_goal, env0 * gd, cnt * gd, tid);
  }
  const bool summary = R.ep_done != nullptr;
  if (R.k == 0) {
    if (summary && tid < cnt) {
      const int e = env0 + tid;
      R.ep_done[e] = 0;
      if (R.ep_return) R.ep_return[e] = 0.0;
      if (R.ep_last) R.ep_last[e] = 0;
      if (R.ep_success) R.ep_success[e] = 0;
    }
    return;
  }
  copy_rows(R.action_row, R.action_in, (size_t)env0 * 6, (size_t)cnt * 6, tid);
  if (tid < cnt) {
    const int e = env0 + tid;
    const float r = R.reward[e];
    const uint8_t term = R.terminated[e], trunc = R.truncated[e], succ = R.is_success[e];
    if (R.reward_row) R.reward_row[e] = r;
    if (R.terminated_row) R.terminated_row[e] = term;
    if (R.truncated_row) R.truncated_row[e] = trunc;
    if (R.is_success_row) R.is_success_row[e] = succ;
    if (R.collision_row) R.collision_row[e] = R.collision[e];
    if (summary && !R.ep_done[e]) {  // model_test.py:42-49: reward summed while the episode runs; closed at `steps == last or terminated`
      if (R.ep_return) R.ep_return[e] += (double)r;
      if (term || R.k == R.num_steps) {
        if (R.ep_success) R.ep_success[e] = succ;
        if (R.ep_last) R.ep_last[e] = R.k - 1;
        R.ep_done[e] = 1;
      }
    }
    if (term | trunc)  // the episode is over: the next one does not start from this plan
      for (int h = 0; h < R.H; h++)
        for (int c = 0; c < 6; c++) R.mean[((size_t)h * R.E + e) * 6 + c] = 0.0f;
  }
  if (R.final_obs_row && R.auto_reset) {
    for (size_t i = tid; i < cnt * od; i += T) {
      const size_t e = env0 + i / od;
      if (R.terminated[e] | R.truncated[e]) R.final_obs_row[env0 * od + i] = R.final_observation[env0 * od + i];
    }
  }
}

unsigned blocks(size_t lanes) { return (unsigned)((lanes + T - 1) / T); }

}  // namespace

void mppi_fanout_launch(const MppiFanout& f, hipStream_t s) {
  hipLaunchKernelGGL(mppi_fanout_kernel, dim3(blocks((size_t)f.E * f.K)), dim3(T), 0, s, f);
}

void mppi_sample_launch(const urgym_mppi& m, uint64_t draw, int iteration, hipStream_t s) {
  hipLaunchKernelGGL(mppi_sample_kernel, dim3(blocks((size_t)m.num_parents * m.samples * m.horizon)), dim3(T), 0, s, m, draw, iteration);
}

void mppi_score_launch(const urgym_mppi& m, const MppiOutcome& o, int h, hipStream_t s) {
  hipLaunchKernelGGL(mppi_score_kernel, dim3(blocks((size_t)m.num_parents * m.samples)), dim3(T), 0, s, m, o, h);
}

void mppi_update_launch(const urgym_mppi& m, hipStream_t s) {
  hipLaunchKernelGGL(mppi_update_kernel, dim3((unsigned)m.num_parents), dim3(MPPI_LANES), 0, s, m);
}

void mppi_record_launch(const MppiRecord& r, hipStream_t s) {
  hipLaunchKernelGGL(mppi_record_kernel, dim3(blocks((size_t)r.E)), dim3(T), 0, s, r);
}

}  // namespace urgym
