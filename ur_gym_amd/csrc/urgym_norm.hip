// urgym_norm.hip — running observation and reward normalization on the device (include/urgym.h, urgym_norm_fold / urgym_norm_rows /
// urgym_norm_batch): the running mean and variance of what the collecting actor saw and of the discounted return,
// folded from the replay ring a collection has just written, and the launch that applies them to rows or to a learner's batch.
//
// The fold is TWO launches whatever the number of slots K:
//   norm_partial_kernel, grid (slabs, K [+ 1]), 256 lanes.  Workgroup (b, k) copies the 128 rows of slab b of slot k -- contiguous in
//     each of the three ring tensors, so consecutive lanes read consecutive addresses, 16 bytes a lane where the slab starts on one --
//     into LDS, then wave q sums rows q, q + 4, ... of the slab with lane j on feature j (an LDS row is then read by consecutive lanes),
//     and waves 0 and 1 join the four chains (wave 0 those of S1, wave 1 those of S2) and write them to the workspace.  The last grid row (norm_reward) is the
//     return group: one lane per env walks the K slots for running_ret, and per slot the workgroup reduces its 128 values through LDS
//     in the same order.
//   norm_combine_kernel, ONE workgroup of 1024 lanes: lane (j, c) = (t % 64, t / 64) adds the slabs c, c + 16, ... of feature j, the 16
//     parts are folded through LDS, and lane (j, 0) merges slot after slot, the state in registers; the state is written once.
// Nothing crosses between workgroups except through the launch boundary; there are no atomics and no arrival counters.  The order of
// every sum is urgym_norm.h's, a function of N alone.
//
// norm_apply_kernel is one grid-stride launch over up to seven segments (urgym_norm_rows: three; urgym_norm_batch: six and the reward):
// every workgroup first forms mean_j and inv_j = 1 / sqrt(var_j + eps) of each segment's features in LDS, once per feature, then maps
// 16 bytes a lane where source and destination are 16-byte aligned, and the tail (or everything) 4 bytes a lane.  An element is read
// and written by the same lane, so a destination may be its source.
//
// norm_snapshot_kernel copies mean, var and count of the four groups from one state to another under a device flag: what an evaluation
// that improved keeps beside the best actor.
//
// This unit is built with -ffp-contract=off: every line of urgym_norm.h is one operation rounded on its own; sqrt and / are the
// correctly rounded ones.
#include <hip/hip_runtime.h>

#include "urgym_norm.h"

namespace urgym {

namespace {

constexpr int PARTIAL_LANES = 256;
constexpr int COMBINE_LANES = NORM_FEATURE_LANES * NORM_PARTS;  // 1024
constexpr int APPLY_LANES = 256;
constexpr int APPLY_MAX_BLOCKS = 2048;
constexpr int APPLY_MAX_DIM = 48;  // a segment's features in LDS; the host refuses more

static_assert(PARTIAL_LANES / 64 == NORM_CHAINS, "one wave per chain");
static_assert(COMBINE_LANES == 1024, "one workgroup");

__device__ inline void copy_rows_to_lds(float* tile, const float* base, int count, int t) {
  if (((uintptr_t)base & 15) == 0) {
    const int vecs = count >> 2;
    const float4* b4 = (const float4*)base;
    float4* t4 = (float4*)tile;
    for (int v = t; v < vecs; v += PARTIAL_LANES) t4[v] = b4[v];
    for (int e = (vecs << 2) + t; e < count; e += PARTIAL_LANES) tile[e] = base[e];
  } else {
    for (int e = t; e < count; e += PARTIAL_LANES) tile[e] = base[e];
  }
}

__global__ void __launch_bounds__(PARTIAL_LANES) norm_partial_kernel(const NormFoldCall P) {
  // the three groups' rows of one slab, each group's block 16-byte aligned: 128 rows x at most 63 features
  __shared__ __attribute__((aligned(16))) float tile[NORM_SLAB_ROWS * NORM_FEATURE_LANES];
  __shared__ double chain[2][NORM_CHAINS][NORM_FEATURE_LANES];
  const int t = threadIdx.x, b = blockIdx.x;
  const int N = P.num_envs, B = norm_slabs(N);
  const int F = P.dim[0] + P.dim[1] + P.dim[2], F1 = F + 1;
  const int row0 = b * NORM_SLAB_ROWS;
  const int rows = min(NORM_SLAB_ROWS, N - row0);
  const int feature_slots = P.norm_obs ? P.num_steps : 0;

  if ((int)blockIdx.y < feature_slots) {
    const int k = blockIdx.y;
    const size_t slot = norm_slot(P.first_slot, k, P.capacity);
    int off = 0;
    for (int g = 0; g < NORM_GROUPS; g++) {
      const int d = P.dim[g];
      copy_rows_to_lds(tile + off, P.rows[g] + (slot * (size_t)N + (size_t)row0) * (size_t)d, rows * d, t);
      off += NORM_SLAB_ROWS * d;
    }
    __syncthreads();
    const int q = t >> 6, j = t & 63;
    if (j < F) {
      int g = 0, jj = j, base = 0;
      while (jj >= P.dim[g]) jj -= P.dim[g], base += NORM_SLAB_ROWS * P.dim[g], g++;
      const int d = P.dim[g];
      double s1 = 0.0, s2 = 0.0;
      for (int r = q; r < rows; r += NORM_CHAINS) {
        const double x = (double)tile[base + r * d + jj];
        const double xx = x * x;
        s1 += x;
        s2 += xx;
      }
      chain[0][q][j] = s1, chain[1][q][j] = s2;
    }
    __syncthreads();
    if (t < 2 * NORM_FEATURE_LANES) {
      const int m = t >> 6;
      if (j < F) P.workspace[(((size_t)k * B + b) * 2 + m) * F1 + j] = norm_slab_join(chain[m][0][j], chain[m][1][j], chain[m][2][j], chain[m][3][j]);
    }
    return;
  }

  // the return group: lane t < 128 is env row0 + t
  double* const rr = (double*)tile;  // [128]
  const int n = row0 + t;
  const bool mine = t < NORM_SLAB_ROWS && n < N;
  double running = mine ? P.state.running_ret[n] : 0.0;
  for (int k = 0; k < P.num_steps; k++) {
    const size_t at = norm_slot(P.first_slot, k, P.capacity) * (size_t)N + (size_t)n;
    if (mine) {
      running = norm_running_ret(running, P.gamma, P.reward[at]);
      rr[t] = running;
    }
    __syncthreads();
    if (t < 2 * NORM_CHAINS) {
      const int q = t & 3, m = t >> 2;
      double s = 0.0;
      for (int r = q; r < rows; r += NORM_CHAINS) {
        const double v = rr[r];
        const double term = m ? v * v : v;
        s += term;
      }
      chain[m][q][0] = s;
    }
    __syncthreads();
    if (t < 2) P.workspace[(((size_t)k * B + b) * 2 + t) * F1 + F] = norm_slab_join(chain[t][0][0], chain[t][1][0], chain[t][2][0], chain[t][3][0]);
    if (mine && (P.terminated[at] | P.truncated[at]) != 0) running = 0.0;
  }
  if (mine) P.state.running_ret[n] = running;
}

__global__ void __launch_bounds__(COMBINE_LANES) norm_combine_kernel(const NormFoldCall P) {
  __shared__ double part[2][NORM_PARTS][NORM_FEATURE_LANES];
  const int t = threadIdx.x, j = t & 63, c = t >> 6;
  const int N = P.num_envs, B = norm_slabs(N);
  const int F = P.dim[0] + P.dim[1] + P.dim[2], F1 = F + 1;
  const bool active = j < F ? P.norm_obs != 0 : (j == F && P.norm_reward != 0);
  // feature j's mean, var and its group's count
  const urgym_norm_state& st = P.state;
  double* const means[4] = {st.observation_mean, st.achieved_goal_mean, st.desired_goal_mean, st.ret_mean};
  double* const vars[4] = {st.observation_var, st.achieved_goal_var, st.desired_goal_var, st.ret_var};
  double* const counts[4] = {st.observation_count, st.achieved_goal_count, st.desired_goal_count, st.ret_count};
  int g = 0, jj = j;
  if (j < F)
    while (jj >= P.dim[g]) jj -= P.dim[g], g++;
  else
    g = 3, jj = 0;
  const bool owner = active && c == 0;
  double mean = 0.0, var = 0.0, count = 0.0;
  if (owner) mean = means[g][jj], var = vars[g][jj], count = counts[g][0];
  const double nn = (double)N;
  for (int k = 0; k < P.num_steps; k++) {
    double p1 = 0.0, p2 = 0.0;
    if (active) {
      const double* ws = P.workspace + ((size_t)k * B * 2) * F1 + j;
      // unrolled so that eight pairs of loads are in flight before the first addition waits; the additions keep the loop's order
#pragma unroll 8
      for (int b = c; b < B; b += NORM_PARTS) {
        p1 += ws[((size_t)b * 2 + 0) * F1];
        p2 += ws[((size_t)b * 2 + 1) * F1];
      }
    }
    part[0][c][j] = p1, part[1][c][j] = p2;
    __syncthreads();
    for (int s = NORM_PARTS / 2; s >= 1; s >>= 1) {
      if (c < s) {
        part[0][c][j] += part[0][c + s][j];
        part[1][c][j] += part[1][c + s][j];
      }
      __syncthreads();
    }
    if (owner) {
      const double tot = count + nn;
      norm_merge(mean, var, count, tot, nn, norm_moments(part[0][0][j], part[1][0][j], nn));
      count = tot;
    }
  }
  if (owner) {
    means[g][jj] = mean, vars[g][jj] = var;
    if (jj == 0) counts[g][0] = count;
  }
}

__device__ inline float apply_one(float x, int j, const double* sm, const double* si, double clip, bool identity, bool reward) {
  if (identity) return x;
  return reward ? norm_reward_value(x, si[j], clip) : norm_value(x, sm[j], si[j], clip);
}

__global__ void __launch_bounds__(APPLY_LANES) norm_apply_kernel(const NormApplyCall P) {
  __shared__ double sm[NORM_MAX_SEGMENTS][APPLY_MAX_DIM];
  __shared__ double si[NORM_MAX_SEGMENTS][APPLY_MAX_DIM];
  const int t = threadIdx.x;
  const bool identity = P.identity != 0;
  if (!identity) {
    for (int e = t; e < P.segments * APPLY_MAX_DIM; e += APPLY_LANES) {
      const int s = e / APPLY_MAX_DIM, j = e % APPLY_MAX_DIM;
      const NormSegment& seg = P.seg[s];
      if (j < seg.dim) {
        sm[s][j] = seg.mean ? seg.mean[j] : 0.0;
        si[s][j] = norm_inv(seg.var[j], P.eps);
      }
    }
    __syncthreads();
  }
  const size_t gid = (size_t)blockIdx.x * APPLY_LANES + t, stride = (size_t)gridDim.x * APPLY_LANES;
  for (int s = 0; s < P.segments; s++) {
    const NormSegment& seg = P.seg[s];
    const size_t total = (size_t)P.count * (size_t)seg.dim;
    const bool reward = seg.mean == nullptr;
    const int d = seg.dim;
    size_t done = 0;
    if ((((uintptr_t)seg.src | (uintptr_t)seg.dst) & 15) == 0) {
      const size_t vecs = total >> 2;
      const float4* s4 = (const float4*)seg.src;
      float4* d4 = (float4*)seg.dst;
      for (size_t v = gid; v < vecs; v += stride) {
        float4 x = s4[v];
        int j = (int)((v << 2) % (size_t)d);
        x.x = apply_one(x.x, j, sm[s], si[s], seg.clip, identity, reward);
        j = j + 1 == d ? 0 : j + 1;
        x.y = apply_one(x.y, j, sm[s], si[s], seg.clip, identity, reward);
        j = j + 1 == d ? 0 : j + 1;
        x.z = apply_one(x.z, j, sm[s], si[s], seg.clip, identity, reward);
        j = j + 1 == d ? 0 : j + 1;
        x.w = apply_one(x.w, j, sm[s], si[s], seg.clip, identity, reward);
        d4[v] = x;
      }
      done = vecs << 2;
    }
    for (size_t e = done + gid; e < total; e += stride) seg.dst[e] = apply_one(seg.src[e], (int)(e % (size_t)d), sm[s], si[s], seg.clip, identity, reward);
  }
}

// the state snapshot under a device flag, the twin of actor_snapshot_kernel's `when`: lane j copies feature j's mean and var, the first
// lane of a group its count.  One workgroup of 64 lanes: at most 63 features and the return group.
__global__ void __launch_bounds__(NORM_FEATURE_LANES) norm_snapshot_kernel(const NormSnapshotCall P) {
  if (P.when != nullptr && P.when[0] == 0) return;
  const int j = threadIdx.x;
  const int F = P.dim[0] + P.dim[1] + P.dim[2];
  if (j > F) return;
  const double* const sm[4] = {P.src.observation_mean, P.src.achieved_goal_mean, P.src.desired_goal_mean, P.src.ret_mean};
  const double* const sv[4] = {P.src.observation_var, P.src.achieved_goal_var, P.src.desired_goal_var, P.src.ret_var};
  const double* const sc[4] = {P.src.observation_count, P.src.achieved_goal_count, P.src.desired_goal_count, P.src.ret_count};
  double* const dm[4] = {P.dst.observation_mean, P.dst.achieved_goal_mean, P.dst.desired_goal_mean, P.dst.ret_mean};
  double* const dv[4] = {P.dst.observation_var, P.dst.achieved_goal_var, P.dst.desired_goal_var, P.dst.ret_var};
  double* const dc[4] = {P.dst.observation_count, P.dst.achieved_goal_count, P.dst.desired_goal_count, P.dst.ret_count};
  int g = 0, jj = j;
  if (j < F)
    while (jj >= P.dim[g]) jj -= P.dim[g], g++;
  else
    g = 3, jj = 0;
  dm[g][jj] = sm[g][jj], dv[g][jj] = sv[g][jj];
  if (jj == 0) dc[g][0] = sc[g][0];
}

}  // namespace

void norm_snapshot_launch(const NormSnapshotCall& call, hipStream_t s) {
  hipLaunchKernelGGL(norm_snapshot_kernel, dim3(1), dim3(NORM_FEATURE_LANES), 0, s, call);
}

void norm_fold_launch(const NormFoldCall& call, hipStream_t s) {
  const int rows = (call.norm_obs ? call.num_steps : 0) + (call.norm_reward ? 1 : 0);
  if (rows == 0) return;
  hipLaunchKernelGGL(norm_partial_kernel, dim3(norm_slabs(call.num_envs), rows), dim3(PARTIAL_LANES), 0, s, call);
  hipLaunchKernelGGL(norm_combine_kernel, dim3(1), dim3(COMBINE_LANES), 0, s, call);
}

void norm_apply_launch(const NormApplyCall& call, hipStream_t s) {
  size_t most = 1;
  for (int i = 0; i < call.segments; i++) most = std::max(most, (size_t)call.count * (size_t)call.seg[i].dim);
  const size_t blocks = std::min((size_t)APPLY_MAX_BLOCKS, (most / 4 + APPLY_LANES - 1) / APPLY_LANES);
  hipLaunchKernelGGL(norm_apply_kernel, dim3((unsigned)std::max((size_t)1, blocks)), dim3(APPLY_LANES), 0, s, call);
}

}  // namespace urgym
