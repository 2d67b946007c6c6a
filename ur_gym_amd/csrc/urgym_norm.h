// urgym_norm.h — running observation and reward normalization on the device (include/urgym.h, "running
// observation and reward normalization on the device"): the arithmetic of the fold and of the normalization, stated once as functions
// the kernels of urgym_norm.hip and tests/norm_harness.cpp (a host program, built without HIP) both compile; and, for HIP units only,
// the seam between urgym_norm.hip and urgym_policy_abi.hip.  Nothing here is exported.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_pack_map.h"  // URGYM_HD

namespace urgym {

// Every function below is ONE float64 operation per line, rounded on its own: the units that compile this are built with
// -ffp-contract=off; sqrt and / are the correctly rounded ones.  ur_gym_amd.evaluation.norm_sums / norm_merge / norm_fold /
// normalize_rows / normalize_reward restate them.

// ---- THE ORDER OF THE SUMS, a function of the row count N alone.
//   slab b holds rows NORM_SLAB_ROWS b .. min(NORM_SLAB_ROWS (b + 1), N) - 1
//   within a slab, chain q = 0 .. NORM_CHAINS - 1 starts at +0.0 and adds rows (slab start) + q, + q + NORM_CHAINS, ... ascending
//   slab  = (chain0 + chain1) + (chain2 + chain3)
//   part c = 0 .. NORM_PARTS - 1 starts at +0.0 and adds slabs c, c + NORM_PARTS, ... ascending
//   part[c] += part[c + s] for s = NORM_PARTS / 2, ..., 1;  the sum is part[0]
// A chain or a part that holds no term is +0.0, and no partial sum is ever -0.0 (each starts at +0.0), so adding an absent term as +0.0
// or skipping it leaves the same bits.
constexpr int NORM_SLAB_ROWS = 128;
constexpr int NORM_CHAINS = 4;
constexpr int NORM_PARTS = 16;
constexpr int NORM_FEATURE_LANES = 64;  // the combine kernel gives a feature one lane of 64: obs_dim + 2 goal_dim + 1 must fit

URGYM_HD inline int norm_slabs(int n) { return (n + NORM_SLAB_ROWS - 1) / NORM_SLAB_ROWS; }

// the four chains of a slab
URGYM_HD inline double norm_slab_join(double c0, double c1, double c2, double c3) {
  const double a = c0 + c1;
  const double b = c2 + c3;
  return a + b;
}

// what one slot contributes to a group: bm and bv from S1, S2 and n = (double)N
struct NormMoments {
  double bm, bv;
};

URGYM_HD inline NormMoments norm_moments(double s1, double s2, double n) {
  const double bm = s1 / n;
  const double m2 = s2 / n;
  const double sq = bm * bm;
  const double d = m2 - sq;
  const double bv = d > 0.0 ? d : 0.0;
  return NormMoments{bm, bv};
}

// SB3's update_from_moments on one feature; tot = count + n is the caller's (one per group)
URGYM_HD inline void norm_merge(double& mean, double& var, double count, double tot, double n, NormMoments b) {
  const double delta = b.bm - mean;
  const double dn = delta * n;
  const double step = dn / tot;
  const double ma = var * count;
  const double mb = b.bv * n;
  const double mab = ma + mb;
  const double d2 = delta * delta;
  const double d2c = d2 * count;
  const double d2cn = d2c * n;
  const double cross = d2cn / tot;
  const double m2 = mab + cross;
  mean = mean + step;
  var = m2 / tot;
}

// the discounted return of the running episode, before the flags are looked at
URGYM_HD inline double norm_running_ret(double running, double gamma, float reward) {
  const double g = running * gamma;
  return g + (double)reward;
}

// ---- normalize
URGYM_HD inline double norm_inv(double var, double eps) {
  const double v = var + eps;
  const double s = sqrt(v);
  return 1.0 / s;
}

URGYM_HD inline float norm_value(float x, double mean, double inv, double clip) {
  const double c = (double)x - mean;
  const double v = c * inv;
  const double lo = v < -clip ? -clip : v;
  const double hi = lo > clip ? clip : lo;
  return (float)hi;
}

URGYM_HD inline float norm_reward_value(float r, double inv, double clip) {
  const double v = (double)r * inv;
  const double lo = v < -clip ? -clip : v;
  const double hi = lo > clip ? clip : lo;
  return (float)hi;
}

// the ring slot of step k of a fold that starts at first_slot
URGYM_HD inline size_t norm_slot(int first_slot, int k, int capacity) { return (size_t)(((int64_t)first_slot + k) % capacity); }

// the float64 words urgym_norm_fold needs for K steps of N envs: per slot and slab S1 and S2 of every feature and of the return
inline uint64_t norm_workspace_doubles(int num_envs, int features, int num_steps) {
  return (uint64_t)num_steps * (uint64_t)norm_slabs(num_envs) * 2u * (uint64_t)(features + 1);
}

// ---- the fold as host loops, in the kernels' order: x is one group's [N][d] rows of one slot (stride d)
inline double norm_sum_host(const double* v, int n) {  // v[0..n): the terms, already float64
  const int slabs = norm_slabs(n);
  double part[NORM_PARTS];
  for (int c = 0; c < NORM_PARTS; c++) {
    double p = 0.0;
    for (int b = c; b < slabs; b += NORM_PARTS) {
      double chain[NORM_CHAINS];
      const int lo = b * NORM_SLAB_ROWS, hi = lo + NORM_SLAB_ROWS < n ? lo + NORM_SLAB_ROWS : n;
      for (int q = 0; q < NORM_CHAINS; q++) {
        double s = 0.0;
        for (int r = lo + q; r < hi; r += NORM_CHAINS) s += v[r];
        chain[q] = s;
      }
      p += norm_slab_join(chain[0], chain[1], chain[2], chain[3]);
    }
    part[c] = p;
  }
  for (int s = NORM_PARTS / 2; s >= 1; s >>= 1)
    for (int c = 0; c < s; c++) part[c] += part[c + s];
  return part[0];
}

// one slot of one group of d features: the sums and the merge.  term/sq: scratch of n doubles each
inline void norm_fold_group_host(double* mean, double* var, double* count, const float* x, int n, int d, double* term, double* sq) {
  const double nn = (double)n;
  const double c = *count;
  const double tot = c + nn;
  for (int j = 0; j < d; j++) {
    for (int r = 0; r < n; r++) {
      const double v = (double)x[(size_t)r * (size_t)d + (size_t)j];
      term[r] = v, sq[r] = v * v;
    }
    norm_merge(mean[j], var[j], c, tot, nn, norm_moments(norm_sum_host(term, n), norm_sum_host(sq, n), nn));
  }
  *count = tot;
}

// one slot of the return group
inline void norm_fold_ret_host(double* mean, double* var, double* count, double* running, const float* reward, const uint8_t* terminated,
                               const uint8_t* truncated, int n, double gamma, double* sq) {
  const double nn = (double)n;
  const double c = *count;
  const double tot = c + nn;
  for (int r = 0; r < n; r++) {
    running[r] = norm_running_ret(running[r], gamma, reward[r]);
    sq[r] = running[r] * running[r];
  }
  norm_merge(*mean, *var, c, tot, nn, norm_moments(norm_sum_host(running, n), norm_sum_host(sq, n), nn));
  *count = tot;
  for (int r = 0; r < n; r++)
    if ((terminated[r] | truncated[r]) != 0) running[r] = 0.0;
}

// what the entry points refuse about the options; nullptr = accepted
inline const char* norm_options_refusal(const urgym_normalization& o) {
  if (o.reserved0 != 0) return "urgym_normalization.reserved0 must be 0";
  if (!(o.gamma >= 0.0 && o.gamma <= 1.0)) return "gamma must be in [0, 1]";
  if (!(o.eps >= 0.0 && o.eps < INFINITY)) return "eps must be finite and at least 0";
  if (!(o.clip_obs > 0.0)) return "clip_obs must be positive (+inf is allowed)";
  if (!(o.clip_reward > 0.0)) return "clip_reward must be positive (+inf is allowed)";
  return nullptr;
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

constexpr int NORM_GROUPS = 3;  // observation, achieved_goal, desired_goal

// include/urgym.h, urgym_norm_fold, validated.  Feature j of the concatenation [observation | achieved_goal | desired_goal | ret] has
// column j of the workspace: ws[((k B + b) 2 + m) (F + 1) + j], m = 0 for S1 and 1 for S2, B = norm_slabs(N).
struct NormFoldCall {
  int num_envs, capacity, first_slot, num_steps;
  int dim[NORM_GROUPS];  // obs_dim, goal_dim, goal_dim
  int norm_obs, norm_reward;
  double gamma;
  urgym_norm_state state;
  const float* rows[NORM_GROUPS];  // the ring's observation, achieved_goal, desired_goal
  const float* reward;
  const uint8_t *terminated, *truncated;
  double* workspace;
};

// urgym_norm_rows / urgym_norm_batch, validated: up to seven segments of one launch.  A segment is `count * dim` floats mapped from src
// to dst with the statistics mean / var of its group; dim == 1 with mean == nullptr is the reward (no mean is subtracted).
constexpr int NORM_MAX_SEGMENTS = 7;
struct NormSegment {
  const float* src;
  float* dst;
  const double *mean, *var;
  int dim;
  double clip;
};
struct NormApplyCall {
  int count, segments, identity;  // identity: copy unchanged (urgym_norm_rows with norm_obs == 0)
  double eps;
  NormSegment seg[NORM_MAX_SEGMENTS];
};

// urgym_norm_snapshot, validated: dst = src for mean, var, count of the four groups where *when != 0 (when == nullptr: always)
struct NormSnapshotCall {
  int dim[NORM_GROUPS];
  urgym_norm_state src, dst;
  const int32_t* when;
};

// The caller has validated everything.
void norm_snapshot_launch(const NormSnapshotCall& call, hipStream_t s);  // ONE launch of one workgroup
void norm_fold_launch(const NormFoldCall& call, hipStream_t s);    // TWO launches
void norm_apply_launch(const NormApplyCall& call, hipStream_t s);  // ONE launch

}  // namespace urgym
#endif
