// urgym_mppi.h — the MPPI planner on the device (include/urgym.h, "sampling-based MPC on the device"): the env
// map, the noise counter, the action line, the score step, the weight, the mean and the shift, stated once as functions the kernels of
// urgym_mppi.hip and tests/mppi_harness.cpp (a host program, built without HIP) both compile; and, for HIP units only, the seam between
// urgym_mppi.hip and urgym_mppi_abi.hip.  The ordered sum is urgym_sac_terms.h's (ordered_partial / ordered_fold, SAC_TERMS_LANES), used
// as it is.  Nothing here is exported.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_sac_terms.h"

namespace urgym {

constexpr uint32_t MPPI_TAG = URGYM_MPPI_TAG;  // counter word 3 of the planner's noise is MPPI_TAG | block
constexpr int MPPI_LANES = SAC_TERMS_LANES;    // ONE workgroup of this many lanes per parent runs the update: lane j < K
static_assert(URGYM_MPPI_SAMPLES_MAX == MPPI_LANES, "one lane per sample");

// Every function below is ONE operation per line, rounded on its own: the units that compile this are built with -ffp-contract=off.
// ur_gym_amd.evaluation.mppi_noise / mppi_actions / mppi_score / mppi_update restate them.

// ---- the env map: planner env n = p * K + j is sample j of parent p
URGYM_HD inline int mppi_parent(int n, int K) { return n / K; }
URGYM_HD inline int mppi_sample(int n, int K) {
  const int p = n / K;
  return n - p * K;
}

// ---- the noise counter of (parent p, iteration i, step h, sample j, draw) and block 0 / 1; the key is (seed lo, seed hi)
struct MppiCounter {
  uint32_t c0, c1, c2, c3;
};
URGYM_HD inline MppiCounter mppi_counter(int p, int i, int h, int j, uint64_t draw, uint32_t block) {
  const uint32_t mid = ((uint32_t)i << 24) | ((uint32_t)h << 16) | (uint32_t)j;  // j < 2^10, h < 2^6, i < 2^3: the fields do not meet
  return MppiCounter{(uint32_t)p, mid, (uint32_t)draw, MPPI_TAG | block};
}

// ---- the action line, float32
URGYM_HD inline float mppi_action(float mean, float eps, float sigma) {
  const float s = sigma * eps;
  const float a = mean + s;
  return fminf(fmaxf(a, -1.0f), 1.0f);
}

// ---- the score step, float64: what one planner env carries, and step h of it
struct MppiLane {
  double ret, g;
  uint8_t alive;
  int32_t end_step;
  uint8_t success, collided;
};
URGYM_HD inline void mppi_score_step(MppiLane& L, int h, int H, double gamma, float reward, uint8_t terminated, uint8_t truncated, uint8_t is_success,
                                     uint8_t collision) {
  if (h == 0) L.ret = 0.0, L.g = 1.0, L.alive = 1, L.end_step = H - 1, L.success = 0, L.collided = 0;
  if (!L.alive) return;
  const double t = L.g * (double)reward;
  L.ret = L.ret + t;
  L.g = L.g * gamma;
  if ((terminated | truncated) == 0) return;
  L.alive = 0;
  L.end_step = h;
  L.success = is_success;
  L.collided = collision;
}

// ---- the weight, float64
URGYM_HD inline bool mppi_finite(double r) { return r - r == 0.0; }  // false for a NaN and for either infinity
// one term of rmax: a return that is not finite is passed over
URGYM_HD inline double mppi_max_term(double r) { return mppi_finite(r) ? r : -INFINITY; }
// the argument of exp
URGYM_HD inline double mppi_exponent(double r, double rmax, double lam) {
  const double d = r - rmax;
  return d / lam;
}
// the weight where exp is not needed: none finite (rmax == -inf) gives the nominal alone; a return that is not finite weighs nothing
URGYM_HD inline bool mppi_weight_fixed(double r, double rmax, int j, double& w) {
  if (rmax == -INFINITY) {
    w = j == 0 ? 1.0 : 0.0;
    return true;
  }
  if (!mppi_finite(r)) {
    w = 0.0;
    return true;
  }
  return false;
}

// ---- the mean and the effective sample size from the ordered sums
URGYM_HD inline double mppi_mean_term(double w, float action) { return w * (double)action; }
URGYM_HD inline double mppi_square_term(double w) { return w * w; }
URGYM_HD inline float mppi_mean(double S, double Z) {
  const double m = S / Z;
  return (float)m;
}
URGYM_HD inline double mppi_ess(double Z, double Q) {
  const double zz = Z * Z;
  return zz / Q;
}

// ---- the shift: the rows of mean that new_mean[h] goes to (-1 = none).  Without shift, row h.  With it, row h - 1, and the last step
// also keeps its own row: mean[h] = new_mean[h + 1] for h < H - 1, mean[H - 1] = new_mean[H - 1]
URGYM_HD inline void mppi_shift_rows(int h, int H, int shift, int& first, int& second) {
  first = second = -1;
  if (!shift) {
    first = h;
    return;
  }
  if (h >= 1) first = h - 1;
  if (h == H - 1) second = h;
}

// The whole update of ONE parent as a host loop, in the kernel's order, given the K weights: ret [K], w [K], actions [H][NK][6] with the
// parent's rows at n0 .. n0 + K - 1; new_mean / mean [H][E][6] at parent p.
inline void mppi_update_host(const double* w, const float* actions, int H, int K, size_t NK, size_t n0, int E, int p, int shift, float* new_mean,
                             float* mean, double* ess) {
  const double Z = ordered_sum(K, [&](int j) { return w[j]; });
  const double Q = ordered_sum(K, [&](int j) { return mppi_square_term(w[j]); });
  *ess = mppi_ess(Z, Q);
  for (int h = 0; h < H; h++)
    for (int c = 0; c < 6; c++) {
      const double S = ordered_sum(K, [&](int j) { return mppi_mean_term(w[j], actions[((size_t)h * NK + n0 + j) * 6 + c]); });
      const float v = mppi_mean(S, Z);
      new_mean[((size_t)h * E + p) * 6 + c] = v;
      int first, second;
      mppi_shift_rows(h, H, shift, first, second);
      if (first >= 0) mean[((size_t)first * E + p) * 6 + c] = v;
      if (second >= 0) mean[((size_t)second * E + p) * 6 + c] = v;
    }
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// what the fan-out moves: the bound buffers of both handles, validated
struct MppiFanout {
  urgym_buffers src, dst;
  int E, K, obs_dim, goal_dim;
};

// the planner's outputs that a score launch reads
struct MppiOutcome {
  const float* reward;
  const uint8_t *terminated, *truncated, *is_success, *collision;
};

// pass k of the closed loop's records (include/urgym.h, THE RECORD): the source's bound buffers and the rows of this pass, each may be null
struct MppiRecord {
  int E, H, obs_dim, goal_dim, auto_reset, k, num_steps;
  const float *observation, *achieved_goal, *desired_goal, *reward, *final_observation;
  const uint8_t *terminated, *truncated, *is_success, *collision;
  const float* action_in;  // action_out of the plan
  float *obs, *ach, *des, *action_row;
  float* reward_row;
  uint8_t *terminated_row, *truncated_row, *is_success_row, *collision_row;
  float* final_obs_row;
  double* ep_return;
  int32_t* ep_last;
  uint8_t *ep_success, *ep_done;
  float* mean;
};

// ONE launch on `s` each.  The caller has validated everything.
void mppi_fanout_launch(const MppiFanout& f, hipStream_t s);
void mppi_sample_launch(const urgym_mppi& m, uint64_t draw, int iteration, hipStream_t s);
void mppi_score_launch(const urgym_mppi& m, const MppiOutcome& o, int h, hipStream_t s);
void mppi_update_launch(const urgym_mppi& m, hipStream_t s);  // one workgroup of MPPI_LANES lanes per parent
void mppi_record_launch(const MppiRecord& r, hipStream_t s);

}  // namespace urgym
#endif
