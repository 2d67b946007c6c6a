// urgym_her.h — hindsight experience replay on the replay ring (include/urgym.h, urgym_replay_sample_hindsight):
// the relabel decision, the episode window of a drawn transition, the choice of the goal entry and the re-scoring of the row against
// the new goal, stated once as functions the gather kernel of urgym_her.hip and tests/her_harness.cpp (a host program, built without
// HIP) both compile.  Nothing here is exported.
//
// The integers are exact.  Every float operation below is float64 with ONE operation per line, rounded on its own: the units that
// compile this are built with -ffp-contract=off.  The pose terms d, th, d0, th0 are inputs here: they come from pos_distance and
// angular_distance of urgym_device.h (the step kernel's own functions), whose sincos and acos no host restates bitwise.
// ur_gym_amd.evaluation.hindsight_pick / hindsight_batch restate this header.
#pragma once
#include <stdint.h>

#include "urgym_pack_map.h"  // URGYM_HD

namespace urgym {

constexpr int HER_HORIZON_MAX = 256;  // URGYM_HER_HORIZON_MAX
constexpr int HER_CHUNK = 8;          // steps whose flag bytes are loaded together before they are scanned
constexpr int HER_GOAL_FUTURE = 0, HER_GOAL_FINAL = 1, HER_GOAL_OWN = 2;  // URGYM_HER_GOAL_*
constexpr int HER_GOAL_OFFSET = 12;   // the goal lies at floats [12, 12 + goal_dim) of an observation row in all four env kinds

// relabel iff w2 < threshold, threshold in [0, 2^32]: 0 never, 2^32 always
URGYM_HD inline bool her_relabels(uint32_t w2, uint64_t threshold) { return (uint64_t)w2 < threshold; }

// H: the steps the episode window of a transition at age p (0 = the oldest valid slot) may hold; never past the newest valid slot
URGYM_HD inline int her_window(int horizon, int filled_steps, int p) {
  const int rest = filled_steps - p;
  return horizon < rest ? horizon : rest;
}

// the slot of step k of a window that starts at age p: (oldest_slot + p + k) % C, with oldest_slot < C and p + k < filled_steps <= C
URGYM_HD inline int her_slot(int oldest_slot, int p, int k, int capacity) {
  const int64_t s = (int64_t)oldest_slot + p + k;  // < 2 C
  return (int)(s >= capacity ? s - capacity : s);
}

// The walk as it stands: F the steps of the episode seen so far (own step included), open = no episode end met yet.
struct HerWalk {
  int F;
  bool open;
};

URGYM_HD inline HerWalk her_begin() { return HerWalk{0, true}; }

// Steps k0 .. k0 + HER_CHUNK - 1 of the window, those below H: ends[j] = terminated | truncated of entry_{k0 + j} (entries at or past
// H are not read).  F ends as the smallest k + 1 <= H whose entry ended an episode, else H.
URGYM_HD inline void her_chunk(HerWalk& w, int k0, int H, const uint32_t (&ends)[HER_CHUNK]) {
  for (int j = 0; j < HER_CHUNK; j++) {
    if (k0 + j >= H || !w.open) continue;
    w.F = k0 + j + 1;
    if (ends[j]) w.open = false;
  }
}

// j: the step of the window whose next_achieved_goal becomes the goal (FUTURE: uniform on [0, F), own step included; FINAL: the
// episode's last).  OWN picks no entry.
URGYM_HD inline int her_pick(int strategy, uint32_t w3, int F) {
  if (strategy == HER_GOAL_FUTURE) return (int)(((uint64_t)w3 * (uint64_t)F) >> 32);
  return F - 1;
}

// what the re-scoring takes from the handle's urgym_config
struct HerRule {
  double distance_threshold, ori_threshold, w_collision, w_success, w_distance, w_orientation;
  int additive;  // 1: Ori and Obs (the sum of terms); 0: Dyn and Sta (the branching reward)
  int goal_dim;  // 6: position and orientation; 3: position alone (th = th0 = 0)
};

struct HerScore {
  float reward;
  uint8_t terminated, is_success;
};

// G(s, d, th) = (s ? w_success : 0) + (coll ? w_collision : 0) + w_distance d + w_orientation th, in this order
URGYM_HD inline double her_goal_terms(const HerRule& R, bool s, bool coll, double d, double th) {
  double g = s ? R.w_success : 0.0;
  const double c = coll ? R.w_collision : 0.0;
  g = g + c;
  const double t = R.w_distance * d;
  g = g + t;
  const double u = R.w_orientation * th;
  g = g + u;
  return g;
}

// The row's reward and flags against the new goal.  r, terminated, is_success: what the ring holds at the drawn entry; d, th: the
// pose terms of next_achieved_goal against the new goal, d0, th0 against next_desired_goal (th = th0 = 0 where goal_dim is 3).
URGYM_HD inline HerScore her_rescore(const HerRule& R, float r, bool terminated, bool succ0, double d, double th, double d0, double th0) {
  const bool coll = terminated && !succ0;
  bool succ = d < R.distance_threshold;
  if (R.goal_dim == 6) succ = succ && th < R.ori_threshold;
  double out;
  if (R.additive) {
    const double g0 = her_goal_terms(R, succ0, coll, d0, th0);
    const double g1 = her_goal_terms(R, succ, coll, d, th);
    out = (double)r - g0;
    out = out + g1;
  } else if (coll) {
    out = R.w_collision;
  } else if (succ) {
    out = R.w_success;
  } else {
    double S = 0.0;  // the part of the stored reward that does not depend on the goal: the link-distance shaping
    if (!succ0) {
      const double t0 = R.w_distance * d0;
      S = (double)r - t0;
      const double u0 = R.w_orientation * th0;
      S = S - u0;
    }
    const double t = R.w_distance * d;
    const double u = R.w_orientation * th;
    out = t + u;
    out = out + S;
  }
  const bool term = succ || coll;
  return HerScore{(float)out, (uint8_t)term, (uint8_t)(term && !coll)};
}

}  // namespace urgym
