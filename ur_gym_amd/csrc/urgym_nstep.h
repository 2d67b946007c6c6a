// urgym_nstep.h — multi-step returns of the replay ring (include/urgym.h, urgym_replay_sample_nstep): the window
// of a drawn transition, the walk that ends it at an episode's end, and the accumulation of the discounted return, stated once as
// functions the gather kernel of urgym_replay.hip and tests/nstep_harness.cpp (a host program, built without HIP) both compile.
// Nothing here is exported.
//
// Every float operation below is float32 with ONE operation per line, rounded on its own: the units that compile this are built with
// -ffp-contract=off (a product is never fused into the sum that takes it).  ur_gym_amd.evaluation.nstep_batch restates it.
#pragma once
#include <stdint.h>

#include "urgym_pack_map.h"  // URGYM_HD

namespace urgym {

constexpr int NSTEP_MAX = 32;   // URGYM_REPLAY_NSTEP_MAX
constexpr int NSTEP_CHUNK = 8;  // steps whose flags and rewards are loaded together before they are scanned

// The flag word of one ring entry: the three bytes as the ring holds them, terminated | truncated << 8 | is_success << 16 (a byte the
// ring does not keep is 0).  An entry ends its episode where either of the first two is non-zero.
constexpr int NSTEP_TRUNCATED_SHIFT = 8, NSTEP_SUCCESS_SHIFT = 16;
constexpr uint32_t NSTEP_ENDS = 0xFFFFu;

// L: the steps a window that starts at age p (0 = the oldest valid slot) may hold; never past the newest valid slot.  p < filled_steps.
URGYM_HD inline int nstep_window(int n_steps, int filled_steps, int p) {
  const int rest = filled_steps - p;
  return n_steps < rest ? n_steps : rest;
}

// the slot of step k of a window that starts at age p: (oldest_slot + p + k) % C, with oldest_slot < C and p + k < filled_steps <= C
URGYM_HD inline int nstep_slot(int oldest_slot, int p, int k, int capacity) {
  const int64_t s = (int64_t)oldest_slot + p + k;  // < 2 C
  return (int)(s >= capacity ? s - capacity : s);
}

// The walk as it stands after some steps: R the return so far, g = gamma^m, m the steps taken, `last` the flag word of entry_{m-1};
// open = no episode end met yet.
struct NstepWalk {
  float R, g;
  int m;
  uint32_t last;
  bool open;
};

URGYM_HD inline NstepWalk nstep_begin(float gamma) { return NstepWalk{0.0f, gamma, 0, 0u, true}; }

// Steps k0 .. k0 + NSTEP_CHUNK - 1 of the window, those below L: flag[j] and reward[j] belong to step k0 + j (entries at or past L
// are not read).  Step 0 starts the return; step k > 0 adds gamma^k reward_k in three roundings.  The walk closes at the first step
// whose entry ended an episode: no later step is taken, so the window never crosses into the env's next episode.
URGYM_HD inline void nstep_chunk(NstepWalk& w, int k0, int L, const uint32_t (&flag)[NSTEP_CHUNK], const float (&reward)[NSTEP_CHUNK], float gamma) {
  for (int j = 0; j < NSTEP_CHUNK; j++) {
    if (k0 + j >= L || !w.open) continue;
    if (k0 + j == 0) {
      w.R = reward[j];
    } else {
      const float t = w.g * reward[j];
      w.R = w.R + t;
      w.g = w.g * gamma;
    }
    w.m = k0 + j + 1;
    w.last = flag[j];
    if (flag[j] & NSTEP_ENDS) w.open = false;
  }
}

}  // namespace urgym
