// urgym_mppi_collect.h — planner-collected experience (include/urgym.h, "MPPI files its transitions into the ring"; DESIGN.md section
// 28): the counter of the exploration noise, which word a component's normal comes from, and the execute line, stated once as functions
// the kernel of urgym_mppi_collect.hip and tests/mppi_collect_harness.cpp (a host program, built without HIP) both compile; and, for HIP
// units only, the seam between urgym_mppi_collect.hip and urgym_mppi_abi.hip.  The counter type is urgym_mppi.h's.  Nothing here is
// exported.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_mppi.h"

namespace urgym {

// Every function below is ONE operation per line, rounded on its own: the units that compile this are built with -ffp-contract=off.
// ur_gym_amd.evaluation.mppi_explore_noise / mppi_execute restate them.

// ---- the exploration counter of (parent p, draw) and block 2 / 3; the key is the planner's, (seed lo, seed hi).  The planner's own
// noise (mppi_counter) takes blocks 0 and 1 only, so word 3 alone keeps the two apart whatever (i, h, j) are.
constexpr uint32_t MPPI_EXPLORE_BLOCK = URGYM_MPPI_EXPLORE_BLOCK;  // the first of the two blocks
static_assert(MPPI_EXPLORE_BLOCK == 2u && (MPPI_TAG & 0xFFu) == 0u, "blocks 0 and 1 are the sample launch's (mppi_counter)");
URGYM_HD inline MppiCounter mppi_explore_counter(int p, uint64_t draw, uint32_t block) {
  return MppiCounter{(uint32_t)p, 0u, (uint32_t)draw, MPPI_TAG | block};
}

// ---- component c of the six normals: pair c / 2 of Box-Muller, its cosine (c even) or its sine; the pair's two words are words
// 2 q and 2 q + 1 of the six, w0 .. w3 from block 2 and w4, w5 from block 3 -- the sample launch's order
URGYM_HD inline uint32_t mppi_explore_block_of(int c) { return MPPI_EXPLORE_BLOCK + (c >= 4 ? 1u : 0u); }
URGYM_HD inline int mppi_explore_first_word(int c) {
  const int q = c / 2;
  return (2 * q) & 3;  // within its block: 0, 2, 0
}

// ---- the execute line, float32
URGYM_HD inline float mppi_executed(float action, float e, float explore_sigma) {
  const float s = explore_sigma * e;
  const float a = action + s;
  return fminf(fmaxf(a, -1.0f), 1.0f);
}
// explore_sigma == 0: no word is drawn, the action travels as its 32 bits (a -0.0 stays -0.0, a NaN keeps its payload)
URGYM_HD inline bool mppi_execute_copies(float explore_sigma) { return explore_sigma == 0.0f; }

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// what the execute launch reads and writes; the caller has validated everything
struct MppiExecute {
  int E;
  float explore_sigma;
  uint64_t seed, draw;
  const float* action_out;  // [E][6]
  float* executed;          // [E][6]: inside a collection, the action rows of the ring slot
  float* explore_eps;       // [E][6] or null
};

// ONE launch on `s`, one lane per (p, c)
void mppi_execute_launch(const MppiExecute& x, hipStream_t s);

}  // namespace urgym
#endif
