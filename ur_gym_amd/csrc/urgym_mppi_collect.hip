// urgym_mppi_collect.hip — the kernel that turns a plan's first action into the action the source executes (include/urgym.h, "MPPI files
// its transitions into the ring"): action_out plus exploration noise, clamped, written where the caller says --
// inside urgym_mppi_collect, straight into the action rows of the ring slot the source step then reads.  urgym_mppi_collect.h states the
// counter and every float operation; the Box-Muller lines are the sample launch's (urgym_mppi.hip), word for word.
//
// This unit is built with -ffp-contract=off.  No LDS, no atomics, and every output has ONE writer: lane (p, c) writes executed[p][c] and
// explore_eps[p][c] and nothing else.  logf, sqrtf, cospif and sinpif are the device library's.
//
// Launch: 256 lanes a workgroup, one lane per (parent p, component c), p * 6 + c consecutive.  A lane draws the ONE Philox block that
// holds its pair's two words (block 2 for c < 4, block 3 for c = 4, 5); with explore_sigma == 0 it draws none and copies 32 bits.
#include "urgym_mppi_collect.h"

#include "urgym_philox.h"
#include "urgym_policy_noise.h"

namespace urgym {

namespace {

constexpr int T = 256;

__global__ void __launch_bounds__(T) mppi_execute_kernel(const MppiExecute X) {
  const size_t at = (size_t)blockIdx.x * T + threadIdx.x;  // p * 6 + c
  if (at >= (size_t)X.E * 6) return;
  if (mppi_execute_copies(X.explore_sigma)) {
    reinterpret_cast<uint32_t*>(X.executed)[at] = reinterpret_cast<const uint32_t*>(X.action_out)[at];
    if (X.explore_eps) X.explore_eps[at] = 0.0f;
    return;
  }
  const int p = (int)(at / 6), c = (int)(at - (size_t)p * 6);
  const MppiCounter k = mppi_explore_counter(p, X.draw, mppi_explore_block_of(c));
  uint32_t w[4];
  philox4x32_10((uint32_t)X.seed, (uint32_t)(X.seed >> 32), k.c0, k.c1, k.c2, k.c3, w);
  const int first = mppi_explore_first_word(c);
  const float m1 = (float)(w[first] >> 8), m2 = (float)(w[first + 1] >> 8);
  // Box-Muller: u1 in (0, 1], u2 in [0, 1), both exact (the sample launch's lines)
  const float r = sqrtf(-2.0f * logf((m1 + 1.0f) * TWO_M24));
  const float turn = 2.0f * (m2 * TWO_M24);  // angle / pi: exact
  const float e = (c & 1) ? r * sinpif(turn) : r * cospif(turn);
  X.executed[at] = mppi_executed(X.action_out[at], e, X.explore_sigma);
  if (X.explore_eps) X.explore_eps[at] = e;
}

}  // namespace

void mppi_execute_launch(const MppiExecute& x, hipStream_t s) {
  hipLaunchKernelGGL(mppi_execute_kernel, dim3((unsigned)(((size_t)x.E * 6 + T - 1) / T)), dim3(T), 0, s, x);
}

}  // namespace urgym
