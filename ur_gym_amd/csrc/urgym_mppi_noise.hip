// urgym_mppi_noise.hip — the kernel of the temporally correlated sampling noise (include/urgym.h, "temporally correlated sampling
// noise").  urgym_mppi_noise.h and urgym_mppi.h state every index and every float operation; the kernel below only
// decides who runs which of them.
//
// This unit is built with -ffp-contract=off.  There are no atomics: every output has ONE writer.  logf, sqrtf, cospif and sinpif are the
// device library's, under the flags of urgym_mppi.hip: xi is bitwise what mppi_sample_kernel writes as eps.
//
// Launch.  mppi_sample_colored_kernel: 256 lanes a workgroup, one lane per (planner env n, Box-Muller pair q).  The recurrence is serial
// in h for each (n, c), so a lane walks the horizon with its two values of the step before in registers.  Pairs 0 and 1 take words 0, 1
// and 2, 3 of block 0, pair 2 takes words 0, 1 of block 1: a lane runs ONE Philox call per step (lanes 0 and 1 of an env both run block
// 0 and take two of its words each; no call goes unused).  The three lanes of an env store 8 bytes each, side by side: consecutive
// lanes write consecutive addresses of eps and of actions.  The other shape
// that was weighed -- one lane per planner env, two Philox calls and three pairs per step in series on a third of the lanes, 24 bytes per
// lane and array -- took 1.5 times (H = 6) to 1.7 times (H = 24) as long at E = K = 256 and was not kept.
// mppi_sample_kernel's lines up to xi are restated here so that the text of urgym_mppi.hip stays what it was.
#include "urgym_mppi_noise.h"

#include "urgym_philox.h"
#include "urgym_policy_noise.h"

namespace urgym {

namespace {

constexpr int T = 256;  // lanes of a workgroup

__global__ void __launch_bounds__(T) mppi_sample_colored_kernel(const urgym_mppi M, const MppiNoise Z, const uint64_t draw, const int iteration) {
  const size_t E = (size_t)M.num_parents, NK = E * (size_t)M.samples;
  const size_t at = (size_t)blockIdx.x * T + threadIdx.x;
  if (at >= NK * 3) return;
  const int n = (int)(at / 3), q = (int)(at % 3);
  const int p = mppi_parent(n, M.samples), j = mppi_sample(n, M.samples);
  const uint32_t k0 = (uint32_t)M.seed, k1 = (uint32_t)(M.seed >> 32);
  const uint32_t block = q == 2 ? 1u : 0u;
  float prev[2] = {0.0f, 0.0f};
  for (int h = 0; h < M.horizon; h++) {
    float xi[2] = {0.0f, 0.0f};
    if (j != 0) {  // mppi_sample_kernel's lines, for pair q alone
      const MppiCounter c = mppi_counter(p, iteration, h, j, draw, block);
      uint32_t w[4];
      philox4x32_10(k0, k1, c.c0, c.c1, c.c2, c.c3, w);
      const float m0 = (float)((q == 1 ? w[2] : w[0]) >> 8), m1 = (float)((q == 1 ? w[3] : w[1]) >> 8);
      const float r = sqrtf(-2.0f * logf((m0 + 1.0f) * TWO_M24));
      const float turn = 2.0f * (m1 * TWO_M24);
      xi[0] = r * cospif(turn);
      xi[1] = r * sinpif(turn);
    }
    const size_t out = ((size_t)h * NK + (size_t)n) * 6 + 2 * (size_t)q;
    const size_t row = ((size_t)h * E + (size_t)p) * 6 + 2 * (size_t)q;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const float e = h == 0 ? xi[c] : mppi_noise_step(Z.beta, Z.scale, prev[c], xi[c]);
      const float width = Z.std ? Z.std[row + c] : M.sigma;
      M.eps[out + c] = e;
      M.actions[out + c] = mppi_action(M.mean[row + c], e, width);
      prev[c] = e;
    }
  }
}

unsigned blocks(size_t lanes) { return (unsigned)((lanes + T - 1) / T); }

}  // namespace

void mppi_sample_colored_launch(const urgym_mppi& m, const MppiNoise& z, uint64_t draw, int iteration, hipStream_t s) {
  const size_t lanes = (size_t)m.num_parents * (size_t)m.samples * 3;
  hipLaunchKernelGGL(mppi_sample_colored_kernel, dim3(blocks(lanes)), dim3(T), 0, s, m, z, draw, iteration);
}

}  // namespace urgym
