// urgym_mppi_guide.hip — the two kernels that put the learner into the planner's loop (include/urgym.h, "MPPI with the learner in the
// loop"): the guide launch, which rewrites the action rows of the samples that follow the actor, and the terminal
// launch, which credits a future with what lies behind the horizon.  urgym_mppi_guide.h states every float operation; the kernels below
// only decide who runs which of them.  The actor and the critic themselves are urgym_actor.hip's and urgym_critic.hip's launches.
//
// This unit is built with -ffp-contract=off.  There are no atomics and every output has ONE writer.
//
// Launches, 256 lanes a workgroup.  mppi_guide_kernel: one lane per (planner env n, component c), n * 6 + c consecutive, so the stores of
// the P guided samples of a parent are one contiguous run of 6 P floats; a lane of an unguided sample exits before it loads anything.
// mppi_terminal_kernel: one lane per planner env; consecutive lanes read and write consecutive addresses of the state rows.
#include "urgym_mppi_guide.h"

namespace urgym {

namespace {

constexpr int T = 256;

__global__ void __launch_bounds__(T) mppi_guide_kernel(const urgym_mppi M, const MppiGuideCall G, const int h) {
  const size_t NK = (size_t)M.num_parents * (size_t)M.samples;
  const size_t at = (size_t)blockIdx.x * T + threadIdx.x;  // n * 6 + c
  if (at >= NK * 6) return;
  const int n = (int)(at / 6);
  if (!mppi_guided(mppi_sample(n, M.samples), G.policy_samples)) return;
  const size_t row = (size_t)h * NK * 6 + at;
  M.actions[row] = mppi_guided_action(G.policy_action[at], M.eps[row], G.policy_sigma);
}

__global__ void __launch_bounds__(T) mppi_terminal_kernel(const urgym_mppi M, const MppiGuideCall G) {
  const size_t NK = (size_t)M.num_parents * (size_t)M.samples;
  const size_t n = (size_t)blockIdx.x * T + threadIdx.x;
  if (n >= NK) return;
  const uint8_t alive = M.alive[n];
  const bool reads = mppi_terminal_reads_value(alive, G.terminal_value);
  const float value = reads ? G.value[n] : 0.0f;
  const double v = mppi_terminal_credit(alive, M.success[n], reads, value, G.fail_cost);
  G.terminal[n] = v;
  if (v != 0.0) M.ret[n] = mppi_terminal_return(M.ret[n], M.g[n], v);
}

unsigned blocks(size_t lanes) { return (unsigned)((lanes + T - 1) / T); }

}  // namespace

void mppi_guide_launch(const urgym_mppi& m, const MppiGuideCall& g, int h, hipStream_t s) {
  hipLaunchKernelGGL(mppi_guide_kernel, dim3(blocks((size_t)m.num_parents * m.samples * 6)), dim3(T), 0, s, m, g, h);
}

void mppi_terminal_launch(const urgym_mppi& m, const MppiGuideCall& g, hipStream_t s) {
  hipLaunchKernelGGL(mppi_terminal_kernel, dim3(blocks((size_t)m.num_parents * m.samples)), dim3(T), 0, s, m, g);
}

}  // namespace urgym
