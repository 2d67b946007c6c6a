// urgym_ik.hip — the kernel of the scripted reach controller (include/urgym.h, "a scripted reach controller on the device"; DESIGN.md
// section 37): one damped least-squares step toward the goal pose per env, written as the action the source step then reads -- inside
// urgym_controller_collect, straight into the action rows of the ring slot.  urgym_ik.h states every float64 operation, those of
// the exploration noise's Box-Muller included (the sample launch's pairing of the words, with ln, cos and sin stated in float64 so that a
// host restates the noise bit for bit); the execute line is urgym_mppi_collect.h's.
//
// This unit is built with -ffp-contract=off.  It carries its own copy of the joint origins (data/ur5e_model.h, handed to the kernel as an
// argument: uniform over the lanes, so they live in scalar registers) and includes nothing of the step unit.  No LDS, no atomics, and
// every output has ONE writer: lane n writes actions[n][0..5] and explore_eps[n][0..5] and nothing else.  sincos and atan2 of the step are
// the device library's; sqrt, frexp and rint are exact or correctly rounded.
//
// Launch: 256 lanes a workgroup, one lane per env.  q and goal are read SoA ([6][N]: consecutive lanes, consecutive doubles).  With
// explore_sigma == 0 a lane draws no Philox word and its action keeps the bits the step gave it.
#include "urgym_ik.h"

#include <string.h>

#include "../../data/ur5e_model.h"
#include "urgym_philox.h"

namespace urgym {

namespace {

constexpr int T = 256;

__global__ void __launch_bounds__(T) ik_actions_kernel(const IkLaunch X) {
  const size_t n = (size_t)blockIdx.x * T + threadIdx.x;
  const size_t N = (size_t)X.N;
  if (n >= N) return;
  const bool rotational = X.rotational != 0;
  double q[6], goal[6];
#pragma unroll
  for (int i = 0; i < 6; i++) q[i] = X.q[(size_t)i * N + n];
#pragma unroll
  for (int i = 0; i < 6; i++) goal[i] = (i < 3 || rotational) ? X.goal[(size_t)i * N + n] : 0.0;
  float a[6];
  ik_action(X.model, q, goal, rotational, X.damping, X.gain, X.action_scale, a);
  float eps[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (!mppi_execute_copies(X.explore_sigma)) {
    const uint32_t k0 = (uint32_t)X.seed, k1 = (uint32_t)(X.seed >> 32);
    const MppiCounter c0 = ik_explore_counter((int)n, X.draw, 0u), c1 = ik_explore_counter((int)n, X.draw, 1u);
    uint32_t u[4], v[4];
    philox4x32_10(k0, k1, c0.c0, c0.c1, c0.c2, c0.c3, u);
    philox4x32_10(k0, k1, c1.c0, c1.c1, c1.c2, c1.c3, v);
    const uint32_t m[6] = {u[0] >> 8, u[1] >> 8, u[2] >> 8, u[3] >> 8, v[0] >> 8, v[1] >> 8};
#pragma unroll
    for (int p = 0; p < 3; p++) ik_box_muller(m[2 * p], m[2 * p + 1], eps[2 * p], eps[2 * p + 1]);  // pairs 0, 1, 2 of the six words
#pragma unroll
    for (int c = 0; c < 6; c++) a[c] = mppi_executed(a[c], eps[c], X.explore_sigma);
  }
#pragma unroll
  for (int c = 0; c < 6; c++) X.actions[n * 6 + c] = a[c];
  if (X.explore_eps) {
#pragma unroll
    for (int c = 0; c < 6; c++) X.explore_eps[n * 6 + c] = eps[c];
  }
}

}  // namespace

void ik_model_fill(IkModel& m) {
  static_assert(sizeof(m.xyz) == sizeof(UR5E_JOINT_XYZ) && sizeof(m.rot) == sizeof(UR5E_JOINT_ROT), "data/ur5e_model.h");
  memcpy(m.xyz, UR5E_JOINT_XYZ, sizeof(m.xyz));
  memcpy(m.rot, UR5E_JOINT_ROT, sizeof(m.rot));
}

void ik_actions_launch(const IkLaunch& x, hipStream_t s) {
  hipLaunchKernelGGL(ik_actions_kernel, dim3((unsigned)(((size_t)x.N + T - 1) / T)), dim3(T), 0, s, x);
}

}  // namespace urgym
