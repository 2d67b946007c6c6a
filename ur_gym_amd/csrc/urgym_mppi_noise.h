// urgym_mppi_noise.h — temporally correlated sampling noise of the MPPI planner (include/urgym.h, "temporally correlated sampling
// noise"): the scale the host forms once per call and the first-order autoregressive recurrence along the horizon,
// stated once as functions the kernel of urgym_mppi_noise.hip and tests/mppi_noise_harness.cpp (a host program, built without HIP) both
// compile; and, for HIP units only, the seam between urgym_mppi_noise.hip and urgym_mppi_abi.hip.  The counter and the action line are
// urgym_mppi.h's, used as they are.  Nothing here is exported.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "urgym_mppi.h"

namespace urgym {

// Every function below is ONE operation per line, rounded on its own: the units that compile this are built with -ffp-contract=off.
// ur_gym_amd.evaluation.mppi_colored_noise restates them.

// ---- the scale, ON THE HOST, once per call: float64 throughout, sqrt the correctly rounded one, then one rounding to float32.  The
// kernel is handed beta and scale; it never forms scale itself.
inline float mppi_noise_scale(float beta) {
  const double b = (double)beta;
  const double bb = b * b;
  const double d = 1.0 - bb;
  const double r = sqrt(d);
  return (float)r;
}

// ---- one step h >= 1 of the recurrence, float32: prev = eps[h - 1], xi = THE SAMPLE's eps of step h
URGYM_HD inline float mppi_noise_step(float beta, float scale, float prev, float xi) {
  const float a = beta * prev;
  const float b = scale * xi;
  return a + b;
}

// The whole recurrence as a host loop over rows of `width` floats: xi, eps [H][width]; eps[0] = xi[0].
inline void mppi_noise_host(const float* xi, int H, size_t width, float beta, float scale, float* eps) {
  for (size_t k = 0; k < width; k++) eps[k] = xi[k];
  for (int h = 1; h < H; h++)
    for (size_t k = 0; k < width; k++) eps[(size_t)h * width + k] = mppi_noise_step(beta, scale, eps[(size_t)(h - 1) * width + k], xi[(size_t)h * width + k]);
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// what the coloured sample reads of urgym_mppi_noise and, where the width is per element, of urgym_mppi_adapt; the caller has
// validated everything
struct MppiNoise {
  float beta, scale;  // scale = mppi_noise_scale(beta), formed by the host
  const float* std;   // [H][E][6] the width of the action line, or null: m.sigma
};

// ONE launch on `s`: one lane per (planner env, Box-Muller pair), each running its own H steps.
void mppi_sample_colored_launch(const urgym_mppi& m, const MppiNoise& z, uint64_t draw, int iteration, hipStream_t s);

}  // namespace urgym
#endif
