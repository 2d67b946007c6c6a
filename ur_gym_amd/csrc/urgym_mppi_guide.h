// urgym_mppi_guide.h — the learner in the planner's loop (include/urgym.h, "MPPI with the learner in the loop"):
// which samples follow the actor, the guided action line and the terminal step, stated once as functions the kernels of
// urgym_mppi_guide.hip and tests/mppi_guide_harness.cpp (a host program, built without HIP) both compile; and, for HIP units only, the
// seam between urgym_mppi_guide.hip and urgym_mppi_abi.hip.  The env map is urgym_mppi.h's, used as it is.  Nothing here is exported.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_mppi.h"

namespace urgym {

// Every function below is ONE operation per line, rounded on its own: the units that compile this are built with -ffp-contract=off.
// ur_gym_amd.evaluation.mppi_guided_actions / mppi_terminal restate them.

// ---- the samples that follow the actor: 1 .. P of every parent (0 is the nominal, the ones past P keep the sample launch's line)
URGYM_HD inline bool mppi_guided(int j, int P) { return j >= 1 && j <= P; }

// ---- the guided action line, float32: the noise is the one the sample launch drew
URGYM_HD inline float mppi_guided_action(float policy_action, float eps, float policy_sigma) {
  const float s = policy_sigma * eps;
  const float a = policy_action + s;
  return fminf(fmaxf(a, -1.0f), 1.0f);
}

// ---- the terminal step, float64
// whether value[n] is read at all: a live future with terminal_value on.  An ended future's value reaches nothing.
URGYM_HD inline bool mppi_terminal_reads_value(uint8_t alive, int terminal_value) { return alive != 0 && terminal_value != 0; }
// the choice between the three cases is a selection; `value` is looked at only where mppi_terminal_reads_value said so
URGYM_HD inline double mppi_terminal_credit(uint8_t alive, uint8_t success, bool reads_value, float value, double fail_cost) {
  if (alive) return reads_value ? (double)value : 0.0;
  if (success) return 0.0;
  return -fail_cost;
}
// ret after the step: untouched where v == 0 (a ret of -0.0 stays -0.0)
URGYM_HD inline double mppi_terminal_return(double ret, double g, double v) {
  if (v != 0.0) {  // true for a NaN
    const double t = g * v;
    ret = ret + t;
  }
  return ret;
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// what the two launches read and write besides urgym_mppi; the caller has validated everything
struct MppiGuideCall {
  int policy_samples, terminal_value;
  float policy_sigma;
  double fail_cost;
  const float* policy_action;  // [E*K][6]
  const float* value;          // [E*K]
  double* terminal;            // [E*K]
};

// ONE launch on `s` each
void mppi_guide_launch(const urgym_mppi& m, const MppiGuideCall& g, int h, hipStream_t s);  // one lane per (n, c)
void mppi_terminal_launch(const urgym_mppi& m, const MppiGuideCall& g, hipStream_t s);      // one lane per planner env

}  // namespace urgym
#endif
