// urgym_mppi_temper.h — the MPPI temperature from a target effective sample size (include/urgym.h, "the temperature from a target
// effective sample size"): the exponential, the weight at a temperature, the effective sample size at a temperature
// and the search, stated once as functions the kernel of urgym_mppi_temper.hip and tests/mppi_temper_harness.cpp (a host program, built
// without HIP) both compile; and, for HIP units only, the seam between urgym_mppi_temper.hip and urgym_mppi_abi.hip.  rmax, the rank, the
// mean, the effective sample size, the std, the shift and the ordered sum are urgym_mppi.h's, urgym_mppi_elite.h's and
// urgym_sac_terms.h's, used as they are.  Nothing here is exported.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/urgym.h"
#include "urgym_mppi.h"
#include "urgym_mppi_elite.h"

namespace urgym {

// Every function below is ONE operation per line, rounded on its own: the units that compile this are built with -ffp-contract=off.
// ur_gym_amd.evaluation.mppi_temper_exp / mppi_temper_solve restate them.

// ---- THE EXPONENTIAL, float64, for x <= 0.  The weights of the untempered updates come from the device library's exp, which no host
// restates bitwise; a search that compares an effective sample size with a target cannot be handed its exponentials, so it has its own.
// x = kf ln 2 + r with |r| <= ln 2 / 2 (a little more at a half-way point of x * LOG2E); exp(r) by the Taylor polynomial of degree 13,
// whose first neglected term is below 2^-58 there; the power of two by its exponent field.
constexpr double MPPI_TEMPER_EXP_MIN = -708.0;  // below it the result is +0.0; at it kf = -1021, so the power of two is normal
constexpr double MPPI_TEMPER_LOG2E = 1.4426950408889634;
constexpr double MPPI_TEMPER_LN2_HI = 6.93147180369123816490e-01;  // fdlibm's split of ln 2: the high part has 21 trailing zero bits, so
constexpr double MPPI_TEMPER_LN2_LO = 1.90821492927058770002e-10;  // kf * LN2_HI is exact for |kf| <= 1022
// one Horner step: p r + c in two roundings
URGYM_HD inline double mppi_temper_horner(double p, double r, double c) {
  const double t = p * r;
  return t + c;
}

// x must not be a NaN and must not be positive (the caller's x is (r - rmax) / lam of a finite r: never either)
URGYM_HD inline double mppi_temper_exp(double x) {
  if (x < MPPI_TEMPER_EXP_MIN) return 0.0;
  const double y = x * MPPI_TEMPER_LOG2E;
  const double kf = rint(y);  // to nearest, ties to even
  const double hi = kf * MPPI_TEMPER_LN2_HI;
  const double r1 = x - hi;
  const double lo = kf * MPPI_TEMPER_LN2_LO;
  const double r = r1 - lo;
  // the Taylor polynomial of degree 13: 1 / n! for n = 13 .. 0, each the correctly rounded float64
  double p = 1.6059043836821613e-10;
  p = mppi_temper_horner(p, r, 2.08767569878681e-09);
  p = mppi_temper_horner(p, r, 2.505210838544172e-08);
  p = mppi_temper_horner(p, r, 2.755731922398589e-07);
  p = mppi_temper_horner(p, r, 2.7557319223985893e-06);
  p = mppi_temper_horner(p, r, 2.48015873015873e-05);
  p = mppi_temper_horner(p, r, 0.0001984126984126984);
  p = mppi_temper_horner(p, r, 0.001388888888888889);
  p = mppi_temper_horner(p, r, 0.008333333333333333);
  p = mppi_temper_horner(p, r, 0.041666666666666664);
  p = mppi_temper_horner(p, r, 0.16666666666666666);
  p = mppi_temper_horner(p, r, 0.5);
  p = mppi_temper_horner(p, r, 1.0);
  p = mppi_temper_horner(p, r, 1.0);
  const uint64_t bits = (uint64_t)(1023 + (int64_t)kf) << 52;  // kf in [-1021, 0]: a normal power of two
  double scale;
  memcpy(&scale, &bits, sizeof(scale));
  return p * scale;
}

// ---- the weight at a temperature, float64: a sample that is not counted (not finite; with elites, no elite) weighs nothing
URGYM_HD inline double mppi_temper_weight(double r, double rmax, double lam, bool counted) {
  if (!counted) return 0.0;
  const double x = mppi_exponent(r, rmax, lam);  // d = r - rmax; x = d / lam
  return mppi_temper_exp(x);
}

// ---- the geometric mean of the bracket
URGYM_HD inline double mppi_temper_mid(double lo, double hi) {
  const double q = lo * hi;
  return sqrt(q);
}

// ---- THE SEARCH as the steps both sides run.  `Ess` is lam -> the effective sample size at lam (Z and Q THE ORDERED SUMs of w and
// w * w, mppi_ess of them); the kernel's folds the sums through LDS, the host's runs ordered_sum.  The number of evaluations depends on
// nothing but which of the three cases holds; inside the bisection there is no early exit.
constexpr uint8_t MPPI_TEMPER_SOLVED = URGYM_MPPI_TEMPER_SOLVED, MPPI_TEMPER_AT_MAX = URGYM_MPPI_TEMPER_AT_MAX, MPPI_TEMPER_AT_MIN = URGYM_MPPI_TEMPER_AT_MIN,
                  MPPI_TEMPER_NO_RETURN = URGYM_MPPI_TEMPER_NO_RETURN;

template <class Ess>
URGYM_HD inline __attribute__((always_inline)) double mppi_temper_search(double target, double lam_min, double lam_max, int steps, Ess ess, uint8_t& saturated) {
  if (ess(lam_max) < target) {
    saturated = MPPI_TEMPER_AT_MAX;
    return lam_max;
  }
  if (ess(lam_min) >= target) {
    saturated = MPPI_TEMPER_AT_MIN;
    return lam_min;
  }
  double lo = lam_min, hi = lam_max;
  for (int i = 0; i < steps; i++) {
    const double mid = mppi_temper_mid(lo, hi);
    const double e = ess(mid);
    if (e >= target) hi = mid;
    else lo = mid;
  }
  saturated = MPPI_TEMPER_SOLVED;
  return hi;
}

// The search and the final weights of ONE parent as a host loop: ret [K], counted [K] (finite without elites, elite with them) -> *lam,
// *saturated, w [K].  `lam_fixed` is urgym_mppi.lam, kept where no return is finite.
inline void mppi_temper_solve_host(const double* ret, const uint8_t* counted, int K, double target, double lam_min, double lam_max, int steps, double lam_fixed,
                                   double* lam, uint8_t* saturated, double* w) {
  double rmax = -INFINITY;
  for (int j = 0; j < K; j++) rmax = fmax(rmax, mppi_max_term(ret[j]));
  if (rmax == -INFINITY) {
    *lam = lam_fixed, *saturated = MPPI_TEMPER_NO_RETURN;
    for (int j = 0; j < K; j++) w[j] = j == 0 ? 1.0 : 0.0;
    return;
  }
  auto ess = [&](double at) {
    const double Z = ordered_sum(K, [&](int j) { return mppi_temper_weight(ret[j], rmax, at, counted[j] != 0); });
    const double Q = ordered_sum(K, [&](int j) { return mppi_square_term(mppi_temper_weight(ret[j], rmax, at, counted[j] != 0)); });
    return mppi_ess(Z, Q);
  };
  *lam = mppi_temper_search(target, lam_min, lam_max, steps, ess, *saturated);
  for (int j = 0; j < K; j++) w[j] = mppi_temper_weight(ret[j], rmax, *lam, counted[j] != 0);
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// what the launch reads of urgym_mppi_temper; the caller has validated everything
struct MppiTemper {
  double target, lam_min, lam_max;
  int steps;
  double* lam_out;     // [E]
  uint8_t* saturated;  // [E] or null
};

// ONE launch on `s`: one workgroup of MPPI_LANES lanes per parent.  a == nullptr: every finite sample counts and nothing of the elite
// update's own outputs is touched; else the rank, the elites and the std of mppi_elite_update_launch.
void mppi_tempered_update_launch(const urgym_mppi& m, const MppiTemper& t, const MppiElite* a, hipStream_t s);

}  // namespace urgym
#endif
