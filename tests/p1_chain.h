// The culling pass of the step kernel's per-env phase (ur_gym_amd/csrc/urgym_hip.hip P1) restated for the host harnesses
// (tests/p1_cull_harness.cpp, tests/verdict_harness.cpp): the chain of joint transforms (fk_joint), the world bounding capsules and the
// scene's boxes (TABLE_* / TRACK_*) on the tables of data/ur5e_model.h; the lower bounds themselves are urgym_device.h's, compiled
// with g++.  Test infrastructure only.
#pragma once
#define URGYM_HOST_HARNESS 1
#include <stdint.h>

#include "../data/ur5e_model.h"
#include "../ur_gym_amd/csrc/urgym_device.h"

namespace p1_chain {
using namespace urgym;

constexpr double M_HULL = 0.001;
constexpr double TABLE_CX = 0.5, TABLE_CY = 0.0, TABLE_CZ = -0.58, TABLE_HX = 0.55, TABLE_HY = 0.9, TABLE_HZ = 0.46;
constexpr double TRACK_CX = 0.0, TRACK_CY = 0.0, TRACK_CZ = -0.06, TRACK_HX = 0.1, TRACK_HY = 0.55, TRACK_HZ = 0.06;
constexpr int PAIRS = 19;  // table x links 2..6, track x links 2..6, (1,3)(1,4)(1,5)(1,6)(2,4)(2,5)(2,6)(3,5)(3,6)

inline void fk_joint(X3& T, int k, double s, double c) {
  const double* F = UR5E_JOINT_ROT[k];
  const double* o = UR5E_JOINT_XYZ[k];
  T.t = T.t + rot(T, d3(o[0], o[1], o[2]));
  double g[9], r[9];
  for (int i = 0; i < 3; i++) {
    g[i * 3 + 0] = F[i * 3 + 0] * c + F[i * 3 + 1] * s;
    g[i * 3 + 1] = F[i * 3 + 1] * c - F[i * 3 + 0] * s;
    g[i * 3 + 2] = F[i * 3 + 2];
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r[i * 3 + j] = fma(T.r[i * 3], g[j], fma(T.r[i * 3 + 1], g[3 + j], T.r[i * 3 + 2] * g[6 + j]));
  for (int i = 0; i < 9; i++) T.r[i] = r[i];
}

struct Pair {
  double d2;      // the squared lower bound
  double root;    // the left side of the root form: sqrt(d2) - radii, as the kernel rounds it
  double ra, rb;  // capsule radii (ra: self pairs only)
};

// the 19 pairs of one pose, in the order of the mask's bits
inline void pairs_of_pose(const double q[6], Pair out[PAIRS]) {
  X3 T;
  for (int i = 0; i < 9; i++) T.r[i] = (i % 4 == 0) ? 1.0 : 0.0;
  T.t = d3(0, 0, 0);
  D3 a0[3], a1[3];
  int self = 10;
  for (int k = 0; k < 6; k++) {
    fk_joint(T, k, std::sin(q[k]), std::cos(q[k]));
    const int link = k + 1;
    const double* c = UR5E_CAPSULE[k];
    const D3 b0 = apply(T, d3(c[0], c[1], c[2])), b1 = apply(T, d3(c[3], c[4], c[5]));
    const double rb = c[6];
    if (k < 3) { a0[k] = b0; a1[k] = b1; }
    if (link >= 2) {
      out[link - 2] = Pair{seg_box_lower_bound2(b0, b1, TABLE_CX, TABLE_CY, TABLE_CZ, TABLE_HX, TABLE_HY, TABLE_HZ),
                           seg_box_lower_bound(b0, b1, TABLE_CX, TABLE_CY, TABLE_CZ, TABLE_HX, TABLE_HY, TABLE_HZ) - rb, 0.0, rb};
      out[5 + link - 2] = Pair{seg_box_lower_bound2(b0, b1, TRACK_CX, TRACK_CY, TRACK_CZ, TRACK_HX, TRACK_HY, TRACK_HZ),
                               seg_box_lower_bound(b0, b1, TRACK_CX, TRACK_CY, TRACK_CZ, TRACK_HX, TRACK_HY, TRACK_HZ) - rb, 0.0, rb};
    }
  }
  // self pairs need the capsules of links 1..3 first: a second pass in the mask's order, (1,3)(1,4)(1,5)(1,6)(2,4)(2,5)(2,6)(3,5)(3,6)
  X3 U;
  for (int i = 0; i < 9; i++) U.r[i] = (i % 4 == 0) ? 1.0 : 0.0;
  U.t = d3(0, 0, 0);
  D3 e0[6], e1[6];
  for (int k = 0; k < 6; k++) {
    fk_joint(U, k, std::sin(q[k]), std::cos(q[k]));
    const double* c = UR5E_CAPSULE[k];
    e0[k] = apply(U, d3(c[0], c[1], c[2]));
    e1[k] = apply(U, d3(c[3], c[4], c[5]));
  }
  for (int A = 1; A <= 3; A++)
    for (int link = A + 2; link <= 6; link++) {
      const double ra = UR5E_CAPSULE[A - 1][6], rb = UR5E_CAPSULE[link - 1][6];
      out[self++] = Pair{segseg_dist2(a0[A - 1], a1[A - 1], e0[link - 1], e1[link - 1]),
                         segseg_dist(a0[A - 1], a1[A - 1], e0[link - 1], e1[link - 1]) - ra - rb, ra, rb};
    }
}

// The two forms of the culling predicate on one pair under the margin sum `lim` (collision margin + hull margin + 1e-6, as the
// kernel forms it): root form `sqrt(d2) - radii <= lim`, squared form `d2 <= cull_bound2(lim + radii)`.
inline double reach_of(const Pair& p, bool self, double lim) { return self ? lim + M_HULL + p.ra + p.rb : lim + p.rb; }  // (left to right, as the kernel forms them)
inline bool kept_root(const Pair& p, bool self, double lim) { return p.root <= (self ? lim + M_HULL : lim); }
inline bool kept_squared(const Pair& p, bool self, double lim) { return p.d2 <= cull_bound2(reach_of(p, self, lim)); }
}  // namespace p1_chain
