// Host harness: the culling predicate of the step kernel's per-env phase (ur_gym_amd/csrc/urgym_hip.hip P1; the lower bounds and
// cull_bound2 are urgym_device.h's, compiled here with g++) in its two forms, on a census of poses:
//   root form     sqrt(d2) - radii <= lim           (what every launch ran before DESIGN.md section 4, round 8, and the launches with the
//                                                     penetration-depth phase still run)
//   squared form  d2 <= cull_bound2(lim + radii)    (the step kernels without that phase)
// The chain of joint transforms, the bounding capsules and the scene's boxes are restated from urgym_hip.hip (fk_joint, the culling
// loop, TABLE_* / TRACK_*) on the tables of data/ur5e_model.h.  Test infrastructure only.
#define URGYM_HOST_HARNESS 1
#include <stdint.h>

#include "../data/ur5e_model.h"
#include "../ur_gym_amd/csrc/urgym_device.h"

using namespace urgym;

namespace {
constexpr double M_HULL = 0.001;
constexpr double TABLE_CX = 0.5, TABLE_CY = 0.0, TABLE_CZ = -0.58, TABLE_HX = 0.55, TABLE_HY = 0.9, TABLE_HZ = 0.46;
constexpr double TRACK_CX = 0.0, TRACK_CY = 0.0, TRACK_CZ = -0.06, TRACK_HX = 0.1, TRACK_HY = 0.55, TRACK_HZ = 0.06;
constexpr int PAIRS = 19;  // table x links 2..6, track x links 2..6, (1,3)(1,4)(1,5)(1,6)(2,4)(2,5)(2,6)(3,5)(3,6)

void fk_joint(X3& T, int k, double s, double c) {
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
void pairs_of_pose(const double q[6], Pair out[PAIRS]) {
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

struct Tally {
  long pairs = 0, kept_root = 0, kept_squared = 0, lost = 0, added = 0, added_outside_band = 0;
};

// both forms on one pair under the margin sum `lim` (collision margin + hull margin + 1e-6, as the kernel forms it)
void judge(const Pair& p, bool self, double lim, Tally& t) {
  const bool root = p.root <= (self ? lim + M_HULL : lim);
  const double reach = self ? lim + M_HULL + p.ra + p.rb : lim + p.rb;  // (left to right, as the kernel forms them)
  const bool squared = p.d2 <= cull_bound2(reach);
  t.pairs++;
  t.kept_root += root;
  t.kept_squared += squared;
  if (root && !squared) t.lost++;
  if (squared && !root) {
    t.added++;
    // the slack band: the distance exceeds the reach by no more than CULL_SLACK, relative (long double: the band itself is not rounded)
    const long double d = std::sqrt((long double)p.d2), r = (long double)reach;
    if (!(d <= r * (1.0L + (long double)CULL_SLACK))) t.added_outside_band++;
  }
}

struct Rng {
  uint64_t st;
  double uniform() {
    st = st * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(st >> 11) * (1.0 / 9007199254740992.0);
  }
};
const double LIMIT[6] = {6.283185307179586, 6.283185307179586, 3.141592653589793, 6.283185307179586, 6.283185307179586, 6.283185307179586};
}  // namespace

// mode 0: joints uniform within their limits; 1: every joint at a limit, at zero or at a multiple of pi / 2; 2: a random pose in which
// one joint is bisected to the very pair of neighbouring float64 values between which the root form of one pair changes its verdict
// (the bound equals lim to within the last bits), both neighbours judged under lim and lim moved by -2 .. +2 ulp.
// out = pairs judged, kept by the root form, kept by the squared form, kept by the root form ONLY (must be 0), kept by the squared form
// only, of those outside the slack band (must be 0), poses, bisections that found a change of verdict.
extern "C" int harness_cull_census(int mode, int count, unsigned long long seed, double collision_margin, long* out) {
  Rng rng{seed * 2862933555777941757ULL + 3037000493ULL};
  Tally t;
  long poses = 0, bisected = 0;
  const double lim = collision_margin + M_HULL + 1e-6;
  Pair pr[PAIRS];
  auto judge_pose = [&](const double q[6], double l) {
    pairs_of_pose(q, pr);
    for (int i = 0; i < PAIRS; i++) judge(pr[i], i >= 10, l, t);
    poses++;
  };
  for (int it = 0; it < count; it++) {
    double q[6];
    for (int k = 0; k < 6; k++) {
      if (mode == 1) {
        const int c = (int)(rng.uniform() * 5);
        q[k] = (c == 0) ? -LIMIT[k] : (c == 1) ? LIMIT[k] : (c == 2) ? 0.0 : (1.5707963267948966 * ((int)(rng.uniform() * 9) - 4));
        if (fabs(q[k]) > LIMIT[k]) q[k] = LIMIT[k];
      } else {
        q[k] = (2.0 * rng.uniform() - 1.0) * LIMIT[k];
      }
    }
    if (mode != 2) {
      judge_pose(q, lim);
      continue;
    }
    const int j = (int)(rng.uniform() * 6), p = (int)(rng.uniform() * PAIRS);
    auto verdict = [&](double x) {
      double qq[6];
      for (int k = 0; k < 6; k++) qq[k] = (k == j) ? x : q[k];
      pairs_of_pose(qq, pr);
      return pr[p].root <= (p >= 10 ? lim + M_HULL : lim);
    };
    double lo = q[j], hi = q[j];
    const bool v_lo = verdict(lo);
    bool found = false;
    for (int tries = 0; tries < 24 && !found; tries++) {
      hi = (2.0 * rng.uniform() - 1.0) * LIMIT[j];
      found = verdict(hi) != v_lo;
    }
    if (!found) continue;
    for (int b = 0; b < 200; b++) {
      const double mid = lo + 0.5 * (hi - lo);
      if (mid == lo || mid == hi) break;
      if (verdict(mid) == v_lo) lo = mid; else hi = mid;
    }
    bisected++;
    for (int side = 0; side < 2; side++) {
      double qq[6];
      for (int k = 0; k < 6; k++) qq[k] = (k == j) ? (side ? hi : lo) : q[k];
      double l = lim;
      for (int u = 0; u < 2; u++) l = std::nextafter(l, 0.0);
      for (int u = -2; u <= 2; u++, l = std::nextafter(l, 1.0)) judge_pose(qq, l);
    }
  }
  out[0] = t.pairs; out[1] = t.kept_root; out[2] = t.kept_squared; out[3] = t.lost; out[4] = t.added; out[5] = t.added_outside_band;
  out[6] = poses; out[7] = bisected;
  return 0;
}
