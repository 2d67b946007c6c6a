// Host harness: the culling predicate of the step kernel's per-env phase (ur_gym_amd/csrc/urgym_hip.hip P1; the lower bounds and
// cull_bound2 are urgym_device.h's, compiled here with g++) in its two forms, on a census of poses:
//   root form     sqrt(d2) - radii <= lim           (what every launch ran before DESIGN.md section 4, round 8, and the launches with the
//                                                     penetration-depth phase still run)
//   squared form  d2 <= cull_bound2(lim + radii)    (the step kernels without that phase)
// The chain of joint transforms, the bounding capsules and the scene's boxes are restated from urgym_hip.hip (fk_joint, the culling
// loop, TABLE_* / TRACK_*) on the tables of data/ur5e_model.h in tests/p1_chain.h, which tests/verdict_harness.cpp shares.  Test
// infrastructure only.
#include "p1_chain.h"

using namespace urgym;
using namespace p1_chain;

namespace {
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
