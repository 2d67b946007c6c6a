// Host harness of the collision-verdict tests (tests/test_verdicts_host.py, tests/golden/gen_verdict_poses.py): what the culling pass
// of the step kernel's per-env phase (ur_gym_amd/csrc/urgym_hip.hip P1) decides with, handed out piece by piece so that each piece can
// be held against the certified brackets of tests/separation_cases.py:
//   the capsule table of data/ur5e_model.h as compiled; the two lower bounds of urgym_device.h on operands of the caller's own; and
//   the 19 pairs of one pose -- squared bound, root-form left side, reach, and the two forms of the predicate as bit masks.
// The chain of joint transforms is the one tests/p1_cull_harness.cpp restates (tests/p1_chain.h).  Test infrastructure only.
#include "p1_chain.h"

using namespace urgym;
using namespace p1_chain;

// out[6][7]: p0.xyz, p1.xyz, radius of links 1..6 (link frame)
extern "C" void harness_capsule_table(double* out) {
  for (int k = 0; k < 6; k++)
    for (int i = 0; i < 7; i++) out[k * 7 + i] = UR5E_CAPSULE[k][i];
}

// seg[n][6] = p.xyz, q.xyz; box[n][6] = centre.xyz, half.xyz; out[n] = seg_box_lower_bound2
extern "C" void harness_seg_box_lower_bound2(int n, const double* seg, const double* box, double* out) {
  for (int i = 0; i < n; i++) {
    const double *s = seg + 6 * i, *b = box + 6 * i;
    out[i] = seg_box_lower_bound2(d3(s[0], s[1], s[2]), d3(s[3], s[4], s[5]), b[0], b[1], b[2], b[3], b[4], b[5]);
  }
}

// a[n][6] = p1.xyz, q1.xyz; b[n][6] = p2.xyz, q2.xyz; out[n] = segseg_dist2
extern "C" void harness_segseg_dist2(int n, const double* a, const double* b, double* out) {
  for (int i = 0; i < n; i++) {
    const double *s = a + 6 * i, *t = b + 6 * i;
    out[i] = segseg_dist2(d3(s[0], s[1], s[2]), d3(s[3], s[4], s[5]), d3(t[0], t[1], t[2]), d3(t[3], t[4], t[5]));
  }
}

// q[n][6] at one collision margin: masks[n][2] = the pairs kept by the root form and by the squared form (bit i = pair i of the
// kernel's mask: table x links 2..6, track x links 2..6, the nine self pairs); bound[n][19] = the capsules' lower bound of the
// distance between the margin-inflated shapes, sqrt(d2) - radii - hull margins (one for a box pair, two for a self pair).
extern "C" void harness_cull_masks(int n, const double* q, double collision_margin, uint32_t* masks, double* bound) {
  const double lim = collision_margin + M_HULL + 1e-6;
  Pair pr[PAIRS];
  for (int e = 0; e < n; e++) {
    pairs_of_pose(q + 6 * e, pr);
    uint32_t root = 0, squared = 0;
    for (int i = 0; i < PAIRS; i++) {
      const bool self = i >= 10;
      if (kept_root(pr[i], self, lim)) root |= 1u << i;
      if (kept_squared(pr[i], self, lim)) squared |= 1u << i;
      bound[e * PAIRS + i] = std::sqrt(pr[i].d2) - pr[i].ra - pr[i].rb - (self ? 2.0 * M_HULL : M_HULL);
    }
    masks[2 * e] = root;
    masks[2 * e + 1] = squared;
  }
}
