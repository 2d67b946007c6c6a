// Host harness for tests/test_trip_exits_host.py: one GJK iteration of ur_gym_amd/csrc/urgym_device.h (gjk_advance: flat termination
// tail, branch-free plane tests, one region for the simplex step), compiled with g++ and run on the CPU, trip by trip, next to the
// iteration AS IT WAS BRANCHED before that change: ref_advance below restates the earlier control flow -- the five-deep `else if`
// tail, the two-armed plane test, the two `if (fin == 0)` nests -- on the same float64 expressions, and says which exit it took.
// Test infrastructure only.
#include <string.h>

#include "device_harness.cpp"  // URGYM_HOST_HARNESS, the device header, the host tables; pose_to_x3(), desc()

namespace {

enum Arm { ARM_NONE = 0, ARM_SEPARATING_AXIS, ARM_DUPLICATE, ARM_F0_F1, ARM_SLIVER, ARM_TOUCHING, ARM_VERDICT, ARM_NO_PROGRESS, ARM_CAP, ARM_INSIDE };

// gjk_advance before the change (the same float64 expressions in the same order; the control flow as it was)
int ref_advance(GjkRun& r, const HullMap& g, const ShapeDesc& A, XRef T, const ShapeDesc& B, double max_d, double verdict_d, int& arm) {
  const double REL_ERROR2 = 1.0e-12;
  const double EPS = 2.220446049250313e-16;
  const D3 W0 = ldw(T, 0), W1 = ldw(T, 1), W2 = ldw(T, 2);
  D3 w;
  {
    X3 TX;
    for (int k = 0; k < 9; k++) TX.r[k] = T.at(k);
    TX.t = d3(T.at(9), T.at(10), T.at(11));
    const D3 dA = rotT(TX, -r.v);
    const D3 q = support_local(g, B, r.v);
    const D3 sA = support_local(g, A, dA);
    const D3 p = apply(TX, sA);
    w = p - q;
  }
  arm = ARM_NONE;
  int fin = 0;
  const double delta = dot(r.v, w);
  if (delta > 0.0 && delta * delta > r.sq * (max_d * max_d)) { fin = 1 | 4; arm = ARM_SEPARATING_AXIS; }
  if (fin == 0) {
    const bool in = (r.n > 0 && len2(W0 - w) <= 1e-12) || (r.n > 1 && len2(W1 - w) <= 1e-12) || (r.n > 2 && len2(W2 - w) <= 1e-12);
    const double f0 = r.sq - delta, f1 = r.sq * REL_ERROR2;
    if (in) { fin = 1; arm = ARM_DUPLICATE; }
    else if (f0 <= f1) { fin = 1; arm = ARM_F0_F1; }
  }
  if (fin == 0) {
    stw(T, r.n, w);
    int n = r.n + 1;
    D3 nv = d3(0, 0, 0);
    bool valid = true;
    int used = 15;
    bool reduce = true;
    if (n == 1) {
      nv = w;
      reduce = false;
    } else if (n == 2) {
      D3 s0 = W0;
      D3 e = w - s0;
      double t = -dot(e, s0);
      used = 3;
      if (t > 0.0) {
        double ee = dot(e, e);
        if (t < ee) t /= ee;
        else { t = 1.0; used = 2; }
      } else {
        t = 0.0;
        used = 1;
      }
      nv = s0 + e * t;
    } else {
      const bool tetra = (n == 4);
      auto face_vertices = [](int f, int& ia, int& ib, int& ic, int& io) {
        ia = (f == 3) ? 1 : 0;
        ib = (f == 0) ? 1 : ((f == 1) ? 2 : 3);
        ic = (f == 0) ? 2 : ((f == 1) ? 3 : ((f == 2) ? 1 : 2));
        io = (f == 0) ? 3 : ((f == 1) ? 1 : ((f == 2) ? 2 : 0));
      };
      int todo = 1;
      bool degen = false;
      if (tetra) {
        todo = 0;
        auto plane = [&](D3 a, D3 b, D3 c, D3 o, int bit) {
          const D3 nrm = cross(b - a, c - a);
          const double signp = -dot(a, nrm), signd = dot(o - a, nrm);
          if (signd * signd < (1.0e-8 * 1.0e-8)) degen = true;
          else if (signp * signd < 0.0) todo |= bit;
        };
        plane(W0, W1, W2, w, 1);
        plane(W0, W2, w, W1, 2);
        plane(W0, w, W1, W2, 4);
        plane(W1, w, W2, W0, 8);
      }
      double best = 1.0e300;
      used = -1;
      while (todo) {
        const int f = __builtin_ctz((unsigned)todo);
        todo &= todo - 1;
        int ia, ib, ic, io;
        face_vertices(f, ia, ib, ic, io);
        const D3 a = ldw(T, ia), b = ldw(T, ib), c = ldw(T, ic);
        int m3;
        const D3 pt = tri_closest(a, b, c, m3);
        const double l = len2(pt);
        if (used < 0 || l < best) {
          best = l;
          nv = pt;
          used = ((m3 & 1) ? (1 << ia) : 0) | ((m3 & 2) ? (1 << ib) : 0) | ((m3 & 4) ? (1 << ic) : 0);
        }
      }
      if (degen) {
        valid = false;
        reduce = false;
      } else if (used < 0) {
        nv = d3(0, 0, 0);
        reduce = false;
      }
    }
    if (reduce) {
      if (n >= 4 && !(used & 8)) { n--; }
      if (n >= 3 && !(used & 4)) { n--; stw(T, 2, ldw(T, n)); }
      if (n >= 2 && !(used & 2)) { n--; stw(T, 1, ldw(T, n)); }
      if (n >= 1 && !(used & 1)) { n--; stw(T, 0, ldw(T, n)); }
    }
    r.n = n;
    if (!valid) { fin = 1; arm = ARM_SLIVER; }
    else {
      const double nsq = len2(nv);
      if (nsq < REL_ERROR2) { r.v = nv; fin = 1; arm = ARM_TOUCHING; }
      else if (nsq <= verdict_d * verdict_d) { r.v = nv; r.info |= GJK_CLOSE; fin = 1; arm = ARM_VERDICT; }
      else {
        const double prev = r.sq;
        r.sq = nsq;
        if (prev - nsq <= EPS * prev) { fin = 1; arm = ARM_NO_PROGRESS; }
        else {
          r.v = nv;
          if (r.iter++ > 1000) { r.info |= GJK_ITERCAP; fin = 3; arm = ARM_CAP; }
          else if (n == 4) { fin = 3; arm = ARM_INSIDE; }
        }
      }
    }
  }
  return fin;
}

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
int run_differences(const GjkRun& a, const GjkRun& b, const double* sa, const double* sb) {
  int bad = 0;
  bad += !same_bits(a.v.x, b.v.x) + !same_bits(a.v.y, b.v.y) + !same_bits(a.v.z, b.v.z) + !same_bits(a.sq, b.sq);
  bad += (a.n != b.n) + (a.iter != b.iter) + (a.info != b.info) + (a.done != b.done) + !same_bits(a.core, b.core);
  for (int k = 0; k < 3 * a.n && k < 12; k++) bad += !same_bits(sa[12 + k], sb[12 + k]);  // the simplex vertices the run holds
  return bad;
}

}  // namespace

// One query, the iteration under test and the earlier form in lockstep from the same start: Bullet's axis, the run as gjk_begin leaves
// it -- or with the run's iteration counter preset (iter0 > 0), which is how the cap is reached without a thousand trips, or its
// squared distance preset (sq0 > 0), which is how the no-progress exit is reached on demand: a first closest point farther away
// than sq0 says is "no progress".  After EVERY trip the exit code and the whole
// run -- v, sq, n, iter, info and the simplex vertices -- are compared bit for bit; after the last, gjk_finish's core distance and
// flags, and once more against gjk_core_distance (gjk_iterate = gjk_advance + gjk_finish) when nothing is preset.
// out[0] mismatches, [1] exit code fin, [2] info after the finish, [3] r.n, [4] r.iter, [5] core distance, [6..8] r.v, [9] the exit
// the earlier form took (Arm), [10] trips, [11] margin sum
extern "C" int harness_trip_exits(int type_a, const double* par_a, const double* pose_a, int type_b, const double* par_b, const double* pose_b,
                                  double max_core_d, double verdict_d, int iter0, double sq0, double* out) {
  const HostTables& tabs = build_host_tables();
  if (!tabs.ok) return -1;
  HullMap g{tabs.recs.data(), tabs.cell.data()};
  double ma, mb;
  const ShapeDesc A = desc(type_a, par_a, &ma), B = desc(type_b, par_b, &mb);
  const X3 Ta = pose_to_x3(pose_a), Tb = pose_to_x3(pose_b);
  double slot_new[GJK_SLOT_DOUBLES] = {0}, slot_ref[GJK_SLOT_DOUBLES] = {0};
  const XRef Tn{slot_new, 1}, Tr{slot_ref, 1};
  store(Tn, rel(Tb, Ta));
  store(Tr, rel(Tb, Ta));
  const D3 v0 = rotT(Tb, d3(0, 1, 0));
  GjkRun rn, rr;
  gjk_begin(rn, v0);
  gjk_begin(rr, v0);
  rn.iter = rr.iter = iter0;
  if (sq0 > 0.0) rn.sq = rr.sq = sq0;
  long bad = 0;
  int trips = 0, fin = 0, arm = ARM_NONE;
  while (fin == 0 && trips < 1200) {
    const int fn = gjk_advance(rn, g, A, Tn, B, max_core_d, verdict_d);
    fin = ref_advance(rr, g, A, Tr, B, max_core_d, verdict_d, arm);
    trips++;
    bad += (fn != fin) + run_differences(rn, rr, slot_new, slot_ref);
    if (fn != fin) break;
  }
  gjk_finish(rn, !(fin & 2), (fin & 4) != 0);
  gjk_finish(rr, !(fin & 2), (fin & 4) != 0);
  bad += run_differences(rn, rr, slot_new, slot_ref);
  if (iter0 == 0 && !(sq0 > 0.0)) {
    double slot[GJK_SLOT_DOUBLES] = {0};
    const XRef Tc{slot, 1};
    store(Tc, rel(Tb, Ta));
    int info;
    const double core = gjk_core_distance(g, A, Tc, B, v0, max_core_d, info, verdict_d);
    bad += !same_bits(core, rr.core) + (info != rr.info);
  }
  out[0] = (double)bad; out[1] = fin; out[2] = rr.info; out[3] = rr.n; out[4] = rr.iter; out[5] = rr.core;
  out[6] = rr.v.x; out[7] = rr.v.y; out[8] = rr.v.z; out[9] = arm; out[10] = trips; out[11] = ma + mb;
  return 0;
}
