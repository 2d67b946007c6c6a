// urgym_ik.h — the scripted reach controller (include/urgym.h, "a scripted reach controller on the device"): the
// chain walk, the geometric Jacobian, the pose error, the damped least-squares step and the counter of the exploration noise, stated once
// as functions the kernel of urgym_ik.hip and tests/ik_harness.cpp (a host program, built without HIP) both compile; and, for HIP units
// only, the seam between urgym_ik.hip and urgym_mppi_abi.hip.  The execute line and the counter type are urgym_mppi_collect.h's, used as
// they are.  Nothing here is exported.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/urgym.h"
#include "urgym_mppi_collect.h"

namespace urgym {

constexpr uint32_t IK_TAG = URGYM_IK_TAG;  // counter word 3 of the controller's exploration noise is IK_TAG | block
static_assert((IK_TAG & 0xFFu) == 0u && IK_TAG != MPPI_TAG, "a tag of its own, the low byte free for the block");

// The joint origins of the URDF chain: joint k is T <- T * [rot[k] | xyz[k]] * Rz(q_k) (data/ur5e_model.h).  The unit that launches the
// kernel fills one from UR5E_JOINT_XYZ / UR5E_JOINT_ROT and hands it over as a kernel argument: the same numbers in every lane.
struct IkModel {
  double xyz[6][3];
  double rot[6][9];
};

// Every function below is ONE float64 operation per line, rounded on its own: the units that compile this are built with
// -ffp-contract=off.  ur_gym_amd.evaluation.ik_actions restates the arithmetic from the URDF's joint origins; sin, cos, sqrt and atan2
// are the library's of whoever compiles this, so the two agree to rounding, not bit for bit.  Every loop has constant bounds and is
// unrolled in the kernel: no array below is indexed by a run-time value.

URGYM_HD inline bool ik_finite(double x) { return x - x == 0.0; }  // false for a NaN and for either infinity

// ---- the chain walk: for joint k its world axis z[k] and origin o[k]; the end-effector frame (R row-major, p) is that of link 6
struct IkChain {
  double z[6][3], o[6][3];
  double R[9], p[3];
};
URGYM_HD inline void ik_chain(const IkModel& M, const double q[6], IkChain& C) {
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double t[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double* F = M.rot[k];
    const double* x = M.xyz[k];
    double s, c;
    sincos(q[k], &s, &c);
#pragma unroll
    for (int i = 0; i < 3; i++) {  // t <- t + R xyz
      const double a = R[i * 3 + 0] * x[0];
      const double b = R[i * 3 + 1] * x[1];
      const double d = R[i * 3 + 2] * x[2];
      const double ab = a + b;
      const double abd = ab + d;
      t[i] = t[i] + abd;
      C.o[k][i] = t[i];
    }
    double G[9];  // G = R F: its third column is the joint's axis, which Rz(q) leaves alone
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double a = R[i * 3 + 0] * F[0 * 3 + j];
        const double b = R[i * 3 + 1] * F[1 * 3 + j];
        const double d = R[i * 3 + 2] * F[2 * 3 + j];
        const double ab = a + b;
        G[i * 3 + j] = ab + d;
      }
#pragma unroll
    for (int i = 0; i < 3; i++) {  // R <- G Rz(q): columns 0 and 1 mix
      const double g0c = G[i * 3 + 0] * c;
      const double g1s = G[i * 3 + 1] * s;
      const double g1c = G[i * 3 + 1] * c;
      const double g0s = G[i * 3 + 0] * s;
      R[i * 3 + 0] = g0c + g1s;
      R[i * 3 + 1] = g1c - g0s;
      R[i * 3 + 2] = G[i * 3 + 2];
      C.z[k][i] = G[i * 3 + 2];
    }
  }
#pragma unroll
  for (int i = 0; i < 9; i++) C.R[i] = R[i];
#pragma unroll
  for (int i = 0; i < 3; i++) C.p[i] = t[i];
}

// ---- the geometric Jacobian, J[r][k]: rows 0..2 = z_k x (p - o_k), rows 3..5 = z_k; without `rotational` rows 3..5 are zero
URGYM_HD inline void ik_jacobian(const IkChain& C, bool rotational, double J[6][6]) {
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double rx = C.p[0] - C.o[k][0];
    const double ry = C.p[1] - C.o[k][1];
    const double rz = C.p[2] - C.o[k][2];
    const double zx = C.z[k][0], zy = C.z[k][1], zz = C.z[k][2];
    const double yz = zy * rz;
    const double zy_ = zz * ry;
    const double zx_ = zz * rx;
    const double xz = zx * rz;
    const double xy = zx * ry;
    const double yx = zy * rx;
    J[0][k] = yz - zy_;
    J[1][k] = zx_ - xz;
    J[2][k] = xy - yx;
    J[3][k] = rotational ? zx : 0.0;
    J[4][k] = rotational ? zy : 0.0;
    J[5][k] = rotational ? zz : 0.0;
  }
}

// ---- quaternions, xyzw
struct IkQuat {
  double x, y, z, w;
};
// rotation matrix -> quaternion with the largest-diagonal branch (what the end-effector read-out of the step kernels uses)
URGYM_HD inline IkQuat ik_quat_of_rotation(const double r[9]) {
  const double tr01 = r[0] + r[4];
  const double tr = tr01 + r[8];
  IkQuat q;
  if (tr > 0.0) {
    const double u = tr + 1.0;
    const double s = sqrt(u);
    const double h = 0.5 / s;
    const double a = r[7] - r[5];
    const double b = r[2] - r[6];
    const double c = r[3] - r[1];
    q.w = 0.5 * s;
    q.x = a * h;
    q.y = b * h;
    q.z = c * h;
  } else if (r[0] >= r[4] && r[0] >= r[8]) {
    const double u0 = r[0] - r[4];
    const double u1 = u0 - r[8];
    const double u = u1 + 1.0;
    const double s = sqrt(u);
    const double h = 0.5 / s;
    const double a = r[7] - r[5];
    const double b = r[3] + r[1];
    const double c = r[6] + r[2];
    q.x = 0.5 * s;
    q.w = a * h;
    q.y = b * h;
    q.z = c * h;
  } else if (r[4] >= r[8]) {
    const double u0 = r[4] - r[8];
    const double u1 = u0 - r[0];
    const double u = u1 + 1.0;
    const double s = sqrt(u);
    const double h = 0.5 / s;
    const double a = r[2] - r[6];
    const double b = r[7] + r[5];
    const double c = r[1] + r[3];
    q.y = 0.5 * s;
    q.w = a * h;
    q.z = b * h;
    q.x = c * h;
  } else {
    const double u0 = r[8] - r[0];
    const double u1 = u0 - r[4];
    const double u = u1 + 1.0;
    const double s = sqrt(u);
    const double h = 0.5 / s;
    const double a = r[3] - r[1];
    const double b = r[2] + r[6];
    const double c = r[5] + r[7];
    q.z = 0.5 * s;
    q.w = a * h;
    q.x = b * h;
    q.y = c * h;
  }
  return q;
}
// pybullet's getQuaternionFromEuler: q = qz(yaw) qy(pitch) qx(roll)
URGYM_HD inline IkQuat ik_quat_from_rpy(double roll, double pitch, double yaw) {
  const double hr = 0.5 * roll;
  const double hp = 0.5 * pitch;
  const double hy = 0.5 * yaw;
  double sr, cr, sp, cp, sy, cy;
  sincos(hr, &sr, &cr);
  sincos(hp, &sp, &cp);
  sincos(hy, &sy, &cy);
  const double srcp = sr * cp;
  const double crsp = cr * sp;
  const double crcp = cr * cp;
  const double srsp = sr * sp;
  const double x0 = srcp * cy;
  const double x1 = crsp * sy;
  const double y0 = crsp * cy;
  const double y1 = srcp * sy;
  const double z0 = crcp * sy;
  const double z1 = srsp * cy;
  const double w0 = crcp * cy;
  const double w1 = srsp * sy;
  return IkQuat{x0 - x1, y0 + y1, z0 - z1, w0 + w1};
}
// a (x) conj(b)
URGYM_HD inline IkQuat ik_quat_mul_conj(const IkQuat& a, const IkQuat& b) {
  const double bx = -b.x, by = -b.y, bz = -b.z, bw = b.w;
  const double x0 = a.w * bx;
  const double x1 = a.x * bw;
  const double x2 = a.y * bz;
  const double x3 = a.z * by;
  const double x01 = x0 + x1;
  const double x012 = x01 + x2;
  const double y0 = a.w * by;
  const double y1 = a.y * bw;
  const double y2 = a.z * bx;
  const double y3 = a.x * bz;
  const double y01 = y0 + y1;
  const double y012 = y01 + y2;
  const double z0 = a.w * bz;
  const double z1 = a.z * bw;
  const double z2 = a.x * by;
  const double z3 = a.y * bx;
  const double z01 = z0 + z1;
  const double z012 = z01 + z2;
  const double w0 = a.w * bw;
  const double w1 = a.x * bx;
  const double w2 = a.y * by;
  const double w3 = a.z * bz;
  const double w01 = w0 - w1;
  const double w012 = w01 - w2;
  return IkQuat{x012 - x3, y012 - y3, z012 - z3, w012 - w3};
}

// ---- the error: e[0:3] = goal - p; e[3:6] = the rotation vector of d = q_goal (x) conj(q_ee), shortest arc; zero without `rotational`
constexpr double IK_SMALL_ANGLE = 1e-12;  // |d.xyz| below which e_rot = 2 d.xyz
URGYM_HD inline void ik_error(const IkChain& C, const double goal[6], bool rotational, double e[6]) {
#pragma unroll
  for (int i = 0; i < 3; i++) e[i] = goal[i] - C.p[i];
  e[3] = e[4] = e[5] = 0.0;
  if (!rotational) return;
  const IkQuat qe = ik_quat_of_rotation(C.R);
  const IkQuat qg = ik_quat_from_rpy(goal[3], goal[4], goal[5]);
  IkQuat d = ik_quat_mul_conj(qg, qe);
  if (d.w < 0.0) d = IkQuat{-d.x, -d.y, -d.z, -d.w};
  const double xx = d.x * d.x;
  const double yy = d.y * d.y;
  const double zz = d.z * d.z;
  const double xy = xx + yy;
  const double nn = xy + zz;
  const double n = sqrt(nn);
  const double half = atan2(n, d.w);
  const double ang = 2.0 * half;
  const double scale = n < IK_SMALL_ANGLE ? 2.0 : ang / n;
  e[3] = d.x * scale;
  e[4] = d.y * scale;
  e[5] = d.z * scale;
}

// ---- A = J J^T + damping^2 I, its lower triangle: A[i][j] at i (i + 1) / 2 + j for j <= i
URGYM_HD constexpr int ik_tri(int i, int j) { return i * (i + 1) / 2 + j; }
URGYM_HD inline void ik_normal_matrix(const double J[6][6], double damping, double A[21]) {
  const double dd = damping * damping;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double s = J[i][0] * J[j][0];
#pragma unroll
      for (int k = 1; k < 6; k++) {
        const double t = J[i][k] * J[j][k];
        s = s + t;
      }
      A[ik_tri(i, j)] = i == j ? s + dd : s;
    }
}

// ---- A y = e by Cholesky, A = L L^T in place (row by row), then L w = e and L^T y = w.  A is symmetric positive definite by
// construction (damping > 0), so no pivot is looked for and every square root has a positive argument.
URGYM_HD inline void ik_cholesky_solve(double A[21], const double e[6], double y[6]) {
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double s = A[ik_tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) {
        const double t = A[ik_tri(i, k)] * A[ik_tri(j, k)];
        s = s - t;
      }
      A[ik_tri(i, j)] = i == j ? sqrt(s) : s / A[ik_tri(j, j)];
    }
  double w[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = e[i];
#pragma unroll
    for (int k = 0; k < i; k++) {
      const double t = A[ik_tri(i, k)] * w[k];
      s = s - t;
    }
    w[i] = s / A[ik_tri(i, i)];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double s = w[i];
#pragma unroll
    for (int k = 5; k > i; k--) {
      const double t = A[ik_tri(k, i)] * y[k];
      s = s - t;
    }
    y[i] = s / A[ik_tri(i, i)];
  }
}

// ---- the step: dq = gain J^T y; a = dq / action_scale; scaled down as a whole where its largest component exceeds 1; one rounding to
// float32.  Returns false where a component is not finite (the caller writes zeros then).
URGYM_HD inline bool ik_step(const double J[6][6], const double y[6], double gain, double action_scale, float out[6]) {
  double a[6];
  double m = 0.0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double s = J[0][k] * y[0];
#pragma unroll
    for (int r = 1; r < 6; r++) {
      const double t = J[r][k] * y[r];
      s = s + t;
    }
    const double dq = gain * s;
    a[k] = dq / action_scale;
    ok = ok && ik_finite(a[k]);
    m = fmax(m, fabs(a[k]));
  }
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double v = m > 1.0 ? a[k] / m : a[k];
    out[k] = (float)v;
  }
  return ok;
}

// ---- one env: q [6], goal [6] (rows 3..5 read with `rotational` only) -> six float32.  A row whose q or goal holds a value that is
// not finite, or whose step does not stay finite, gets six +0.0f.
URGYM_HD inline void ik_action(const IkModel& M, const double q[6], const double goal[6], bool rotational, double damping, double gain,
                               double action_scale, float out[6]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; i++) ok = ok && ik_finite(q[i]) && (i >= 3 && !rotational ? true : ik_finite(goal[i]));
  if (ok) {
    IkChain C;
    ik_chain(M, q, C);
    double J[6][6], e[6], A[21], y[6];
    ik_jacobian(C, rotational, J);
    ik_error(C, goal, rotational, e);
    ik_normal_matrix(J, damping, A);
    ik_cholesky_solve(A, e, y);
    ok = ik_step(J, y, gain, action_scale, out);
  }
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 6; k++) out[k] = 0.0f;
  }
}

// ---- Box-Muller on one pair of 24-bit integers (m1, m2 = w >> 8 of two Philox words), the sample launch's pairing: u1 = (m1 + 1) 2^-24
// in (0, 1], the angle 2 pi u2 with u2 = m2 2^-24 in [0, 1); r = sqrt(-2 ln u1); the pair is (r cos, r sin).  Unlike the sample launch,
// ln, cos and sin are NOT the device library's: they are stated here in float64, one operation per line -- frexp, rint, sqrt and the four
// basic operations are exact or correctly rounded wherever this compiles -- so that a host restates the noise bit for bit
// (evaluation.ik_explore_noise), as urgym_mppi_temper.h states its exponential.  Each is good to about 1e-13, far below the one rounding
// to float32 at the end.
// ln(M 2^-24) for an integer M in [1, 2^24]: M = f 2^e with f in [sqrt(1/2), sqrt(2)); ln f = 2 atanh(s), s = (f - 1) / (f + 1),
// |s| <= 0.172, by its series up to s^13 (the next term is below 3e-13)
URGYM_HD inline double ik_ln_unit(double M) {
  int e;
  double f = frexp(M, &e);
  if (f < 0.7071067811865476) {
    f = f * 2.0;
    e = e - 1;
  }
  const double num = f - 1.0;
  const double den = f + 1.0;
  const double s = num / den;
  const double z = s * s;
  double p = 1.0 / 13.0;
  p = p * z;
  p = p + 1.0 / 11.0;
  p = p * z;
  p = p + 1.0 / 9.0;
  p = p * z;
  p = p + 1.0 / 7.0;
  p = p * z;
  p = p + 1.0 / 5.0;
  p = p * z;
  p = p + 1.0 / 3.0;
  p = p * z;
  p = p + 1.0;
  const double t = s * p;
  const double l = 2.0 * t;
  const double k = (double)(e - 24);
  const double kl = k * 0.6931471805599453;
  return kl + l;
}
// cos and sin of pi t for t = m2 2^-23 in [0, 2): t = k / 2 + r with k = rint(2 t) and |r| <= 1/4 (exact), x = pi r, the Taylor
// polynomials of sin up to x^13 and of cos up to x^14 (|x| <= 0.786: the next terms are below 3e-14), then the quadrant k & 3
URGYM_HD inline void ik_sincospi(double t, double& sn, double& cs) {
  const double t2 = t * 2.0;
  const double k = rint(t2);
  const double half = k * 0.5;
  const double r = t - half;
  const double x = 3.141592653589793 * r;
  const double z = x * x;
  double ps = 1.0 / 6227020800.0;
  ps = ps * z;
  ps = ps + -1.0 / 39916800.0;
  ps = ps * z;
  ps = ps + 1.0 / 362880.0;
  ps = ps * z;
  ps = ps + -1.0 / 5040.0;
  ps = ps * z;
  ps = ps + 1.0 / 120.0;
  ps = ps * z;
  ps = ps + -1.0 / 6.0;
  ps = ps * z;
  ps = ps + 1.0;
  const double s = x * ps;
  double pc = -1.0 / 87178291200.0;
  pc = pc * z;
  pc = pc + 1.0 / 479001600.0;
  pc = pc * z;
  pc = pc + -1.0 / 3628800.0;
  pc = pc * z;
  pc = pc + 1.0 / 40320.0;
  pc = pc * z;
  pc = pc + -1.0 / 720.0;
  pc = pc * z;
  pc = pc + 1.0 / 24.0;
  pc = pc * z;
  pc = pc + -1.0 / 2.0;
  pc = pc * z;
  const double c = pc + 1.0;
  const int q = (int)k & 3;
  sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
  cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}
URGYM_HD inline void ik_box_muller(uint32_t m1, uint32_t m2, float& first, float& second) {
  const double M = (double)m1 + 1.0;
  const double ln = ik_ln_unit(M);
  const double a = -2.0 * ln;
  const double r = sqrt(a);
  const double t = (double)m2 * (1.0 / 8388608.0);  // the angle / pi = 2 u2: exact
  double sn, cs;
  ik_sincospi(t, sn, cs);
  const double x = r * cs;
  const double y = r * sn;
  first = (float)x;
  second = (float)y;
}

// ---- the exploration counter of (env n, draw) and block 0 / 1; the key is the controller's, (seed lo, seed hi).  Words w0 .. w3 of
// the six come from block 0, w4 and w5 from block 1: the sample launch's order (urgym_mppi.hip).
URGYM_HD inline MppiCounter ik_explore_counter(int n, uint64_t draw, uint32_t block) {
  return MppiCounter{(uint32_t)n, 0u, (uint32_t)draw, IK_TAG | block};
}

}  // namespace urgym

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace urgym {

// what the action launch reads and writes; the caller has validated everything
struct IkLaunch {
  int N;
  int rotational;  // the env kind's goal has six floats
  double damping, gain, action_scale;
  float explore_sigma;
  uint64_t seed, draw;
  const double *q, *goal;  // [6][N] each, the handle's bound state
  float* actions;          // [N][6]: inside a collection, the action rows of the ring slot
  float* explore_eps;      // [N][6] or null
  IkModel model;
};

// the joint origins of data/ur5e_model.h
void ik_model_fill(IkModel& m);
// ONE launch on `s`, one lane per env
void ik_actions_launch(const IkLaunch& x, hipStream_t s);

}  // namespace urgym
#endif
