// Batched LocalizeViewToReconstruction, calibrated path (localize_view_to_reconstruction.cc:185-198): RANSAC over P3P
// for many candidate views at once, on the chunked evaluate-then-replay scaffold of ransac_core.h (the loop itself is
// the host's, side_calls.h).  What is this call's own: one preparation launch, the problem the scaffold's three
// per-chunk kernels are instantiated with, one final launch:
//
//   localize_prepare_kernel     one thread per correspondence: the normalised feature
//                               (PixelToNormalizedCoordinates(pixel).hnormalized(), pixel_to_camera) and the world
//                               point (point.hnormalized()), structure of arrays in view-major order
//   LocalizeProblem             a sample of three, PoseFromThreePoints (perspective_three_point.cc) and position =
//                               -R^T t: four poses or none; one wavefront scores all four poses of an iteration per load
//                               of a correspondence; the squared reprojection error against the threshold
//   localize_final_kernel       one wavefront per selected view: the best model's inlier mask and count (:332-341),
//                               the status, and the pose into the extrinsics of a localised view
//
// The arithmetic of the hypothesis, scoring and final kernels is never contracted into FMA (#pragma clang fp
// contract(off) in every body) and uses only + - * / and sqrt, which round correctly: a CPU model that evaluates the
// same expressions in the same order sees the same roundings, hence the same costs.  The one exception is the
// preparation launch: pixel_to_camera is shared with the other calls and compiled as they compile it.
#pragma once
#include <hip/hip_runtime.h>

#include "ransac_core.h"
#include "rotation_kernels.h"
#include "track_estimate_kernels.h"
#include "vec3.h"

namespace tmi {

constexpr int kQuarticBisections = 200;  // of the resolvent cubic; stops early at neighbouring doubles

// The correspondence planes of RansacBatch: the normalised feature, then the world point.
enum { kLocFx, kLocFy, kLocWx, kLocWy, kLocWz };

__global__ __launch_bounds__(256) void localize_prepare_kernel(long long M, const unsigned long long* __restrict__ keys,
                                                               const int* __restrict__ slot_pt,
                                                               const double* __restrict__ obs_xy,
                                                               const double* __restrict__ pts,
                                                               const int4* __restrict__ cam,
                                                               const double* __restrict__ intr, RansacBatch B) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= M) return;
  const int c = (int)(keys[o] >> 32);
  const int4 rec = cam[c];
  double K[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) K[j] = j < rec.z ? intr[rec.y + j] : 0.0;
  const double px[2] = {obs_xy[2 * o], obs_xy[2 * o + 1]};
  double u[3];
  pixel_to_camera(rec.x, K, px, u);
  const double* X = pts + 4 * (long long)slot_pt[o];
  B.plane[kLocFx][o] = u[0];
  B.plane[kLocFy][o] = u[1];
  B.plane[kLocWx][o] = X[0] / X[3];
  B.plane[kLocWy][o] = X[1] / X[3];
  B.plane[kLocWz][o] = X[2] / X[3];
}

// rows: tx = f0, tz = (f0 x f1) normalised, ty = tz x tx
__device__ __forceinline__ void p3p_frame(const double f0[3], const double f1[3], double T[9]) {
#pragma clang fp contract(off)
  T[0] = f0[0];
  T[1] = f0[1];
  T[2] = f0[2];
  cross3(f0, f1, T + 6);
  normalize3(T + 6);
  cross3(T + 6, T, T + 3);
}
__device__ __forceinline__ void matvec3(const double T[9], const double a[3], double r[3]) {
#pragma clang fp contract(off)
  r[0] = dot3(T, a);
  r[1] = dot3(T + 3, a);
  r[2] = dot3(T + 6, a);
}

// The real parts of the four roots of x^4 + B x^3 + C x^2 + D x + E in ascending order: Ferrari's factorisation into two
// quadratics through a positive root of the resolvent cubic (found by bisection, so with + - * only), two Newton steps
// on every real root, an insertion sort.
__device__ __forceinline__ void quartic_real_parts(double B, double C, double D, double E, double x[4]) {
#pragma clang fp contract(off)
  const double B2 = B * B;
  const double p = C - 0.375 * B2;
  const double q = (D - 0.5 * (B * C)) + 0.125 * (B2 * B);
  const double r = ((E - 0.25 * (B * D)) + 0.0625 * (B2 * C)) - 0.01171875 * (B2 * B2);
  // y^4 + p y^2 + q y + r = (y^2 + s1 y + m1) (y^2 + s2 y + m2)
  double s1, s2, m1, m2;
  double z = -1.0;
  const double c2 = 2.0 * p, c1 = p * p - 4.0 * r, c0 = q * q;
  if (q == 0.0) {
    if (r >= 0.0) z = 2.0 * sqrt(r) - p;
  } else {
    double hi = fabs(c2) > fabs(c1) ? fabs(c2) : fabs(c1);
    hi = (hi > c0 ? hi : c0) + 1.0;
    double lo = 0.0;
    for (int it = 0; it < kQuarticBisections; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (!(mid > lo) || !(mid < hi)) break;
      const double g = ((mid + c2) * mid + c1) * mid - c0;
      if (g > 0.0) hi = mid; else lo = mid;
    }
    z = hi;
  }
  if (z > 0.0) {
    const double s = sqrt(z);
    const double half = 0.5 * (p + z), qs = (0.5 * q) / s;
    s1 = s;
    s2 = -s;
    m1 = half - qs;
    m2 = half + qs;
  } else {  // q == 0 without a positive root of the resolvent: a biquadratic with real factors y^2 + m
    const double disc = sqrt(c1);
    s1 = 0.0;
    s2 = 0.0;
    m1 = 0.5 * (p - disc);
    m2 = 0.5 * (p + disc);
  }
  const double shift = 0.25 * B;
  bool real[4];
  {
    const double d1 = s1 * s1 - 4.0 * m1;
    if (d1 >= 0.0) {
      const double sq = sqrt(d1);
      x[0] = 0.5 * (-s1 - sq) - shift;
      x[1] = 0.5 * (-s1 + sq) - shift;
      real[0] = real[1] = true;
    } else {
      x[0] = x[1] = -0.5 * s1 - shift;
      real[0] = real[1] = false;
    }
    const double d2 = s2 * s2 - 4.0 * m2;
    if (d2 >= 0.0) {
      const double sq = sqrt(d2);
      x[2] = 0.5 * (-s2 - sq) - shift;
      x[3] = 0.5 * (-s2 + sq) - shift;
      real[2] = real[3] = true;
    } else {
      x[2] = x[3] = -0.5 * s2 - shift;
      real[2] = real[3] = false;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!real[k]) continue;
    double v = x[k];
    for (int it = 0; it < 2; ++it) {
      const double f = (((v + B) * v + C) * v + D) * v + E;
      const double df = ((4.0 * v + 3.0 * B) * v + 2.0 * C) * v + D;
      const double step = f / df;
      if (df != 0.0 && step == step && fabs(step) < 1.0e300) v = v - step;
    }
    x[k] = v;
  }
  // insertion sort, as a fixed network of compare-exchanges in insertion order (a NaN never moves)
#define TMI_LOC_CSWAP(a, b) { if (x[a] > x[b]) { const double t_ = x[a]; x[a] = x[b]; x[b] = t_; } }
  TMI_LOC_CSWAP(0, 1)
  TMI_LOC_CSWAP(1, 2)
  TMI_LOC_CSWAP(0, 1)
  TMI_LOC_CSWAP(2, 3)
  TMI_LOC_CSWAP(1, 2)
  TMI_LOC_CSWAP(0, 1)
#undef TMI_LOC_CSWAP
}

// PoseFromThreePoints and position = -R^T t: poses [4][12] (R row-major, position).  false: no model.
__device__ bool p3p_poses(const double feat[3][2], const double Xw[3][3], double* poses) {
#pragma clang fp contract(off)
  double f[3][3], X[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double n = sqrt((feat[i][0] * feat[i][0] + feat[i][1] * feat[i][1]) + 1.0);
    f[i][0] = feat[i][0] / n;
    f[i][1] = feat[i][1] / n;
    f[i][2] = 1.0 / n;
#pragma unroll
    for (int a = 0; a < 3; ++a) X[i][a] = Xw[i][a];
  }
  double w10[3], w20[3], cr[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    w10[a] = X[1][a] - X[0][a];
    w20[a] = X[2][a] - X[0][a];
  }
  cross3(w10, w20, cr);
  if (dot3(cr, cr) < 1e-6) return false;
  double T[9], ip[3];
  p3p_frame(f[0], f[1], T);
  matvec3(T, f[2], ip);
  if (ip[2] > 0.0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double t = f[0][a];
      f[0][a] = f[1][a];
      f[1][a] = t;
      t = X[0][a];
      X[0][a] = X[1][a];
      X[1][a] = t;
    }
    p3p_frame(f[0], f[1], T);
    matvec3(T, f[2], ip);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      w10[a] = X[1][a] - X[0][a];
      w20[a] = X[2][a] - X[0][a];
    }
  }
  double N[9], wp[3];
  const double d = sqrt(dot3(w10, w10));
#pragma unroll
  for (int a = 0; a < 3; ++a) N[a] = w10[a] / d;
  cross3(N, w20, N + 6);
  normalize3(N + 6);
  cross3(N + 6, N, N + 3);
  matvec3(N, w20, wp);
  const double f1 = ip[0] / ip[2], f2 = ip[1] / ip[2];
  const double p1 = wp[0], p2 = wp[1];
  const double cosb = dot3(f[0], f[1]);
  double b = 1.0 / (1.0 - cosb * cosb) - 1.0;
  b = cosb < 0.0 ? -sqrt(b) : sqrt(b);
  // the quartic in cos(theta), highest power first
  const double F1 = f1 * f1, F2 = f2 * f2, P1 = p1 * p1, P2 = p2 * p2, D2 = d * d, Bb = b * b, f12 = f1 * f2;
  const double a4 = -(P2 * P2) * ((F2 + F1) + 1.0);
  const double a3 = (2.0 * (P2 * p2) * d) * (b * (1.0 + F2) - f12);
  const double a2 = P2 * ((((((((((F2 * P2 + F1 * P2) - F2 * P1) - F2 * (D2 * Bb)) - F2 * D2) + 2.0 * (p1 * d)) +
                              2.0 * (f12 * (p1 * (d * b)))) - P1 * F1) + 2.0 * (p1 * (F2 * d))) - D2 * Bb) - 2.0 * P1);
  const double a1 = (2.0 * (p2 * d)) * (((b * P1 + f12 * P2) - F2 * (P2 * b)) - p1 * (d * b));
  const double a0 = (((((((F2 * (P2 * D2) - 2.0 * (f12 * (P2 * (p1 * (d * b))))) + 2.0 * (P1 * (p1 * d))) - P1 * D2) +
                        F2 * (P2 * P1)) - P1 * P1) - 2.0 * (F2 * (P2 * (p1 * d)))) + P2 * (F1 * P1)) +
                    F2 * (P2 * (D2 * Bb));
  if (a4 == 0.0) return false;
  double ct[4];
  quartic_real_parts(a3 / a4, a2 / a4, a1 / a4, a0 / a4, ct);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double c = ct[k];
    const double cot = (((-f1 * p1) / f2 - c * p2) + d * b) / ((((-f1 * c) * p2) / f2 + p1) - d);
    const double st = sqrt(1.0 - c * c);
    const double sa = sqrt(1.0 / (cot * cot + 1.0));
    double ca = sqrt(1.0 - sa * sa);
    if (cot < 0.0) ca = -ca;
    const double kk = sa * b + ca;
    const double cnu[3] = {(d * ca) * kk, ((c * d) * sa) * kk, ((st * d) * sa) * kk};
    double t0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) t0[a] = X[0][a] + ((N[a] * cnu[0] + N[3 + a] * cnu[1]) + N[6 + a] * cnu[2]);
    const double Q[9] = {-ca, -sa * c, -sa * st, sa, -ca * c, -ca * st, 0.0, -st, c};
    double A[9];  // Q N
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) A[3 * i + j] = (Q[3 * i] * N[j] + Q[3 * i + 1] * N[3 + j]) + Q[3 * i + 2] * N[6 + j];
    double* R = poses + 12 * k;  // T^T (Q N)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[3 * i + j] = (T[i] * A[j] + T[3 + i] * A[3 + j]) + T[6 + i] * A[6 + j];
    double t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = -((R[3 * i] * t0[0] + R[3 * i + 1] * t0[1]) + R[3 * i + 2] * t0[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) R[9 + j] = -((R[j] * t[0] + R[3 + j] * t[1]) + R[6 + j] * t[2]);
  }
  return true;
}

// 1 where the squared reprojection error |hnormalized(R (X - c)) - feature|^2 is not below the threshold (NaN included)
__device__ __forceinline__ int localize_outlier(const double* __restrict__ P, double X, double Y, double Z, double fx,
                                                double fy, double thresh) {
#pragma clang fp contract(off)
  const double d0 = X - P[9], d1 = Y - P[10], d2 = Z - P[11];
  const double r0 = (P[0] * d0 + P[1] * d1) + P[2] * d2;
  const double r1 = (P[3] * d0 + P[4] * d1) + P[5] * d2;
  const double r2 = (P[6] * d0 + P[7] * d1) + P[8] * d2;
  const double du = r0 / r2 - fx, dv = r1 / r2 - fy;
  return (du * du + dv * dv) < thresh ? 0 : 1;
}

struct LocalizeProblem {
  static constexpr int kSample = 3, kSlots = 4, kModel = 12, kScoreSlots = 4, kPlanes = 5, kThreads = 64, kSlab = 0;
  // four poses or none, so the four flags are equal
  __device__ static void models(const double pts[kPlanes][kSample], double*, double* __restrict__ poses, int* has) {
    double feat[3][2], X[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      feat[k][0] = pts[kLocFx][k];
      feat[k][1] = pts[kLocFy][k];
      X[k][0] = pts[kLocWx][k];
      X[k][1] = pts[kLocWy][k];
      X[k][2] = pts[kLocWz][k];
    }
    if (p3p_poses(feat, X, poses)) has[0] = has[1] = has[2] = has[3] = 1;
  }
  __device__ __forceinline__ static int outlier(const double* __restrict__ P, const double x[kPlanes], double thresh) {
    return localize_outlier(P, x[kLocWx], x[kLocWy], x[kLocWz], x[kLocFx], x[kLocFy], thresh);
  }
};

// One wavefront per selected view.  status: 2 no model, 3 fewer than min_num_inliers inliers, 0 localised (the pose
// goes to ext: position, then Ceres' RotationMatrixToAngleAxis of R).
__global__ __launch_bounds__(64) void localize_final_kernel(RansacBatch B, int min_num_inliers,
                                                            unsigned char* __restrict__ slot_inlier,
                                                            int* __restrict__ num_inliers,
                                                            signed char* __restrict__ status, double* __restrict__ pose_out,
                                                            double* __restrict__ ext) {
#pragma clang fp contract(off)
  const int s = blockIdx.x;
  const int lane = threadIdx.x;
  const int count = ransac_final_inliers<LocalizeProblem>(B, s, lane, slot_inlier, num_inliers, status);
  if (count < 0) return;
  const double* P = B.state[s].model;
  if (lane == 0) {
    const int code = count < min_num_inliers ? 3 : 0;
    status[s] = (signed char)code;
    double Rc[9], aa[3];  // column-major for rotation_matrix_to_angle_axis
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rc[i + 3 * j] = P[3 * i + j];
    rot::rotation_matrix_to_angle_axis(Rc, aa);
    double* po = pose_out + 6 * s;
    po[0] = P[9];
    po[1] = P[10];
    po[2] = P[11];
    po[3] = aa[0];
    po[4] = aa[1];
    po[5] = aa[2];
    if (code == 0) {
      double* e = ext + 6 * (long long)B.sel_item[s];
#pragma unroll
      for (int q = 0; q < 6; ++q) e[q] = po[q];
    }
  }
}

}  // namespace tmi
