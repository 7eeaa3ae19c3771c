// Batched EstimateUncalibratedRelativePose (estimate_uncalibrated_relative_pose.cc:67-172): RANSAC over the normalised
// eight-point fundamental matrix for many view pairs at once, on the chunked evaluate-then-replay scaffold of
// ransac_core.h (the loop itself is the host's, side_calls.h).  What is this call's own: the problem the scaffold's
// three per-chunk kernels are instantiated with, and one final launch:
//
//   EightPointProblem      a sample of eight; the normalised eight-point F (8x9 elimination with full pivoting IN LDS,
//                          one 3x3 Jacobi SVD), the focal lengths from F, the essential matrix' decomposition (one 3x3
//                          Jacobi SVD) and the cheirality vote over the eight sampled points: one model (F, R, position,
//                          f1, f2) or none; cheirality and the squared Sampson distance against the threshold
//   two_view_final_kernel  one wavefront per attempted pair: the best model's inlier mask and count, the status, the
//                          model (F column-major, the rotation as angle-axis)
//
// The 8x9 constraint matrix does not fit one thread's registers beside the rest, so every thread owns an 9x9 slab of LDS
// (rows 0..7 the matrix, row 8 the column permutation), element e of thread t at lds[e * 64 + t]: a wavefront's 64 lanes
// always touch 64 consecutive doubles whatever e each lane asks for, so the data-dependent pivot rows and columns cost no
// bank conflict, and no index into a register array is ever dynamic (scratch stays 0).  The pivot search walks (row,
// column) in ascending order with a strict >, so the pivot and tie rules are those of the C ABI's text whatever the
// mapping.
//
// The arithmetic of steps 3 to 6 is never contracted into FMA (#pragma clang fp contract(off) in every body) and uses
// only + - * / and sqrt: a CPU model that evaluates the same expressions in the same order sees the same roundings.
#pragma once
#include <hip/hip_runtime.h>

#include "ransac_core.h"
#include "rotation_kernels.h"
#include "vec3.h"

namespace tmi {

constexpr int kTwoViewJacobiSweeps = 10;  // of the cyclic one-sided Jacobi iteration on a 3x3 matrix

// NormalizeImagePoints (pose/util.cc:82-115) on eight points: nf = sqrt(2) / rms, T = [nf 0 tx; 0 nf ty; 0 0 1].
__device__ __forceinline__ void two_view_normalization(const double x[8], const double y[8], double* nf, double* tx,
                                                       double* ty) {
#pragma clang fp contract(off)
  double sx = x[0], sy = y[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    sx = sx + x[k];
    sy = sy + y[k];
  }
  const double cx = sx / 8.0, cy = sy / 8.0;
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double dx = x[k] - cx, dy = y[k] - cy;
    ss = ss + (dx * dx + dy * dy);
  }
  const double rms = sqrt(ss / 8.0);
  *nf = 1.4142135623730951 / rms;
  *tx = -(*nf * cx);
  *ty = -(*nf * cy);
}

// One-sided (Hestenes) Jacobi SVD of the 3x3 matrix whose COLUMNS are a0, a1, a2: kTwoViewJacobiSweeps sweeps over the
// column pairs (0,1), (0,2), (1,2); v0, v1, v2 are the columns of V.  Afterwards the columns are sorted by descending
// squared norm (a stable bubble network: a tie keeps the lower column first); column j of A is sigma_j u_j.
#define TMI_TV_ROTATE(ap, aq, vp, vq)                                                   \
  {                                                                                     \
    const double alpha = (ap[0] * ap[0] + ap[1] * ap[1]) + ap[2] * ap[2];               \
    const double beta = (aq[0] * aq[0] + aq[1] * aq[1]) + aq[2] * aq[2];                \
    const double gamma = (ap[0] * aq[0] + ap[1] * aq[1]) + ap[2] * aq[2];               \
    if (gamma != 0.0) {                                                                 \
      const double zeta = (beta - alpha) / (2.0 * gamma);                               \
      const double az = zeta < 0.0 ? -zeta : zeta;                                      \
      double t = 1.0 / (az + sqrt(1.0 + zeta * zeta));                                  \
      if (zeta < 0.0) t = -t;                                                           \
      const double c = 1.0 / sqrt(1.0 + t * t);                                         \
      const double s = c * t;                                                           \
      _Pragma("unroll") for (int r_ = 0; r_ < 3; ++r_) {                                \
        const double p_ = ap[r_], q_ = aq[r_];                                          \
        ap[r_] = c * p_ - s * q_;                                                       \
        aq[r_] = s * p_ + c * q_;                                                       \
        const double vp_ = vp[r_], vq_ = vq[r_];                                        \
        vp[r_] = c * vp_ - s * vq_;                                                     \
        vq[r_] = s * vp_ + c * vq_;                                                     \
      }                                                                                 \
    }                                                                                   \
  }
#define TMI_TV_SORT(na, nb, aa, ab, va, vb)       \
  if (na < nb) {                                  \
    double t_ = na;                               \
    na = nb;                                      \
    nb = t_;                                      \
    _Pragma("unroll") for (int r_ = 0; r_ < 3; ++r_) { \
      t_ = aa[r_];                                \
      aa[r_] = ab[r_];                            \
      ab[r_] = t_;                                \
      t_ = va[r_];                                \
      va[r_] = vb[r_];                            \
      vb[r_] = t_;                                \
    }                                             \
  }
__host__ __device__ __forceinline__ void two_view_jacobi_svd(double a0[3], double a1[3], double a2[3], double v0[3], double v1[3],
                                                    double v2[3]) {
#pragma clang fp contract(off)
  v0[0] = 1.0; v0[1] = 0.0; v0[2] = 0.0;
  v1[0] = 0.0; v1[1] = 1.0; v1[2] = 0.0;
  v2[0] = 0.0; v2[1] = 0.0; v2[2] = 1.0;
  for (int sweep = 0; sweep < kTwoViewJacobiSweeps; ++sweep) {
    TMI_TV_ROTATE(a0, a1, v0, v1)
    TMI_TV_ROTATE(a0, a2, v0, v2)
    TMI_TV_ROTATE(a1, a2, v1, v2)
  }
  double n0 = (a0[0] * a0[0] + a0[1] * a0[1]) + a0[2] * a0[2];
  double n1 = (a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2];
  double n2 = (a2[0] * a2[0] + a2[1] * a2[1]) + a2[2] * a2[2];
  TMI_TV_SORT(n0, n1, a0, a1, v0, v1)
  TMI_TV_SORT(n1, n2, a1, a2, v1, v2)
  TMI_TV_SORT(n0, n1, a0, a1, v0, v1)
}
#undef TMI_TV_ROTATE
#undef TMI_TV_SORT

// The null vector of the rank-2 matrix with rows r0, r1, r2: the cross product of two rows with the largest squared
// norm, in the order r0 x r1, r0 x r2, r1 x r2 with a strict > (its sign and length are whatever the product gives).
__device__ __forceinline__ void two_view_null_vector(const double r0[3], const double r1[3], const double r2[3],
                                                     double e[3]) {
#pragma clang fp contract(off)
  double c[3];
  cross3(r0, r1, e);
  double best = dot3(e, e);
  cross3(r0, r2, c);
  double n = dot3(c, c);
  if (n > best) {
    best = n;
    e[0] = c[0]; e[1] = c[1]; e[2] = c[2];
  }
  cross3(r1, r2, c);
  n = dot3(c, c);
  if (n > best) {
    e[0] = c[0]; e[1] = c[1]; e[2] = c[2];
  }
}

// The two expressions of IsTriangulatedPointInFrontOfCameras (triangulation.cc:216-232) for the normalised pair
// (u1, v1), (u2, v2) under rotation R (row-major) and position p; in front when both are > 0.
__host__ __device__ __forceinline__ void two_view_cheirality(const double* __restrict__ R, double px, double py, double pz, double u1,
                                                    double v1, double u2, double v2, double* e1, double* e2) {
#pragma clang fp contract(off)
  const double d0 = (R[0] * u2 + R[3] * v2) + R[6];
  const double d1 = (R[1] * u2 + R[4] * v2) + R[7];
  const double d2 = (R[2] * u2 + R[5] * v2) + R[8];
  const double dir1_sq = (u1 * u1 + v1 * v1) + 1.0;
  const double dir2_sq = (d0 * d0 + d1 * d1) + d2 * d2;
  const double dir1_dir2 = (u1 * d0 + v1 * d1) + d2;
  const double dir1_pos = (u1 * px + v1 * py) + pz;
  const double dir2_pos = (d0 * px + d1 * py) + d2 * pz;
  *e1 = dir2_sq * dir1_pos - dir1_dir2 * dir2_pos;
  *e2 = dir1_dir2 * dir1_pos - dir1_sq * dir2_pos;
}

// Steps 3 to 5 for one sample.  A: this thread's LDS slab, element e at A[e * 64].  model: kTwoViewModel doubles.
__device__ bool two_view_model(const double x1[8], const double y1[8], const double x2[8], const double y2[8],
                               double* __restrict__ A, double* __restrict__ model) {
#pragma clang fp contract(off)
#define TMI_TV_A(r, c) A[((r) * 9 + (c)) * 64]
  double nf1, tx1, ty1, nf2, tx2, ty2;
  two_view_normalization(x1, y1, &nf1, &tx1, &ty1);
  two_view_normalization(x2, y2, &nf2, &tx2, &ty2);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double a = nf1 * x1[k] + tx1, b = nf1 * y1[k] + ty1;
    const double c = nf2 * x2[k] + tx2, d = nf2 * y2[k] + ty2;
    TMI_TV_A(k, 0) = c * a;
    TMI_TV_A(k, 1) = c * b;
    TMI_TV_A(k, 2) = c;
    TMI_TV_A(k, 3) = d * a;
    TMI_TV_A(k, 4) = d * b;
    TMI_TV_A(k, 5) = d;
    TMI_TV_A(k, 6) = a;
    TMI_TV_A(k, 7) = b;
    TMI_TV_A(k, 8) = 1.0;
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) TMI_TV_A(8, c) = (double)c;
  // elimination with full pivoting (FullPivLU): the pivot is the entry of largest magnitude, the lowest (row, column)
  // among equals
  double max_pivot = 0.0, min_pivot = 0.0;
  for (int k = 0; k < 8; ++k) {
    double big = -1.0;
    int pr = k, pc = k;
    for (int r = k; r < 8; ++r)
      for (int c = k; c < 9; ++c) {
        const double v = TMI_TV_A(r, c);
        const double m = v < 0.0 ? -v : v;
        if (m > big) {
          big = m;
          pr = r;
          pc = c;
        }
      }
    if (!(big > 0.0)) return false;  // the rest is zero (or NaN): rank < 8
    if (k == 0 || big > max_pivot) max_pivot = big;
    if (k == 0 || big < min_pivot) min_pivot = big;
    if (pr != k)
      for (int c = 0; c < 9; ++c) {
        const double t = TMI_TV_A(k, c);
        TMI_TV_A(k, c) = TMI_TV_A(pr, c);
        TMI_TV_A(pr, c) = t;
      }
    if (pc != k)
      for (int r = 0; r < 9; ++r) {
        const double t = TMI_TV_A(r, k);
        TMI_TV_A(r, k) = TMI_TV_A(r, pc);
        TMI_TV_A(r, pc) = t;
      }
    const double piv = TMI_TV_A(k, k);
    for (int r = k + 1; r < 8; ++r) {
      const double m = TMI_TV_A(r, k) / piv;
      for (int c = k + 1; c < 9; ++c) TMI_TV_A(r, c) = TMI_TV_A(r, c) - m * TMI_TV_A(k, c);
    }
  }
  // FullPivLU's rank with its default threshold for an 8x9 matrix
  if (!(min_pivot > (8.0 * 2.220446049250313e-16) * max_pivot)) return false;
  // the kernel: z[8] = 1 in the permuted order, back-substitution, the columns' permutation undone through LDS
  double z[9];
  z[8] = 1.0;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    double acc = 0.0;
#pragma unroll
    for (int c = k + 1; c < 9; ++c) acc = acc + TMI_TV_A(k, c) * z[c];
    z[k] = -acc / TMI_TV_A(k, k);
  }
  int perm[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) perm[c] = (int)TMI_TV_A(8, c);
#pragma unroll
  for (int c = 0; c < 9; ++c) TMI_TV_A(0, perm[c]) = z[c];
  double f[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) f[c] = TMI_TV_A(0, c);
  {
    double ss = 0.0, big = -1.0, lead = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      ss = ss + f[c] * f[c];
      const double m = f[c] < 0.0 ? -f[c] : f[c];
      if (m > big) {
        big = m;
        lead = f[c];
      }
    }
    double nrm = sqrt(ss);
    if (lead < 0.0) nrm = -nrm;
#pragma unroll
    for (int c = 0; c < 9; ++c) f[c] = f[c] / nrm;
  }
  // the nearest rank-2 matrix of M = [f0 f1 f2; f3 f4 f5; f6 f7 f8] (the lazy transpose of the reference resolved)
  double a0[3] = {f[0], f[3], f[6]}, a1[3] = {f[1], f[4], f[7]}, a2[3] = {f[2], f[5], f[8]};
  double v0[3], v1[3], v2[3];
  two_view_jacobi_svd(a0, a1, a2, v0, v1, v2);
  double M[3][3], G[3][3], Fm[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[r][c] = a0[r] * v0[c] + a1[r] * v1[c];
  // F = T2^T M T1
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    G[r][0] = M[r][0] * nf1;
    G[r][1] = M[r][1] * nf1;
    G[r][2] = (M[r][0] * tx1 + M[r][1] * ty1) + M[r][2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    Fm[0][c] = nf2 * G[0][c];
    Fm[1][c] = nf2 * G[1][c];
    Fm[2][c] = (tx2 * G[0][c] + ty2 * G[1][c]) + G[2][c];
  }
  // FocalLengthsFromFundamentalMatrix: the epipoles F e1 = 0, F^T e2 = 0
  double e1[3], e2[3];
  two_view_null_vector(Fm[0], Fm[1], Fm[2], e1);
  {
    const double c0[3] = {Fm[0][0], Fm[1][0], Fm[2][0]}, c1[3] = {Fm[0][1], Fm[1][1], Fm[2][1]},
                 c2[3] = {Fm[0][2], Fm[1][2], Fm[2][2]};
    two_view_null_vector(c0, c1, c2, e2);
  }
  if (e1[0] == 0.0 || e2[0] == 0.0) return false;
  // the in-plane rotations [c -s 0; s c 0; 0 0 1] with c = e_x / r, s = -e_y / r, r = sqrt(e_x^2 + e_y^2)
  const double r1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1]), r2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1]);
  const double cs1 = e1[0] / r1, sn1 = -e1[1] / r1, cs2 = e2[0] / r2, sn2 = -e2[1] / r2;
  const double re1x = cs1 * e1[0] - sn1 * e1[1], re1z = e1[2];
  const double re2x = cs2 * e2[0] - sn2 * e2[1], re2z = e2[2];
  double H[2][2];  // (F R1^T), rows 0 and 1, columns 0 and 1
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    H[r][0] = Fm[r][0] * cs1 - Fm[r][1] * sn1;
    H[r][1] = Fm[r][0] * sn1 + Fm[r][1] * cs1;
  }
  const double rf00 = cs2 * H[0][0] - sn2 * H[1][0], rf01 = cs2 * H[0][1] - sn2 * H[1][1];
  const double rf10 = sn2 * H[0][0] + cs2 * H[1][0], rf11 = sn2 * H[0][1] + cs2 * H[1][1];
  const double fa = (rf00 / re2z) / re1z, fb = rf01 / re2z, fc = rf10 / re1z, fd = rf11;
  const double f1_sq = (((-fa * fc) * re1x) * re1x) / ((((fa * fc) * re1z) * re1z) + fb * fd);
  const double f2_sq = (((-fa * fb) * re2x) * re2x) / ((((fa * fb) * re2z) * re2z) + fc * fd);
  if (!(f1_sq >= 0.0) || !(f2_sq >= 0.0)) return false;  // negative, or NaN (the latter a DEVIATION)
  const double fl1 = sqrt(f1_sq), fl2 = sqrt(f2_sq);
  // E = diag(f2, f2, 1) F diag(f1, f1, 1) and its decomposition
  {
    const double k1[3] = {fl1, fl1, 1.0}, k2[3] = {fl2, fl2, 1.0};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      a0[r] = (k2[r] * Fm[r][0]) * k1[0];
      a1[r] = (k2[r] * Fm[r][1]) * k1[1];
      a2[r] = (k2[r] * Fm[r][2]) * k1[2];
    }
  }
  two_view_jacobi_svd(a0, a1, a2, v0, v1, v2);
  double u0[3], u1[3], u2[3], t[3];
  {
    const double s0 = sqrt(dot3(a0, a0)), s1 = sqrt(dot3(a1, a1));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      u0[r] = a0[r] / s0;
      u1[r] = a1[r] / s1;
    }
  }
  // with both determinants fixed to +1 the third columns are the cross products of the first two
  cross3(u0, u1, u2);
  cross3(v0, v1, v2);
  t[0] = u2[0]; t[1] = u2[1]; t[2] = u2[2];
  normalize3(t);
  double R1[9], R2[9], q1[3], q2[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      R1[3 * r + c] = (u0[r] * v1[c] - u1[r] * v0[c]) + u2[r] * v2[c];
      R2[3 * r + c] = (u1[r] * v0[c] - u0[r] * v1[c]) + u2[r] * v2[c];
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    q1[c] = (R1[c] * t[0] + R1[3 + c] * t[1]) + R1[6 + c] * t[2];
    q2[c] = (R2[c] * t[0] + R2[3 + c] * t[1]) + R2[6 + c] * t[2];
  }
  // the four candidates (R1, -q1), (R1, q1), (R2, -q2), (R2, q2); the position's sign flips both expressions exactly
  int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double p1 = x1[k] / fl1, p2 = y1[k] / fl1, p3 = x2[k] / fl2, p4 = y2[k] / fl2;
    double ea, eb;
    two_view_cheirality(R1, -q1[0], -q1[1], -q1[2], p1, p2, p3, p4, &ea, &eb);
    n0 += (ea > 0.0 && eb > 0.0) ? 1 : 0;
    n1 += (-ea > 0.0 && -eb > 0.0) ? 1 : 0;
    two_view_cheirality(R2, -q2[0], -q2[1], -q2[2], p1, p2, p3, p4, &ea, &eb);
    n2 += (ea > 0.0 && eb > 0.0) ? 1 : 0;
    n3 += (-ea > 0.0 && -eb > 0.0) ? 1 : 0;
  }
  int best = 0, best_n = n0;  // std::max_element: the first of the largest
  if (n1 > best_n) { best = 1; best_n = n1; }
  if (n2 > best_n) { best = 2; best_n = n2; }
  if (n3 > best_n) { best = 3; best_n = n3; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) model[3 * r + c] = Fm[r][c];
#pragma unroll
  for (int q = 0; q < 9; ++q) model[9 + q] = best < 2 ? R1[q] : R2[q];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double q = best < 2 ? q1[c] : q2[c];
    model[18 + c] = (best & 1) ? q : -q;
  }
  model[21] = fl1;
  model[22] = fl2;
  model[23] = 0.0;
  return true;
#undef TMI_TV_A
}

// 1 where the correspondence is no inlier of the model: behind a camera, or a squared Sampson distance of the centred
// pixels (pose/util.cc:56-68) that is not below the threshold (NaN included)
__device__ __forceinline__ int two_view_outlier(const double* __restrict__ m, double x1, double y1, double x2, double y2,
                                                double thresh) {
#pragma clang fp contract(off)
  double ea, eb;
  two_view_cheirality(m + 9, m[18], m[19], m[20], x1 / m[21], y1 / m[21], x2 / m[22], y2 / m[22], &ea, &eb);
  const double l0 = (m[0] * x1 + m[1] * y1) + m[2];
  const double l1 = (m[3] * x1 + m[4] * y1) + m[5];
  const double l2 = (m[6] * x1 + m[7] * y1) + m[8];
  const double num = (x2 * l0 + y2 * l1) + l2;
  const double g0 = (x2 * m[0] + y2 * m[3]) + m[6];
  const double g1 = (x2 * m[1] + y2 * m[4]) + m[7];
  const double den = ((g0 * g0 + g1 * g1) + l0 * l0) + l1 * l1;
  const double err = (num * num) / den;
  return (ea > 0.0 && eb > 0.0 && err < thresh) ? 0 : 1;
}

// The correspondence planes of RansacBatch are x1, y1, x2, y2: centred pixels.
struct TwoViewOutlier {
  static constexpr int kModel = kTwoViewModel, kPlanes = 4;
  __device__ __forceinline__ static int outlier(const double* __restrict__ m, const double x[kPlanes], double thresh) {
    return two_view_outlier(m, x[0], x[1], x[2], x[3], thresh);
  }
};

struct EightPointProblem : TwoViewOutlier {
  static constexpr int kSample = 8, kSlots = 1, kScoreSlots = 1, kThreads = 64, kSlab = 81;
  __device__ static void models(const double pts[kPlanes][kSample], double* slab, double* __restrict__ model, int* has) {
    if (two_view_model(pts[0], pts[1], pts[2], pts[3], slab, model)) has[0] = 1;
  }
};

// One wavefront per attempted pair.  status 2: no model.  model_out [num_selected 17]: F column-major, f1, f2, the
// rotation as angle-axis (Ceres' RotationMatrixToAngleAxis), the position.
__global__ __launch_bounds__(64) void two_view_final_kernel(RansacBatch B, unsigned char* __restrict__ slot_inlier,
                                                            int* __restrict__ num_inliers,
                                                            signed char* __restrict__ status,
                                                            double* __restrict__ model_out) {
#pragma clang fp contract(off)
  const int s = blockIdx.x;
  const int lane = threadIdx.x;
  double* mo = model_out + 17 * s;
  if (ransac_final_inliers<TwoViewOutlier>(B, s, lane, slot_inlier, num_inliers, status) < 0) {
    if (lane < 17) mo[lane] = 0.0;
    return;
  }
  const double* m = B.state[s].model;
  if (lane == 0) {
    status[s] = 0;
    double Rc[9], aa[3];  // column-major for rotation_matrix_to_angle_axis
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Rc[i + 3 * j] = m[9 + 3 * i + j];
        mo[i + 3 * j] = m[3 * i + j];
      }
    rot::rotation_matrix_to_angle_axis(Rc, aa);
    mo[9] = m[21];
    mo[10] = m[22];
    mo[11] = aa[0];
    mo[12] = aa[1];
    mo[13] = aa[2];
    mo[14] = m[18];
    mo[15] = m[19];
    mo[16] = m[20];
  }
}

}  // namespace tmi
