// Batched EstimateAbsolutePoseWithKnownOrientation (estimators/estimate_absolute_pose_with_known_orientation.cc:54-150)
// and EstimateRelativePoseWithKnownOrientation (estimators/estimate_relative_pose_with_known_orientation.cc:19-82): the
// two RANSACs over a sample of TWO that the reference runs once a view's rotation is known, for many views or view
// pairs at once, on the chunked evaluate-then-replay scaffold of ransac_core.h (the loop itself is the host's,
// side_calls.h), with either scoring.  What is these calls' own:
//
//   rotate_features_kernel             one thread per correspondence: feature <- hnormalized(R^T (u, v, 1)), R Ceres'
//                                      AngleAxisToRotationMatrix of the item's angle-axis (RotateCorrespondences, :54-73;
//                                      the relative call's features are "rotated to be in the same world coordinate
//                                      system" by the caller in the reference -- rf = hnormalize(R^t K^-1 [u v 1]^t),
//                                      relative_pose_from_two_points_with_known_rotation.h:43-47 -- here by this kernel,
//                                      feature1 with the first view's rotation, feature2 with the second's)
//   KnownOrientationAbsoluteProblem    PositionFromTwoRays (pose/position_from_two_rays.cc:56-83) in closed form, the
//                                      squared reprojection error of X - c (:106-113), no cheirality test
//   KnownOrientationRelativeProblem    RelativePoseFromTwoPointsWithKnownRotation
//                                      (pose/relative_pose_from_two_points_with_known_rotation.cc:51-88), the squared
//                                      Sampson distance under [-t]x (:52-58), no cheirality test
//   known_orientation_*_final_kernel   one wavefront per attempted item: inlier mask and count, status, the 3 doubles
//
// THE POSITION.  The 4x3 system has rows [1 0 -u_k], [0 1 -v_k] and right side (X_k - u_k Z_k, Y_k - v_k Z_k), k = 1, 2.
// Its normal equations are [2 0 -su; 0 2 -sv; -su -sv n22] with su = u1 + u2, sv = v1 + v2, n22 = (u1^2 + v1^2) +
// (u2^2 + v2^2).  Eliminating c_x and c_y (pivots 2 and 2, exact) leaves the pivot q / 2 for c_z with q = du^2 + dv^2,
// du = u1 - u2, dv = v1 - v2, computed from the DIFFERENCES (never as n22 - (su^2 + sv^2) / 2, which cancels):
//   c_z = -((du dbx + dv dby) / q),   c_x = ((b0 + u1 c_z) + (b2 + u2 c_z)) / 2,   c_y likewise,
// the least-squares solution the reference's QR gives, in one fixed sequence.
// RANK RULE (the reference: ColPivHouseholderQR::rank() != 3, threshold 3 DBL_EPSILON on the diagonal of R, whose
// squares are the pivots here): rank 3 iff  q / 2 > (3 DBL_EPSILON)^2 max(2, n22),  the smallest pivot of the normal
// equations against their largest diagonal entry.  Two equal rotated features (q == 0), or a NaN, give no model.
//
// THE BASELINE DIRECTION.  Rows e_k = (y2 - y1, x1 - x2, y1 x2 - x1 y2) of the two correspondences (:65-74).
// RANK RULE (the reference: FullPivLU::dimensionOfKernel() != 1, threshold 2 DBL_EPSILON): two steps of elimination with
// full pivoting under the sibling calls' rules -- the pivot is the entry of largest magnitude, strict >, ties to the
// lowest (row, column) -- and rank 2 iff  min(p0, p1) > 2 DBL_EPSILON max(p0, p1).  The null vector is the cross product
// e_0 x e_1 divided by its norm sqrt((c0^2 + c1^2) + c2^2); a norm that is 0 or not finite gives no model.
// SIGN RULE: the sign is that of e_0 x e_1 AS COMPUTED, rows in sample order, no flip (the reference's is whatever
// FullPivLU::kernel() leaves; only the direction up to sign is the estimate, and the Sampson distance does not see it).
//
// The arithmetic of the problems is never contracted into FMA (#pragma clang fp contract(off) in every body) and uses
// only + - * /, sqrt and comparisons: a CPU model that evaluates the same expressions in the same order sees the same
// roundings.  The rotation is the engine's one restatement of AngleAxisToRotationMatrix (track_estimate_kernels.h), which
// calls sin and cos: the rotated features are an OUTPUT of the calls, so that a model can start from the device's.
#pragma once
#include <hip/hip_runtime.h>

#include "ransac_core.h"
#include "track_estimate_kernels.h"

namespace tmi {

// One thread per correspondence o of the attempted items: (u[o], v[o]) <- hnormalized(R(orientation of o's item)^T (u, v, 1)).
// sel_ptr [S + 1] ascending from 0; orientation [3 S] angle-axis per attempted item.
__global__ __launch_bounds__(256) void rotate_features_kernel(int S, const long long* __restrict__ sel_ptr,
                                                              const double* __restrict__ orientation,
                                                              double* __restrict__ u, double* __restrict__ v) {
#pragma clang fp contract(off)
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (S <= 0 || o >= sel_ptr[S]) return;
  int lo = 0, hi = S - 1;  // the item s with sel_ptr[s] <= o < sel_ptr[s + 1] (empty items cannot hold o)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sel_ptr[mid] <= o) lo = mid; else hi = mid - 1;
  }
  double R[9];  // column-major: R(r, c) = R[r + 3 c]
  angle_axis_to_rotation_matrix(orientation + 3 * (long long)lo, R);
  const double x = u[o], y = v[o];
  const double r0 = (R[0] * x + R[1] * y) + R[2];
  const double r1 = (R[3] * x + R[4] * y) + R[5];
  const double r2 = (R[6] * x + R[7] * y) + R[8];
  u[o] = r0 / r2;
  v[o] = r1 / r2;
}

constexpr double kKnownOrientationEps = 2.220446049250313e-16;
constexpr double kPositionRankThreshold = (3.0 * kKnownOrientationEps) * (3.0 * kKnownOrientationEps);
constexpr double kBaselineRankThreshold = 2.0 * kKnownOrientationEps;

// The correspondence planes of RansacBatch are u, v (the ROTATED feature), X, Y, Z.  The model is the position.
struct KnownOrientationAbsoluteProblem {
  static constexpr int kSample = 2, kSlots = 1, kModel = 3, kScoreSlots = 1, kPlanes = 5, kThreads = 64, kSlab = 0;
  __device__ static void models(const double pts[kPlanes][kSample], double*, double* __restrict__ c, int* has) {
#pragma clang fp contract(off)
    const double u1 = pts[0][0], v1 = pts[1][0], u2 = pts[0][1], v2 = pts[1][1];
    const double b0 = pts[2][0] - u1 * pts[4][0], b1 = pts[3][0] - v1 * pts[4][0];
    const double b2 = pts[2][1] - u2 * pts[4][1], b3 = pts[3][1] - v2 * pts[4][1];
    const double du = u1 - u2, dv = v1 - v2;
    const double q = du * du + dv * dv;
    const double n22 = (u1 * u1 + v1 * v1) + (u2 * u2 + v2 * v2);
    const double big = n22 > 2.0 ? n22 : 2.0;
    if (!(q * 0.5 > kPositionRankThreshold * big)) return;  // rank < 3 (or a NaN)
    const double dbx = b0 - b2, dby = b1 - b3;
    const double cz = -((du * dbx + dv * dby) / q);
    c[0] = ((b0 + u1 * cz) + (b2 + u2 * cz)) * 0.5;
    c[1] = ((b1 + v1 * cz) + (b3 + v2 * cz)) * 0.5;
    c[2] = cz;
    has[0] = 1;
  }
  // :106-113: |hnormalized(X - c) - (u, v)|^2
  __device__ __forceinline__ static double residual(const double* __restrict__ c, const double x[kPlanes]) {
#pragma clang fp contract(off)
    const double d0 = x[2] - c[0], d1 = x[3] - c[1], d2 = x[4] - c[2];
    const double du = d0 / d2 - x[0], dv = d1 / d2 - x[1];
    return du * du + dv * dv;
  }
  // 1 where the residual is not below the threshold (NaN included)
  __device__ __forceinline__ static int outlier(const double* __restrict__ c, const double x[kPlanes], double thresh) {
    return residual(c, x) < thresh ? 0 : 1;
  }
};

// The correspondence planes of RansacBatch are x1, y1, x2, y2 (both features ROTATED).  The model is the unit direction.
struct KnownOrientationRelativeProblem {
  static constexpr int kSample = 2, kSlots = 1, kModel = 3, kScoreSlots = 1, kPlanes = 4, kThreads = 64, kSlab = 0;
  __device__ static void models(const double pts[kPlanes][kSample], double*, double* __restrict__ t, int* has) {
#pragma clang fp contract(off)
    double e[2][3];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double x1 = pts[0][k], y1 = pts[1][k], x2 = pts[2][k], y2 = pts[3][k];
      e[k][0] = -y1 + y2;
      e[k][1] = -x2 + x1;
      e[k][2] = y1 * x2 - x1 * y2;
    }
    // two steps of elimination with full pivoting, for the rank alone; every index is static
    double p0 = -1.0;
    int pr = 0, pc = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double m = e[r][c] < 0.0 ? -e[r][c] : e[r][c];
        if (m > p0) {
          p0 = m;
          pr = r;
          pc = c;
        }
      }
    if (!(p0 > 0.0)) return;  // all zero (or NaN): rank 0
    double a[3], b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a[c] = pr == 0 ? e[0][c] : e[1][c];
      b[c] = pr == 0 ? e[1][c] : e[0][c];
    }
    const double piv = pc == 0 ? a[0] : (pc == 1 ? a[1] : a[2]);
    const double mult = (pc == 0 ? b[0] : (pc == 1 ? b[1] : b[2])) / piv;
    double p1 = -1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = b[c] - mult * a[c];
      const double m = v < 0.0 ? -v : v;
      if (c != pc && m > p1) p1 = m;
    }
    if (!(p1 > 0.0)) return;  // rank 1
    const double mn = p1 < p0 ? p1 : p0, mx = p1 < p0 ? p0 : p1;
    if (!(mn > kBaselineRankThreshold * mx)) return;
    const double c0 = e[0][1] * e[1][2] - e[0][2] * e[1][1];
    const double c1 = e[0][2] * e[1][0] - e[0][0] * e[1][2];
    const double c2 = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    const double nrm = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(nrm > 0.0) || !(nrm <= 1.7976931348623157e308)) return;
    t[0] = c0 / nrm;
    t[1] = c1 / nrm;
    t[2] = c2 / nrm;
    has[0] = 1;
  }
  // :52-58: SquaredSampsonDistance (pose/util.cc:56-68) under F = CrossProductMatrix(-t) = [0 t2 -t1; -t2 0 t0;
  // t1 -t0 0], its zero entries left out of the sums.  There is no behind-camera rule.
  __device__ __forceinline__ static double residual(const double* __restrict__ t, const double x[kPlanes]) {
#pragma clang fp contract(off)
    const double l0 = t[2] * x[1] - t[1];
    const double l1 = t[0] - t[2] * x[0];
    const double l2 = t[1] * x[0] - t[0] * x[1];
    const double num = (x[2] * l0 + x[3] * l1) + l2;
    const double g0 = t[1] - x[3] * t[2];
    const double g1 = x[2] * t[2] - t[0];
    const double den = ((g0 * g0 + g1 * g1) + l0 * l0) + l1 * l1;
    return (num * num) / den;
  }
  __device__ __forceinline__ static int outlier(const double* __restrict__ t, const double x[kPlanes], double thresh) {
    return residual(t, x) < thresh ? 0 : 1;
  }
};

// One wavefront per attempted item.  status 2: no model (the 3 doubles are 0), else 0.  model_out [num_selected 3].
template <class P>
__device__ __forceinline__ void known_orientation_final(const RansacBatch& B, unsigned char* __restrict__ slot_inlier,
                                                        int* __restrict__ num_inliers, signed char* __restrict__ status,
                                                        double* __restrict__ model_out) {
  const int s = blockIdx.x;
  const int lane = threadIdx.x;
  double* mo = model_out + 3 * s;
  if (ransac_final_inliers<P>(B, s, lane, slot_inlier, num_inliers, status) < 0) {
    if (lane < 3) mo[lane] = 0.0;
    return;
  }
  if (lane == 0) status[s] = 0;
  if (lane < 3) mo[lane] = B.state[s].model[lane];
}

__global__ __launch_bounds__(64) void known_orientation_absolute_final_kernel(
    RansacBatch B, unsigned char* __restrict__ slot_inlier, int* __restrict__ num_inliers,
    signed char* __restrict__ status, double* __restrict__ model_out) {
  known_orientation_final<KnownOrientationAbsoluteProblem>(B, slot_inlier, num_inliers, status, model_out);
}

__global__ __launch_bounds__(64) void known_orientation_relative_final_kernel(
    RansacBatch B, unsigned char* __restrict__ slot_inlier, int* __restrict__ num_inliers,
    signed char* __restrict__ status, double* __restrict__ model_out) {
  known_orientation_final<KnownOrientationRelativeProblem>(B, slot_inlier, num_inliers, status, model_out);
}

}  // namespace tmi
