// Batched EstimateHomography (estimators/estimate_homography.cc:54-117): RANSAC over the normalised four-point
// homography for many view pairs at once, on the chunked evaluate-then-replay scaffold of ransac_core.h (the loop itself
// is the host's, side_calls.h), with either scoring: the integer outlier count (ransac_score_kernel,
// ransac_replay_kernel) or MLESAC (ransac_score_mle_kernel, ransac_replay_mle_kernel).  What is this call's own: the
// problem the scaffold's kernels are instantiated with, and one final launch:
//
//   HomographyProblem        a sample of four; FourPointHomography (pose/four_point_homography.cc:72-101): the two
//                            normalisations, the 8x9 rows of CreateActionConstraint, the null vector by elimination with
//                            full pivoting IN LDS, H = T2^-1 reshape(null) T1: one model (H row-major) or none; the
//                            asymmetric transfer error as residual, outlier written on it
//   homography_final_kernel  one wavefront per attempted pair: the best model's inlier mask and count, the status, H
//                            column-major
//
// The elimination is the eight-point call's (two_view_ransac_kernels.h) on another matrix: every thread owns a 9x9 slab
// of LDS (rows 0..7 the matrix, row 8 the column permutation), element e of thread t at lds[e * 64 + t], so that the
// data-dependent pivot rows and columns cost neither a bank conflict nor a dynamic index into a register array
// (scratch stays 0).  The pivot search walks (row, column) in ascending order with a strict >.
//
// The arithmetic is never contracted into FMA (#pragma clang fp contract(off) in every body) and uses only + - * /,
// sqrt and comparisons: a CPU model that evaluates the same expressions in the same order sees the same roundings.
#pragma once
#include <hip/hip_runtime.h>

#include "ransac_core.h"

namespace tmi {

// NormalizeImagePoints (pose/util.cc:82-115) on four points: the centroid (sums in sample order, / 4),
// nf = sqrt(2) / rms, T = [nf 0 -nf cx; 0 nf -nf cy; 0 0 1].
__device__ __forceinline__ void homography_normalization(const double x[4], const double y[4], double* nf, double* cx,
                                                         double* cy) {
#pragma clang fp contract(off)
  double sx = x[0], sy = y[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    sx = sx + x[k];
    sy = sy + y[k];
  }
  *cx = sx / 4.0;
  *cy = sy / 4.0;
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double dx = x[k] - *cx, dy = y[k] - *cy;
    ss = ss + (dx * dx + dy * dy);
  }
  const double rms = sqrt(ss / 4.0);
  *nf = 1.4142135623730951 / rms;
}

// FourPointHomography for one sample.  A: this thread's LDS slab, element e at A[e * 64].  H: 9 doubles, row-major.
__device__ bool homography_model(const double x1[4], const double y1[4], const double x2[4], const double y2[4],
                                 double* __restrict__ A, double* __restrict__ H) {
#pragma clang fp contract(off)
#define TMI_HG_A(r, c) A[((r) * 9 + (c)) * 64]
  double nf1, cx1, cy1, nf2, cx2, cy2;
  homography_normalization(x1, y1, &nf1, &cx1, &cy1);
  homography_normalization(x2, y2, &nf2, &cx2, &cy2);
  // rms == 0 (four times the same point), or a NaN or infinite input: no model
  if (!(nf1 <= 1.7976931348623157e308) || !(nf2 <= 1.7976931348623157e308)) return false;
  const double tx1 = -(nf1 * cx1), ty1 = -(nf1 * cy1), tx2 = -(nf2 * cx2), ty2 = -(nf2 * cy2);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = nf1 * x1[k] + tx1, b = nf1 * y1[k] + ty1;
    const double c = nf2 * x2[k] + tx2, d = nf2 * y2[k] + ty2;
    // CreateActionConstraint (:55-64)
    TMI_HG_A(2 * k, 0) = 0.0;
    TMI_HG_A(2 * k, 1) = 0.0;
    TMI_HG_A(2 * k, 2) = 0.0;
    TMI_HG_A(2 * k, 3) = -a;
    TMI_HG_A(2 * k, 4) = -b;
    TMI_HG_A(2 * k, 5) = -1.0;
    TMI_HG_A(2 * k, 6) = a * d;
    TMI_HG_A(2 * k, 7) = b * d;
    TMI_HG_A(2 * k, 8) = d;
    TMI_HG_A(2 * k + 1, 0) = a;
    TMI_HG_A(2 * k + 1, 1) = b;
    TMI_HG_A(2 * k + 1, 2) = 1.0;
    TMI_HG_A(2 * k + 1, 3) = 0.0;
    TMI_HG_A(2 * k + 1, 4) = 0.0;
    TMI_HG_A(2 * k + 1, 5) = 0.0;
    TMI_HG_A(2 * k + 1, 6) = -(a * c);
    TMI_HG_A(2 * k + 1, 7) = -(b * c);
    TMI_HG_A(2 * k + 1, 8) = -c;
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) TMI_HG_A(8, c) = (double)c;
  // elimination with full pivoting: the pivot is the entry of largest magnitude, the lowest (row, column) among equals
  double max_pivot = 0.0, min_pivot = 0.0;
  for (int k = 0; k < 8; ++k) {
    double big = -1.0;
    int pr = k, pc = k;
    for (int r = k; r < 8; ++r)
      for (int c = k; c < 9; ++c) {
        const double v = TMI_HG_A(r, c);
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
        const double t = TMI_HG_A(k, c);
        TMI_HG_A(k, c) = TMI_HG_A(pr, c);
        TMI_HG_A(pr, c) = t;
      }
    if (pc != k)
      for (int r = 0; r < 9; ++r) {
        const double t = TMI_HG_A(r, k);
        TMI_HG_A(r, k) = TMI_HG_A(r, pc);
        TMI_HG_A(r, pc) = t;
      }
    const double piv = TMI_HG_A(k, k);
    for (int r = k + 1; r < 8; ++r) {
      const double m = TMI_HG_A(r, k) / piv;
      for (int c = k + 1; c < 9; ++c) TMI_HG_A(r, c) = TMI_HG_A(r, c) - m * TMI_HG_A(k, c);
    }
  }
  // the rank with FullPivLU's default threshold for an 8x9 matrix
  if (!(min_pivot > (8.0 * 2.220446049250313e-16) * max_pivot)) return false;
  // the null vector: z[8] = 1 in the permuted order, back-substitution, the columns' permutation undone through LDS
  double z[9];
  z[8] = 1.0;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    double acc = 0.0;
#pragma unroll
    for (int c = k + 1; c < 9; ++c) acc = acc + TMI_HG_A(k, c) * z[c];
    z[k] = -acc / TMI_HG_A(k, k);
  }
  int perm[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) perm[c] = (int)TMI_HG_A(8, c);
#pragma unroll
  for (int c = 0; c < 9; ++c) TMI_HG_A(0, perm[c]) = z[c];
  double h[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) h[c] = TMI_HG_A(0, c);
  {
    double ss = 0.0, big = -1.0, lead = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      ss = ss + h[c] * h[c];
      const double m = h[c] < 0.0 ? -h[c] : h[c];
      if (m > big) {
        big = m;
        lead = h[c];
      }
    }
    double nrm = sqrt(ss);
    if (lead < 0.0) nrm = -nrm;
#pragma unroll
    for (int c = 0; c < 9; ++c) h[c] = h[c] / nrm;
  }
  // H = T2^-1 M T1 for M = [h0 h1 h2; h3 h4 h5; h6 h7 h8], T2^-1 = [1/nf2 0 cx2; 0 1/nf2 cy2; 0 0 1]
  const double inv2 = 1.0 / nf2;
  double G[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    G[r][0] = h[3 * r] * nf1;
    G[r][1] = h[3 * r + 1] * nf1;
    G[r][2] = (h[3 * r] * tx1 + h[3 * r + 1] * ty1) + h[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    H[c] = inv2 * G[0][c] + cx2 * G[2][c];
    H[3 + c] = inv2 * G[1][c] + cy2 * G[2][c];
    H[6 + c] = G[2][c];
  }
  return true;
#undef TMI_HG_A
}

// The correspondence planes of RansacBatch are x1, y1, x2, y2, in whatever units the caller uses.
struct HomographyProblem {
  static constexpr int kSample = 4, kSlots = 1, kModel = 9, kScoreSlots = 1, kPlanes = 4, kThreads = 64, kSlab = 81;
  __device__ static void models(const double pts[kPlanes][kSample], double* slab, double* __restrict__ model, int* has) {
    if (homography_model(pts[0], pts[1], pts[2], pts[3], slab, model)) has[0] = 1;
  }
  // HomographyEstimator::Error (estimate_homography.cc:90-96): the squared distance in image 2 of x2 to H x1
  __device__ __forceinline__ static double residual(const double* __restrict__ m, const double x[kPlanes]) {
#pragma clang fp contract(off)
    const double p0 = (m[0] * x[0] + m[1] * x[1]) + m[2];
    const double p1 = (m[3] * x[0] + m[4] * x[1]) + m[5];
    const double p2 = (m[6] * x[0] + m[7] * x[1]) + m[8];
    const double dx = x[2] - p0 / p2, dy = x[3] - p1 / p2;
    return dx * dx + dy * dy;
  }
  // 1 where the residual is not below the threshold (NaN included)
  __device__ __forceinline__ static int outlier(const double* __restrict__ m, const double x[kPlanes], double thresh) {
    return residual(m, x) < thresh ? 0 : 1;
  }
};

// One wavefront per attempted pair.  status 2: no model.  model_out [num_selected 9]: H column-major.
__global__ __launch_bounds__(64) void homography_final_kernel(RansacBatch B, unsigned char* __restrict__ slot_inlier,
                                                              int* __restrict__ num_inliers,
                                                              signed char* __restrict__ status,
                                                              double* __restrict__ model_out) {
  const int s = blockIdx.x;
  const int lane = threadIdx.x;
  double* mo = model_out + 9 * s;
  if (ransac_final_inliers<HomographyProblem>(B, s, lane, slot_inlier, num_inliers, status) < 0) {
    if (lane < 9) mo[lane] = 0.0;
    return;
  }
  const double* m = B.state[s].model;
  if (lane == 0) status[s] = 0;
  if (lane < 9) mo[lane] = m[3 * (lane % 3) + lane / 3];
}

}  // namespace tmi
