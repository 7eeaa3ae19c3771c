// Batched TwoViewMatchGeometricVerification::BundleAdjustRelativePose (reference
// src/theia/sfm/two_view_match_geometric_verification.cc:256-324, the one caller of BundleAdjustTwoViews): what the
// reference does around the two-view solve, per view pair, in two launches of their own on either side of
// two_view_lm_kernel (two_view_kernels.h):
//
//   two_view_triangulate_kernel  TriangulatePoints (:185-254) per correspondence, in input order: the two rays
//                                Camera::PixelToUnitDepthRay(feature).normalized(), SufficientTriangulationAngle,
//                                TriangulateMidpoint over the origins {C1, C2}, AcceptableReprojectionError (:72-83)
//                                in camera 1 and then camera 2; the survivors compacted in their original order;
//                                the gates on min_num_inlier_matches before (:171-176, `<=`) and after (:268, `<`)
//   (two_view_lm_kernel)         BundleAdjustTwoViews on the compacted survivors, range end from corr_end
//   two_view_accept_kernel       the filter after the adjustment (:295-314) on the adjusted cameras and points, the
//                                scatter back through the original index, the last test of VerifyMatches (:181, `>`)
//
// Geometry of two_view_lm_kernel: ONE WAVEFRONT PER VIEW PAIR, four pairs per 256-thread workgroup, the pair index
// made wave-uniform so that the camera records are scalar loads, lane i on correspondences c0 + i, c0 + i + 64, ...
// No atomics, no LDS, no state shared between waves: a pair's bytes depend on the pair alone.
//
// The triangulation is a launch of its own because of the iterative undistortion in the ray code: inlined into a
// solve it costs the solve its occupancy.
//
// Correspondence status: -1 not attempted, 0 kept, 1 insufficient angle, 2 triangulation failed, 3 bad reprojection
// of the triangulated point, 4 bad reprojection after the adjustment.  Pair status: 1 too few correspondences,
// 2 too few triangulated, 3 the adjustment failed, 4 too few verified, 0 verified.
#pragma once
#include <hip/hip_runtime.h>

#include "camera_models.h"
#include "kernels.h"
#include "track_estimate_kernels.h"
#include "two_view_kernels.h"

namespace tmi {

struct TwoViewVerifyArgs {
  long long min_matches;  // min_num_inlier_matches
  double cos_min;         // cos(min_triangulation_angle_degrees)
  double tri_max_sq;      // triangulation_max_reprojection_error ^ 2
  double final_max_sq;    // final_max_reprojection_error ^ 2
};

// Device buffers of one verification call beside the TwoViewBatch.  The compacted arrays are what two_view_lm_kernel
// reads as its feat1 / feat2 / points; pair p owns [corr_ptr[p], corr_end[p]) of them.
struct TwoViewVerifyBuffers {
  double* feat1_c;           // [2 N] survivors' features, compacted
  double* feat2_c;
  double* points_c;          // [4 N] survivors' points, compacted (triangulated, then adjusted in place)
  long long* orig;           // [N] survivors' original correspondence index
  long long* corr_end;       // [P] corr_ptr[p] + survivors; corr_ptr[p] for a gated pair
  double* points_out;        // [4 N] points at their original index
  signed char* corr_status;  // [N] preset to -1
  signed char* pair_status;  // [P]
  int* pair_count;           // [P] correspondences at status 0
};

// AcceptableReprojectionError (:72-83) in camera 1 and then camera 2: false where Camera::ProjectPoint's depth is < 0
// or the squared error is not strictly below max_sq.
__device__ __forceinline__ bool tv_acceptable(int model1, int model2, const double* E1, const double* K1,
                                              const double* E2, const double* K2, const double X[4],
                                              const double f1[2], const double f2[2], double max_sq) {
  double px[2];
  if (project_point_depth(model1, E1, K1, X, px) < 0) return false;
  double dx = f1[0] - px[0], dy = f1[1] - px[1];
  if (!(dx * dx + dy * dy < max_sq)) return false;
  if (project_point_depth(model2, E2, K2, X, px) < 0) return false;
  dx = f2[0] - px[0];
  dy = f2[1] - px[1];
  return dx * dx + dy * dy < max_sq;
}

// wave-uniform pair index (a scalar register: what it indexes is loaded by scalar loads)
__device__ __forceinline__ int tv_wave_pair() {
  return __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
}

// Steps 1-3.  B.feat1 / B.feat2: the caller's correspondences; B.ext2 / B.intr*: the cameras as given.
__global__ __launch_bounds__(256) void two_view_triangulate_kernel(TwoViewBatch B, TwoViewVerifyArgs V,
                                                                   TwoViewVerifyBuffers O) {
  const int lane = threadIdx.x & 63;
  const int pair = tv_wave_pair();
  if (pair >= B.num_pairs) return;  // wave-uniform; no workgroup barrier below
  const long long c0 = B.corr_ptr[pair], c1 = B.corr_ptr[pair + 1];
  if (c1 - c0 <= V.min_matches) {  // :171-176: BundleAdjustRelativePose is not entered, :181 cannot hold
    if (lane == 0) {
      O.corr_end[pair] = c0;
      O.pair_status[pair] = 1;
      O.pair_count[pair] = 0;
    }
    return;
  }
  const int model1 = B.model1[pair], model2 = B.model2[pair];
  double E1[6], E2[6], K1[10], K2[10];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    E1[i] = B.ext1[(size_t)pair * 6 + i];
    E2[i] = B.ext2[(size_t)pair * 6 + i];
  }
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    K1[i] = B.intr1[(size_t)pair * 10 + i];
    K2[i] = B.intr2[(size_t)pair * 10 + i];
  }
  double R1[9], R2[9];
  angle_axis_to_rotation_matrix(E1 + 3, R1);
  angle_axis_to_rotation_matrix(E2 + 3, R2);
  const unsigned long long below = (1ull << lane) - 1ull;
  long long kept = 0;  // survivors of the trips so far (wave-uniform)
  for (long long t0 = c0; t0 < c1; t0 += 64) {
    const long long q = t0 + lane;
    int st = -1;
    double f1[2], f2[2], X[4];
    if (q < c1) {
      f1[0] = B.feat1[2 * q];
      f1[1] = B.feat1[2 * q + 1];
      f2[0] = B.feat2[2 * q];
      f2[1] = B.feat2[2 * q + 1];
      double d1[3], d2[3];
      pixel_unit_ray(model1, K1, R1, f1, d1);
      pixel_unit_ray(model2, K2, R2, f2, d2);
      if (!(d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2] < V.cos_min)) {
        st = 1;  // SufficientTriangulationAngle over the one pair of rays
      } else {
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double b[3] = {0.0, 0.0, 0.0};
        midpoint_accumulate(d1, E1, A, b);
        midpoint_accumulate(d2, E2, A, b);
        if (!midpoint_solve(A, b, 2.0, X))
          st = 2;
        else
          st = tv_acceptable(model1, model2, E1, K1, E2, K2, X, f1, f2, V.tri_max_sq) ? 0 : 3;
      }
      O.corr_status[q] = (signed char)st;
    }
    const unsigned long long keep = __ballot(st == 0);
    if (st == 0) {
      const long long w = c0 + kept + (long long)__popcll(keep & below);  // w <= q: order is kept
      O.feat1_c[2 * w] = f1[0];
      O.feat1_c[2 * w + 1] = f1[1];
      O.feat2_c[2 * w] = f2[0];
      O.feat2_c[2 * w + 1] = f2[1];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        O.points_c[4 * w + a] = X[a];
        O.points_out[4 * q + a] = X[a];
      }
      O.orig[w] = q;
    }
    kept += (long long)__popcll(keep);
  }
  if (lane == 0) {
    const bool enough = !(kept < V.min_matches);  // :268
    O.corr_end[pair] = enough ? c0 + kept : c0;
    O.pair_status[pair] = enough ? 0 : 2;
    O.pair_count[pair] = (int)kept;
  }
}

// Steps 4 (the status), 5 and 6, for the pairs the triangulation left at status 0.  B: the batch two_view_lm_kernel ran
// on (compacted features and points, adjusted cameras).
__global__ __launch_bounds__(256) void two_view_accept_kernel(TwoViewBatch B, TwoViewVerifyArgs V, TwoViewVerifyBuffers O,
                                                              const signed char* __restrict__ termination) {
  const int lane = threadIdx.x & 63;
  const int pair = tv_wave_pair();
  if (pair >= B.num_pairs) return;
  if (O.pair_status[pair] != 0) return;
  const int term = termination[pair];
  if (term != 0 && term != 1) {  // :291-293; the points keep the triangulated values
    if (lane == 0) O.pair_status[pair] = 3;
    return;
  }
  const long long c0 = B.corr_ptr[pair], c1 = O.corr_end[pair];
  const int model1 = B.model1[pair], model2 = B.model2[pair];
  double E1[6], E2[6], K1[10], K2[10];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    E1[i] = B.ext1[(size_t)pair * 6 + i];
    E2[i] = B.ext2[(size_t)pair * 6 + i];
  }
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    K1[i] = B.intr1[(size_t)pair * 10 + i];
    K2[i] = B.intr2[(size_t)pair * 10 + i];
  }
  long long kept = 0;
  for (long long t0 = c0; t0 < c1; t0 += 64) {
    const long long w = t0 + lane;
    bool ok = false;
    if (w < c1) {
      const double f1[2] = {B.feat1[2 * w], B.feat1[2 * w + 1]};
      const double f2[2] = {B.feat2[2 * w], B.feat2[2 * w + 1]};
      double X[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) X[a] = B.points[4 * w + a];
      ok = tv_acceptable(model1, model2, E1, K1, E2, K2, X, f1, f2, V.final_max_sq);
      const long long q = O.orig[w];
      O.corr_status[q] = ok ? 0 : 4;
#pragma unroll
      for (int a = 0; a < 4; ++a) O.points_out[4 * q + a] = X[a];
    }
    kept += (long long)__popcll(__ballot(ok));
  }
  if (lane == 0) {
    O.pair_status[pair] = kept > V.min_matches ? 0 : 4;  // :181
    O.pair_count[pair] = (int)kept;
  }
}

}  // namespace tmi
