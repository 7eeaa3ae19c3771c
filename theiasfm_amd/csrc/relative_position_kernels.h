// Batched theia::OptimizeRelativePositionWithKnownRotation
// (optimize_relative_position_with_known_rotation.cc:53-197; called once per view-graph edge from
// reconstruction_estimator_utils.cc:244-269): the unit direction t of camera 2's position in camera 1's
// frame from the pair's correspondences and the two known world-to-camera rotations, by iteratively
// reweighted least squares on the epipolar constraint t^T c_i = 0.
//
// ONE WAVEFRONT PER PAIR, four pairs per 256-thread workgroup, every pair of the batch in one launch.
//
// (Where the views carry a camera model, relative_position_normalise_kernel turns the pixels into normalised
// coordinates first; the solve below always reads normalised features.)
//
//   phase 1  lane l takes correspondences l, l + 64, ...: the constraint column (:53-79)
//              a = R1^T [f1; 1],  b = R2^T [f2; 1],  c = R1 (b x a).
//            Pairs of up to kRelPosRegColumns * 64 correspondences keep their columns in registers; longer
//            pairs write them once to three coalesced planes of a per-call scratch buffer and every lane
//            streams its own columns back each iteration (24 B per correspondence: L2 resident).
//   phase 2  IRLS (:128-184), replicated in every lane, no divergence.  The reference's iteration k is
//              w <- max(w, 1e-7);  M = sum c c^T / w;  t = eigenvector of M's smallest eigenvalue;
//              w <- |t^T c|;  cost = sum w.
//            The weights are a function of t alone, so they are not stored: ONE pass per iteration forms
//            w = |t^T c|, the cost of t AND the M of the next iteration -- seven independent wave_sum
//            butterflies that interleave instead of two dependent rounds.  (The M formed in the pass that
//            ends the loop is not used.)  The 3 x 3 eigen-problem is cyclic Jacobi in registers.
//   phase 3  IsTriangulatedPointInFrontOfCameras (triangulation.cc:216-232) counted for t and for -t in one
//            pass over the features (read again rather than kept: 4 doubles per correspondence would double
//            the register footprint of phase 2), the flip (:189-194), and lane 0 stores the results.
//
// No atomics and no LDS: a pair's result depends on nothing but the pair, bit for bit.
//
// status: 0 the convergence counter reached 10; 1 stopped at 100 iterations (the reference returns true and
// the position for both); 2 a non-finite M or t (position not written); -1 a pair without correspondences
// (position not written).
#pragma once
#include <hip/hip_runtime.h>

#include "track_estimate_kernels.h"

namespace tmi {

constexpr int kRelPosRegColumns = 8;  // columns per lane held in registers: pairs of up to 512 correspondences
constexpr int kRelPosMaxIterations = 100;     // optimize_relative_position_with_known_rotation.cc:130
constexpr int kRelPosMaxInnerIterations = 10;  // :131
constexpr double kRelPosMinWeight = 1e-7;      // :132
constexpr double kRelPosTolerance = 1e-5;      // :138 (kEpsilon of the IRLS loop)

struct RelativePositionBatch {
  int num_pairs;
  const double* view_rot;       // [3 V] angle-axis, world to camera
  const int* view_model;        // [V], or null: the features are normalised coordinates
  const double* view_intr;      // [10 V]
  const int* pair_view1;        // [P]
  const int* pair_view2;
  const long long* corr_ptr;    // [P + 1]
  const double* feat1;          // [2 N] normalised coordinates (the solve) / what the caller gave (normalise)
  const double* feat2;
  const long long* scratch_ptr; // [P] offset of the pair's columns in a scratch plane, -1 = in registers
  double* scratch;              // [3 scratch_len] planes x | y | z
  long long scratch_len;
  double* pos2;                 // [3 P] out (status 0 / 1)
  signed char* status;          // [P]
  int* iters;
  double* cost;
  int* in_front;
};

namespace relpos {

// One Jacobi rotation in the (p, q) plane of the symmetric A (r = the third index) and of the vectors V:
// Rutishauser's formulas (Handbook for Automatic Computation II/1; Numerical Recipes "jacobi").
__device__ __forceinline__ void jacobi_rotate(int sweep, double& app, double& aqq, double& apq, double& arp, double& arq,
                                              double& v0p, double& v0q, double& v1p, double& v1q, double& v2p,
                                              double& v2q) {
  const double g = 100.0 * fabs(apq);
  if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
    apq = 0.0;
    return;
  }
  if (apq == 0.0) return;
  double h = aqq - app, t;
  if (fabs(h) + g == fabs(h)) {
    t = apq / h;
  } else {
    const double theta = 0.5 * h / apq;
    t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
  h = t * apq;
  app -= h;
  aqq += h;
  apq = 0.0;
  double x = arp, y = arq;
  arp = x - s * (y + x * tau);
  arq = y + s * (x - y * tau);
  x = v0p, y = v0q;
  v0p = x - s * (y + x * tau);
  v0q = y + s * (x - y * tau);
  x = v1p, y = v1q;
  v1p = x - s * (y + x * tau);
  v1q = y + s * (x - y * tau);
  x = v2p, y = v2q;
  v2p = x - s * (y + x * tau);
  v2q = y + s * (x - y * tau);
}

// Eigenvector of the smallest eigenvalue of the symmetric M = [m0 m1 m2; m1 m3 m4; m2 m4 m5] (unit norm up to
// round-off: a column of a product of plane rotations).  Cyclic Jacobi; the inputs are wave-uniform, so is the
// control flow.  A non-finite M leaves the sweeps without converging and returns non-finite values.
__device__ __forceinline__ void smallest_eigenvector(const double (&M)[6], double (&t)[3]) {
  double a00 = M[0], a01 = M[1], a02 = M[2], a11 = M[3], a12 = M[4], a22 = M[5];
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    if (fabs(a01) + fabs(a02) + fabs(a12) == 0.0) break;
    jacobi_rotate(sweep, a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobi_rotate(sweep, a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobi_rotate(sweep, a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  // the first of equal eigenvalues
  if (a00 <= a11 && a00 <= a22) {
    t[0] = v00, t[1] = v10, t[2] = v20;
  } else if (a11 <= a22) {
    t[0] = v01, t[1] = v11, t[2] = v21;
  } else {
    t[0] = v02, t[1] = v12, t[2] = v22;
  }
  if (!(a00 == a00 && a11 == a11 && a22 == a22)) t[0] = a00 + a11 + a22;  // NaN in, NaN out
}

// One correspondence's share of an IRLS pass at t: the weight |t^T c| into the cost, c c^T / max(w, 1e-7)
// into the upper triangle of the next M.  first: the weights of the first iteration are 1 and there is no cost yet.
__device__ __forceinline__ void accumulate(bool first, const double (&t)[3], double cx, double cy, double cz,
                                           double (&M)[6], double& cost) {
  double w = 1.0;
  if (!first) {
    w = fabs(t[0] * cx + t[1] * cy + t[2] * cz);
    cost += w;
    w = fmax(w, kRelPosMinWeight);
  }
  const double inv = 1.0 / w;
  const double sx = cx * inv, sy = cy * inv, sz = cz * inv;
  M[0] += sx * cx;
  M[1] += sx * cy;
  M[2] += sx * cz;
  M[3] += sy * cy;
  M[4] += sy * cz;
  M[5] += sz * cz;
}

}  // namespace relpos

// Pixels to normalised image coordinates, for batches whose views carry a camera model:
// PixelToNormalizedCoordinates(...).hnormalized() (reconstruction_estimator_utils.cc:84-88) of both features of
// every correspondence, once, into out1 / out2 [2 N].  Same geometry as the solve (a wave per pair, lane l takes
// correspondences l, l + 64, ...): a pair's views are wave-uniform, so model and intrinsics are scalar loads.
// A launch of its own because the iterative undistortion inside the solve costs it a third of its occupancy
// (241 VGPRs against 168) and the sign test of phase 3 would have to run it a second time.
__global__ __launch_bounds__(256) void relative_position_normalise_kernel(RelativePositionBatch B,
                                                                          double* __restrict__ out1,
                                                                          double* __restrict__ out2) {
  const int lane = threadIdx.x & 63;
  const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (p >= B.num_pairs) return;
  const long long c0 = B.corr_ptr[p], c1 = B.corr_ptr[p + 1];
  for (int side = 0; side < 2; ++side) {
    const int v = side ? B.pair_view2[p] : B.pair_view1[p];
    const int model = B.view_model[v];
    const double* __restrict__ K = B.view_intr + (size_t)10 * v;  // zero padded
    const double* __restrict__ in = side ? B.feat2 : B.feat1;
    double* __restrict__ out = side ? out2 : out1;
    for (long long i = c0 + lane; i < c1; i += 64) {
      const double px[2] = {in[2 * i], in[2 * i + 1]};
      double pt[3];
      pixel_to_camera(model, K, px, pt);
      out[2 * i] = pt[0] / pt[2];
      out[2 * i + 1] = pt[1] / pt[2];
    }
  }
}

__global__ __launch_bounds__(256) void relative_position_kernel(RelativePositionBatch B) {
  const int lane = threadIdx.x & 63;
  // (readfirstlane: the compiler cannot see that a wave's lanes share p; with it the pair's scalars load into SGPRs)
  const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (p >= B.num_pairs) return;
  const long long c0 = B.corr_ptr[p], n = B.corr_ptr[p + 1] - c0;
  if (n <= 0) {
    if (lane == 0) {
      B.status[p] = -1;
      B.iters[p] = 0;
      B.cost[p] = 0.0;
      B.in_front[p] = 0;
    }
    return;
  }
  const int v1 = B.pair_view1[p], v2 = B.pair_view2[p];
  const double* __restrict__ f1 = B.feat1 + 2 * c0;
  const double* __restrict__ f2 = B.feat2 + 2 * c0;
  double R1[9], R2[9];  // column-major
  {
    const double aa1[3] = {B.view_rot[(size_t)3 * v1], B.view_rot[(size_t)3 * v1 + 1], B.view_rot[(size_t)3 * v1 + 2]};
    const double aa2[3] = {B.view_rot[(size_t)3 * v2], B.view_rot[(size_t)3 * v2 + 1], B.view_rot[(size_t)3 * v2 + 2]};
    angle_axis_to_rotation_matrix(aa1, R1);
    angle_axis_to_rotation_matrix(aa2, R2);
  }

  // ---- phase 1: the constraint columns ----
  const long long soff = B.scratch_ptr[p];
  const bool stream = soff >= 0;  // wave-uniform
  double* __restrict__ px = B.scratch + soff;
  double* __restrict__ py = px + B.scratch_len;
  double* __restrict__ pz = py + B.scratch_len;
  double C[kRelPosRegColumns][3];
#pragma unroll
  for (int k = 0; k < kRelPosRegColumns; ++k) C[k][0] = C[k][1] = C[k][2] = 0.0;
  const int nk = (int)((n + 63) >> 6);  // columns of the busiest lane
  // a run-time loop around one copy of the column code; the selects keep C in registers.  Columns past n stay 0:
  // they add +0 to every sum.
  for (int k = 0; k < nk; ++k) {
    const long long i = lane + 64 * (long long)k;
    double c[3] = {0.0, 0.0, 0.0};
    if (i < n) {
      const double h1[2] = {f1[2 * i], f1[2 * i + 1]}, h2[2] = {f2[2 * i], f2[2 * i + 1]};
      double a[3], b[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        a[j] = R1[3 * j] * h1[0] + R1[3 * j + 1] * h1[1] + R1[3 * j + 2];  // R1^T [f1; 1]
        b[j] = R2[3 * j] * h2[0] + R2[3 * j + 1] * h2[1] + R2[3 * j + 2];  // R2^T [f2; 1]
      }
      const double x[3] = {b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]};
#pragma unroll
      for (int r = 0; r < 3; ++r) c[r] = R1[r] * x[0] + R1[3 + r] * x[1] + R1[6 + r] * x[2];
      if (stream) {
        px[i] = c[0];
        py[i] = c[1];
        pz[i] = c[2];
      }
    }
    if (!stream) {
#pragma unroll
      for (int kk = 0; kk < kRelPosRegColumns; ++kk)
        if (kk == k) C[kk][0] = c[0], C[kk][1] = c[1], C[kk][2] = c[2];
    }
  }

  // ---- phase 2: IRLS ----
  double t[3] = {0.0, 0.0, 0.0}, M[6], cost = 0.0;
  int inner = 0, iter = 0, status = 1;
  bool first = true;
  for (;;) {
    double Ma[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ca = 0.0;
    if (stream) {
      for (long long i = lane; i < n; i += 64) relpos::accumulate(first, t, px[i], py[i], pz[i], Ma, ca);
    } else {
#pragma unroll
      for (int k = 0; k < kRelPosRegColumns; ++k)
        if (k < nk) relpos::accumulate(first, t, C[k][0], C[k][1], C[k][2], Ma, ca);
    }
    const double new_cost = wave_sum(ca);
    if (!first) {
      const double delta = fmax(fabs(cost - new_cost), 1.0 - (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]));
      inner = (delta <= kRelPosTolerance) ? inner + 1 : 0;
      cost = new_cost;
      if (inner >= kRelPosMaxInnerIterations) status = 0;
      if (iter >= kRelPosMaxIterations || inner >= kRelPosMaxInnerIterations) break;
    }
    first = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) M[i] = wave_sum(Ma[i]);
    double tn[3];
    relpos::smallest_eigenvector(M, tn);
    const double chk = (M[0] + M[1] + M[2] + M[3] + M[4] + M[5]) + (tn[0] + tn[1] + tn[2]);
    if (!(fabs(chk) <= 1.7976931348623157e308)) {  // a non-finite M or t
      status = 2;
      break;
    }
    t[0] = tn[0], t[1] = tn[1], t[2] = tn[2];
    ++iter;
  }

  // ---- phase 3: the sign ----
  int front = 0;
  if (status != 2) {
    double R[9];  // R = R2 R1^T, column-major
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[r + 3 * c] = R2[r] * R1[c] + R2[r + 3] * R1[c + 3] + R2[r + 6] * R1[c + 6];
    double fp = 0.0, fm = 0.0;
    for (long long i = lane; i < n; i += 64) {
      const double d1[3] = {f1[2 * i], f1[2 * i + 1], 1.0}, h2[2] = {f2[2 * i], f2[2 * i + 1]};
      double d2[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) d2[k] = R[3 * k] * h2[0] + R[3 * k + 1] * h2[1] + R[3 * k + 2];  // R^T [f2; 1]
      const double s1 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
      const double s2 = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
      const double s12 = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
      const double t1 = d1[0] * t[0] + d1[1] * t[1] + d1[2] * t[2];
      const double t2 = d2[0] * t[0] + d2[1] * t[1] + d2[2] * t[2];
      const double e1 = s2 * t1 - s12 * t2, e2 = s12 * t1 - s1 * t2;
      if (e1 > 0.0 && e2 > 0.0) fp += 1.0;
      if (e1 < 0.0 && e2 < 0.0) fm += 1.0;  // the same test at -t
    }
    const long long np = (long long)wave_sum(fp), nm = (long long)wave_sum(fm);
    front = (int)np;
    if (!(np > n / 2)) {
      t[0] = -t[0], t[1] = -t[1], t[2] = -t[2];
      front = (int)nm;
    }
  }
  if (lane != 0) return;
  B.status[p] = (signed char)status;
  B.iters[p] = iter;
  B.cost[p] = cost;
  B.in_front[p] = front;
  if (status != 2) {
    B.pos2[3 * (size_t)p] = t[0];
    B.pos2[3 * (size_t)p + 1] = t[1];
    B.pos2[3 * (size_t)p + 2] = t[2];
  }
}

}  // namespace tmi
