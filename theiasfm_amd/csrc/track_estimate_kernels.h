// Batched TrackEstimator::EstimateTrack (estimate_track.cc:205-264) on the resident
// track-major SELL-64 layout (kernels.h track_map: thread per track, 16 or 64 lanes per
// track on the long slices).  Three launches, each over the attempted tracks only:
//
//   track_rays_kernel         every observation's viewing ray, once:
//                             Camera::PixelToUnitDepthRay(pixel).normalized()
//                             (camera.cc:215-223, estimate_track.cc:75-76) into a
//                             per-observation scratch buffer [3 x slot]
//   track_triangulate_kernel  SufficientTriangulationAngle (triangulation.cc:236-250) on
//                             those rays, then TriangulateMidpoint (triangulation.cc:130-157)
//   (track_lm_kernel)         BundleAdjustTrack on the tracks still at status 0 (track_kernels.h)
//   track_accept_kernel       AcceptableReprojectionError (estimate_track.cc:90-115)
//
// Status per padded track: -1 not attempted, 0 estimated, 1 too few views or insufficient
// angle, 2 triangulation failed, 3 track BA failed, 4 bad reprojection.  The point is
// written by the triangulation (statuses 0, 3, 4 from then on) and by the track BA.
#pragma once
#include <hip/hip_runtime.h>

#include "camera_models.h"
#include "device_view.h"
#include "kernels.h"

namespace tmi {

// ceres::AngleAxisToRotationMatrix (Ceres 1.x rotation.h), column-major R(r, c) = R[r + 3 c],
// with its first-order branch at theta^2 <= DBL_EPSILON (Camera::GetOrientationAsRotationMatrix,
// camera.cc:254).  Not AngleAxisRotatePoint: the expressions (and so the rounding) differ.
__device__ __forceinline__ void angle_axis_to_rotation_matrix(const double aa[3], double R[9]) {
  const double theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (theta2 > kDblEpsilon) {
    const double theta = sqrt(theta2);
    const double wx = aa[0] / theta, wy = aa[1] / theta, wz = aa[2] / theta;
    const double c = cos(theta), s = sin(theta);
    const double omc = 1.0 - c;
    R[0] = c + wx * wx * omc;
    R[1] = wz * s + wx * wy * omc;
    R[2] = -wy * s + wx * wz * omc;
    R[3] = wx * wy * omc - wz * s;
    R[4] = c + wy * wy * omc;
    R[5] = wx * s + wy * wz * omc;
    R[6] = wy * s + wx * wz * omc;
    R[7] = -wx * s + wy * wz * omc;
    R[8] = c + wz * wz * omc;
  } else {
    R[0] = 1.0;
    R[1] = aa[2];
    R[2] = -aa[1];
    R[3] = -aa[2];
    R[4] = 1.0;
    R[5] = aa[0];
    R[6] = aa[1];
    R[7] = -aa[0];
    R[8] = 1.0;
  }
}

// UndistortPoint of the three iterative models (pinhole_camera_model.h:259-296,
// pinhole_radial_tangential_camera_model.h:293-355, fisheye_camera_model.h:269-335):
// at most 100 fixed-point steps, stopping once both coordinates move by less than 1e-10.
// Same expressions as oracle/ba_oracle.c undistort_iterative.
__device__ __forceinline__ void undistort_iterative(int model, const double* K, const double d[2], double u[2]) {
  u[0] = d[0];
  u[1] = d[1];
  for (int it = 0; it < 100; ++it) {
    const double p0 = u[0], p1 = u[1];
    const double r_sq = u[0] * u[0] + u[1] * u[1];
    if (model == 0) {
      const double dd = 1.0 + r_sq * (K[5] + K[6] * r_sq);
      u[0] = d[0] / dd;
      u[1] = d[1] / dd;
    } else if (model == 1) {
      const double rd = 1.0 + K[5] * r_sq + K[6] * r_sq * r_sq + K[7] * r_sq * r_sq * r_sq;
      const double tx = K[9] * (r_sq + 2.0 * u[0] * u[0]) + 2.0 * K[8] * u[0] * u[1];
      const double ty = K[8] * (r_sq + 2.0 * u[1] * u[1]) + 2.0 * K[9] * u[0] * u[1];
      u[0] = (d[0] - tx) / rd;
      u[1] = (d[1] - ty) / rd;
    } else {
      const double r = sqrt(r_sq);
      if (r < 1e-8) {
        u[0] = d[0];
        u[1] = d[1];
        return;
      }
      const double theta = atan2(r, 1.0);
      const double t2 = theta * theta;
      const double theta_d = theta * (1.0 + K[5] * t2 + K[6] * t2 * t2 + K[7] * t2 * t2 * t2 + K[8] * t2 * t2 * t2 * t2);
      u[0] = r * d[0] / theta_d;
      u[1] = r * d[1] / theta_d;
    }
    if (fabs(u[0] - p0) < 1e-10 && fabs(u[1] - p1) < 1e-10) break;
  }
}

// PixelToCameraCoordinates of the five models (intrinsics layouts of camera_models.h): the
// undistorted point on the z = 1 plane.  FOV (fov_camera_model.h:262-306) and DIVISION
// (division_undistortion_camera_model.h:291-310) are closed form.  oracle_pixel_to_camera restates
// the same code on the CPU.
__device__ __forceinline__ void pixel_to_camera(int model, const double* K, const double px[2], double pt[3]) {
  double d[2];
  if (model <= 2) {
    const double fy = K[0] * K[1];
    d[1] = (px[1] - K[4]) / fy;
    d[0] = (px[0] - K[3] - d[1] * K[2]) / K[0];
    double u[2];
    undistort_iterative(model, K, d, u);
    pt[0] = u[0];
    pt[1] = u[1];
  } else if (model == 3) {
    const double fy = K[0] * K[1];
    d[0] = (px[0] - K[2]) / K[0];
    d[1] = (px[1] - K[3]) / fy;
    const double omega = K[4];
    const double r_d_sq = d[0] * d[0] + d[1] * d[1];
    double r_u;
    if (omega < 1e-3) {
      r_u = (omega * omega * r_d_sq) / 3.0 - omega * omega / 12.0 + 1.0;
    } else if (r_d_sq < 1e-3) {
      r_u = (omega * (omega * omega * r_d_sq + 3.0)) / (6.0 * tan(omega / 2.0));
    } else {
      const double r_d = sqrt(r_d_sq);
      r_u = tan(r_d * omega) / (2.0 * r_d * tan(omega / 2.0));
    }
    pt[0] = r_u * d[0];
    pt[1] = r_u * d[1];
  } else {
    const double fy = K[0] * K[1];
    d[0] = px[0] - K[2];
    d[1] = px[1] - K[3];
    const double r_d_sq = d[0] * d[0] + d[1] * d[1];
    const double undistortion = 1.0 / (1.0 + K[4] * r_d_sq);
    pt[0] = d[0] * undistortion / K[0];
    pt[1] = d[1] * undistortion / fy;
  }
  pt[2] = 1.0;
}

// Camera::PixelToUnitDepthRay(pixel).normalized() (camera.cc:215-223): R^T PixelToCameraCoordinates(pixel), R
// column-major as angle_axis_to_rotation_matrix writes it, normalized as Eigen's normalized() does (divided by the
// norm when the squared norm is positive).
__device__ __forceinline__ void pixel_unit_ray(int model, const double* K, const double R[9], const double px[2],
                                               double r[3]) {
  double u[3];
  pixel_to_camera(model, K, px, u);
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] = R[3 * c] * u[0] + R[3 * c + 1] * u[1] + R[3 * c + 2] * u[2];  // R^T u
  const double n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  if (n2 > 0.0) {
    const double n = sqrt(n2);
    r[0] /= n;
    r[1] /= n;
    r[2] /= n;
  }
}

// One ray of TriangulateMidpoint (triangulation.cc:130-157): A += I - d d^T (lower triangle 00 10 11 20 21 22),
// b += (I - d d^T) o.  The w row of the 4 x 4 homogeneous form (d_w = 0) adds 1 to A_ww and b_w: the ray count.
__device__ __forceinline__ void midpoint_accumulate(const double d[3], const double o[3], double A[6], double b[3]) {
  double T[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) T[r][c] = (r == c ? 1.0 : 0.0) - d[r] * d[c];
  A[0] += T[0][0];
  A[1] += T[1][0];
  A[2] += T[1][1];
  A[3] += T[2][0];
  A[4] += T[2][1];
  A[5] += T[2][2];
#pragma unroll
  for (int r = 0; r < 3; ++r) b[r] += T[r][0] * o[0] + T[r][1] * o[1] + T[r][2] * o[2];
}

// The solve of TriangulateMidpoint over n rays: Eigen's unblocked LLT of [[A, 0], [0, n]] in its column order
// (LLT.h llt_inplace::unblocked: pivot x = A_kk - |L_k,0:k|^2, failure where x <= 0) and the two triangular solves.
// A_w* = 0 and A_ww = n, so w = (n / sqrt n) / sqrt n: 1 up to round-off, as in the reference.  False: the LLT failed.
__device__ __forceinline__ bool midpoint_solve(const double A[6], const double b[3], double n, double X[4]) {
  double L00, L10, L11, L20, L21, L22, L33;
  bool ok = true;
  {
    double x = A[0];
    if (x <= 0.0) ok = false;
    L00 = sqrt(x);
    L10 = A[1] / L00;
    L20 = A[3] / L00;
    x = A[2] - L10 * L10;
    if (x <= 0.0) ok = false;
    L11 = sqrt(x);
    L21 = (A[4] - L20 * L10) / L11;
    x = A[5] - (L20 * L20 + L21 * L21);
    if (x <= 0.0) ok = false;
    L22 = sqrt(x);
    x = n;  // row w of L below the 3 x 3 block is zero
    if (x <= 0.0) ok = false;
    L33 = sqrt(x);
  }
  if (!ok) return false;
  // L y = b, L^T X = y
  const double y0 = b[0] / L00;
  const double y1 = (b[1] - y0 * L10) / L11;
  const double y2 = (b[2] - y0 * L20 - y1 * L21) / L22;
  const double y3 = n / L33;
  X[3] = y3 / L33;
  X[2] = y2 / L22;
  X[1] = (y1 - L21 * X[2]) / L11;
  X[0] = (y0 - (L10 * X[1] + L20 * X[2])) / L00;
  return true;
}

// attempt[lp]: the caller's mask on the padded track order (constant points are skipped here).
__device__ __forceinline__ bool track_attempted(const DeviceView& v, const unsigned char* __restrict__ attempt, int lp) {
  return attempt[lp] != 0 && !v.pt_const[lp];
}

// ray[3 e .. 3 e + 2] of observation slot e = R^T PixelToCameraCoordinates(pixel), normalized as Eigen's
// normalized() does (divided by the norm when the squared norm is positive).  The iterative undistortion is up
// to 100 steps: it runs once per observation here and the pair scan reads the stored rays.
__global__ __launch_bounds__(256) void track_rays_kernel(DeviceView v, const unsigned char* __restrict__ attempt,
                                                         double* __restrict__ ray) {
  const TrackMap tm = track_map(v);
  if (!tm.valid || tm.k == 0 || !track_attempted(v, attempt, tm.lp)) return;
  for (int j = tm.j0; j < tm.k; j += tm.jstep) {
    const size_t e = tm.base + (size_t)j * 64;
    const int cam = v.obs_cam[e];
    const int4 rec = v.cam_rec[cam];
    const double* Kp = v.intr + rec.y;
    double Kv[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) Kv[i] = (i < rec.z) ? Kp[i] : 0.0;
    const double aa[3] = {v.ext[(size_t)cam * 6 + 3], v.ext[(size_t)cam * 6 + 4], v.ext[(size_t)cam * 6 + 5]};
    double R[9];
    angle_axis_to_rotation_matrix(aa, R);
    const double px[2] = {v.obs_xy[2 * e], v.obs_xy[2 * e + 1]};
    double r[3];
    pixel_unit_ray(rec.x, Kv, R, px, r);
    ray[3 * e] = r[0];
    ray[3 * e + 1] = r[1];
    ray[3 * e + 2] = r[2];
  }
}

// Steps 1-4 of EstimateTrack.  status[lp] is written for every valid padded track; the point only on success.
//   A = sum (I - d d^T), b = sum (I - d d^T) [o; 1] over the 4 x 4 homogeneous form (d_w = 0), then Eigen's
//   unblocked LLT (LLT.h llt_inplace::unblocked: pivot x = A_kk - |L_k,0:k|^2, failure where x <= 0) and the two
//   triangular solves.  A_w* = 0 and A_ww = n, so w = (n / sqrt n) / sqrt n: 1 up to round-off, as in the reference.
__global__ __launch_bounds__(256) void track_triangulate_kernel(DeviceView v, const unsigned char* __restrict__ attempt,
                                                                const double* __restrict__ ray, double cos_min,
                                                                signed char* __restrict__ status) {
  const TrackMap tm = track_map(v);
  if (!tm.valid) return;
  const int lp = tm.lp;
  const int k = tm.k;
  if (k == 0 || !track_attempted(v, attempt, lp)) {  // padding, or not asked for (unobserved tracks have no slot)
    if (tm.leader) status[lp] = -1;
    return;
  }
  if (k < 2) {  // estimate_track.cc:224-230 (kMinNumObservationsForTriangulation)
    if (tm.leader) status[lp] = 1;
    return;
  }
  const size_t base = tm.base;
  // SufficientTriangulationAngle: some pair with dot < cos(min angle); lanes split the outer index
  double sufficient = 0.0;
  for (int i = tm.j0; i < k && sufficient == 0.0; i += tm.jstep) {
    const size_t ei = base + (size_t)i * 64;
    const double ri[3] = {ray[3 * ei], ray[3 * ei + 1], ray[3 * ei + 2]};
    for (int j = i + 1; j < k; ++j) {
      const size_t ej = base + (size_t)j * 64;
      if (ri[0] * ray[3 * ej] + ri[1] * ray[3 * ej + 1] + ri[2] * ray[3 * ej + 2] < cos_min) {
        sufficient = 1.0;
        break;
      }
    }
  }
  if (group_sum(sufficient, tm.wide) == 0.0) {
    if (tm.leader) status[lp] = 1;
    return;
  }
  // TriangulateMidpoint: the 3 x 3 block of A (lower triangle) and b[0:3]; A_ww = b_w = n
  double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // 00 10 11 20 21 22
  double b[3] = {0.0, 0.0, 0.0};
  for (int j = tm.j0; j < k; j += tm.jstep) {
    const size_t e = base + (size_t)j * 64;
    const int cam = v.obs_cam[e];
    const double d[3] = {ray[3 * e], ray[3 * e + 1], ray[3 * e + 2]};
    const double o[3] = {v.ext[(size_t)cam * 6], v.ext[(size_t)cam * 6 + 1], v.ext[(size_t)cam * 6 + 2]};
    midpoint_accumulate(d, o, A, b);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) A[i] = group_sum(A[i], tm.wide);
#pragma unroll
  for (int i = 0; i < 3; ++i) b[i] = group_sum(b[i], tm.wide);
  if (!tm.leader) return;
  double X[4];
  if (!midpoint_solve(A, b, (double)k, X)) {
    status[lp] = 2;
    return;
  }
  double* P = v.pts + (size_t)lp * 4;
  P[0] = X[0];
  P[1] = X[1];
  P[2] = X[2];
  P[3] = X[3];
  status[lp] = 0;
}

// Steps 5-6: tracks at status 0 after the triangulation.  term (NULL without the track BA): the track BA's
// termination, status 3 unless CONVERGENCE / NO_CONVERGENCE.  Then AcceptableReprojectionError: any
// Camera::ProjectPoint depth < 0, or a mean squared reprojection error not below max_sq, gives status 4.
__global__ __launch_bounds__(256) void track_accept_kernel(DeviceView v, double max_sq,
                                                           const signed char* __restrict__ term,
                                                           signed char* __restrict__ status) {
  const TrackMap tm = track_map(v);
  if (!tm.valid) return;
  const int lp = tm.lp;
  const int k = tm.k;
  if (k == 0 || status[lp] != 0) return;
  if (term && term[lp] != 0 && term[lp] != 1) {
    if (tm.leader) status[lp] = 3;
    return;
  }
  double X[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) X[i] = v.pts[(size_t)lp * 4 + i];
  double behind = 0.0, sum = 0.0;
  for (int j = tm.j0; j < k; j += tm.jstep) {
    const size_t e = tm.base + (size_t)j * 64;
    const int cam = v.obs_cam[e];
    const int4 rec = v.cam_rec[cam];
    const double* Kp = v.intr + rec.y;
    double Kv[10], E[6], px[2];
#pragma unroll
    for (int i = 0; i < 10; ++i) Kv[i] = (i < rec.z) ? Kp[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) E[i] = v.ext[(size_t)cam * 6 + i];
    if (project_point_depth(rec.x, E, Kv, X, px) < 0) {
      behind = 1.0;
      break;
    }
    const double dx = v.obs_xy[2 * e] - px[0], dy = v.obs_xy[2 * e + 1] - px[1];
    sum += dx * dx + dy * dy;
  }
  behind = group_sum(behind, tm.wide);
  sum = group_sum(sum, tm.wide);
  if (!tm.leader) return;
  if (behind > 0.0 || !(sum / (double)k < max_sq)) status[lp] = 4;
}

}  // namespace tmi
