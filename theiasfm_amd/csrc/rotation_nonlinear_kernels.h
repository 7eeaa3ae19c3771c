// theia::NonlinearRotationEstimator (nonlinear_rotation_estimator.cc:49-100) on the view table and edge list of the
// nonlinear position estimator (PoseGraph, pose_graph.h; G.edge_value holds the relative rotations): global orientations
// from relative rotations by Levenberg-Marquardt on r_e = RotationMatrixToAngleAxis(R2 R1^T Rrel^T)
// (pairwise_rotation_error.h:65-95, weight 1) under SoftLOneLoss with Ceres' corrector.
//
// The unknowns are the angle-axis rotations of the n free views, x laid out [n][3]; free view v has column
// pg::column_of(v, fixed).  G.fixed_view = G.num_views says that no view is held: every view has a column then.  The two
// halves of an edge's Jacobian, J1 with respect to x[view1] and J2 with respect to x[view2], are independent, so an edge
// leaves a record of 27 doubles in planes of E:
//    0.. 5  B11 = J1~^T J1~, upper triangle (00, 01, 02, 11, 12, 22)
//    6..11  B22 = J2~^T J2~, upper triangle
//   12..20  B12 = J1~^T J2~, row major
//   21..23  q1 = J1~^T r~        24..26  q2 = J2~^T r~
// The normal matrix has B11 / B22 in the diagonal block of view1 / view2, B12 in block (view1, view2) and its transpose in
// block (view2, view1); the gradient has q1 at view1 and q2 at view2.  nlr::RotationBlocks tells the shared
// nlp_scale_kernel and nlp_assemble_kernel (position_nonlinear_kernels.h) where these are; the damped copy, the
// factorisation, the step and the reductions are the position estimator's.
//
// nlr_edge_kernel<true>   one thread per edge: the three matrices, the residual and its 3 x 6 Jacobian by forward-mode
//                         dual numbers through Ceres' rotation code with every branch taken on the values (what Ceres'
//                         autodiff evaluates), the SoftLOne scaling, the record, the residual and the block's part of the
//                         cost.  R1 carries three derivatives (x[view1]) and R2 three (x[view2]); only the product
//                         R2 (Rrel R1)^T and what follows carry six, which keeps the kernel out of scratch.
// nlr_edge_kernel<false>  the residual alone at the candidate -- the same code on duals without derivatives, so the value
//                         has the same bits -- and from the records of the current linearisation the block's part of the
//                         model cost change -(s . q + (s^T B s) / 2), s the step over the edge's two views.
//
// Plain grid launches, no atomics, no expression contracted into FMA.  The host loop is normal_lm_solve
// (pose_graph_calls.h).
#pragma once
#include <hip/hip_runtime.h>

#include "pose_graph.h"
#include "position_nonlinear_kernels.h"

namespace tmi {
namespace nlr {

constexpr int kRecordPlanes = 27;

// a value and N derivatives; N = 0: the value alone
template <int N>
struct Dual {
  double a;
  double v[N > 0 ? N : 1];
};

template <int N>
__device__ __forceinline__ Dual<N> cst(double c) {
  Dual<N> r;
  r.a = c;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = 0.0;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator+(const Dual<N>& f, const Dual<N>& g) {
#pragma clang fp contract(off)
  Dual<N> r;
  r.a = f.a + g.a;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] + g.v[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(const Dual<N>& f, const Dual<N>& g) {
#pragma clang fp contract(off)
  Dual<N> r;
  r.a = f.a - g.a;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] - g.v[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(const Dual<N>& f) {
  Dual<N> r;
  r.a = -f.a;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = -f.v[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(const Dual<N>& f, const Dual<N>& g) {
#pragma clang fp contract(off)
  Dual<N> r;
  r.a = f.a * g.a;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = f.a * g.v[i] + f.v[i] * g.a;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(const Dual<N>& f, double c) {
#pragma clang fp contract(off)
  Dual<N> r;
  r.a = f.a * c;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * c;
  return r;
}
// Ceres' Jet division: by the inverse of g's value
template <int N>
__device__ __forceinline__ Dual<N> operator/(const Dual<N>& f, const Dual<N>& g) {
#pragma clang fp contract(off)
  Dual<N> r;
  const double gi = 1.0 / g.a;
  const double fr = f.a * gi;
  r.a = fr;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = (f.v[i] - fr * g.v[i]) * gi;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> dsqrt(const Dual<N>& f) {
#pragma clang fp contract(off)
  Dual<N> r;
  const double t = sqrt(f.a);
  const double s = 1.0 / (2.0 * t);
  r.a = t;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = f.v[i] * s;
  return r;
}
// atan2(g, f) as Ceres' Jet has it
template <int N>
__device__ __forceinline__ Dual<N> datan2(const Dual<N>& g, const Dual<N>& f) {
#pragma clang fp contract(off)
  Dual<N> r;
  const double tmp = 1.0 / (f.a * f.a + g.a * g.a);
  r.a = atan2(g.a, f.a);
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = tmp * (f.a * g.v[i] - g.a * f.v[i]);
  return r;
}

// ceres::AngleAxisToRotationMatrix (Ceres 1.x rotation.h) of x, the derivatives with respect to x itself; column-major,
// R(r, c) = R[r + 3 c].  Both branches as the Jets take them: theta^2 > epsilon on the value, else the first-order matrix
// (whose derivatives are not zero: the spanning tree's root starts at exactly 0).
template <int N>
__device__ __forceinline__ void angle_axis_to_rotation_matrix(const double x[3], Dual<N> R[9]) {
#pragma clang fp contract(off)
  Dual<N> aa[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    aa[k] = cst<N>(x[k]);
    if (k < N) aa[k].v[k] = 1.0;
  }
  const Dual<N> one = cst<N>(1.0);
  const Dual<N> theta2 = (aa[0] * aa[0] + aa[1] * aa[1]) + aa[2] * aa[2];
  if (theta2.a > kDblEpsilon) {
    const Dual<N> theta = dsqrt(theta2);
    const Dual<N> wx = aa[0] / theta, wy = aa[1] / theta, wz = aa[2] / theta;
    double sv, cv;
    sincos(theta.a, &sv, &cv);
    Dual<N> s, c;
    s.a = sv;
    c.a = cv;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      s.v[i] = cv * theta.v[i];
      c.v[i] = -(sv * theta.v[i]);
    }
    const Dual<N> omc = one - c;
    R[0] = c + wx * wx * omc;
    R[1] = wz * s + wx * wy * omc;
    R[2] = wx * wz * omc - wy * s;
    R[3] = wx * wy * omc - wz * s;
    R[4] = c + wy * wy * omc;
    R[5] = wx * s + wy * wz * omc;
    R[6] = wy * s + wx * wz * omc;
    R[7] = wy * wz * omc - wx * s;
    R[8] = c + wz * wz * omc;
  } else {
    R[0] = one;
    R[1] = aa[2];
    R[2] = -aa[1];
    R[3] = -aa[2];
    R[4] = one;
    R[5] = aa[0];
    R[6] = aa[1];
    R[7] = -aa[0];
    R[8] = one;
  }
}

// the branch of RotationMatrixToQuaternion for a negative trace on the largest diagonal entry I (rot::
// quaternion_from_diagonal on duals)
template <int I, int N>
__device__ __forceinline__ void quaternion_from_diagonal(const Dual<N> R[9], Dual<N> q[4]) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  const Dual<N> half = cst<N>(0.5);
  Dual<N> t = dsqrt(((R[4 * I] - R[4 * J]) - R[4 * K]) + cst<N>(1.0));
  q[I + 1] = half * t;
  t = half / t;
  q[0] = (R[K + 3 * J] - R[J + 3 * K]) * t;
  q[J + 1] = (R[J + 3 * I] + R[I + 3 * J]) * t;
  q[K + 1] = (R[K + 3 * I] + R[I + 3 * K]) * t;
}

// ceres::RotationMatrixToAngleAxis on duals: RotationMatrixToQuaternion on the trace or on the largest diagonal entry,
// then QuaternionToAngleAxis with its sin^2 > 0 / k = 2 branches and the atan2 on (-sin, -cos) for a negative scalar part.
template <int N>
__device__ __forceinline__ void rotation_matrix_to_angle_axis(const Dual<N> R[9], Dual<N> aa[3]) {
  Dual<N> q[4];
  const Dual<N> half = cst<N>(0.5);
  const Dual<N> trace = (R[0] + R[4]) + R[8];
  if (trace.a >= 0.0) {
    Dual<N> t = dsqrt(trace + cst<N>(1.0));
    q[0] = half * t;
    t = half / t;
    q[1] = (R[2 + 3 * 1] - R[1 + 3 * 2]) * t;
    q[2] = (R[0 + 3 * 2] - R[2 + 3 * 0]) * t;
    q[3] = (R[1 + 3 * 0] - R[0 + 3 * 1]) * t;
  } else {
    int i = 0;
    if (R[4].a > R[0].a) i = 1;
    if (R[8].a > (i ? R[4].a : R[0].a)) i = 2;
    if (i == 0) {
      quaternion_from_diagonal<0>(R, q);
    } else if (i == 1) {
      quaternion_from_diagonal<1>(R, q);
    } else {
      quaternion_from_diagonal<2>(R, q);
    }
  }
  const Dual<N> s2 = (q[1] * q[1] + q[2] * q[2]) + q[3] * q[3];
  Dual<N> k = cst<N>(2.0);
  if (s2.a > 0.0) {
    const Dual<N> s = dsqrt(s2);
    const Dual<N> two_theta = (q[0].a < 0.0 ? datan2(-s, -q[0]) : datan2(s, q[0])) * 2.0;
    k = two_theta / s;
  }
  aa[0] = q[1] * k;
  aa[1] = q[2] * k;
  aa[2] = q[3] * k;
}

// The residual of an edge at x1, x2 with relative rotation rel: err [3] with 2 * N3 derivatives, x1's first (N3 = 3), or
// the value alone (N3 = 0).
template <int N3>
__device__ __forceinline__ void pairwise_rotation_error(const double x1[3], const double x2[3], const double rel[3],
                                                        Dual<2 * N3> err[3]) {
#pragma clang fp contract(off)
  double Rrel[9];
  tmi::angle_axis_to_rotation_matrix(rel, Rrel);
  Dual<N3> A[9];  // Rrel R1
  {
    Dual<N3> R1[9];
    angle_axis_to_rotation_matrix<N3>(x1, R1);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r)
        A[r + 3 * c] = (R1[3 * c] * Rrel[r] + R1[3 * c + 1] * Rrel[r + 3]) + R1[3 * c + 2] * Rrel[r + 6];
  }
  Dual<N3> R2[9];
  angle_axis_to_rotation_matrix<N3>(x2, R2);
  // L = R2 A^T = R2 R1^T Rrel^T: L(r, c) = sum_k R2(r, k) A(c, k); the derivatives of A are x1's, those of R2 are x2's
  Dual<2 * N3> L[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      Dual<2 * N3>& l = L[r + 3 * c];
      l.a = (R2[r].a * A[c].a + R2[r + 3].a * A[c + 3].a) + R2[r + 6].a * A[c + 6].a;
#pragma unroll
      for (int i = 0; i < N3; ++i) {
        l.v[i] = (R2[r].a * A[c].v[i] + R2[r + 3].a * A[c + 3].v[i]) + R2[r + 6].a * A[c + 6].v[i];
        l.v[N3 + i] = (R2[r].v[i] * A[c].a + R2[r + 3].v[i] * A[c + 3].a) + R2[r + 6].v[i] * A[c + 6].a;
      }
    }
  rotation_matrix_to_angle_axis<2 * N3>(L, err);
}

// the rotation of view v in x [n][3]; a held view's is read from `held` (the caller's value; null for a step: 0)
__device__ __forceinline__ void load_rotation(const double* __restrict__ x, int v, int fixed,
                                              const double* __restrict__ held, double p[3]) {
  const int c = pg::column_of(v, fixed);
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = c >= 0 ? x[3 * c + k] : (held ? held[k] : 0.0);
}

// The policy of nlp_scale_kernel and nlp_assemble_kernel for the 27-plane record (see the top of the file).
struct RotationBlocks {
  static __device__ __forceinline__ double diag(const double* __restrict__ rec, size_t E, size_t e, bool row_is_view2,
                                                int i, int j) {
    return rec[(size_t)((row_is_view2 ? 6 : 0) + nlp::sym_plane(i, j)) * E + e];
  }
  // block (view1, view2) is B12, block (view2, view1) its transpose
  static __device__ __forceinline__ double off(const double* __restrict__ rec, size_t E, size_t e, bool row_is_view2,
                                               int i, int j) {
    return rec[(size_t)(12 + (row_is_view2 ? 3 * j + i : 3 * i + j)) * E + e];
  }
  static __device__ __forceinline__ double finish_off(double x) { return x; }
  static __device__ __forceinline__ double grad(const double* __restrict__ rec, size_t E, size_t e, bool row_is_view2,
                                                int k) {
    return rec[(size_t)((row_is_view2 ? 24 : 21) + k) * E + e];
  }
};

}  // namespace nlr

// RECORDS: x the point of the linearisation; rec [27][E], residual [3 E] and part_cost are written.
// otherwise: x the candidate, step [n][3] what led to it; part_cost and part_mcc are written, rec is read.
// held [3]: the rotation of the held view (not read where no view is held).
template <bool RECORDS>
__global__ __launch_bounds__(256) void nlr_edge_kernel(PoseGraph G, double width, const double* __restrict__ x,
                                                       const double* __restrict__ step,
                                                       const double* __restrict__ held, double* __restrict__ rec,
                                                       double* __restrict__ residual, double* __restrict__ part_cost,
                                                       double* __restrict__ part_mcc) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int e = blockIdx.x * 256 + threadIdx.x;
  const size_t E = (size_t)G.num_pairs;
  double cost = 0.0, mcc = 0.0;
  if (e < G.num_pairs) {
    const int v1 = G.pair_view1[e], v2 = G.pair_view2[e];
    double x1[3], x2[3], rel[3];
    nlr::load_rotation(x, v1, G.fixed_view, held, x1);
    nlr::load_rotation(x, v2, G.fixed_view, held, x2);
    lud::load_direction(G.edge_value, e, rel);
    constexpr int N3 = RECORDS ? 3 : 0;
    nlr::Dual<2 * N3> err[3];
    nlr::pairwise_rotation_error<N3>(x1, x2, rel, err);
    const double sq = pg::sq3(err[0].a, err[1].a, err[2].a);
    double rho[3];
    loss_eval(2, width, sq, rho);
    cost = 0.5 * rho[0];
    if (RECORDS) {
      // Ceres' corrector: SoftLOneLoss has rho'' < 0 everywhere, so the shortcut sqrt(rho') on both is all there is
      const double sqrt_rho1 = sqrt(rho[1]);
      double rt[3], J[3][6];  // J[k][0..2] = J1~ row k, J[k][3..5] = J2~ row k
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        rt[k] = sqrt_rho1 * err[k].a;
#pragma unroll
        for (int i = 0; i < 6; ++i) J[k][i] = sqrt_rho1 * err[k].v[RECORDS ? i : 0];
        residual[3 * (size_t)e + k] = err[k].a;
      }
      // B11 and B22, upper triangles; B12 in full; q1 and q2: sums over the residual's rows k = 0, 1, 2 in that order
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int plane = 6 * h;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = i; j < 3; ++j)
            rec[(size_t)(plane++) * E + e] =
                (J[0][3 * h + i] * J[0][3 * h + j] + J[1][3 * h + i] * J[1][3 * h + j]) + J[2][3 * h + i] * J[2][3 * h + j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
          rec[(size_t)(21 + 3 * h + i) * E + e] =
              (J[0][3 * h + i] * rt[0] + J[1][3 * h + i] * rt[1]) + J[2][3 * h + i] * rt[2];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          rec[(size_t)(12 + 3 * i + j) * E + e] = (J[0][i] * J[0][3 + j] + J[1][i] * J[1][3 + j]) + J[2][i] * J[2][3 + j];
    } else {
      double s[6];
      nlr::load_rotation(step, v1, G.fixed_view, nullptr, s);
      nlr::load_rotation(step, v2, G.fixed_view, nullptr, s + 3);
      // s . q and s^T B s = s1^T B11 s1 + 2 s1^T B12 s2 + s2^T B22 s2
      double sq_form = 0.0, lin = 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double* sh = s + 3 * h;
        const size_t p = (size_t)6 * h;
        const double B0 = rec[(p + 0) * E + e], B1 = rec[(p + 1) * E + e], B2 = rec[(p + 2) * E + e],
                     B3 = rec[(p + 3) * E + e], B4 = rec[(p + 4) * E + e], B5 = rec[(p + 5) * E + e];
        const double Bs[3] = {(B0 * sh[0] + B1 * sh[1]) + B2 * sh[2], (B1 * sh[0] + B3 * sh[1]) + B4 * sh[2],
                              (B2 * sh[0] + B4 * sh[1]) + B5 * sh[2]};
        sq_form += lud::dot3(sh, Bs);
        const double q[3] = {rec[(size_t)(21 + 3 * h) * E + e], rec[(size_t)(22 + 3 * h) * E + e],
                             rec[(size_t)(23 + 3 * h) * E + e]};
        lin += lud::dot3(sh, q);
      }
      double Cs[3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
        Cs[i] = (rec[(size_t)(12 + 3 * i) * E + e] * s[3] + rec[(size_t)(13 + 3 * i) * E + e] * s[4]) +
                rec[(size_t)(14 + 3 * i) * E + e] * s[5];
      sq_form += 2.0 * lud::dot3(s, Cs);
      mcc = -(lin + 0.5 * sq_form);
    }
  }
  const double cost_total = pg::block_sum(cost, part);
  if (threadIdx.x == 0) part_cost[blockIdx.x] = cost_total;
  if (!RECORDS) {
    const double mcc_total = pg::block_sum(mcc, part);
    if (threadIdx.x == 0) part_mcc[blockIdx.x] = mcc_total;
  }
}

}  // namespace tmi
