// theia::RobustRotationEstimator (robust_rotation_estimator.cc:66-282; Chatterjee and Govindu, ICCV 2013) on a view
// table and an edge list: global orientations from relative rotations by L1 minimisation (ADMM,
// math/l1_solver.h:120-178) followed by iteratively reweighted least squares.
//
// The reference's matrix A (:101-147) holds a -I3 block at view1 and a +I3 block at view2 of every edge, and the IRLS
// weights are one scalar per edge (:198-203), so A^T W A = L_w (x) I3 with L_w the weighted graph Laplacian without the
// fixed view's row and column: every linear solve of the algorithm is ONE symmetric positive definite system of order
// n = V - 1 with THREE right-hand sides (dense_cholesky.h: dense_cholesky_factor once for the L1 phase and once per
// IRLS iteration, dense_cholesky_substitute<3> per solve).  Vectors over the views are [n][3], over the edges [E][3].
// Free view v has column v - (v > fixed).
//
// rotation_residual_kernel   one thread per edge: r_e = MultiplyRotations(-o[view2], MultiplyRotations(rel_e, o[view1]))
//                            (:256-272), the IRLS weight sigma / (|r_e|^2 + sigma^2)^2 (:198-203) and the block's part
//                            of |r|^2.
// rotation_update_kernel     one thread per free view: o[v] = MultiplyRotations(o[v], step[v]) (:240-252) and the
//                            block's part of sum |step[v]| (:274-282).
// laplacian_assemble_kernel  one workgroup per row of L_w: the workgroup zero-fills the row, then one thread per entry
//                            of the row's list SORTED BY (NEIGHBOUR, EDGE) that starts a neighbour's run adds the run's
//                            weights in ascending edge index and stores minus the sum; the diagonal is the sum of the
//                            view's weights in ascending edge index (irls_rhs_kernel), or its degree with unit weights.
//                            No atomics; a row longer than the workgroup is strided.
// admm_view_kernel           one thread per free view, one walk of its row in ascending edge index for three sums:
//                            A^T (b + z - u) (the next x-update's right-hand side), A^T (z - z_old) and A^T u with the
//                            blocks' parts of their squared norms (l1_solver.h:140, :160-161, :166-168).
// admm_edge_kernel           one thread per edge: A x, the z and u updates (:147-156), z - z_old, and the blocks'
//                            parts of |A x - z - b|^2, |A x|^2 and |z|^2 (:159, :162-163).
// irls_rhs_kernel            one thread per free view: A^T W r and the view's weight sum (:206-216).
// The graph (PoseGraph), the sums (pg::block_sum, reduce_partials_kernel) and the ADMM row update (pg::admm_row) are
// pose_graph.h's.
//
// Every kernel is a plain grid launch; nothing waits on another workgroup.  The loops stay on the host
// (pose_graph_calls.h).
// The arithmetic written here is never contracted into FMA (#pragma clang fp contract(off) in every body), so a CPU
// model that evaluates the same expressions in the same order sees the same roundings.
#pragma once
#include <hip/hip_runtime.h>

#include "pose_graph.h"
#include "track_estimate_kernels.h"

namespace tmi {

constexpr int kRotationMaxOrder = 11000;  // n = V - 1: the dense matrix is 8 n^2 bytes = 968 MB

namespace rot {

// the branch of RotationMatrixToQuaternion for a negative trace, on the largest diagonal entry I (a template: a
// dynamically indexed array would go to scratch)
template <int I>
__device__ __forceinline__ void quaternion_from_diagonal(const double R[9], double q[4]) {
#pragma clang fp contract(off)
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  double t = sqrt(R[4 * I] - R[4 * J] - R[4 * K] + 1.0);
  q[I + 1] = 0.5 * t;
  t = 0.5 / t;
  q[0] = (R[K + 3 * J] - R[J + 3 * K]) * t;
  q[J + 1] = (R[J + 3 * I] + R[I + 3 * J]) * t;
  q[K + 1] = (R[K + 3 * I] + R[I + 3 * K]) * t;
}

// ceres::RotationMatrixToAngleAxis of Ceres 1.x: RotationMatrixToQuaternion on the trace or on the
// largest diagonal entry, then QuaternionToAngleAxis with its atan2 on (-sin, -cos) for a negative scalar part.
// R is column-major, R(r, c) = R[r + 3 c].
__device__ __forceinline__ void rotation_matrix_to_angle_axis(const double R[9], double aa[3]) {
#pragma clang fp contract(off)
  double q[4];
  const double trace = R[0] + R[4] + R[8];
  if (trace >= 0.0) {
    double t = sqrt(trace + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (R[2 + 3 * 1] - R[1 + 3 * 2]) * t;
    q[2] = (R[0 + 3 * 2] - R[2 + 3 * 0]) * t;
    q[3] = (R[1 + 3 * 0] - R[0 + 3 * 1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > (i ? R[4] : R[0])) i = 2;
    if (i == 0) {
      quaternion_from_diagonal<0>(R, q);
    } else if (i == 1) {
      quaternion_from_diagonal<1>(R, q);
    } else {
      quaternion_from_diagonal<2>(R, q);
    }
  }
  const double s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  double k = 2.0;
  if (s2 > 0.0) {
    const double s = sqrt(s2);
    const double c = q[0];
    const double two_theta = 2.0 * (c < 0.0 ? atan2(-s, -c) : atan2(s, c));
    k = two_theta / s;
  }
  aa[0] = q[1] * k;
  aa[1] = q[2] * k;
  aa[2] = q[3] * k;
}

// theia::MultiplyRotations (math/rotation.cc:122-132): the angle-axis of R(a) R(b)
__device__ __forceinline__ void multiply_rotations(const double a[3], const double b[3], double out[3]) {
#pragma clang fp contract(off)
  double Ra[9], Rb[9], P[9];
  angle_axis_to_rotation_matrix(a, Ra);
  angle_axis_to_rotation_matrix(b, Rb);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r + 3 * c] = (Ra[r] * Rb[3 * c] + Ra[r + 3] * Rb[3 * c + 1]) + Ra[r + 6] * Rb[3 * c + 2];
  rotation_matrix_to_angle_axis(P, out);
}

}  // namespace rot

__global__ __launch_bounds__(256) void rotation_residual_kernel(PoseGraph G, const double* __restrict__ o,
                                                                double sigma, double* __restrict__ r,
                                                                double* __restrict__ w, double* __restrict__ part_rr) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int e = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  if (e < G.num_pairs) {
    const int a = G.pair_view1[e], b = G.pair_view2[e];
    const double o1[3] = {o[3 * a], o[3 * a + 1], o[3 * a + 2]};
    const double m2[3] = {-o[3 * b], -o[3 * b + 1], -o[3 * b + 2]};
    const double rel[3] = {G.edge_value[3 * (size_t)e], G.edge_value[3 * (size_t)e + 1], G.edge_value[3 * (size_t)e + 2]};
    double t[3], res[3];
    rot::multiply_rotations(rel, o1, t);
    rot::multiply_rotations(m2, t, res);
    r[3 * (size_t)e] = res[0];
    r[3 * (size_t)e + 1] = res[1];
    r[3 * (size_t)e + 2] = res[2];
    sq = pg::sq3(res[0], res[1], res[2]);
    const double d = sq + sigma * sigma;
    w[e] = sigma / (d * d);
  }
  const double total = pg::block_sum(sq, part);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void rotation_update_kernel(int n, int fixed, const double* __restrict__ step,
                                                              double* __restrict__ o, double* __restrict__ part_step) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int c = blockIdx.x * 256 + threadIdx.x;
  double len = 0.0;
  if (c < n) {
    const int v = pg::view_of(c, fixed);
    const double cur[3] = {o[3 * v], o[3 * v + 1], o[3 * v + 2]};
    const double s[3] = {step[3 * c], step[3 * c + 1], step[3 * c + 2]};
    double next[3];
    rot::multiply_rotations(cur, s, next);
    o[3 * v] = next[0];
    o[3 * v + 1] = next[1];
    o[3 * v + 2] = next[2];
    len = sqrt(pg::sq3(s[0], s[1], s[2]));
  }
  const double total = pg::block_sum(len, part);
  if (threadIdx.x == 0) part_step[blockIdx.x] = total;
}

// blockIdx.x = the row (column index c).  w null: unit weights; diag null: the degree.
__global__ __launch_bounds__(256) void laplacian_assemble_kernel(PoseGraph G, int n, const double* __restrict__ w,
                                                                 const double* __restrict__ diag,
                                                                 double* __restrict__ A) {
#pragma clang fp contract(off)
  const int c = blockIdx.x;
  double* row = A + (size_t)c * n;
  for (int j = threadIdx.x; j < n; j += 256) row[j] = 0.0;
  __syncthreads();
  const int r0 = G.lap_ptr[c], r1 = G.lap_ptr[c + 1];
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const int2 ent = G.lap_row[r];
    if (r > r0 && G.lap_row[r - 1].x == ent.x) continue;  // not the first of its neighbour's run
    double sum = 0.0;
    for (int q = r; q < r1; ++q) {
      const int2 nxt = G.lap_row[q];
      if (nxt.x != ent.x) break;
      sum += w ? w[nxt.y] : 1.0;
    }
    row[ent.x] = -sum;  // (ent.x != c: no view pairs with itself; one thread per neighbour)
  }
  if (threadIdx.x == 0) {
    const int v = pg::view_of(c, G.fixed_view);
    row[c] = diag ? diag[c] : (double)(G.row_ptr[v + 1] - G.row_ptr[v]);
  }
}

// rhs [n][3] = A^T (b + z - u); part_s / part_t: the blocks' parts of |-rho A^T dz|^2 and |rho A^T u|^2
__global__ __launch_bounds__(256) void admm_view_kernel(PoseGraph G, int n, double rho, const double* __restrict__ b,
                                                        const double* __restrict__ z, const double* __restrict__ u,
                                                        const double* __restrict__ dz, double* __restrict__ rhs,
                                                        double* __restrict__ part_s, double* __restrict__ part_t) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int c = blockIdx.x * 256 + threadIdx.x;
  double ss = 0.0, tt = 0.0;
  if (c < n) {
    const int v = pg::view_of(c, G.fixed_view);
    double acc[3] = {0.0, 0.0, 0.0}, as[3] = {0.0, 0.0, 0.0}, at[3] = {0.0, 0.0, 0.0};
    const int r0 = G.row_ptr[v], r1 = G.row_ptr[v + 1];
    for (int r = r0; r < r1; ++r) {
      const int code = G.row[r].y;
      const size_t e3 = 3 * (size_t)(code >> 1);
      const double sign = (code & 1) ? 1.0 : -1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double uu = u[e3 + k];
        acc[k] += sign * ((b[e3 + k] + z[e3 + k]) - uu);
        as[k] += sign * dz[e3 + k];
        at[k] += sign * uu;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      rhs[3 * c + k] = acc[k];
      as[k] = -rho * as[k];
      at[k] = rho * at[k];
    }
    ss = pg::sq3(as[0], as[1], as[2]);
    tt = pg::sq3(at[0], at[1], at[2]);
  }
  const double s_total = pg::block_sum(ss, part);
  const double t_total = pg::block_sum(tt, part);
  if (threadIdx.x == 0) {
    part_s[blockIdx.x] = s_total;
    part_t[blockIdx.x] = t_total;
  }
}

// l1_solver.h:147-163 with the shrinkage by 1 / rho
__global__ __launch_bounds__(256) void admm_edge_kernel(PoseGraph G, double rho, double alpha,
                                                        const double* __restrict__ x, const double* __restrict__ b,
                                                        double* __restrict__ z, double* __restrict__ u,
                                                        double* __restrict__ dz, double* __restrict__ part_r,
                                                        double* __restrict__ part_ax, double* __restrict__ part_z) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int e = blockIdx.x * 256 + threadIdx.x;
  double rr = 0.0, aa = 0.0, zz = 0.0;
  if (e < G.num_pairs) {
    const int c1 = pg::column_of(G.pair_view1[e], G.fixed_view), c2 = pg::column_of(G.pair_view2[e], G.fixed_view);
    const double kappa = 1.0 / rho;
    double res[3], axv[3], zn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t i = 3 * (size_t)e + k;
      const double x1 = c1 >= 0 ? x[3 * c1 + k] : 0.0, x2 = c2 >= 0 ? x[3 * c2 + k] : 0.0;
      const double ax = x2 - x1;
      double zk = z[i], uk = u[i], dzk;
      pg::admm_row(ax, b[i], /*l1=*/true, alpha, kappa, zk, uk, dzk, res[k]);
      z[i] = zk;
      dz[i] = dzk;
      u[i] = uk;
      axv[k] = ax;
      zn[k] = zk;
    }
    rr = pg::sq3(res[0], res[1], res[2]);
    aa = pg::sq3(axv[0], axv[1], axv[2]);
    zz = pg::sq3(zn[0], zn[1], zn[2]);
  }
  const double r_total = pg::block_sum(rr, part);
  const double a_total = pg::block_sum(aa, part);
  const double z_total = pg::block_sum(zz, part);
  if (threadIdx.x == 0) {
    part_r[blockIdx.x] = r_total;
    part_ax[blockIdx.x] = a_total;
    part_z[blockIdx.x] = z_total;
  }
}

// rhs [n][3] = A^T W r, diag [n] = the view's weight sum, both in ascending edge index
__global__ __launch_bounds__(256) void irls_rhs_kernel(PoseGraph G, int n, const double* __restrict__ w,
                                                       const double* __restrict__ r, double* __restrict__ rhs,
                                                       double* __restrict__ diag) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int v = pg::view_of(c, G.fixed_view);
  double acc[3] = {0.0, 0.0, 0.0}, d = 0.0;
  const int r0 = G.row_ptr[v], r1 = G.row_ptr[v + 1];
  for (int q = r0; q < r1; ++q) {
    const int code = G.row[q].y;
    const int e = code >> 1;
    const double we = w[e];
    const double sw = (code & 1) ? we : -we;
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += sw * r[3 * (size_t)e + k];
    d += we;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) rhs[3 * c + k] = acc[k];
  diag[c] = d;
}

}  // namespace tmi
