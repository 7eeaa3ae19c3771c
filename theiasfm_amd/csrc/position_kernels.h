// theia::LeastUnsquaredDeviationPositionEstimator (least_unsquared_deviation_position_estimator.cc:75-212; Ozyesil and
// Singer, CVPR 2015) on a view table and an edge list: camera positions from global orientations and relative
// translation directions by the constrained L1 problem of math/constrained_l1_solver.cc:49-187 (ADMM).
//
// The unknowns are the positions of the n = V - 1 free views and one scale s_e per edge; the rows are
// p[view2] - p[view1] - s_e t_e per edge (L1) and s_e (>= 1 through b = 1 and the projection z >= 0).  With
// d_e = |t_e|^2 + 1 and W_e = I3 - t_e t_e^T / d_e, eliminating the scales from A^T A leaves S of order 3 n: the diagonal
// block of a view is the sum of W_e over its edges, block (view1, view2) of an edge is -W_e, the fixed view's rows and
// columns are absent.  S is fixed: dense_cholesky_factor once per call, dense_cholesky_substitute<1> per iteration on a
// vector laid out [n][3].  Free view v has column v - (v > fixed).  d_e is recomputed from t_e where it is used.
//
// lud_direction_kernel  one thread per edge: t_e = R(view_rotation[view1])^T position_2 (:56-63), R Ceres'
//                       AngleAxisToRotationMatrix.  Not launched without view_rotation: position_2 is t_e then.
// lud_assemble_kernel   one workgroup per free view for its three rows of S: the workgroup zero-fills them, then the
//                       thread that starts a neighbour's run in the list SORTED BY (NEIGHBOUR, EDGE) adds the run's W_e in
//                       ascending edge index and stores minus the sum (one writer per 3 x 3 block); threads 0..8 each add
//                       one entry of the diagonal block over the view's whole row in ascending edge index.  No atomics; a
//                       list longer than the workgroup is strided.
// lud_edge_kernel       one thread per edge: s_e = (q_s[e] + t_e . (p[view2] - p[view1])) / d_e, A x for the edge's four
//                       rows, the z and u updates (:141-150, the last row by max(., 0)), z - z_old, the block's parts of
//                       |A x - z - b|^2, |A x|^2 and |z|^2 (:153-155), the edge's scale entries of A^T (b + z - u),
//                       A^T (z - z_old) and A^T u, and the block's parts of the last two's squared norms.
// lud_view_kernel       one thread per free view, one walk of its row in ascending edge index: the position part of the
//                       three A^T products, the right-hand side of the next solve (q_p with t_e q_s[e] / d_e subtracted at
//                       view1 and added at view2) and the block's parts of the squared norms (:154, :158-160).
// Sums over the edges and the views: pg::block_sum and reduce_partials_kernel (pose_graph.h), a reduction of fixed
// shape.  The edges' and the views' parts of one norm lie side by side in one array and are reduced as one quantity.
//
// Every kernel is a plain grid launch; nothing waits on another workgroup.  The loop stays on the host (pose_graph_calls.h).
// The arithmetic written here is never contracted into FMA (#pragma clang fp contract(off) in every body), so a CPU
// model that evaluates the same expressions in the same order sees the same roundings.
#pragma once
#include <hip/hip_runtime.h>

#include "pose_graph.h"
#include "track_estimate_kernels.h"

namespace tmi {

namespace lud {

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// t_e and d_e = |t_e|^2 + 1
__device__ __forceinline__ double load_direction(const double* __restrict__ t, int e, double out[3]) {
#pragma clang fp contract(off)
  out[0] = t[3 * (size_t)e];
  out[1] = t[3 * (size_t)e + 1];
  out[2] = t[3 * (size_t)e + 2];
  return pg::sq3(out[0], out[1], out[2]) + 1.0;
}

// entry (i, j) of W_e
__device__ __forceinline__ double w_entry(const double t[3], double d, int i, int j) {
#pragma clang fp contract(off)
  return (i == j ? 1.0 : 0.0) - (t[i] * t[j]) / d;
}

}  // namespace lud

__global__ __launch_bounds__(256) void lud_direction_kernel(int E, const double* __restrict__ view_rotation,
                                                            const int* __restrict__ pair_view1,
                                                            const double* __restrict__ position2,
                                                            double* __restrict__ t) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int a = pair_view1[e];
  const double aa[3] = {view_rotation[3 * a], view_rotation[3 * a + 1], view_rotation[3 * a + 2]};
  const double p[3] = {position2[3 * (size_t)e], position2[3 * (size_t)e + 1], position2[3 * (size_t)e + 2]};
  double R[9];
  angle_axis_to_rotation_matrix(aa, R);
#pragma unroll
  for (int k = 0; k < 3; ++k) t[3 * (size_t)e + k] = (R[3 * k] * p[0] + R[3 * k + 1] * p[1]) + R[3 * k + 2] * p[2];
}

// blockIdx.x = the free view's column c; S is N x N row major, N = 3 n.
__global__ __launch_bounds__(256) void lud_assemble_kernel(PoseGraph G, int N, double* __restrict__ S) {
#pragma clang fp contract(off)
  const int c = blockIdx.x;
  double* rows = S + (size_t)3 * c * N;  // rows 3 c .. 3 c + 2 are contiguous
  for (size_t j = threadIdx.x; j < (size_t)3 * N; j += 256) rows[j] = 0.0;
  __syncthreads();
  const int r0 = G.lap_ptr[c], r1 = G.lap_ptr[c + 1];
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const int2 ent = G.lap_row[r];
    if (r > r0 && G.lap_row[r - 1].x == ent.x) continue;  // not the first of its neighbour's run
    double sum[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = r; q < r1; ++q) {
      const int2 nxt = G.lap_row[q];
      if (nxt.x != ent.x) break;
      double t[3];
      const double d = lud::load_direction(G.edge_value, nxt.y, t);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) sum[3 * i + j] += lud::w_entry(t, d, i, j);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) rows[(size_t)i * N + 3 * ent.x + j] = -sum[3 * i + j];  // (ent.x != c)
  }
  if (threadIdx.x < 9) {
    const int i = threadIdx.x / 3, j = threadIdx.x - 3 * i;
    const int v = pg::view_of(c, G.fixed_view);
    double sum = 0.0;
    for (int r = G.row_ptr[v]; r < G.row_ptr[v + 1]; ++r) {
      double t[3];
      const double d = lud::load_direction(G.edge_value, G.row[r].y >> 1, t);
      const double ti = i == 0 ? t[0] : (i == 1 ? t[1] : t[2]), tj = j == 0 ? t[0] : (j == 1 ? t[1] : t[2]);
      sum += (i == j ? 1.0 : 0.0) - (ti * tj) / d;  // (lud::w_entry on selects: a dynamic index would go to scratch)
    }
    rows[(size_t)i * N + 3 * c + j] = sum;
  }
}

// p [n][3] the solve's result, qs [E] the scale entries of A^T (b + z - u) it was solved for (overwritten by the next
// ones); z, u, dz [4 E]: rows 3 e + k, then 3 E + e.  scale [E] = s_e and ax [3 E] = the L1 rows of A x are the call's
// outputs after the last iteration.  part_s / part_t: the blocks' parts of the scale entries of |-rho A^T dz|^2 and
// |rho A^T u|^2.
__global__ __launch_bounds__(256) void lud_edge_kernel(PoseGraph G, double rho, double alpha,
                                                       const double* __restrict__ p, double* __restrict__ qs,
                                                       double* __restrict__ z, double* __restrict__ u,
                                                       double* __restrict__ dz, double* __restrict__ scale,
                                                       double* __restrict__ ax, double* __restrict__ part_r,
                                                       double* __restrict__ part_ax, double* __restrict__ part_z,
                                                       double* __restrict__ part_s, double* __restrict__ part_t) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int E = G.num_pairs;
  double rr = 0.0, aa = 0.0, zz = 0.0, ss = 0.0, tt = 0.0;
  if (e < E) {
    const int c1 = pg::column_of(G.pair_view1[e], G.fixed_view), c2 = pg::column_of(G.pair_view2[e], G.fixed_view);
    const double kappa = 1.0 / rho;
    double t[3], dp[3];
    const double d = lud::load_direction(G.edge_value, e, t);
#pragma unroll
    for (int k = 0; k < 3; ++k) dp[k] = (c2 >= 0 ? p[3 * c2 + k] : 0.0) - (c1 >= 0 ? p[3 * c1 + k] : 0.0);
    const double s = (qs[e] + lud::dot3(t, dp)) / d;
    double axv[3], zn[3], un[3], dzn[3], res[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t i = 3 * (size_t)e + k;
      axv[k] = dp[k] - s * t[k];
      zn[k] = z[i];
      un[k] = u[i];
      pg::admm_row(axv[k], 0.0, true, alpha, kappa, zn[k], un[k], dzn[k], res[k]);
      z[i] = zn[k];
      u[i] = un[k];
      dz[i] = dzn[k];
      ax[i] = axv[k];
      y[k] = (0.0 + zn[k]) - un[k];
    }
    const size_t i = 3 * (size_t)E + e;
    double zs = z[i], us = u[i], dzs, ress;
    pg::admm_row(s, 1.0, false, alpha, kappa, zs, us, dzs, ress);
    z[i] = zs;
    u[i] = us;
    dz[i] = dzs;
    scale[e] = s;
    qs[e] = ((1.0 + zs) - us) - lud::dot3(t, y);
    const double sd = -rho * (dzs - lud::dot3(t, dzn)), su = rho * (us - lud::dot3(t, un));
    rr = pg::sq3(res[0], res[1], res[2]) + ress * ress;
    aa = pg::sq3(axv[0], axv[1], axv[2]) + s * s;
    zz = pg::sq3(zn[0], zn[1], zn[2]) + zs * zs;
    ss = sd * sd;
    tt = su * su;
  }
  const double r_total = pg::block_sum(rr, part);
  const double a_total = pg::block_sum(aa, part);
  const double z_total = pg::block_sum(zz, part);
  const double s_total = pg::block_sum(ss, part);
  const double t_total = pg::block_sum(tt, part);
  if (threadIdx.x == 0) {
    part_r[blockIdx.x] = r_total;
    part_ax[blockIdx.x] = a_total;
    part_z[blockIdx.x] = z_total;
    part_s[blockIdx.x] = s_total;
    part_t[blockIdx.x] = t_total;
  }
}

// rhs [n][3] = the position part of A^T (b + z - u) with t_e q_s[e] / d_e subtracted at view1 and added at view2;
// part_s / part_t: the blocks' parts of the position entries of |-rho A^T dz|^2 and |rho A^T u|^2.
__global__ __launch_bounds__(256) void lud_view_kernel(PoseGraph G, int n, double rho, const double* __restrict__ qs,
                                                       const double* __restrict__ z, const double* __restrict__ u,
                                                       const double* __restrict__ dz, double* __restrict__ rhs,
                                                       double* __restrict__ part_s, double* __restrict__ part_t) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int c = blockIdx.x * 256 + threadIdx.x;
  double ss = 0.0, tt = 0.0;
  if (c < n) {
    const int v = pg::view_of(c, G.fixed_view);
    double acc[3] = {0.0, 0.0, 0.0}, sch[3] = {0.0, 0.0, 0.0}, as[3] = {0.0, 0.0, 0.0}, at[3] = {0.0, 0.0, 0.0};
    const int r0 = G.row_ptr[v], r1 = G.row_ptr[v + 1];
    for (int r = r0; r < r1; ++r) {
      const int code = G.row[r].y;
      const int e = code >> 1;
      const size_t e3 = 3 * (size_t)e;
      const double sign = (code & 1) ? 1.0 : -1.0;
      double t[3];
      const double d = lud::load_direction(G.edge_value, e, t);
      const double g = qs[e] / d;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double uu = u[e3 + k];
        acc[k] += sign * ((0.0 + z[e3 + k]) - uu);
        sch[k] += sign * (t[k] * g);
        as[k] += sign * dz[e3 + k];
        at[k] += sign * uu;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      rhs[3 * c + k] = acc[k] + sch[k];
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

}  // namespace tmi
