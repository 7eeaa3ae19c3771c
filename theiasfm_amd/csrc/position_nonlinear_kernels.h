// theia::NonlinearPositionEstimator (nonlinear_position_estimator.cc:86-214; Wilson and Snavely, ECCV 2014) on the view
// table and edge list of the LUD estimator (PoseGraph, pose_graph.h): camera positions from global
// orientations and relative translation directions by Levenberg-Marquardt on r_e = d / |d| - t_e, d = p[view2] - p[view1]
// (pairwise_translation_error.h:63-88), under HuberLoss with Ceres' corrector.
//
// The unknowns are the positions of the n = V - 1 free views, x laid out [n][3]; free view v has column v - (v > fixed).
// Per linearisation every edge leaves a record of nine doubles in planes of E -- the upper triangle of B_e = J~^T J~
// (00, 01, 02, 11, 12, 22) and q_e = J~^T r~ -- with J~ and r~ the corrected Jacobian with respect to p[view2] and the
// corrected residual; the Jacobian with respect to p[view1] is -J~.  The normal matrix M of order N = 3 n (row major,
// lower triangle) has +B_e in the diagonal blocks of both views and -B_e in block (view1, view2); the gradient has +q_e
// at view2 and -q_e at view1.  M is kept; every factorisation works on a damped copy (pose_graph_calls.h).
//
// nlp_edge_kernel<true>   one thread per edge: residual, both norm branches, both Huber branches, the record, the
//                         residual itself (an output of the call) and the block's part of the cost.
// nlp_edge_kernel<false>  the same evaluation at the candidate x + step without writing records: the block's parts of
//                         the candidate's cost and, from the records of the current linearisation, of the model cost
//                         change -(J~ step) . (r~ + J~ step / 2) = -(sd . q_e + (sd^T B_e sd) / 2), sd the step's
//                         difference over the edge.
// nlp_scale_kernel        one thread per free view: the three diagonal entries over the view's row in ascending edge
//                         index, scale = 1 / (1 + sqrt(.)) (Ceres' Jacobi scaling; once, from the first linearisation).
// nlp_assemble_kernel     one workgroup per free view for its three rows of M up to the diagonal: the workgroup zero-fills
//                         them, then the thread that starts a neighbour's run in the list SORTED BY (NEIGHBOUR, EDGE),
//                         for the neighbours of a smaller column only, adds the run's B_e in ascending edge index and
//                         stores minus the scaled sum (one writer per 3 x 3 block, each edge's block written once, in the
//                         triangle the factorisation reads); threads 0..5 each add one entry of the diagonal block's
//                         lower triangle over the view's whole row in ascending edge index and threads 6..8 one entry of
//                         the gradient.  A list longer than the workgroup is strided; a hub's row is walked by one thread.
// nlp_copy_lower_kernel   the lower triangle of M into the matrix that is factored, one workgroup per row.
// nlp_lm_diagonal_kernel  one thread per diagonal entry: A_ii + clamp(A_ii, lo, hi) / radius into the copy.
// nlp_step_kernel         one thread per entry: step = -(scale y), candidate = x + step, the block's parts of |step|^2
//                         and |candidate|^2.
// nlp_absmax_kernel       one workgroup: max |unscaled gradient| (a maximum does not depend on the order).
// Sums: pg::block_sum and reduce_partials_kernel (pose_graph.h), a reduction of fixed shape.
// nlp_scale_kernel and nlp_assemble_kernel are templates on a policy that says where an edge's record holds the entries
// of the blocks and of the gradient (nlp::PositionBlocks here: the walks, the orders and the arithmetic above); the
// nonlinear rotation estimator instantiates them, and uses the other kernels as they are, with nlr::RotationBlocks
// (rotation_nonlinear_kernels.h).  G.fixed_view = G.num_views means that no view is fixed (that estimator's case).
//
// Every kernel is a plain grid launch; nothing waits on another workgroup and no atomic is used.  The loop stays on the
// host (pose_graph_calls.h).  The arithmetic written here is never contracted into FMA (#pragma clang fp contract(off) in every
// body), so a CPU model that evaluates the same expressions in the same order sees the same roundings.
#pragma once
#include <hip/hip_runtime.h>

#include "pose_graph.h"
#include "position_kernels.h"

namespace tmi {
namespace nlp {

// plane of entry (i, j) of the symmetric B_e among 00, 01, 02, 11, 12, 22
__device__ __forceinline__ int sym_plane(int i, int j) {
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a == 0 ? b : (a == 1 ? 2 + b : 5);
}

// The edge at positions p1, p2 with direction t under HuberLoss(width): the residual r, the corrected residual rt, the
// six entries of the corrected (symmetric) Jacobian Jt with respect to p2, and rho(|r|^2).
__device__ __forceinline__ double evaluate(const double p1[3], const double p2[3], const double t[3], double width,
                                           double r[3], double rt[3], double Jt[6]) {
#pragma clang fp contract(off)
  const double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  double norm = sqrt(pg::sq3(d[0], d[1], d[2]));
  const bool small = norm < 1e-12;
  if (small) norm = 1.0;
  const double u[3] = {d[0] / norm, d[1] / norm, d[2] / norm};
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = u[k] - t[k];
  const double sq = pg::sq3(r[0], r[1], r[2]);
  double rho[3];
  loss_eval(1, width, sq, rho);
  // Ceres' corrector (corrector.cc) where |r|^2 = 0 or rho'' <= 0: sqrt(rho') on the residual and on the Jacobian.
  // HuberLoss has rho'' <= 0 on both branches, so the alpha of the other case never arises (theia_mi355_ba.h, step 4).
  const double sqrt_rho1 = sqrt(rho[1]);
  // J = (I - u u^T) / norm, I on the small-norm branch: symmetric, entries 00 01 02 11 12 22
  Jt[0] = sqrt_rho1 * (small ? 1.0 : (1.0 - u[0] * u[0]) / norm);
  Jt[1] = sqrt_rho1 * (small ? 0.0 : (0.0 - u[0] * u[1]) / norm);
  Jt[2] = sqrt_rho1 * (small ? 0.0 : (0.0 - u[0] * u[2]) / norm);
  Jt[3] = sqrt_rho1 * (small ? 1.0 : (1.0 - u[1] * u[1]) / norm);
  Jt[4] = sqrt_rho1 * (small ? 0.0 : (0.0 - u[1] * u[2]) / norm);
  Jt[5] = sqrt_rho1 * (small ? 1.0 : (1.0 - u[2] * u[2]) / norm);
#pragma unroll
  for (int k = 0; k < 3; ++k) rt[k] = sqrt_rho1 * r[k];
  return rho[0];
}

// the position of view v in x [n][3]; the fixed view is at 0
__device__ __forceinline__ void load_position(const double* __restrict__ x, int v, int fixed, double p[3]) {
  const int c = pg::column_of(v, fixed);
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = c >= 0 ? x[3 * c + k] : 0.0;
}

// What nlp_scale_kernel and nlp_assemble_kernel read from an edge's record, for this estimator: the Jacobian with respect
// to p[view1] is -J~, so one symmetric B_e serves the diagonal blocks of both views and, negated, the block between them.
// `row_is_view2`: the view whose rows are assembled is the edge's view2.  (nlr::RotationBlocks, rotation_nonlinear_kernels.h,
// is the other policy: two independent Jacobian halves.)
struct PositionBlocks {
  // entry (i, j) of the edge's part of the row view's diagonal block
  static __device__ __forceinline__ double diag(const double* __restrict__ rec, size_t E, size_t e, bool, int i, int j) {
    return rec[(size_t)sym_plane(i, j) * E + e];
  }
  // entry (i, j) of the edge's part of block (row view, neighbour), before finish_off
  static __device__ __forceinline__ double off(const double* __restrict__ rec, size_t E, size_t e, bool, int i, int j) {
    return rec[(size_t)sym_plane(i, j) * E + e];
  }
  static __device__ __forceinline__ double finish_off(double x) { return -x; }
  // entry k of the edge's part of the row view's gradient
  static __device__ __forceinline__ double grad(const double* __restrict__ rec, size_t E, size_t e, bool row_is_view2,
                                                int k) {
    const double q = rec[(size_t)(6 + k) * E + e];
    return row_is_view2 ? q : -q;
  }
};

}  // namespace nlp

// RECORDS: x the point of the linearisation; rec [9][E], residual [3 E] and part_cost are written.
// otherwise: x the candidate, step [n][3] what led to it; part_cost and part_mcc are written, rec is read.
template <bool RECORDS>
__global__ __launch_bounds__(256) void nlp_edge_kernel(PoseGraph G, double width, const double* __restrict__ x,
                                                       const double* __restrict__ step, double* __restrict__ rec,
                                                       double* __restrict__ residual, double* __restrict__ part_cost,
                                                       double* __restrict__ part_mcc) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int e = blockIdx.x * 256 + threadIdx.x;
  const size_t E = (size_t)G.num_pairs;
  double cost = 0.0, mcc = 0.0;
  if (e < G.num_pairs) {
    const int v1 = G.pair_view1[e], v2 = G.pair_view2[e];
    double p1[3], p2[3], t[3], r[3], rt[3], Jt[6];
    nlp::load_position(x, v1, G.fixed_view, p1);
    nlp::load_position(x, v2, G.fixed_view, p2);
    lud::load_direction(G.edge_value, e, t);
    cost = 0.5 * nlp::evaluate(p1, p2, t, width, r, rt, Jt);
    if (RECORDS) {
      // B = Jt^T Jt and q = Jt^T rt, Jt symmetric: rows (0 1 2), (1 3 4), (2 4 5)
      rec[0 * E + e] = (Jt[0] * Jt[0] + Jt[1] * Jt[1]) + Jt[2] * Jt[2];
      rec[1 * E + e] = (Jt[0] * Jt[1] + Jt[1] * Jt[3]) + Jt[2] * Jt[4];
      rec[2 * E + e] = (Jt[0] * Jt[2] + Jt[1] * Jt[4]) + Jt[2] * Jt[5];
      rec[3 * E + e] = (Jt[1] * Jt[1] + Jt[3] * Jt[3]) + Jt[4] * Jt[4];
      rec[4 * E + e] = (Jt[1] * Jt[2] + Jt[3] * Jt[4]) + Jt[4] * Jt[5];
      rec[5 * E + e] = (Jt[2] * Jt[2] + Jt[4] * Jt[4]) + Jt[5] * Jt[5];
      rec[6 * E + e] = (Jt[0] * rt[0] + Jt[1] * rt[1]) + Jt[2] * rt[2];
      rec[7 * E + e] = (Jt[1] * rt[0] + Jt[3] * rt[1]) + Jt[4] * rt[2];
      rec[8 * E + e] = (Jt[2] * rt[0] + Jt[4] * rt[1]) + Jt[5] * rt[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) residual[3 * (size_t)e + k] = r[k];
    } else {
      double s1[3], s2[3];
      nlp::load_position(step, v1, G.fixed_view, s1);
      nlp::load_position(step, v2, G.fixed_view, s2);
      const double sd[3] = {s2[0] - s1[0], s2[1] - s1[1], s2[2] - s1[2]};
      const double B0 = rec[0 * E + e], B1 = rec[1 * E + e], B2 = rec[2 * E + e], B3 = rec[3 * E + e],
                   B4 = rec[4 * E + e], B5 = rec[5 * E + e];
      const double q[3] = {rec[6 * E + e], rec[7 * E + e], rec[8 * E + e]};
      const double Bs[3] = {(B0 * sd[0] + B1 * sd[1]) + B2 * sd[2], (B1 * sd[0] + B3 * sd[1]) + B4 * sd[2],
                            (B2 * sd[0] + B4 * sd[1]) + B5 * sd[2]};
      mcc = -(lud::dot3(sd, q) + 0.5 * lud::dot3(sd, Bs));
    }
  }
  const double cost_total = pg::block_sum(cost, part);
  if (threadIdx.x == 0) part_cost[blockIdx.x] = cost_total;
  if (!RECORDS) {
    const double mcc_total = pg::block_sum(mcc, part);
    if (threadIdx.x == 0) part_mcc[blockIdx.x] = mcc_total;
  }
}

template <class Blocks>
__global__ __launch_bounds__(256) void nlp_scale_kernel(PoseGraph G, int n, const double* __restrict__ rec,
                                                        double* __restrict__ scale) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const size_t E = (size_t)G.num_pairs;
  const int v = pg::view_of(c, G.fixed_view);
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
  for (int r = G.row_ptr[v]; r < G.row_ptr[v + 1]; ++r) {
    const int code = G.row[r].y;
    const size_t e = (size_t)(code >> 1);
    d0 += Blocks::diag(rec, E, e, code & 1, 0, 0);
    d1 += Blocks::diag(rec, E, e, code & 1, 1, 1);
    d2 += Blocks::diag(rec, E, e, code & 1, 2, 2);
  }
  scale[3 * c] = 1.0 / (1.0 + sqrt(d0));
  scale[3 * c + 1] = 1.0 / (1.0 + sqrt(d1));
  scale[3 * c + 2] = 1.0 / (1.0 + sqrt(d2));
}

// blockIdx.x = the free view's column c; M is N x N row major, N = 3 n.  diag [N]: the scaled diagonal of M; g [N]: the
// scaled gradient; gabs [N]: |the unscaled gradient|.
template <class Blocks>
__global__ __launch_bounds__(256) void nlp_assemble_kernel(PoseGraph G, int N, const double* __restrict__ rec,
                                                           const double* __restrict__ scale, double* __restrict__ M,
                                                           double* __restrict__ diag, double* __restrict__ g,
                                                           double* __restrict__ gabs) {
#pragma clang fp contract(off)
  const int c = blockIdx.x;
  const size_t E = (size_t)G.num_pairs;
  const int width = 3 * c + 3;  // the rows' part up to the diagonal block
  double* rows = M + (size_t)3 * c * N;
  for (int j = threadIdx.x; j < 3 * width; j += 256) {
    const int i = j / width;
    rows[(size_t)i * N + (j - i * width)] = 0.0;
  }
  __syncthreads();
  const int r0 = G.lap_ptr[c], r1 = G.lap_ptr[c + 1];
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const int2 ent = G.lap_row[r];
    if (ent.x >= c) continue;                              // the other triangle
    if (r > r0 && G.lap_row[r - 1].x == ent.x) continue;  // not the first of its neighbour's run
    const int row_view = pg::view_of(c, G.fixed_view);
    double sum[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = r; q < r1; ++q) {
      const int2 nxt = G.lap_row[q];
      if (nxt.x != ent.x) break;
      const bool row_is_view2 = G.pair_view2[nxt.y] == row_view;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) sum[3 * i + j] += Blocks::off(rec, E, (size_t)nxt.y, row_is_view2, i, j);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        rows[(size_t)i * N + 3 * ent.x + j] = Blocks::finish_off((sum[3 * i + j] * scale[3 * c + i]) * scale[3 * ent.x + j]);
  }
  if (threadIdx.x < 9) {
    const int v = pg::view_of(c, G.fixed_view);
    const int row_begin = G.row_ptr[v], row_end = G.row_ptr[v + 1];
    if (threadIdx.x < 6) {
      // the lower triangle of the diagonal block: (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
      const int i = threadIdx.x < 1 ? 0 : (threadIdx.x < 3 ? 1 : 2);
      const int j = threadIdx.x - (i * (i + 1)) / 2;
      double sum = 0.0;
      for (int r = row_begin; r < row_end; ++r) {
        const int code = G.row[r].y;
        sum += Blocks::diag(rec, E, (size_t)(code >> 1), code & 1, i, j);
      }
      const double a = (sum * scale[3 * c + i]) * scale[3 * c + j];
      rows[(size_t)i * N + 3 * c + j] = a;
      if (i == j) diag[3 * c + i] = a;
    } else {
      const int k = threadIdx.x - 6;
      double sum = 0.0;
      for (int r = row_begin; r < row_end; ++r) {
        const int code = G.row[r].y;
        sum += Blocks::grad(rec, E, (size_t)(code >> 1), code & 1, k);
      }
      g[3 * c + k] = sum * scale[3 * c + k];
      gabs[3 * c + k] = fabs(sum);
    }
  }
}

// blockIdx.x = the row
__global__ __launch_bounds__(256) void nlp_copy_lower_kernel(int N, const double* __restrict__ M,
                                                             double* __restrict__ A) {
  const size_t base = (size_t)blockIdx.x * N;
  for (int j = threadIdx.x; j <= (int)blockIdx.x; j += 256) A[base + j] = M[base + j];
}

__global__ __launch_bounds__(256) void nlp_lm_diagonal_kernel(int N, const double* __restrict__ diag, double lo,
                                                              double hi, double radius, double* __restrict__ A) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double d = diag[i];
  A[(size_t)i * N + i] = d + fmin(fmax(d, lo), hi) / radius;
}

__global__ __launch_bounds__(256) void nlp_step_kernel(int N, const double* __restrict__ x,
                                                       const double* __restrict__ scale, const double* __restrict__ y,
                                                       double* __restrict__ step, double* __restrict__ cand,
                                                       double* __restrict__ part_step, double* __restrict__ part_x) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double ss = 0.0, xx = 0.0;
  if (i < N) {
    const double s = -(scale[i] * y[i]);
    const double xc = x[i] + s;
    step[i] = s;
    cand[i] = xc;
    ss = s * s;
    xx = xc * xc;
  }
  const double s_total = pg::block_sum(ss, part);
  const double x_total = pg::block_sum(xx, part);
  if (threadIdx.x == 0) {
    part_step[blockIdx.x] = s_total;
    part_x[blockIdx.x] = x_total;
  }
}

__global__ __launch_bounds__(256) void nlp_absmax_kernel(int N, const double* __restrict__ gabs,
                                                         double* __restrict__ out) {
  __shared__ double part[256];
  double m = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) m = fmax(m, gabs[i]);
  part[threadIdx.x] = m;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (threadIdx.x < half) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = part[0];
}

}  // namespace tmi
