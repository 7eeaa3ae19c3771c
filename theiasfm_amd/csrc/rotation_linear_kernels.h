// theia::LinearRotationEstimator (linear_rotation_estimator.cc:78-203; Martinec and Pajdla, CVPR 2007) on the view table
// and edge list of the other rotation estimators: global orientations as the three eigenvectors of the smallest
// eigenvalues of M = sum over the edges of [-R12 | I]^T [-R12 | I], a symmetric block graph Laplacian of order n = 3 V
// (degree * I3 on the diagonal, -R12^T at block (view1, view2), -R12 at block (view2, view1)).
//
// The reference asks Spectra for them by shift-invert Lanczos at sigma = 0.  Here: subspace (block inverse) iteration
// with Rayleigh-Ritz on a block of kBlock = 6 columns (the reference's ncv) through ONE dense factorisation of
// M + mu I (dense_cholesky.h), mu = relative_shift * the largest degree -- the shift leaves the eigenvectors where they
// are and makes the exactly singular noise-free matrix factorable.  Blocks over the rows are [n][6], row major.
//
// lin_edge_matrix_kernel  one thread per edge: Ceres' AngleAxisToRotationMatrix of rotation_2 (column major)
// lin_assemble_kernel     one workgroup per view: zero-fills the view's three rows of the dense matrix, then the threads
//                         stride over the view's edge row and each writes its neighbour's 3 x 3 block (a pair appears
//                         once, so a block has one writer and there is nothing to sum); the diagonal is the degree
//                         (an integer, exact in any order) plus mu.  A hub's row is no thread's serial loop.
// lin_start_kernel        Q[i][j] = 2 u - 1, u from word 6 i + j of the splitmix64 stream of `seed`
// lin_apply_kernel        Z = M Q straight from the edge rows, one thread per (view, column): degree * Q_v minus the
//                         sum over the view's edges in ascending edge index of R^T Q_nbr (view is view1) or R Q_nbr
// lin_mgs_kernel          step j of modified Gram-Schmidt on the six columns, on UNNORMALISED dots: launch j applies
//                         step j - 1 (q = y / sqrt(s_jj), y_k -= (s_jk / sqrt(s_jj)) q for the later columns) from the
//                         block parts of launch j - 1, which every workgroup sums itself in ascending block order, and
//                         writes the block parts of y_j . y_k, k >= j.  Seven launches a pass; the host runs two passes
//                         (the first block of the iteration is as ill-conditioned as 1 / relative_shift).
// lin_gram_kernel         the block parts of the upper triangle of T = Q^T Z (21 entries)
// lin_ritz_kernel         one thread: sums the parts in ascending block order, then the 6 x 6 symmetric eigenproblem by
//                         cyclic Jacobi -- kJacobiSweeps sweeps of the pairs (0,1) (0,2) ... (4,5) in that order, a pair
//                         with a zero off-diagonal entry skipped -- eigenvalues ascending (first of equals first), every
//                         Ritz vector signed so that its coefficient of largest magnitude (first of equals) is positive
// lin_rotate_kernel       Q = Y W, Z = Z W and the block parts of |Z_j - theta_j Q_j|^2 for the first three pairs
// lin_project_kernel      one thread per view: the view's 3 x 3 block of the first three columns to SO(3) as U V^T of
//                         a one-sided Jacobi SVD (Hestenes), negated where the determinant is negative
//                         (ProjectToRotationMatrix, pose/util.cc:121-133), then RotationMatrixToAngleAxis
//
// Every kernel is a plain grid launch, nothing waits on another workgroup, the loop is the host's
// (pose_graph_calls.h; the graph is pose_graph.h's PoseGraph with no view held).  No FMA contraction,
// no atomics, every sum of fixed shape: the same bits from call to call.
#pragma once
#include <hip/hip_runtime.h>

#include "pose_graph.h"
#include "ransac_core.h"
#include "rotation_kernels.h"

namespace tmi {
namespace lin {

constexpr int kBlock = 6;          // columns of the iteration block: the reference's ncv
constexpr int kGram = 21;          // upper triangle of a 6 x 6 matrix
constexpr int kJacobiSweeps = 12;  // of the 6 x 6 problem; convergence is quadratic and 6 sweeps reach rounding
constexpr int kSvdSweeps = 12;     // of the 3 x 3 one-sided Jacobi
// the doubles of the small result block: W [36] row major (column j the j-th Ritz vector), theta [6], residual^2 [3]
constexpr int kSmallW = 0, kSmallTheta = 36, kSmallResidual = 42, kSmallWords = 48;

// the sum over the workgroups of value k of parts [num_blocks][stride], ascending
__device__ __forceinline__ double sum_parts(const double* __restrict__ parts, int num_blocks, int stride, int k) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int b = 0; b < num_blocks; ++b) s += parts[(size_t)b * stride + k];
  return s;
}

// one Jacobi rotation of the symmetric 6 x 6 matrix A on the pair (P, Q), accumulated into the columns of W
template <int P, int Q>
__device__ __forceinline__ void jacobi_pair(double A[kBlock][kBlock], double W[kBlock][kBlock]) {
#pragma clang fp contract(off)
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double zeta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < kBlock; ++k) {  // columns P and Q
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq;
    A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < kBlock; ++k) {  // rows P and Q
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk;
    A[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < kBlock; ++k) {
    const double wkp = W[k][P], wkq = W[k][Q];
    W[k][P] = c * wkp - s * wkq;
    W[k][Q] = s * wkp + c * wkq;
  }
}

template <int P>
__device__ __forceinline__ void jacobi_row(double A[kBlock][kBlock], double W[kBlock][kBlock]) {
  if constexpr (P + 1 < kBlock) jacobi_pair<P, P + 1>(A, W);
  if constexpr (P + 2 < kBlock) jacobi_pair<P, P + 2>(A, W);
  if constexpr (P + 3 < kBlock) jacobi_pair<P, P + 3>(A, W);
  if constexpr (P + 4 < kBlock) jacobi_pair<P, P + 4>(A, W);
  if constexpr (P + 5 < kBlock) jacobi_pair<P, P + 5>(A, W);
}

// one one-sided Jacobi rotation of the columns (P, Q) of the 3 x 3 matrix A (A[c] is column c), accumulated into V
template <int P, int Q>
__device__ __forceinline__ void svd_pair(double A[3][3], double V[3][3]) {
#pragma clang fp contract(off)
  const double alpha = pg::sq3(A[P][0], A[P][1], A[P][2]);
  const double beta = pg::sq3(A[Q][0], A[Q][1], A[Q][2]);
  const double gamma = (A[P][0] * A[Q][0] + A[P][1] * A[Q][1]) + A[P][2] * A[Q][2];
  if (gamma == 0.0) return;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ap = A[P][k], aq = A[Q][k];
    A[P][k] = c * ap - s * aq;
    A[Q][k] = s * ap + c * aq;
    const double vp = V[P][k], vq = V[Q][k];
    V[P][k] = c * vp - s * vq;
    V[Q][k] = s * vp + c * vq;
  }
}

}  // namespace lin

__global__ __launch_bounds__(256) void lin_edge_matrix_kernel(int num_pairs, const double* __restrict__ rel,
                                                              double* __restrict__ R) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= num_pairs) return;
  const double aa[3] = {rel[3 * (size_t)e], rel[3 * (size_t)e + 1], rel[3 * (size_t)e + 2]};
  double M[9];
  angle_axis_to_rotation_matrix(aa, M);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[9 * (size_t)e + k] = M[k];
}

// blockIdx.x = the view; A [n][n], n = 3 V, receives M + mu I
__global__ __launch_bounds__(256) void lin_assemble_kernel(PoseGraph G, int n, double mu, double* __restrict__ A) {
#pragma clang fp contract(off)
  const int v = blockIdx.x;
  double* rows = A + (size_t)3 * v * n;
  for (size_t j = threadIdx.x; j < (size_t)3 * n; j += 256) rows[j] = 0.0;
  __syncthreads();
  const int r0 = G.row_ptr[v], r1 = G.row_ptr[v + 1];
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const int2 ent = G.row[r];
    const double* R = G.edge_value + 9 * (size_t)(ent.y >> 1);
    const bool second = ent.y & 1;
    // block (view1, view2) = -R^T, block (view2, view1) = -R; R(a, b) = R[a + 3 b]
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) rows[(size_t)a * n + 3 * ent.x + b] = -(second ? R[a + 3 * b] : R[b + 3 * a]);
  }
  if (threadIdx.x < 3) rows[(size_t)threadIdx.x * n + 3 * v + threadIdx.x] = (double)(r1 - r0) + mu;
}

__global__ __launch_bounds__(256) void lin_start_kernel(int n, unsigned long long seed, double* __restrict__ Q) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * lin::kBlock) return;
  const double u = ((double)(splitmix64_word(seed, (unsigned long long)i) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  Q[i] = 2.0 * u - 1.0;
}

// one thread per (view, column)
__global__ __launch_bounds__(256) void lin_apply_kernel(PoseGraph G, const double* __restrict__ Q,
                                                        double* __restrict__ Z) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= G.num_views * lin::kBlock) return;
  const int v = t / lin::kBlock, j = t - v * lin::kBlock;
  const int r0 = G.row_ptr[v], r1 = G.row_ptr[v + 1];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int r = r0; r < r1; ++r) {
    const int2 ent = G.row[r];
    const double* R = G.edge_value + 9 * (size_t)(ent.y >> 1);
    const bool second = ent.y & 1;
    const double* q = Q + (size_t)3 * ent.x * lin::kBlock + j;
    const double x0 = q[0], x1 = q[lin::kBlock], x2 = q[2 * lin::kBlock];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double m0 = second ? R[a] : R[3 * a], m1 = second ? R[a + 3] : R[3 * a + 1],
                   m2 = second ? R[a + 6] : R[3 * a + 2];
      acc[a] += (m0 * x0 + m1 * x1) + m2 * x2;
    }
  }
  const double deg = (double)(r1 - r0);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const size_t i = (size_t)(3 * v + a) * lin::kBlock + j;
    Z[i] = deg * Q[i] - acc[a];
  }
}

// launch j = 0 .. 6 of one pass over Y [n][6]; prev / next: block parts [num_blocks][6] of launch j - 1 / this one
__global__ __launch_bounds__(256) void lin_mgs_kernel(int n, int j, double* __restrict__ Y,
                                                      const double* __restrict__ prev, double* __restrict__ next) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  __shared__ double s[lin::kBlock];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double y[lin::kBlock];
#pragma unroll
  for (int k = 0; k < lin::kBlock; ++k) y[k] = i < n ? Y[(size_t)i * lin::kBlock + k] : 0.0;
  if (j > 0) {
    if (threadIdx.x < lin::kBlock) s[threadIdx.x] = lin::sum_parts(prev, gridDim.x, lin::kBlock, threadIdx.x);
    __syncthreads();
    // (static indices: a dynamically indexed y[] would go to scratch)
    double sjj = 0.0, yj = 0.0;
#pragma unroll
    for (int k = 0; k < lin::kBlock; ++k)
      if (k == j - 1) {
        sjj = s[k];
        yj = y[k];
      }
    const double inv = sjj > 0.0 ? 1.0 / sqrt(sjj) : 0.0;  // a column that vanished stays zero
    const double q = yj * inv;
#pragma unroll
    for (int k = 0; k < lin::kBlock; ++k) {
      if (k == j - 1) y[k] = q;
      if (k >= j) y[k] -= (s[k] * inv) * q;
    }
    if (i < n) {
#pragma unroll
      for (int k = 0; k < lin::kBlock; ++k)
        if (k >= j - 1) Y[(size_t)i * lin::kBlock + k] = y[k];
    }
  }
  if (j >= lin::kBlock) return;
  double yj = 0.0;
#pragma unroll
  for (int k = 0; k < lin::kBlock; ++k)
    if (k == j) yj = y[k];
#pragma unroll
  for (int k = 0; k < lin::kBlock; ++k) {
    const double total = pg::block_sum(k >= j ? yj * y[k] : 0.0, part);
    if (threadIdx.x == 0) next[(size_t)blockIdx.x * lin::kBlock + k] = total;
  }
}

// parts [num_blocks][21]: entry (a, b), a <= b, of Q^T Z at index a (11 - a) / 2 + b
__global__ __launch_bounds__(256) void lin_gram_kernel(int n, const double* __restrict__ Q,
                                                       const double* __restrict__ Z, double* __restrict__ parts) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double q[lin::kBlock], z[lin::kBlock];
#pragma unroll
  for (int k = 0; k < lin::kBlock; ++k) {
    q[k] = i < n ? Q[(size_t)i * lin::kBlock + k] : 0.0;
    z[k] = i < n ? Z[(size_t)i * lin::kBlock + k] : 0.0;
  }
  int at = 0;
#pragma unroll
  for (int a = 0; a < lin::kBlock; ++a)
#pragma unroll
    for (int b = a; b < lin::kBlock; ++b) {
      const double total = pg::block_sum(q[a] * z[b], part);
      if (threadIdx.x == 0) parts[(size_t)blockIdx.x * lin::kGram + at] = total;
      ++at;
    }
}

// one workgroup; small: see kSmallW
__global__ __launch_bounds__(64) void lin_ritz_kernel(const double* __restrict__ parts, int num_blocks,
                                                      double* __restrict__ small) {
#pragma clang fp contract(off)
  __shared__ double t[lin::kGram];
  if (threadIdx.x < lin::kGram) t[threadIdx.x] = lin::sum_parts(parts, num_blocks, lin::kGram, threadIdx.x);
  __syncthreads();
  if (threadIdx.x != 0) return;
  double A[lin::kBlock][lin::kBlock], W[lin::kBlock][lin::kBlock];
  int at = 0;
#pragma unroll
  for (int a = 0; a < lin::kBlock; ++a)
#pragma unroll
    for (int b = a; b < lin::kBlock; ++b) {
      A[a][b] = t[at];
      A[b][a] = t[at];
      ++at;
    }
#pragma unroll
  for (int a = 0; a < lin::kBlock; ++a)
#pragma unroll
    for (int b = 0; b < lin::kBlock; ++b) W[a][b] = a == b ? 1.0 : 0.0;
  for (int sweep = 0; sweep < lin::kJacobiSweeps; ++sweep) {
    lin::jacobi_row<0>(A, W);
    lin::jacobi_row<1>(A, W);
    lin::jacobi_row<2>(A, W);
    lin::jacobi_row<3>(A, W);
    lin::jacobi_row<4>(A, W);
  }
  // ascending eigenvalues, the first of equals first: column j's rank is the number of columns that go before it
#pragma unroll
  for (int j = 0; j < lin::kBlock; ++j) {
    int rank = 0;
#pragma unroll
    for (int k = 0; k < lin::kBlock; ++k) rank += (A[k][k] < A[j][j]) || (A[k][k] == A[j][j] && k < j);
    double big = 0.0, sign = 1.0;
#pragma unroll
    for (int k = 0; k < lin::kBlock; ++k)
      if (fabs(W[k][j]) > big) {
        big = fabs(W[k][j]);
        sign = W[k][j] < 0.0 ? -1.0 : 1.0;
      }
    small[lin::kSmallTheta + rank] = A[j][j];
#pragma unroll
    for (int k = 0; k < lin::kBlock; ++k) small[lin::kSmallW + k * lin::kBlock + rank] = sign * W[k][j];
  }
}

// Q = Y W, Z = Z W; res0 / res1 / res2 [num_blocks]: the block parts of |Z_j - theta_j Q_j|^2
__global__ __launch_bounds__(256) void lin_rotate_kernel(int n, const double* __restrict__ small,
                                                         const double* __restrict__ Y, double* __restrict__ Z,
                                                         double* __restrict__ Q, double* __restrict__ res0,
                                                         double* __restrict__ res1, double* __restrict__ res2) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  __shared__ double w[lin::kSmallResidual];
  if (threadIdx.x < lin::kSmallResidual) w[threadIdx.x] = small[threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  double y[lin::kBlock], z[lin::kBlock], r[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < lin::kBlock; ++k) {
    y[k] = i < n ? Y[(size_t)i * lin::kBlock + k] : 0.0;
    z[k] = i < n ? Z[(size_t)i * lin::kBlock + k] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < lin::kBlock; ++j) {
    double qj = 0.0, zj = 0.0;
#pragma unroll
    for (int k = 0; k < lin::kBlock; ++k) {
      qj += y[k] * w[lin::kSmallW + k * lin::kBlock + j];
      zj += z[k] * w[lin::kSmallW + k * lin::kBlock + j];
    }
    if (i < n) {
      Q[(size_t)i * lin::kBlock + j] = qj;
      Z[(size_t)i * lin::kBlock + j] = zj;
    }
    if (j < 3) {
      const double d = zj - w[lin::kSmallTheta + j] * qj;
      r[j] = d * d;
    }
  }
  const double t0 = pg::block_sum(r[0], part);
  const double t1 = pg::block_sum(r[1], part);
  const double t2 = pg::block_sum(r[2], part);
  if (threadIdx.x == 0) {
    res0[blockIdx.x] = t0;
    res1[blockIdx.x] = t1;
    res2[blockIdx.x] = t2;
  }
}

// one thread per view: rotation [3 V] angle-axis, reflected [V] 1 where the projection was negated
__global__ __launch_bounds__(256) void lin_project_kernel(int num_views, const double* __restrict__ Q,
                                                          double* __restrict__ rotation, int* __restrict__ reflected) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= num_views) return;
  // A[c] = column c of the view's block B (B(r, c) = Q[3 v + r][c]); B V = U Sigma at the end
  double A[3][3], V[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      A[c][r] = Q[(size_t)(3 * v + r) * lin::kBlock + c];
      V[c][r] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < lin::kSvdSweeps; ++sweep) {
    lin::svd_pair<0, 1>(A, V);
    lin::svd_pair<0, 2>(A, V);
    lin::svd_pair<1, 2>(A, V);
  }
  double sigma[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sigma[c] = sqrt(pg::sq3(A[c][0], A[c][1], A[c][2]));
    const double inv = sigma[c] > 0.0 ? 1.0 / sigma[c] : 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) A[c][r] *= inv;  // A[c] = u_c
  }
  // a block of rank two: the missing left vector is the cross product of the other two, so that U stays orthogonal
  // (its sign is free, as the reference's SVD leaves it; the determinant test below settles the result's)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int a = (c + 1) % 3, b = (c + 2) % 3;
    if (!(sigma[c] > 0.0) && sigma[a] > 0.0 && sigma[b] > 0.0) {
      A[c][0] = A[a][1] * A[b][2] - A[a][2] * A[b][1];
      A[c][1] = A[a][2] * A[b][0] - A[a][0] * A[b][2];
      A[c][2] = A[a][0] * A[b][1] - A[a][1] * A[b][0];
    }
  }
  // R = U V^T, column major R(r, c) = R[r + 3 c] = sum_k u_k[r] v_k[c]
  double R[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) R[r + 3 * c] = (A[0][r] * V[0][c] + A[1][r] * V[1][c]) + A[2][r] * V[2][c];
  const double det = (R[0] * (R[4] * R[8] - R[7] * R[5]) - R[3] * (R[1] * R[8] - R[7] * R[2])) +
                     R[6] * (R[1] * R[5] - R[4] * R[2]);
  const int negate = det < 0.0;
  if (negate) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = -R[k];
  }
  double aa[3];
  rot::rotation_matrix_to_angle_axis(R, aa);
  rotation[3 * (size_t)v] = aa[0];
  rotation[3 * (size_t)v + 1] = aa[1];
  rotation[3 * (size_t)v + 2] = aa[2];
  reflected[v] = negate;
}

}  // namespace tmi
