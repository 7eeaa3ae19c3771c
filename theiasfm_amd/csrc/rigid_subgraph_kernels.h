// theia::ExtractMaximallyParallelRigidSubgraph (extract_maximally_parallel_rigid_subgraph.cc:53-228; Kennedy, Daniilidis,
// Naroditsky and Taylor, IROS 2012) on the view table and edge list of the view-pair filters: the null space of the
// angle measurements t_ij x (c_j - c_i) = 0 and, per fixed view, the views whose null-space rows become parallel once
// the fixed view's rows are taken away.
//
// The reference forms the dense 3 E x 3 V matrix A and asks a full-pivot LU of A^T A for its kernel.  Here: L = A^T A is
// a block graph Laplacian of order n = 3 V (C_e^T C_e = |d|^2 I - d d^T on both diagonal blocks of an edge, its negative
// off the diagonal; A is never formed), L + mu I is factored ONCE (dense_cholesky.h) and the null space comes from block
// inverse iteration with Rayleigh-Ritz on a block of run-time width m, the way rotation_linear_kernels.h does it for
// six columns.  A block over the rows is stored in chunks of kChunk = 8 columns, [m / 8][n][8], so that the
// substitution runs chunk by chunk on the kernel dense_cholesky.h already has for 8 right-hand sides.
//
// rsg_edge_kernel       one thread per edge: d = R(orientation of view1)^T position_2 (Ceres' AngleAxisToRotationMatrix,
//                       as orientation_filter_kernel forms it) and the six distinct entries xx xy xz yy yz zz of C^T C
// rsg_diag_kernel       one thread per (view, entry): the view's diagonal block, the sum over its edges in the caller's
//                       edge order
// rsg_scale_kernel      ONE workgroup: the largest diagonal entry of L (a maximum: exact in any order)
// rsg_assemble_kernel   one workgroup per view: zero-fills the view's three rows of the dense matrix, then every thread
//                       writes its neighbours' blocks -C^T C (a pair appears once: one writer, nothing to sum); the
//                       diagonal block is rsg_diag_kernel's plus mu = relative_shift x the largest diagonal entry
// rsg_start_kernel      Q[i][c] = 2 u - 1, u from word m i + c of the splitmix64 stream of state 0
// rsg_mgs_kernel        step j of modified Gram-Schmidt on the m columns, on unnormalised dots (lin_mgs_kernel's
//                       scheme): launch j applies step j - 1 from the block parts of launch j - 1 and writes the block
//                       parts of y_j . y_k, k >= j -- thread k of a workgroup walks the workgroup's 256 rows in
//                       ascending order.  m + 1 launches a pass, two passes an iteration.
// rsg_apply_kernel      Z = L Y from the edge rows, one thread per (view, column): the sum over the view's edges in
//                       ascending edge index of C^T C (y_view - y_neighbour) -- the unshifted, unfactored operator
// rsg_gram_kernel       the block parts of T = Y^T Z, one workgroup per (row block, row of T)
// rsg_ritz_kernel       ONE workgroup, T in LDS (m <= 128: 128 KB): the parts summed in ascending block order, then
//                       cyclic Jacobi, kJacobiSweeps sweeps of m - 1 rounds of m / 2 disjoint pairs (the round-robin
//                       order: round r pairs r with m - 1 and (r + i) mod (m - 1) with (r - i) mod (m - 1)), a pair
//                       with a zero off-diagonal entry skipped; theta ascending, the first of equals first
// rsg_rotate_kernel     Q = Y W and the block parts of |Z W_j - theta_j Q_j|^2, one thread per (row, chunk of 8 columns)
// rsg_residual_kernel   the residuals' parts summed in ascending block order
// rsg_null_kernel       N [n][k] row major from the first k columns of the block
// rsg_rows_kernel       for a batch of fixed views f: M = N - replicate(N_f), the row norms, the rows normalised, IN THAT
//                       ORDER (:114-125; a row of squared norm 0 is left alone, as Eigen's normalize() leaves it); the
//                       rows are stored coordinate-major and view-minor, Mt[f][3][k][V], for the search's loads
// rsg_component_kernel  the search (:127-167), grid = tiles of 256 views i x the batch's fixed views f.  The workgroup
//                       stages the normalised rows of kTileJ views j in LDS; each thread owns one (f, i): its zero flag
//                       (all three norms < 1e-10), then for every j the three dot products over the k columns in
//                       ascending column, and 1 - |dot| < 1e-5 for all three.  It writes the one byte flag[f][i]: i is
//                       f, a zero view, or parallel to at least one other non-fixed non-zero view.  A workgroup stops
//                       scanning when every one of its threads has its answer, which changes no byte.
// rsg_count_kernel      one workgroup per fixed view: the size of its component (integers: exact in any order)
// rsg_pick_kernel       ONE workgroup: the largest component, the smallest fixed view among equals (:208-214)
//
// Every kernel is a plain grid launch, nothing waits on another workgroup, the loop is the host's (pose_graph_calls.h).
// No FMA contraction, no atomics, every sum of fixed shape, no byte written by a thread that does not own it: the same
// bits from call to call.
#pragma once
#include <hip/hip_runtime.h>

#include "pose_graph.h"
#include "ransac_core.h"
#include "rotation_kernels.h"

namespace tmi {
namespace rsg {

constexpr int kChunk = 8;           // columns of one chunk of a block: the substitution's right-hand sides
constexpr int kStartWidth = 8;      // the first block width m
constexpr int kMaxWidth = 128;      // T [m][m] in LDS: 128 KB of the CU's 160 KB
constexpr int kJacobiSweeps = 16;   // convergence is quadratic; log2(128) + a few sweeps reach rounding
constexpr int kTileJ = 16;          // views j staged at a time by the search: 3 x 16 accumulators a thread
constexpr double kMaxNorm = 1e-10;         // extract_maximally_parallel_rigid_subgraph.cc:108
constexpr double kMaxCosDistance = 1e-5;   // :107

// element (row i, column c) of a block [m / 8][n][8]
__device__ __forceinline__ size_t at(int n, int i, int c) { return ((size_t)(c >> 3) * n + i) * kChunk + (c & 7); }

// entry (a, b) of the symmetric 3 x 3 matrix stored xx xy xz yy yz zz
__device__ __forceinline__ double sym(const double* __restrict__ s, int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return s[lo == 0 ? hi : lo + hi + 1];
}

// the sum over the workgroups of value k of parts [num_blocks][stride], ascending
__device__ __forceinline__ double sum_parts(const double* __restrict__ parts, int num_blocks, int stride, int k) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int b = 0; b < num_blocks; ++b) s += parts[(size_t)b * stride + k];
  return s;
}

// the LDS of rsg_ritz_kernel: T [m][m], then per pair of a round c, s (doubles) and p, q (ints)
inline size_t ritz_lds_bytes(int m) { return ((size_t)m * m + m) * sizeof(double) + (size_t)m * sizeof(int); }
// the LDS of rsg_component_kernel: the tile [3 k][kTileJ] and the tile's usable flags
inline size_t component_lds_bytes(int k) { return (size_t)3 * k * kTileJ * sizeof(double) + kTileJ * sizeof(int); }

}  // namespace rsg

// orientation [3 V] of the problem's views, view1 [E] on them, position2 [3 E]; S [6 E]
__global__ __launch_bounds__(256) void rsg_edge_kernel(int num_pairs, const double* __restrict__ orientation,
                                                       const int* __restrict__ view1,
                                                       const double* __restrict__ position2, double* __restrict__ S) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= num_pairs) return;
  const int a = view1[e];
  const double aa[3] = {orientation[3 * (size_t)a], orientation[3 * (size_t)a + 1], orientation[3 * (size_t)a + 2]};
  const double p[3] = {position2[3 * (size_t)e], position2[3 * (size_t)e + 1], position2[3 * (size_t)e + 2]};
  double R[9];  // column major: R(r, c) = R[r + 3 c]
  angle_axis_to_rotation_matrix(aa, R);
  double d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = (R[3 * c] * p[0] + R[3 * c + 1] * p[1]) + R[3 * c + 2] * p[2];  // R^T p
  // C = [d]x; C^T C = |d|^2 I - d d^T
  double* s = S + 6 * (size_t)e;
  s[0] = d[2] * d[2] + d[1] * d[1];
  s[1] = -(d[0] * d[1]);
  s[2] = -(d[0] * d[2]);
  s[3] = d[2] * d[2] + d[0] * d[0];
  s[4] = -(d[1] * d[2]);
  s[5] = d[1] * d[1] + d[0] * d[0];
}

// D [6 V]: the diagonal blocks of L
__global__ __launch_bounds__(256) void rsg_diag_kernel(PoseGraph G, double* __restrict__ D) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 6 * G.num_views) return;
  const int v = t / 6, q = t - 6 * v;
  double acc = 0.0;
  for (int r = G.row_ptr[v]; r < G.row_ptr[v + 1]; ++r) acc += G.edge_value[6 * (size_t)(G.row[r].y >> 1) + q];
  D[t] = acc;
}

// scale[0] = the largest diagonal entry of L
__global__ __launch_bounds__(256) void rsg_scale_kernel(int num_views, const double* __restrict__ D,
                                                        double* __restrict__ scale) {
  __shared__ double part[256];
  double best = 0.0;
  for (int v = threadIdx.x; v < num_views; v += 256)
    best = fmax(best, fmax(D[6 * (size_t)v], fmax(D[6 * (size_t)v + 3], D[6 * (size_t)v + 5])));
  part[threadIdx.x] = best;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (threadIdx.x < half) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) scale[0] = part[0];
}

// blockIdx.x = the view; A [n][n], n = 3 V, receives L + mu I
__global__ __launch_bounds__(256) void rsg_assemble_kernel(PoseGraph G, int n, const double* __restrict__ D,
                                                           const double* __restrict__ scale, double relative_shift,
                                                           double* __restrict__ A) {
#pragma clang fp contract(off)
  const int v = blockIdx.x;
  double* rows = A + (size_t)3 * v * n;
  for (size_t j = threadIdx.x; j < (size_t)3 * n; j += 256) rows[j] = 0.0;
  __syncthreads();
  for (int r = G.row_ptr[v] + threadIdx.x; r < G.row_ptr[v + 1]; r += 256) {
    const int2 ent = G.row[r];
    const double* s = G.edge_value + 6 * (size_t)(ent.y >> 1);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) rows[(size_t)a * n + 3 * ent.x + b] = -rsg::sym(s, a, b);
  }
  if (threadIdx.x < 9) {
    const int a = threadIdx.x / 3, b = threadIdx.x - 3 * a;
    const double mu = relative_shift * scale[0];
    rows[(size_t)a * n + 3 * v + b] = rsg::sym(D + 6 * (size_t)v, a, b) + (a == b ? mu : 0.0);
  }
}

__global__ __launch_bounds__(256) void rsg_start_kernel(int n, int m, double* __restrict__ Q) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n * m) return;
  const int i = t / m, c = t - i * m;
  const double u = ((double)(splitmix64_word(0ull, (unsigned long long)t) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  Q[rsg::at(n, i, c)] = 2.0 * u - 1.0;
}

// launch j = 0 .. m of one pass over Y; prev / next: block parts [num_blocks][m] of launch j - 1 / this one
__global__ __launch_bounds__(256) void rsg_mgs_kernel(int n, int m, int j, double* __restrict__ Y,
                                                      const double* __restrict__ prev, double* __restrict__ next) {
#pragma clang fp contract(off)
  __shared__ double s[rsg::kMaxWidth];
  __shared__ double yj[256];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  if (j > 0) {
    if (tid < m && tid >= j - 1) s[tid] = rsg::sum_parts(prev, gridDim.x, m, tid);
    __syncthreads();
    const double sjj = s[j - 1];
    const double inv = sjj > 0.0 ? 1.0 / sqrt(sjj) : 0.0;  // a column that vanished stays zero
    if (i < n) {
      const double q = Y[rsg::at(n, i, j - 1)] * inv;
      Y[rsg::at(n, i, j - 1)] = q;
      for (int k = j; k < m; ++k) Y[rsg::at(n, i, k)] -= (s[k] * inv) * q;
    }
  }
  if (j >= m) return;
  yj[tid] = i < n ? Y[rsg::at(n, i, j)] : 0.0;
  __syncthreads();  // (and the rows written above are the workgroup's own: visible to it from here)
  const int k = j + tid;
  if (k >= m) return;
  const int i0 = blockIdx.x * 256;
  const int count = min(256, n - i0);
  double acc = 0.0;
  for (int r = 0; r < count; ++r) acc += yj[r] * Y[rsg::at(n, i0 + r, k)];
  next[(size_t)blockIdx.x * m + k] = acc;
}

// one thread per (view, column)
__global__ __launch_bounds__(256) void rsg_apply_kernel(PoseGraph G, int m, const double* __restrict__ Y,
                                                        double* __restrict__ Z) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= G.num_views * m) return;
  const int v = t / m, c = t - v * m;
  const int n = 3 * G.num_views;
  const double y0 = Y[rsg::at(n, 3 * v, c)], y1 = Y[rsg::at(n, 3 * v + 1, c)], y2 = Y[rsg::at(n, 3 * v + 2, c)];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int r = G.row_ptr[v]; r < G.row_ptr[v + 1]; ++r) {
    const int2 ent = G.row[r];
    const double* s = G.edge_value + 6 * (size_t)(ent.y >> 1);
    const double d0 = y0 - Y[rsg::at(n, 3 * ent.x, c)], d1 = y1 - Y[rsg::at(n, 3 * ent.x + 1, c)],
                 d2 = y2 - Y[rsg::at(n, 3 * ent.x + 2, c)];
    acc[0] += (s[0] * d0 + s[1] * d1) + s[2] * d2;
    acc[1] += (s[1] * d0 + s[3] * d1) + s[4] * d2;
    acc[2] += (s[2] * d0 + s[4] * d1) + s[5] * d2;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) Z[rsg::at(n, 3 * v + a, c)] = acc[a];
}

// grid (row blocks, m), 128 threads; parts [num_blocks][m][m]: row blockIdx.y of Y^T Z over the block's 256 rows
__global__ __launch_bounds__(128) void rsg_gram_kernel(int n, int m, const double* __restrict__ Y,
                                                       const double* __restrict__ Z, double* __restrict__ parts) {
#pragma clang fp contract(off)
  __shared__ double ya[256];
  const int a = blockIdx.y;
  const int i0 = blockIdx.x * 256;
  const int count = min(256, n - i0);
  for (int r = threadIdx.x; r < 256; r += 128) ya[r] = r < count ? Y[rsg::at(n, i0 + r, a)] : 0.0;
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= m) return;
  double acc = 0.0;
  for (int r = 0; r < count; ++r) acc += ya[r] * Z[rsg::at(n, i0 + r, k)];
  parts[((size_t)blockIdx.x * m + a) * m + k] = acc;
}

// one workgroup.  small: Wtmp [m][m] (the accumulated rotations), W [m][m] (row major, column j the j-th Ritz
// vector), theta [m], residual^2 [m]
__global__ __launch_bounds__(256) void rsg_ritz_kernel(const double* __restrict__ parts, int num_blocks, int m, int live,
                                                       double* __restrict__ small) {
#pragma clang fp contract(off)
  extern __shared__ double rsg_ritz_lds[];
  double* T = rsg_ritz_lds;
  double* cs = T + (size_t)m * m;                     // c [m / 2], s [m / 2]
  int* pq = reinterpret_cast<int*>(cs + m);           // p [m / 2], q [m / 2]
  const int tid = threadIdx.x, half = m / 2;
  double* Wt = small;
  double* W = small + (size_t)m * m;
  double* theta = W + (size_t)m * m;
  for (int e = tid; e < m * m; e += 256) {
    const int a = e / m, b = e - a * m;
    if (a <= b) {  // the upper triangle of Y^T Z is taken for both
      const double v = rsg::sum_parts(parts, num_blocks, m * m, e);
      T[a * m + b] = v;
      T[b * m + a] = v;
    }
    Wt[e] = a == b ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int sweep = 0; sweep < rsg::kJacobiSweeps; ++sweep) {
    for (int round = 0; round < m - 1; ++round) {
      if (tid < half) {
        int a = round, b = m - 1;
        if (tid > 0) {
          a = (round + tid) % (m - 1);
          b = (round - tid + (m - 1)) % (m - 1);
        }
        const int p = a < b ? a : b, q = a < b ? b : a;
        const double apq = T[p * m + q];
        double c = 1.0, s = 0.0;
        if (apq != 0.0) {
          const double zeta = (T[q * m + q] - T[p * m + p]) / (2.0 * apq);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        cs[tid] = c;
        cs[half + tid] = s;
        pq[tid] = p;
        pq[half + tid] = q;
      }
      __syncthreads();
      for (int e = tid; e < m * half; e += 256) {  // columns p and q of T and of the accumulated rotations
        const int k = e / half, pi = e - k * half;
        const int p = pq[pi], q = pq[half + pi];
        const double c = cs[pi], s = cs[half + pi];
        const double akp = T[k * m + p], akq = T[k * m + q];
        T[k * m + p] = c * akp - s * akq;
        T[k * m + q] = s * akp + c * akq;
        const double wkp = Wt[k * m + p], wkq = Wt[k * m + q];
        Wt[k * m + p] = c * wkp - s * wkq;
        Wt[k * m + q] = s * wkp + c * wkq;
      }
      __syncthreads();
      for (int e = tid; e < m * half; e += 256) {  // rows p and q of T
        const int pi = e / m, k = e - pi * m;
        const int p = pq[pi], q = pq[half + pi];
        const double c = cs[pi], s = cs[half + pi];
        const double apk = T[p * m + k], aqk = T[q * m + k];
        T[p * m + k] = c * apk - s * aqk;
        T[q * m + k] = s * apk + c * aqk;
      }
      __syncthreads();
    }
  }
  // ascending eigenvalues, the first of equals first: column j's rank is the number of columns that go before it.
  // The columns from `live` on are zero columns of Y (the block is wider than the matrix): no rotation touched them and
  // they stay where they are.
  for (int j = tid; j < m; j += 256) {
    const double tj = T[j * m + j];
    int rank = j;
    if (j < live) {
      rank = 0;
      for (int k = 0; k < live; ++k) {
        const double tk = T[k * m + k];
        rank += (tk < tj) || (tk == tj && k < j);
      }
    }
    theta[rank] = tj;
    for (int k = 0; k < m; ++k) W[k * m + rank] = Wt[k * m + j];
  }
}

// grid (row blocks, m / 8); parts [num_blocks][m]: the block parts of |Z W_j - theta_j Q_j|^2
__global__ __launch_bounds__(256) void rsg_rotate_kernel(int n, int m, const double* __restrict__ small,
                                                         const double* __restrict__ Y, const double* __restrict__ Z,
                                                         double* __restrict__ Q, double* __restrict__ parts) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const double* W = small + (size_t)m * m;
  const double* theta = W + (size_t)m * m;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * rsg::kChunk;
  double q[rsg::kChunk], z[rsg::kChunk];
#pragma unroll
  for (int jj = 0; jj < rsg::kChunk; ++jj) q[jj] = z[jj] = 0.0;
  if (i < n) {
    for (int k = 0; k < m; ++k) {
      const double yk = Y[rsg::at(n, i, k)], zk = Z[rsg::at(n, i, k)];
      const double* w = W + (size_t)k * m + c0;
#pragma unroll
      for (int jj = 0; jj < rsg::kChunk; ++jj) {
        q[jj] += yk * w[jj];
        z[jj] += zk * w[jj];
      }
    }
#pragma unroll
    for (int jj = 0; jj < rsg::kChunk; ++jj) Q[rsg::at(n, i, c0 + jj)] = q[jj];
  }
#pragma unroll
  for (int jj = 0; jj < rsg::kChunk; ++jj) {
    const double d = z[jj] - theta[c0 + jj] * q[jj];
    const double total = pg::block_sum(d * d, part);
    if (threadIdx.x == 0) parts[(size_t)blockIdx.x * m + c0 + jj] = total;
  }
}

// one workgroup of 128 threads: small's residual^2 [m]
__global__ __launch_bounds__(128) void rsg_residual_kernel(const double* __restrict__ parts, int num_blocks, int m,
                                                           double* __restrict__ small) {
  if ((int)threadIdx.x < m)
    small[(size_t)2 * m * m + m + threadIdx.x] = rsg::sum_parts(parts, num_blocks, m, threadIdx.x);
}

__global__ __launch_bounds__(256) void rsg_null_kernel(int n, int k, const double* __restrict__ Q,
                                                       double* __restrict__ N) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n * k) return;
  const int i = t / k, c = t - i * k;
  N[t] = Q[rsg::at(n, i, c)];
}

// one thread per (fixed view f0 + fb, coordinate d, view i), i fastest; Mt [F][3][k][V], norms [F][3][V]
__global__ __launch_bounds__(256) void rsg_rows_kernel(int num_views, int k, int f0, int num_fixed,
                                                       const double* __restrict__ N, double* __restrict__ Mt,
                                                       double* __restrict__ norms) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)num_fixed * 3 * num_views) return;
  const int fb = (int)(t / (3 * num_views));
  const int rem = (int)(t - (long long)fb * 3 * num_views);
  const int d = rem / num_views, i = rem - d * num_views;
  const double* ni = N + (size_t)(3 * i + d) * k;
  const double* nf = N + (size_t)(3 * (f0 + fb) + d) * k;
  double ss = 0.0;
  for (int c = 0; c < k; ++c) {
    const double v = ni[c] - nf[c];
    ss += v * v;
  }
  const double norm = sqrt(ss);
  norms[((size_t)fb * 3 + d) * num_views + i] = norm;
  double* out = Mt + ((size_t)fb * 3 + d) * k * num_views + i;
  for (int c = 0; c < k; ++c) {
    const double v = ni[c] - nf[c];
    out[(size_t)c * num_views] = ss > 0.0 ? v / norm : v;
  }
}

// grid (tiles of 256 views i, the batch's fixed views); flag [V][V]: flag[f][i]
__global__ __launch_bounds__(256) void rsg_component_kernel(int num_views, int k, int f0, const double* __restrict__ Mt,
                                                            const double* __restrict__ norms,
                                                            unsigned char* __restrict__ flag) {
#pragma clang fp contract(off)
  extern __shared__ double rsg_component_lds[];
  double* tile = rsg_component_lds;                                                   // [3 k][kTileJ]
  int* usable = reinterpret_cast<int*>(tile + (size_t)3 * k * rsg::kTileJ);           // [kTileJ]
  const int tid = threadIdx.x;
  const int fb = blockIdx.y, f = f0 + fb;
  const int i = blockIdx.x * 256 + tid;
  const double* M = Mt + (size_t)fb * 3 * k * num_views;
  const double* nr = norms + (size_t)fb * 3 * num_views;
  const bool inside = i < num_views;
  const bool zero = inside && nr[i] < rsg::kMaxNorm && nr[num_views + i] < rsg::kMaxNorm &&
                    nr[2 * (size_t)num_views + i] < rsg::kMaxNorm;
  const bool active = inside && i != f && !zero;
  bool found = false;
  for (int j0 = 0; j0 < num_views; j0 += rsg::kTileJ) {
    if (__syncthreads_and(!active || found)) break;  // (also: nobody still reads the tile of the last round)
    for (int e = tid; e < 3 * k * rsg::kTileJ; e += 256) {
      const int row = e / rsg::kTileJ, jj = e - row * rsg::kTileJ;
      tile[e] = j0 + jj < num_views ? M[(size_t)row * num_views + j0 + jj] : 0.0;
    }
    if (tid < rsg::kTileJ) {
      const int j = j0 + tid;
      usable[tid] = j < num_views && j != f &&
                    !(nr[j] < rsg::kMaxNorm && nr[num_views + j] < rsg::kMaxNorm &&
                      nr[2 * (size_t)num_views + j] < rsg::kMaxNorm);
    }
    __syncthreads();
    if (active && !found) {
      double acc[3][rsg::kTileJ];
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int jj = 0; jj < rsg::kTileJ; ++jj) acc[d][jj] = 0.0;
      for (int c = 0; c < k; ++c) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const double own = M[(size_t)(d * k + c) * num_views + i];
          const double* row = tile + (size_t)(d * k + c) * rsg::kTileJ;
#pragma unroll
          for (int jj = 0; jj < rsg::kTileJ; ++jj) acc[d][jj] += own * row[jj];
        }
      }
#pragma unroll
      for (int jj = 0; jj < rsg::kTileJ; ++jj) {
        const bool parallel = 1.0 - fabs(acc[0][jj]) < rsg::kMaxCosDistance &&
                              1.0 - fabs(acc[1][jj]) < rsg::kMaxCosDistance &&
                              1.0 - fabs(acc[2][jj]) < rsg::kMaxCosDistance;
        if (parallel && usable[jj] && j0 + jj != i) found = true;
      }
    }
  }
  if (inside) flag[(size_t)f * num_views + i] = (unsigned char)(i == f || zero || found);
}

// blockIdx.x = the fixed view: size[f] = the number of set flags of its row
__global__ __launch_bounds__(256) void rsg_count_kernel(int num_views, const unsigned char* __restrict__ flag,
                                                        int* __restrict__ size) {
  __shared__ int part[256];
  const unsigned char* row = flag + (size_t)blockIdx.x * num_views;
  int count = 0;
  for (int i = threadIdx.x; i < num_views; i += 256) count += row[i];
  part[threadIdx.x] = count;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) size[blockIdx.x] = part[0];
}

// one workgroup: pick[0] = the fixed view of the largest component, the smallest among equals; pick[1] = its size
__global__ __launch_bounds__(256) void rsg_pick_kernel(int num_views, const int* __restrict__ size,
                                                       int* __restrict__ pick) {
  __shared__ int best_size[256], best_view[256];
  int bs = -1, bv = 0x7fffffff;
  for (int f = threadIdx.x; f < num_views; f += 256)
    if (size[f] > bs) {  // (ascending f: the first of equals stays)
      bs = size[f];
      bv = f;
    }
  best_size[threadIdx.x] = bs;
  best_view[threadIdx.x] = bv;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (threadIdx.x < half) {
      const int os = best_size[threadIdx.x + half], ov = best_view[threadIdx.x + half];
      if (os > best_size[threadIdx.x] || (os == best_size[threadIdx.x] && ov < best_view[threadIdx.x])) {
        best_size[threadIdx.x] = os;
        best_view[threadIdx.x] = ov;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    pick[0] = best_view[0];
    pick[1] = best_size[0];
  }
}

}  // namespace tmi
