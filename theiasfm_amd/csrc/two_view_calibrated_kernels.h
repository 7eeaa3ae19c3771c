// Batched EstimateRelativePose (estimators/estimate_relative_pose.cc:59-144): RANSAC over the minimal five-point
// essential matrix (pose/five_point_relative_pose.cc:212-299) for many calibrated view pairs at once, on the chunked
// evaluate-then-replay scaffold of ransac_core.h, with the outlier test and the final kernel of
// two_view_ransac_kernels.h (a model is stored with focal lengths 1, so that the centred-pixel code scores normalised
// points unchanged).  What is this call's own is FivePointProblem, which the scaffold's three per-chunk kernels are
// instantiated with: a sample of five, 32 hypotheses per workgroup; the 5x9 kernel, the 10x20 constraint matrix and its
// solve, the action matrix' real eigenvalues and their vectors, and per real root the decomposition of E with the
// cheirality vote over the five sampled points: 0 to 10 models in 10 slots, one wavefront scoring one slot (an empty
// slot returns at once).
//
// A hypothesis' state (45, then 200, then 2 x 100 doubles) does not fit a thread's registers, and every pivot is
// data-dependent, so each thread owns a slab of kCalibSlab doubles of LDS, element e of thread t at lds[e * 32 + t]: the
// 32 lanes of a workgroup touch 32 consecutive doubles (all 64 banks once) whatever e each lane asks for, and no index
// into a register array is ever dynamic (scratch stays 0).  32 threads x 220 doubles are 55 KB, two workgroups per
// compute unit; 64 threads would take 110 KB and leave one.  The slab's plan:
//
//   step 3a   [0, 45) the 5x9 matrix, [48, 84) the kernel basis on its way to registers
//   step 3b/c [0, 200) the 10x20 constraint matrix, eliminated in place; afterwards [0, 100) holds X in the pivot order
//   step 3d   [100, 200) the action matrix, reduced to Hessenberg form and iterated on; [200, 210) the eigenvalues
//   step 3e   [100, 200) A - lambda I per root, [200, 210) the back-substitution, [210, 220) the real roots, ascending
//
// One elimination routine (calib_eliminate) serves 3a, 3c and 3e; a column permutation is ten nibbles of one 64-bit
// integer.  Everything up to E is __host__ __device__ with the slab's stride a template parameter, so that a host
// program can run the same text against the numpy model.  Only + - * / sqrt and fabs are used and nothing is
// contracted into FMA (#pragma clang fp contract(off) in every body).
#pragma once
#include <hip/hip_runtime.h>

#include "two_view_ransac_kernels.h"

namespace tmi {

constexpr int kCalibSlots = 10;         // models per sample
constexpr int kCalibThreads = 32;       // hypotheses per workgroup
constexpr int kCalibSlab = 220;         // doubles of LDS per hypothesis
constexpr int kCalibQrSweeps = 30;      // of the QR iteration on one block before the sample is given up
constexpr double kCalibEps = 2.220446049250313e-16;
constexpr unsigned long long kCalibIdentity = 0xfedcba9876543210ull;

__host__ __device__ __forceinline__ int calib_nibble(unsigned long long p, int k) { return (int)((p >> (4 * k)) & 15ull); }
__host__ __device__ __forceinline__ unsigned long long calib_swap_nibbles(unsigned long long p, int a, int b) {
  const unsigned long long x = ((p >> (4 * a)) ^ (p >> (4 * b))) & 15ull;
  return p ^ (x << (4 * a)) ^ (x << (4 * b));
}

// `steps` steps of Gaussian elimination with full pivoting on the nrows x ncols matrix at A (row stride ld): the pivot
// is the entry of largest magnitude among rows k.. and columns k .. npiv - 1, the lowest (row, column) among equals
// (ascending walk, strict >); the row swap covers all ncols columns, the column swap all rows.  false: a pivot is not
// > 0 (NaN included), or the smallest pivot is not above thr x the largest (FullPivLU's rank test).
template <int S>
__host__ __device__ bool calib_eliminate(double* A, int ld, int nrows, int npiv, int ncols, int steps, double thr,
                                         unsigned long long* perm_out) {
#pragma clang fp contract(off)
  unsigned long long perm = kCalibIdentity;
  double max_pivot = 0.0, min_pivot = 0.0;
  for (int k = 0; k < steps; ++k) {
    double big = -1.0;
    int pr = k, pc = k;
    for (int r = k; r < nrows; ++r)
      for (int c = k; c < npiv; ++c) {
        const double m = __builtin_fabs(A[(r * ld + c) * S]);
        if (m > big) {
          big = m;
          pr = r;
          pc = c;
        }
      }
    if (!(big > 0.0)) return false;
    if (k == 0 || big > max_pivot) max_pivot = big;
    if (k == 0 || big < min_pivot) min_pivot = big;
    if (pr != k)
      for (int c = 0; c < ncols; ++c) {
        const double t = A[(k * ld + c) * S];
        A[(k * ld + c) * S] = A[(pr * ld + c) * S];
        A[(pr * ld + c) * S] = t;
      }
    if (pc != k) {
      for (int r = 0; r < nrows; ++r) {
        const double t = A[(r * ld + k) * S];
        A[(r * ld + k) * S] = A[(r * ld + pc) * S];
        A[(r * ld + pc) * S] = t;
      }
      perm = calib_swap_nibbles(perm, k, pc);
    }
    const double piv = A[(k * ld + k) * S];
    for (int r = k + 1; r < nrows; ++r) {
      const double m = A[(r * ld + k) * S] / piv;
      for (int c = k + 1; c < ncols; ++c) A[(r * ld + c) * S] = A[(r * ld + c) * S] - m * A[(k * ld + c) * S];
    }
  }
  *perm_out = perm;
  return min_pivot > thr * max_pivot;
}

// MultiplyDegOnePoly and MultiplyDegTwoDegOnePoly (five_point_relative_pose.cc:65-140), their association order kept.
__host__ __device__ __forceinline__ void calib_mul11(const double* a, const double* b, double* o) {
#pragma clang fp contract(off)
  o[0] = a[0] * b[0];
  o[1] = a[0] * b[1] + a[1] * b[0];
  o[2] = a[1] * b[1];
  o[3] = a[0] * b[2] + a[2] * b[0];
  o[4] = a[1] * b[2] + a[2] * b[1];
  o[5] = a[2] * b[2];
  o[6] = a[0] * b[3] + a[3] * b[0];
  o[7] = a[1] * b[3] + a[3] * b[1];
  o[8] = a[2] * b[3] + a[3] * b[2];
  o[9] = a[3] * b[3];
}
__host__ __device__ __forceinline__ void calib_mul21(const double* a, const double* b, double* o) {
#pragma clang fp contract(off)
  o[0] = a[0] * b[0];
  o[1] = a[0] * b[1] + a[1] * b[0];
  o[2] = a[1] * b[1] + a[2] * b[0];
  o[3] = a[2] * b[1];
  o[4] = a[0] * b[2] + a[3] * b[0];
  o[5] = (a[1] * b[2] + a[3] * b[1]) + a[4] * b[0];
  o[6] = a[2] * b[2] + a[4] * b[1];
  o[7] = a[3] * b[2] + a[5] * b[0];
  o[8] = a[4] * b[2] + a[5] * b[1];
  o[9] = a[5] * b[2];
  o[10] = a[0] * b[3] + a[6] * b[0];
  o[11] = (a[1] * b[3] + a[6] * b[1]) + a[7] * b[0];
  o[12] = a[2] * b[3] + a[7] * b[1];
  o[13] = (a[3] * b[3] + a[6] * b[2]) + a[8] * b[0];
  o[14] = (a[4] * b[3] + a[7] * b[2]) + a[8] * b[1];
  o[15] = a[5] * b[3] + a[8] * b[2];
  o[16] = a[6] * b[3] + a[9] * b[0];
  o[17] = a[7] * b[3] + a[9] * b[1];
  o[18] = a[8] * b[3] + a[9] * b[2];
  o[19] = a[9] * b[3];
}

// Step 3a: the kernel basis NS [9][4] of the 5x9 epipolar matrix, FullPivLU::kernel()'s.
template <int S>
__host__ __device__ bool calib_kernel_basis(const double x1[5], const double y1[5], const double x2[5],
                                            const double y2[5], double* A, double NS[36]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    A[(k * 9 + 0) * S] = x2[k] * x1[k];
    A[(k * 9 + 1) * S] = y2[k] * x1[k];
    A[(k * 9 + 2) * S] = x1[k];
    A[(k * 9 + 3) * S] = x2[k] * y1[k];
    A[(k * 9 + 4) * S] = y2[k] * y1[k];
    A[(k * 9 + 5) * S] = y1[k];
    A[(k * 9 + 6) * S] = x2[k];
    A[(k * 9 + 7) * S] = y2[k];
    A[(k * 9 + 8) * S] = 1.0;
  }
  unsigned long long perm;
  if (!calib_eliminate<S>(A, 9, 5, 9, 9, 5, 5.0 * kCalibEps, &perm)) return false;
  // vector j: the free permuted column 5 + j set to 1, the other free ones 0, back-substitution in ascending columns
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double z[5];
#pragma unroll
    for (int k = 4; k >= 0; --k) {
      double acc = 0.0;
#pragma unroll
      for (int c = k + 1; c < 5; ++c) acc = acc + A[(k * 9 + c) * S] * z[c];
      acc = acc + A[(k * 9 + 5 + j) * S];
      z[k] = -acc / A[(k * 9 + k) * S];
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) A[(48 + 4 * calib_nibble(perm, c) + j) * S] = z[c];
#pragma unroll
    for (int c = 5; c < 9; ++c) A[(48 + 4 * calib_nibble(perm, c) + j) * S] = c == 5 + j ? 1.0 : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 36; ++q) NS[q] = A[(48 + q) * S];
  return true;
}

// Step 3b: the 10x20 constraint matrix (BuildConstraintMatrix, :142-206) into A [0, 200).  ns(i, j), entry (i, j) of E
// over the basis, is row i + 3 j of NS (:256-260).  E E^T is symmetric bit for bit (a product and a two-term sum
// commute), so six of its nine polynomials are formed.
template <int S>
__host__ __device__ void calib_constraint_matrix(const double NS[36], double* A) {
#pragma clang fp contract(off)
#define TMI_CAL_NS(i, j) (NS + 4 * ((i) + 3 * (j)))
#define TMI_CAL_SYM(i, j) ((i) <= (j) ? ((i) == 0 ? (j) : (i) + (j) + 1) : ((j) == 0 ? (i) : (i) + (j) + 1))
  double eet[6][10], trace[10];  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      double m0[10], m1[10], m2[10];
      calib_mul11(TMI_CAL_NS(i, 0), TMI_CAL_NS(j, 0), m0);
      calib_mul11(TMI_CAL_NS(i, 1), TMI_CAL_NS(j, 1), m1);
      calib_mul11(TMI_CAL_NS(i, 2), TMI_CAL_NS(j, 2), m2);
#pragma unroll
      for (int q = 0; q < 10; ++q) eet[TMI_CAL_SYM(i, j)][q] = 2.0 * ((m0[q] + m1[q]) + m2[q]);
    }
#pragma unroll
  for (int q = 0; q < 10; ++q) trace[q] = (eet[0][q] + eet[3][q]) + eet[5][q];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double a[20], b[20], c[20], d[20];
      calib_mul21(eet[TMI_CAL_SYM(i, 0)], TMI_CAL_NS(0, j), a);
      calib_mul21(eet[TMI_CAL_SYM(i, 1)], TMI_CAL_NS(1, j), b);
      calib_mul21(eet[TMI_CAL_SYM(i, 2)], TMI_CAL_NS(2, j), c);
      calib_mul21(trace, TMI_CAL_NS(i, j), d);
#pragma unroll
      for (int q = 0; q < 20; ++q) A[((3 * i + j) * 20 + q) * S] = ((a[q] + b[q]) + c[q]) - 0.5 * d[q];
    }
  {
    double p[10], q[10], d0[20], d1[20], d2[20];
    calib_mul11(TMI_CAL_NS(0, 1), TMI_CAL_NS(1, 2), p);
    calib_mul11(TMI_CAL_NS(0, 2), TMI_CAL_NS(1, 1), q);
#pragma unroll
    for (int k = 0; k < 10; ++k) p[k] = p[k] - q[k];
    calib_mul21(p, TMI_CAL_NS(2, 0), d0);
    calib_mul11(TMI_CAL_NS(0, 2), TMI_CAL_NS(1, 0), p);
    calib_mul11(TMI_CAL_NS(0, 0), TMI_CAL_NS(1, 2), q);
#pragma unroll
    for (int k = 0; k < 10; ++k) p[k] = p[k] - q[k];
    calib_mul21(p, TMI_CAL_NS(2, 1), d1);
    calib_mul11(TMI_CAL_NS(0, 0), TMI_CAL_NS(1, 1), p);
    calib_mul11(TMI_CAL_NS(0, 1), TMI_CAL_NS(1, 0), q);
#pragma unroll
    for (int k = 0; k < 10; ++k) p[k] = p[k] - q[k];
    calib_mul21(p, TMI_CAL_NS(2, 2), d2);
#pragma unroll
    for (int k = 0; k < 20; ++k) A[(180 + k) * S] = (d0[k] + d1[k]) + d2[k];
  }
#undef TMI_CAL_NS
#undef TMI_CAL_SYM
}

// Step 3c: C[:, :10] X = C[:, 10:] in place; afterwards row k of X in the pivot order (the variable
// calib_nibble(perm, k)) is at A [10 k, 10 k + 10).  false: rank < 10 at 10 eps (a DEVIATION: the reference solves on).
template <int S>
__host__ __device__ bool calib_solve_constraints(double* A, unsigned long long* perm) {
#pragma clang fp contract(off)
  if (!calib_eliminate<S>(A, 20, 10, 10, 20, 10, 10.0 * kCalibEps, perm)) return false;
  for (int k = 9; k >= 0; --k) {
    const double piv = A[(k * 20 + k) * S];
    for (int j = 10; j < 20; ++j) {
      double acc = 0.0;
      for (int c = k + 1; c < 10; ++c) acc = acc + A[(k * 20 + c) * S] * A[(c * 20 + j) * S];
      A[(k * 20 + j) * S] = (A[(k * 20 + j) * S] - acc) / piv;
    }
  }
  // compact in ascending order: element 10 k + j never overtakes what is still to be read at 20 k' + 10 + j'
  for (int k = 0; k < 10; ++k)
    for (int j = 0; j < 10; ++j) {
      const double v = A[(k * 20 + 10 + j) * S];
      A[(k * 10 + j) * S] = v;
    }
  return true;
}

// The action matrix (:271-279) into H (row stride 10), minus lam on the diagonal: rows 0..5 are X's rows 0, 1, 2, 4, 5,
// 7, rows 6..9 hold -1 at columns 0, 1, 3, 6.
template <int S>
__host__ __device__ void calib_action_matrix(const double* X, unsigned long long perm, double lam, double* H) {
#pragma clang fp contract(off)
  for (int r = 0; r < 6; ++r) {
    const int v = (int)((0x754210ull >> (4 * r)) & 15ull);
    int kk = 0;
    for (int k = 0; k < 10; ++k) kk = calib_nibble(perm, k) == v ? k : kk;
    for (int c = 0; c < 10; ++c) H[(r * 10 + c) * S] = X[(kk * 10 + c) * S];
  }
  for (int r = 6; r < 10; ++r) {
    const int one = (int)((0x6310ull >> (4 * (r - 6))) & 15ull);
    for (int c = 0; c < 10; ++c) H[(r * 10 + c) * S] = c == one ? -1.0 : 0.0;
  }
  for (int k = 0; k < 10; ++k) H[(k * 11) * S] = H[(k * 11) * S] - lam;
}

__host__ __device__ __forceinline__ double calib_sign(double a, double b) {
  a = a < 0.0 ? -a : a;
  return b >= 0.0 ? a : -a;
}

// Step 3d: the eigenvalues of the 10x10 matrix at H (destroyed) by the reduction to Hessenberg form with stabilised
// elementary similarity transformations and the Francis double-shift QR iteration (EISPACK elmhes and hqr, without
// balancing), into wr [10]; bit k of *real_mask is set where root k is real: a 1x1 block of the real Schur form, or a
// member of a 2x2 block whose discriminant is >= 0.  false: a block took more than kCalibQrSweeps sweeps.  Every loop
// has a fixed bound.
template <int S>
__host__ __device__ bool calib_real_eigenvalues(double* H, double* wr, unsigned* real_mask) {
#pragma clang fp contract(off)
#define TMI_CAL_H(r, c) H[((r) * 10 + (c)) * S]
  const int n = 10;
  for (int m = 1; m < n - 1; ++m) {
    double x = 0.0;
    int i = m;
    for (int j = m; j < n; ++j)
      if (__builtin_fabs(TMI_CAL_H(j, m - 1)) > __builtin_fabs(x)) {
        x = TMI_CAL_H(j, m - 1);
        i = j;
      }
    if (i != m) {
      for (int j = m - 1; j < n; ++j) {
        const double t = TMI_CAL_H(i, j);
        TMI_CAL_H(i, j) = TMI_CAL_H(m, j);
        TMI_CAL_H(m, j) = t;
      }
      for (int j = 0; j < n; ++j) {
        const double t = TMI_CAL_H(j, i);
        TMI_CAL_H(j, i) = TMI_CAL_H(j, m);
        TMI_CAL_H(j, m) = t;
      }
    }
    if (x != 0.0)
      for (int r = m + 1; r < n; ++r) {
        double y = TMI_CAL_H(r, m - 1);
        if (y != 0.0) {
          y = y / x;
          TMI_CAL_H(r, m - 1) = y;
          for (int j = m; j < n; ++j) TMI_CAL_H(r, j) = TMI_CAL_H(r, j) - y * TMI_CAL_H(m, j);
          for (int j = 0; j < n; ++j) TMI_CAL_H(j, m) = TMI_CAL_H(j, m) + y * TMI_CAL_H(j, r);
        }
      }
  }
  for (int i = 2; i < n; ++i)
    for (int j = 0; j < i - 1; ++j) TMI_CAL_H(i, j) = 0.0;
  double anorm = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = i > 0 ? i - 1 : 0; j < n; ++j) anorm = anorm + __builtin_fabs(TMI_CAL_H(i, j));
  unsigned mask = 0;
  int nn = n - 1, its = 0;
  double t = 0.0;
  for (int guard = 0; guard < n * (kCalibQrSweeps + 2) && nn >= 0; ++guard) {
    int l = nn;
    for (; l >= 1; --l) {
      double s = __builtin_fabs(TMI_CAL_H(l - 1, l - 1)) + __builtin_fabs(TMI_CAL_H(l, l));
      if (s == 0.0) s = anorm;
      if (__builtin_fabs(TMI_CAL_H(l, l - 1)) + s == s) {
        TMI_CAL_H(l, l - 1) = 0.0;
        break;
      }
    }
    double x = TMI_CAL_H(nn, nn);
    if (l == nn) {  // one root
      wr[nn * S] = x + t;
      mask |= 1u << nn;
      nn -= 1;
      its = 0;
      continue;
    }
    double y = TMI_CAL_H(nn - 1, nn - 1);
    double w = TMI_CAL_H(nn, nn - 1) * TMI_CAL_H(nn - 1, nn);
    if (l == nn - 1) {  // two roots
      const double p = 0.5 * (y - x);
      const double q = p * p + w;
      double z = sqrt(q < 0.0 ? -q : q);
      x = x + t;
      if (q >= 0.0) {
        z = p + calib_sign(z, p);
        wr[(nn - 1) * S] = x + z;
        wr[nn * S] = z != 0.0 ? x - w / z : x + z;
        mask |= 3u << (nn - 1);
      } else {
        wr[(nn - 1) * S] = x + p;
        wr[nn * S] = x + p;
      }
      nn -= 2;
      its = 0;
      continue;
    }
    if (its == kCalibQrSweeps) return false;
    if (its == 10 || its == 20) {  // the exceptional shift
      t = t + x;
      for (int i = 0; i <= nn; ++i) TMI_CAL_H(i, i) = TMI_CAL_H(i, i) - x;
      const double s = __builtin_fabs(TMI_CAL_H(nn, nn - 1)) + __builtin_fabs(TMI_CAL_H(nn - 1, nn - 2));
      x = 0.75 * s;
      y = x;
      w = -0.4375 * (s * s);
    }
    ++its;
    double p = 0.0, q = 0.0, r = 0.0, z = 0.0;
    int m = nn - 2;
    for (; m >= l; --m) {
      z = TMI_CAL_H(m, m);
      r = x - z;
      double s = y - z;
      p = (r * s - w) / TMI_CAL_H(m + 1, m) + TMI_CAL_H(m, m + 1);
      q = ((TMI_CAL_H(m + 1, m + 1) - z) - r) - s;
      r = TMI_CAL_H(m + 2, m + 1);
      s = (__builtin_fabs(p) + __builtin_fabs(q)) + __builtin_fabs(r);
      p = p / s;
      q = q / s;
      r = r / s;
      if (m == l) break;
      const double u = __builtin_fabs(TMI_CAL_H(m, m - 1)) * (__builtin_fabs(q) + __builtin_fabs(r));
      const double v = __builtin_fabs(p) * ((__builtin_fabs(TMI_CAL_H(m - 1, m - 1)) + __builtin_fabs(z)) +
                                            __builtin_fabs(TMI_CAL_H(m + 1, m + 1)));
      if (u + v == v) break;
    }
    for (int i = m + 2; i <= nn; ++i) {
      TMI_CAL_H(i, i - 2) = 0.0;
      if (i != m + 2) TMI_CAL_H(i, i - 3) = 0.0;
    }
    for (int k = m; k <= nn - 1; ++k) {
      if (k != m) {
        p = TMI_CAL_H(k, k - 1);
        q = TMI_CAL_H(k + 1, k - 1);
        r = k != nn - 1 ? TMI_CAL_H(k + 2, k - 1) : 0.0;
        x = (__builtin_fabs(p) + __builtin_fabs(q)) + __builtin_fabs(r);
        if (x == 0.0) continue;
        p = p / x;
        q = q / x;
        r = r / x;
      }
      const double s = calib_sign(sqrt((p * p + q * q) + r * r), p);
      if (s == 0.0) continue;
      if (k == m) {
        if (l != m) TMI_CAL_H(k, k - 1) = -TMI_CAL_H(k, k - 1);
      } else {
        TMI_CAL_H(k, k - 1) = -(s * x);
      }
      p = p + s;
      x = p / s;
      y = q / s;
      z = r / s;
      q = q / p;
      r = r / p;
      for (int j = k; j <= nn; ++j) {
        p = TMI_CAL_H(k, j) + q * TMI_CAL_H(k + 1, j);
        if (k != nn - 1) {
          p = p + r * TMI_CAL_H(k + 2, j);
          TMI_CAL_H(k + 2, j) = TMI_CAL_H(k + 2, j) - p * z;
        }
        TMI_CAL_H(k + 1, j) = TMI_CAL_H(k + 1, j) - p * y;
        TMI_CAL_H(k, j) = TMI_CAL_H(k, j) - p * x;
      }
      const int mmin = nn < k + 3 ? nn : k + 3;
      for (int i = l; i <= mmin; ++i) {
        p = x * TMI_CAL_H(i, k) + y * TMI_CAL_H(i, k + 1);
        if (k != nn - 1) {
          p = p + z * TMI_CAL_H(i, k + 2);
          TMI_CAL_H(i, k + 2) = TMI_CAL_H(i, k + 2) - p * r;
        }
        TMI_CAL_H(i, k + 1) = TMI_CAL_H(i, k + 1) - p * q;
        TMI_CAL_H(i, k) = TMI_CAL_H(i, k) - p;
      }
    }
  }
  if (nn >= 0) return false;
  *real_mask = mask;
  return true;
#undef TMI_CAL_H
}

// Steps 3a to 3d on the slab A.  NS: the kernel basis; afterwards A [0, 100) holds X (with *perm), A [210, 210 + count)
// the real roots in ascending order (an insertion sort with a strict >).  Returns their count, -1 without a model.
template <int S>
__host__ __device__ int calib_real_roots(const double x1[5], const double y1[5], const double x2[5], const double y2[5],
                                         double* A, double NS[36], unsigned long long* perm) {
#pragma clang fp contract(off)
  if (!calib_kernel_basis<S>(x1, y1, x2, y2, A, NS)) return -1;
  calib_constraint_matrix<S>(NS, A);
  if (!calib_solve_constraints<S>(A, perm)) return -1;
  calib_action_matrix<S>(A, *perm, 0.0, A + 100 * S);
  unsigned mask = 0;
  if (!calib_real_eigenvalues<S>(A + 100 * S, A + 200 * S, &mask)) return -1;
  int count = 0;
  for (int k = 0; k < 10; ++k)
    if ((mask >> k) & 1u) {
      const double v = A[(200 + k) * S];
      int q = count;
      for (; q > 0 && A[(210 + q - 1) * S] > v; --q) A[(210 + q) * S] = A[(210 + q - 1) * S];
      A[(210 + q) * S] = v;
      ++count;
    }
  return count;
}

// Step 3e for the root lam: the null vector of A - lam I by nine elimination steps (the tenth pivot is the root's own
// residual and is not tested), the tenth permuted entry set to 1; E = NS x (its last four entries), unit norm, the
// largest-magnitude entry positive, as e [9] column-major (:293-294).  false: rank < 9 at 10 eps.
template <int S>
__host__ __device__ bool calib_essential_for_root(double* A, const double NS[36], unsigned long long perm, double lam,
                                                  double e[9]) {
#pragma clang fp contract(off)
  double* W = A + 100 * S;
  double* z = A + 200 * S;
  calib_action_matrix<S>(A, perm, lam, W);
  unsigned long long wperm;
  if (!calib_eliminate<S>(W, 10, 10, 10, 10, 9, 10.0 * kCalibEps, &wperm)) return false;
  z[9 * S] = 1.0;
  for (int k = 8; k >= 0; --k) {
    double acc = 0.0;
    for (int c = k + 1; c < 10; ++c) acc = acc + W[(k * 10 + c) * S] * z[c * S];
    z[k * S] = -acc / W[(k * 10 + k) * S];
  }
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
  for (int c = 0; c < 10; ++c) {
    const int v = calib_nibble(wperm, c);
    const double zc = z[c * S];
    t0 = v == 6 ? zc : t0;
    t1 = v == 7 ? zc : t1;
    t2 = v == 8 ? zc : t2;
    t3 = v == 9 ? zc : t3;
  }
  double ss = 0.0, big = -1.0, lead = 0.0;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    e[r] = ((NS[4 * r] * t0 + NS[4 * r + 1] * t1) + NS[4 * r + 2] * t2) + NS[4 * r + 3] * t3;
    ss = ss + e[r] * e[r];
    const double m = __builtin_fabs(e[r]);
    if (m > big) {
      big = m;
      lead = e[r];
    }
  }
  double nrm = sqrt(ss);
  if (lead < 0.0) nrm = -nrm;
#pragma unroll
  for (int r = 0; r < 9; ++r) e[r] = e[r] / nrm;
  return true;
}

// Step 4: GetBestPoseFromEssentialMatrix on the five sampled correspondences, the arithmetic of two_view_model's
// decomposition with focal lengths 1.  model: kTwoViewModel doubles (E row-major, R row-major, position, 1, 1, 0).
// Returns the number of points in front of both cameras under the chosen candidate.
__host__ __device__ inline int calib_pose_from_essential(const double e[9], const double x1[5], const double y1[5],
                                                         const double x2[5], const double y2[5],
                                                         double* __restrict__ model) {
#pragma clang fp contract(off)
  double a0[3] = {e[0], e[1], e[2]}, a1[3] = {e[3], e[4], e[5]}, a2[3] = {e[6], e[7], e[8]};  // the columns of E
  double v0[3], v1[3], v2[3];
  two_view_jacobi_svd(a0, a1, a2, v0, v1, v2);
  double u0[3], u1[3], u2[3], t[3];
  {
    const double s0 = sqrt(dot3(a0, a0)), s1 = sqrt(dot3(a1, a1));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      u0[r] = a0[r] / s0;
      u1[r] = a1[r] / s1;
    }
  }
  cross3(u0, u1, u2);
  cross3(v0, v1, v2);
  t[0] = u2[0]; t[1] = u2[1]; t[2] = u2[2];
  normalize3(t);
  double R1[9], R2[9], q1[3], q2[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      R1[3 * r + c] = (u0[r] * v1[c] - u1[r] * v0[c]) + u2[r] * v2[c];
      R2[3 * r + c] = (u1[r] * v0[c] - u0[r] * v1[c]) + u2[r] * v2[c];
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    q1[c] = (R1[c] * t[0] + R1[3 + c] * t[1]) + R1[6 + c] * t[2];
    q2[c] = (R2[c] * t[0] + R2[3 + c] * t[1]) + R2[6 + c] * t[2];
  }
  int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double ea, eb;
    two_view_cheirality(R1, -q1[0], -q1[1], -q1[2], x1[k], y1[k], x2[k], y2[k], &ea, &eb);
    n0 += (ea > 0.0 && eb > 0.0) ? 1 : 0;
    n1 += (-ea > 0.0 && -eb > 0.0) ? 1 : 0;
    two_view_cheirality(R2, -q2[0], -q2[1], -q2[2], x1[k], y1[k], x2[k], y2[k], &ea, &eb);
    n2 += (ea > 0.0 && eb > 0.0) ? 1 : 0;
    n3 += (-ea > 0.0 && -eb > 0.0) ? 1 : 0;
  }
  int best = 0, best_n = n0;  // std::max_element: the first of the largest
  if (n1 > best_n) { best = 1; best_n = n1; }
  if (n2 > best_n) { best = 2; best_n = n2; }
  if (n3 > best_n) { best = 3; best_n = n3; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) model[3 * r + c] = e[r + 3 * c];
#pragma unroll
  for (int q = 0; q < 9; ++q) model[9 + q] = best < 2 ? R1[q] : R2[q];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double q = best < 2 ? q1[c] : q2[c];
    model[18 + c] = (best & 1) ? q : -q;
  }
  model[21] = 1.0;
  model[22] = 1.0;
  model[23] = 0.0;
  return best_n;
}

// Steps 3 and 4 for one sample: up to kCalibSlots models of kTwoViewModel doubles each at `models`, in ascending order
// of the eigenvalue; a root whose best candidate has fewer than 4 points in front is dropped
// (estimate_relative_pose.cc:94-104).  Returns the number of models.
template <int S>
__host__ __device__ int calib_models(const double x1[5], const double y1[5], const double x2[5], const double y2[5],
                                     double* A, double* __restrict__ models) {
  double NS[36];
  unsigned long long perm;
  const int roots = calib_real_roots<S>(x1, y1, x2, y2, A, NS, &perm);
  int count = 0;
  for (int q = 0; q < roots; ++q) {
    double e[9];
    if (!calib_essential_for_root<S>(A, NS, perm, A[(210 + q) * S], e)) continue;
    if (calib_pose_from_essential(e, x1, y1, x2, y2, models + kTwoViewModel * count) >= 4) ++count;
  }
  return count;
}

#ifdef __HIPCC__
struct FivePointProblem : TwoViewOutlier {
  static constexpr int kSample = 5, kSlots = kCalibSlots, kScoreSlots = 1, kThreads = kCalibThreads, kSlab = kCalibSlab;
  __device__ static void models(const double pts[kPlanes][kSample], double* slab, double* __restrict__ models, int* has) {
    const int count = calib_models<kCalibThreads>(pts[0], pts[1], pts[2], pts[3], slab, models);
    for (int k = 0; k < count; ++k) has[k] = 1;
  }
};
#endif  // __HIPCC__

}  // namespace tmi
