// The trust-region core of the batched small-problem solvers track_lm_kernel (track_kernels.h), view_lm_kernel
// (view_kernels.h) and two_view_angular_kernel (two_view_kernels.h).  Each runs Ceres 1.14's TrustRegionMinimizer
// with the Levenberg-Marquardt strategy (the rules of tmi_ba_solver_solve, engine.hip) on one item of a batch; what
// differs between them -- how they linearise, form and evaluate the candidate, write results and share the work
// between lanes -- stays in the kernels.  The step handling, the options, the register Cholesky solve and the output
// record are here once.  (two_view_lm_kernel still carries its own copy: see two_view_kernels.h.)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/theia_mi355_ba.h"
#include "kernels.h"

namespace tmi {

// Solver options of one batched solve (the fields of tmi_ba_options the trust-region loop reads).
struct SmallLmArgs {
  int loss_type;
  double loss_width;
  int jacobi_scaling;
  int max_num_iterations;
  int max_num_consecutive_invalid_steps;
  double function_tolerance, gradient_tolerance, parameter_tolerance;
  double initial_radius, max_radius, min_radius;
  double min_relative_decrease;
  double lm_lo, lm_hi;
};

inline SmallLmArgs small_lm_args(const tmi_ba_options* O) {
  SmallLmArgs A;
  A.loss_type = O->loss_function_type;
  A.loss_width = O->robust_loss_width;
  A.jacobi_scaling = O->jacobi_scaling;
  A.max_num_iterations = O->max_num_iterations;
  A.max_num_consecutive_invalid_steps = O->max_num_consecutive_invalid_steps;
  A.function_tolerance = O->function_tolerance;
  A.gradient_tolerance = O->gradient_tolerance;
  A.parameter_tolerance = O->parameter_tolerance;
  A.initial_radius = O->initial_trust_region_radius;
  A.max_radius = O->max_trust_region_radius;
  A.min_radius = O->min_trust_region_radius;
  A.min_relative_decrease = O->min_relative_decrease;
  A.lm_lo = O->min_lm_diagonal;
  A.lm_hi = O->max_lm_diagonal;
  return A;
}

// Ceres Solver::Options defaults, the iteration limit and the loss aside: what a solve gets that sets no other
// option (bundle_adjust_two_views.cc:57-69 overrides none of these).
inline SmallLmArgs ceres_default_lm_args(int max_num_iterations, int loss_type, double loss_width) {
  SmallLmArgs A;
  A.loss_type = loss_type;
  A.loss_width = loss_width;
  A.jacobi_scaling = 1;
  A.max_num_iterations = max_num_iterations;
  A.max_num_consecutive_invalid_steps = 5;
  A.function_tolerance = 1e-6;
  A.gradient_tolerance = 1e-10;
  A.parameter_tolerance = 1e-8;
  A.initial_radius = 1e4;
  A.max_radius = 1e16;
  A.min_radius = 1e-32;
  A.min_relative_decrease = 1e-3;
  A.lm_lo = 1e-6;
  A.lm_hi = 1e32;
  return A;
}

// Per-item outputs of a batched solve.  term: 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE, 3 residual evaluation
// failed at the start point, -1 nothing to solve.
struct SmallLmOut {
  signed char* term;
  int* iters;
  double* c0;  // initial cost
  double* c1;  // final cost
  __device__ __forceinline__ void write(size_t i, int t, int it, double initial, double final_cost) const {
    term[i] = (signed char)t;
    iters[i] = it;
    c0[i] = initial;
    c1[i] = final_cost;
  }
};

// Trust-region state of one item and Ceres' step handling (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc).
// The tests that can end the solve return true and set *term (0 CONVERGENCE, 2 FAILURE).
struct TrustRegion {
  double radius, decrease_factor;
  int invalid_run;

  __device__ __forceinline__ explicit TrustRegion(const SmallLmArgs& A)
      : radius(A.initial_radius), decrease_factor(2.0), invalid_run(0) {}

  // the LM diagonal entry of a column with Gauss-Newton diagonal d (before the division by the radius)
  __device__ __forceinline__ static double lm_diag(const SmallLmArgs& A, double d) {
    return fmin(fmax(d, A.lm_lo), A.lm_hi);
  }

  // HandleInvalidStep: FAILURE after too many in a row, else the radius shrinks
  __device__ __forceinline__ bool invalid_step(const SmallLmArgs& A, int* term) {
    if (++invalid_run >= A.max_num_consecutive_invalid_steps) {
      *term = 2;
      return true;
    }
    shrink();
    return too_small(A, term);
  }

  // a usable step at the candidate cost: the step-norm and the cost-change tests
  __device__ __forceinline__ bool converged(const SmallLmArgs& A, double step_norm, double x_norm, double cost,
                                            double cand_cost, int* term) {
    invalid_run = 0;
    if (step_norm <= A.parameter_tolerance * (x_norm + A.parameter_tolerance) ||
        fabs(cost - cand_cost) <= A.function_tolerance * cost) {
      *term = 0;
      return true;
    }
    return false;
  }

  // accept or reject the step by its relative decrease: HandleSuccessfulStep grows the radius, a rejection shrinks it
  __device__ __forceinline__ bool accept(const SmallLmArgs& A, double relative_decrease) {
    if (relative_decrease > A.min_relative_decrease) {
      radius = radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * relative_decrease - 1.0, 3.0));
      radius = fmin(A.max_radius, radius);
      decrease_factor = 2.0;
      return true;
    }
    shrink();
    return false;
  }

  __device__ __forceinline__ bool too_small(const SmallLmArgs& A, int* term) const {
    if (!(radius < A.min_radius)) return false;
    *term = 0;
    return true;
  }

 private:
  __device__ __forceinline__ void shrink() {
    radius /= decrease_factor;
    decrease_factor *= 2.0;
  }
};

// Cholesky factor L of the packed symmetric N x N matrix A with the diagonal entries damped(A_jj).  A pivot that is not
// positive is replaced by 1 and the result is false.  reciprocal: the columns below the pivot l are formed as
// t * (1 / l), else as t / l (two_view_angular_kernel); the two round differently.  (damped is called where the pivot
// is formed: an array of damped diagonals computed ahead costs track_lm_kernel registers and occupancy.)
template <int N, class Damped>
__device__ __forceinline__ bool small_chol(const double (&A)[sym_size(N)], Damped damped, double (&L)[N][N],
                                           bool reciprocal = true) {
  bool pd = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = damped(A[sym_idx(j, j, N)]);
#pragma unroll
    for (int m = 0; m < j; ++m) d -= L[j][m] * L[j][m];
    if (!(d > 0.0)) {
      pd = false;
      d = 1.0;
    }
    const double l = sqrt(d);
    L[j][j] = l;
    const double il = 1.0 / l;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double t = A[sym_idx(j, i, N)];
#pragma unroll
      for (int m = 0; m < j; ++m) t -= L[i][m] * L[j][m];
      L[i][j] = reciprocal ? t * il : t / l;
    }
  }
  return pd;
}

// L L^T y = b by forward and back substitution
template <int N>
__device__ __forceinline__ void small_chol_solve(const double (&L)[N][N], const double (&b)[N], double (&y)[N]) {
  double z[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double t = b[i];
#pragma unroll
    for (int m = 0; m < i; ++m) t -= L[i][m] * z[m];
    z[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double t = z[i];
#pragma unroll
    for (int m = i + 1; m < N; ++m) t -= L[m][i] * y[m];
    y[i] = t / L[i][i];
  }
}

// (A with the diagonal damped) y = b: small_chol, then small_chol_solve; false if not positive definite
template <int N, class Damped>
__device__ __forceinline__ bool small_solve(const double (&A)[sym_size(N)], Damped damped, const double (&b)[N],
                                            double (&y)[N], bool reciprocal = true) {
  double L[N][N];
  const bool pd = small_chol<N>(A, damped, L, reciprocal);
  small_chol_solve<N>(L, b, y);
  return pd;
}

// model cost change of the step -y with the packed Gauss-Newton matrix A and gradient g: y^T g - 1/2 y^T A y
template <int N>
__device__ __forceinline__ double model_cost_change(const double (&A)[sym_size(N)], const double (&g)[N],
                                                    const double (&y)[N]) {
  double yg = 0.0, yAy = 0.0;
#pragma unroll
  for (int a = 0; a < N; ++a) {
    yg += y[a] * g[a];
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < N; ++b) t += A[a <= b ? sym_idx(a, b, N) : sym_idx(b, a, N)] * y[b];
    yAy += y[a] * t;
  }
  return yg - 0.5 * yAy;
}

}  // namespace tmi
