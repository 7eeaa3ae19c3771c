// Host side of the global pose estimators: RobustRotationEstimator, LeastUnsquaredDeviationPositionEstimator,
// NonlinearPositionEstimator, NonlinearRotationEstimator and LinearRotationEstimator on one scaffold.  Every call turns a
// view table and an edge list into the rows of a PoseGraph (pose_graph.h; built by pose_graph_host.h, uploaded by
// PoseGraphDevice), works on ONE dense symmetric positive definite matrix of order <= kRotationMaxOrder (DenseSpd) and
// loops on the host around a substitution, a few per-edge and per-view kernels and one read-back of a few sums and the
// pivot flag (ScalarFetch), with its device time in three classes (ClassSeconds).  Written on one_shot.h.
#pragma once

#include "pose_graph_host.h"

namespace {
// The largest order n = V - 1 the calls take (TMI_BA_ROTATION_MAX_ORDER lowers it: a diagnostic knob, so that a small
// graph reaches the refusal).
int rotation_order_cap() {
  int cap = kRotationMaxOrder;
  if (const char* e = getenv("TMI_BA_ROTATION_MAX_ORDER")) cap = std::max(0, std::min(cap, atoi(e)));
  return cap;
}

// The rows of a graph on the device.  upload() is the only place that uploads them: G is complete after it, with
// edge_value the caller's device array.
struct PoseGraphDevice {
  PoseGraph G;
  int upload(OneShot* s, int V, int fixed_view, const EdgeRows& rows, int E, const int32_t* view1, const int32_t* view2,
             const double* edge_value) {
    int *d_v1, *d_v2, *d_ptr, *d_lptr;
    int2 *d_row, *d_lrow;
    TMI_HIP(s->upload(&d_v1, (const int*)view1, (size_t)E));
    TMI_HIP(s->upload(&d_v2, (const int*)view2, (size_t)E));
    TMI_HIP(s->upload(&d_ptr, rows.row_ptr.data(), rows.row_ptr.size()));
    TMI_HIP(s->upload(&d_row, rows.row.data(), rows.row.size()));
    TMI_HIP(s->upload(&d_lptr, rows.lap_ptr.data(), rows.lap_ptr.size()));
    TMI_HIP(s->upload(&d_lrow, rows.lap_row.data(), rows.lap_row.size()));
    G = PoseGraph{V, E, fixed_view, d_v1, d_v2, edge_value, d_ptr, d_row, d_lptr, d_lrow};
    return TMI_BA_OK;
  }
};

// Device time in three classes.  begin(c) marks the stream and says that what is queued until the next mark belongs to
// class c; end() closes the last interval (ScalarFetch::fetch calls it); collect(), after the stream has been waited
// for, adds the intervals to their classes.  An interval that is read only after the NEXT synchronisation -- a
// linearisation, queued after the step that it follows has been read back -- has marks of its own (begin_deferred,
// end_deferred) and belongs to the graph kernels.
struct ClassSeconds {
  enum Class { kFactor = 0, kSubstitution = 1, kGraph = 2 };
  double seconds[3] = {0.0, 0.0, 0.0};
  StreamTimer timer, deferred;
  Class of[StreamTimer::kMaxMarks] = {};
  bool pending = false;
  explicit ClassSeconds(hipStream_t st) : timer(st, StreamTimer::kMaxMarks), deferred(st, 2) {}
  hipError_t status() const { return timer.status != hipSuccess ? timer.status : deferred.status; }
  hipError_t begin(Class c) {
    of[timer.marked] = c;
    return timer.mark();
  }
  hipError_t end() { return timer.marked > 0 ? timer.mark() : hipSuccess; }
  hipError_t begin_deferred() {
    deferred.marked = 0;
    return deferred.mark();
  }
  hipError_t end_deferred() {
    pending = true;
    return deferred.mark();
  }
  void collect() {
    for (int m = 0; m + 1 < timer.marked; ++m) seconds[of[m]] += timer.seconds(m, m + 1);
    timer.marked = 0;
    if (pending) seconds[kGraph] += deferred.seconds();
    pending = false;
  }
  template <class Sum>
  void write(Sum* sum) const {
    sum->factor_seconds = seconds[kFactor];
    sum->substitution_seconds = seconds[kSubstitution];
    sum->graph_seconds = seconds[kGraph];
    sum->kernel_seconds = seconds[kFactor] + seconds[kSubstitution] + seconds[kGraph];
  }
};

// The dense symmetric positive definite matrix of a call (dense_cholesky.h): A [N][N], overwritten by its factor, the
// factorisation's workspace, the substitution's [nrhs N] and the pivot flag (cleared here; a pivot that is not positive
// sets it).
struct DenseSpd {
  int N = 0;
  double *A = nullptr, *cdiag = nullptr, *tmp = nullptr;
  int* flag = nullptr;
  int32_t* factorizations = nullptr;  // the summary's counter (null: none)
  int alloc(OneShot* s, int N_, int nrhs, int32_t* counter) {
    N = N_;
    factorizations = counter;
    TMI_HIP(s->alloc(&A, (size_t)N * N));
    TMI_HIP(s->alloc(&cdiag, (size_t)kPanel * ((size_t)(N + kPanel - 1) / kPanel) * kPanel));
    TMI_HIP(s->alloc(&tmp, (size_t)nrhs * N));
    TMI_HIP(s->alloc_filled(&flag, 1, 0));
    return TMI_BA_OK;
  }
  void factor(hipStream_t st) {
    dense_cholesky_factor(A, N, cdiag, flag, st);
    if (factorizations) ++*factorizations;
  }
  template <int NRHS>
  void substitute(hipStream_t st, double* rhs, double* x) {
    dense_cholesky_substitute<NRHS>(A, N, rhs, x, tmp, st);
  }
};

// The read-back that ends every step of a loop: a few sums of block parts (set(); reduce_partials_kernel), optionally
// max |.| of a vector behind them (absmax), into the device words d_norms, and from there with the pivot flag into
// pinned memory.
struct ScalarFetch {
  Pinned<double> pinned;
  double *h_norms = nullptr, *d_norms = nullptr;
  int *h_flag = nullptr, *d_flag = nullptr;
  ReduceJobs jobs;
  const double* absmax = nullptr;  // [absmax_n]: its max |.| goes behind the sums
  int absmax_n = 0;
  int alloc(OneShot* s, int* pivot_flag, int words = 6) {
    d_flag = pivot_flag;
    memset(&jobs, 0, sizeof(jobs));
    TMI_HIP(s->alloc(&d_norms, (size_t)words + 2));
    TMI_HIP(pinned.alloc((size_t)words + 2));
    h_norms = pinned.get();
    h_flag = reinterpret_cast<int*>(h_norms + words);
    return TMI_BA_OK;
  }
  void set(int q, const double* part, int count) {
    jobs.part[q] = part;
    jobs.count[q] = count;
  }
  int flag() const { return *h_flag; }
  hipError_t clear_flag(hipStream_t st) { return hipMemsetAsync(d_flag, 0, sizeof(int), st); }
  // The sums of the first `count` quantities into d_norms[at ..], the closing mark, then `words` doubles of d_norms
  // (< 0: the sums, and max |.| where it is asked for) and the pivot flag (with_flag) to the host, the stream waited
  // for, and the marked intervals to their classes.
  int fetch(OneShot* s, ClassSeconds* T, int count, int at = 0, int words = -1, bool with_flag = true) {
    hipStream_t st = s->stream;
    if (count > 0) hipLaunchKernelGGL(reduce_partials_kernel, dim3(count), dim3(256), 0, st, jobs, d_norms + at);
    if (absmax) hipLaunchKernelGGL(nlp_absmax_kernel, dim3(1), dim3(256), 0, st, absmax_n, absmax, d_norms + count);
    if (words < 0) words = count + (absmax ? 1 : 0);
    TMI_HIP(T->end());
    ReadBack rb(st);
    rb.add(h_norms, d_norms, (size_t)words);
    if (with_flag) rb.add(h_flag, d_flag, 1);
    TMI_HIP(rb.finish());
    T->collect();
    return TMI_BA_OK;
  }
};

// ---- RobustRotationEstimator (rotation_kernels.h) ----------------------------------------------
// What the rotation estimator asks of its arguments; null: fine.
const char* check_rotation_arguments(const tmi_ba_relative_rotation_batch* B, const tmi_ba_robust_rotation_options* o,
                                     int fixed_view, const double* view_rotation) {
  const int V = B->num_views, E = B->num_pairs;
  if (V < 0 || E < 0) return "robust rotations: negative size";
  if (E == 0) return "robust rotations: no relative rotation (the reference CHECK_GTs the number of constraints)";
  if (!B->pair_view1 || !B->pair_view2 || !B->pair_rotation) return "robust rotations: missing array";
  if (fixed_view < 0 || fixed_view >= V) return "robust rotations: fixed_view out of range";
  if (!(o->l1_step_convergence_threshold > 0.0) || !std::isfinite(o->l1_step_convergence_threshold) ||
      !(o->irls_step_convergence_threshold > 0.0) || !std::isfinite(o->irls_step_convergence_threshold))
    return "robust rotations: a step threshold that is not positive and finite";
  if (!(o->irls_loss_parameter_sigma > 0.0) || !std::isfinite(o->irls_loss_parameter_sigma))
    return "robust rotations: sigma is not positive and finite";
  if (o->max_num_l1_iterations < 0 || o->max_num_irls_iterations < 0)
    return "robust rotations: negative iteration count";
  for (int e = 0; e < E; ++e) {
    const int a = B->pair_view1[e], b = B->pair_view2[e];
    if (a < 0 || a >= V || b < 0 || b >= V) return "robust rotations: view index out of range";
    if (a == b) return "robust rotations: a view paired with itself";
  }
  if (!all_finite(view_rotation, (size_t)3 * V)) return "robust rotations: non-finite view_rotation";
  if (!all_finite(B->pair_rotation, (size_t)3 * E)) return "robust rotations: non-finite pair_rotation";
  if (!view_components(V, E, B->pair_view1, B->pair_view2).all_reach(fixed_view))
    return "robust rotations: a view is not connected to fixed_view";
  return nullptr;
}
}  // namespace
extern "C" {

void tmi_ba_robust_rotation_options_init(tmi_ba_robust_rotation_options* o) {
  if (!o) return;
  o->max_num_l1_iterations = 5;  // robust_rotation_estimator.h:63-82
  o->l1_step_convergence_threshold = 0.001;
  o->max_num_irls_iterations = 100;
  o->irls_step_convergence_threshold = 0.001;
  o->irls_loss_parameter_sigma = 5.0 * (M_PI / 180.0);
}

int32_t tmi_ba_estimate_global_rotations_robust(const tmi_ba_relative_rotation_batch* Bh,
                                                const tmi_ba_robust_rotation_options* opt, int32_t fixed_view,
                                                int32_t device, double* view_rotation, double* pair_residual,
                                                int32_t* l1_admm_iterations, double* l1_average_step,
                                                double* irls_average_step, double* irls_squared_residual,
                                                tmi_ba_robust_rotation_summary* sum) {
  if (!Bh || !opt || !view_rotation || !sum)
    return bad_argument("robust rotations: null batch, options, view_rotation or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is touched
  if (const char* why = check_rotation_arguments(Bh, opt, fixed_view, view_rotation)) return bad_argument(why);
  const int V = Bh->num_views, E = Bh->num_pairs, n = V - 1;
  if (n > rotation_order_cap()) {
    g_last_error = "robust rotations: num_views - 1 exceeds the dense solver's cap (see the header)";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  if (E > (1 << 30)) return bad_argument("robust rotations: more than 2^30 pairs");
  const EdgeRows rows = build_edge_rows(V, E, Bh->pair_view1, Bh->pair_view2, fixed_view);
  const int L1 = opt->max_num_l1_iterations, IR = opt->max_num_irls_iterations;
  std::vector<int> admm_trace;
  std::vector<double> l1_trace, irls_trace, irls_sq_trace;
  return one_shot_batch(device, "robust rotations: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    int rc;
    double *d_rel, *d_o, *d_r, *d_w, *d_z, *d_u, *d_dz, *d_rhs, *d_x, *d_diag_w, *d_part;
    TMI_HIP(s->upload(&d_rel, Bh->pair_rotation, (size_t)3 * E));
    TMI_HIP(s->upload(&d_o, (const double*)view_rotation, (size_t)3 * V));
    PoseGraphDevice graph;
    if ((rc = graph.upload(s, V, fixed_view, rows, E, Bh->pair_view1, Bh->pair_view2, d_rel))) return rc;
    const PoseGraph& G = graph.G;
    TMI_HIP(s->alloc(&d_r, (size_t)3 * E));
    TMI_HIP(s->alloc(&d_w, (size_t)E));
    TMI_HIP(s->alloc(&d_z, (size_t)3 * E));
    TMI_HIP(s->alloc(&d_u, (size_t)3 * E));
    TMI_HIP(s->alloc(&d_dz, (size_t)3 * E));
    TMI_HIP(s->alloc(&d_rhs, (size_t)3 * n));
    TMI_HIP(s->alloc(&d_x, (size_t)3 * n));
    TMI_HIP(s->alloc(&d_diag_w, (size_t)n));
    const int nbE = (E + 255) / 256, nbV = (n + 255) / 256;
    TMI_HIP(s->alloc(&d_part, (size_t)4 * nbE + (size_t)3 * nbV));
    double *p_r = d_part, *p_ax = p_r + nbE, *p_z = p_ax + nbE, *p_rr = p_z + nbE, *p_s = p_rr + nbE, *p_t = p_s + nbV,
           *p_step = p_t + nbV;
    DenseSpd lap;  // the Laplacian, order n, three right-hand sides
    if ((rc = lap.alloc(s, n, 3, &sum->num_factorizations))) return rc;
    ScalarFetch F;  // the ADMM norms, or |r|^2 and the step sum
    if ((rc = F.alloc(s, lap.flag))) return rc;
    hipStream_t st = s->stream;
    const dim3 edge_grid(nbE), view_grid(nbV), block(256);
    const double sigma = opt->irls_loss_parameter_sigma;
    ClassSeconds T(st);
    TMI_HIP(T.status());
    const char* pivot = "robust rotations: a pivot of the Laplacian's Cholesky factorisation is not positive";

    // ---- ComputeResiduals, and the factorisation of the L1 phase (:149-155) ----
    TMI_HIP(T.begin(T.kFactor));
    if (L1 > 0) {
      hipLaunchKernelGGL(laplacian_assemble_kernel, dim3(n), block, 0, st, G, n, nullptr, nullptr, lap.A);
      lap.factor(st);
    }
    TMI_HIP(T.begin(T.kGraph));
    hipLaunchKernelGGL(rotation_residual_kernel, edge_grid, block, 0, st, G, d_o, sigma, d_r, d_w, p_rr);
    F.set(0, p_rr, nbE);
    if ((rc = F.fetch(s, &T, 1))) return rc;
    if (F.flag()) {
      s->error = pivot;
      return TMI_BA_ERR_LINEAR_SOLVER;
    }
    double r_sq = F.h_norms[0];

    // ---- SolveL1Regression (:156-169) ----
    const double rho = 1.0, alpha = 1.0, abs_tol = 1e-4, rel_tol = 1e-2;  // l1_solver.h:89-98
    const double primal_abs = std::sqrt(3.0 * (double)E) * abs_tol, dual_abs = std::sqrt(3.0 * (double)n) * abs_tol;
    int budget = 5;
    for (int outer = 0; outer < L1; ++outer) {
      const double rhs_norm = std::sqrt(r_sq);
      TMI_HIP(T.begin(T.kGraph));
      TMI_HIP(hipMemsetAsync(d_z, 0, (size_t)3 * E * sizeof(double), st));
      TMI_HIP(hipMemsetAsync(d_u, 0, (size_t)3 * E * sizeof(double), st));
      TMI_HIP(hipMemsetAsync(d_dz, 0, (size_t)3 * E * sizeof(double), st));
      hipLaunchKernelGGL(admm_view_kernel, view_grid, block, 0, st, G, n, rho, d_r, d_z, d_u, d_dz, d_rhs, p_s, p_t);
      F.set(0, p_r, nbE);
      F.set(1, p_ax, nbE);
      F.set(2, p_z, nbE);
      F.set(3, p_s, nbV);
      F.set(4, p_t, nbV);
      int ran = 0;
      for (int it = 0; it < budget; ++it) {
        TMI_HIP(T.begin(T.kSubstitution));
        lap.substitute<3>(st, d_rhs, d_x);
        TMI_HIP(T.begin(T.kGraph));
        hipLaunchKernelGGL(admm_edge_kernel, edge_grid, block, 0, st, G, rho, alpha, d_x, d_r, d_z, d_u, d_dz, p_r, p_ax,
                           p_z);
        hipLaunchKernelGGL(admm_view_kernel, view_grid, block, 0, st, G, n, rho, d_r, d_z, d_u, d_dz, d_rhs, p_s, p_t);
        if ((rc = F.fetch(s, &T, 5))) return rc;
        ++ran;
        if (admm_converged(F.h_norms, rhs_norm, primal_abs, dual_abs, rel_tol).converged) break;
      }
      // UpdateGlobalRotations, ComputeResiduals, ComputeAverageStepSize
      TMI_HIP(T.begin(T.kGraph));
      hipLaunchKernelGGL(rotation_update_kernel, view_grid, block, 0, st, n, fixed_view, d_x, d_o, p_step);
      hipLaunchKernelGGL(rotation_residual_kernel, edge_grid, block, 0, st, G, d_o, sigma, d_r, d_w, p_rr);
      F.set(0, p_rr, nbE);
      F.set(1, p_step, nbV);
      if ((rc = F.fetch(s, &T, 2))) return rc;
      r_sq = F.h_norms[0];
      const double avg = F.h_norms[1] / (double)n;
      admm_trace.push_back(ran);
      l1_trace.push_back(avg);
      sum->num_l1_iterations++;
      sum->num_admm_iterations += ran;
      if (avg <= opt->l1_step_convergence_threshold) {
        sum->l1_converged = 1;
        break;
      }
      budget *= 2;
    }

    // ---- SolveIRLS (:189-234) ----
    F.set(0, p_rr, nbE);
    F.set(1, p_step, nbV);
    for (int it = 0; it < IR; ++it) {
      TMI_HIP(T.begin(T.kFactor));
      hipLaunchKernelGGL(irls_rhs_kernel, view_grid, block, 0, st, G, n, d_w, d_r, d_rhs, d_diag_w);
      hipLaunchKernelGGL(laplacian_assemble_kernel, dim3(n), block, 0, st, G, n, d_w, d_diag_w, lap.A);
      lap.factor(st);
      TMI_HIP(T.begin(T.kSubstitution));
      lap.substitute<3>(st, d_rhs, d_x);
      TMI_HIP(T.begin(T.kGraph));
      hipLaunchKernelGGL(rotation_update_kernel, view_grid, block, 0, st, n, fixed_view, d_x, d_o, p_step);
      hipLaunchKernelGGL(rotation_residual_kernel, edge_grid, block, 0, st, G, d_o, sigma, d_r, d_w, p_rr);
      if ((rc = F.fetch(s, &T, 2))) return rc;
      if (F.flag()) {
        s->error = pivot;
        return TMI_BA_ERR_LINEAR_SOLVER;
      }
      r_sq = F.h_norms[0];
      const double avg = F.h_norms[1] / (double)n;
      irls_trace.push_back(avg);
      irls_sq_trace.push_back(r_sq);
      sum->num_irls_iterations++;
      if (avg < opt->irls_step_convergence_threshold) {
        sum->irls_converged = 1;
        break;
      }
    }

    // the results, only now: a failure above leaves the caller's arrays as they were
    std::vector<double> o_h((size_t)3 * V), r_h(pair_residual ? (size_t)3 * E : 0);
    TMI_HIP(s->download(o_h.data(), d_o, o_h.size()));
    TMI_HIP(s->download(r_h.data(), d_r, r_h.size()));
    TMI_HIP(hipStreamSynchronize(st));
    std::copy(o_h.begin(), o_h.end(), view_rotation);
    if (pair_residual) std::copy(r_h.begin(), r_h.end(), pair_residual);
    if (l1_admm_iterations) std::copy(admm_trace.begin(), admm_trace.end(), l1_admm_iterations);
    if (l1_average_step) std::copy(l1_trace.begin(), l1_trace.end(), l1_average_step);
    if (irls_average_step) std::copy(irls_trace.begin(), irls_trace.end(), irls_average_step);
    if (irls_squared_residual) std::copy(irls_sq_trace.begin(), irls_sq_trace.end(), irls_squared_residual);
    sum->num_views = V;
    sum->num_pairs = E;
    T.write(sum);
    return TMI_BA_OK;
  });
}
}  // extern "C"

// ---- LeastUnsquaredDeviationPositionEstimator (position_kernels.h) ------------------------------
namespace {
// What the position estimator asks of its arguments beyond check_view_pair_batch, the connection to fixed_view apart;
// null: fine.  Nothing is allocated here.
const char* check_lud_arguments(const tmi_ba_view_pair_batch* B, const tmi_ba_lud_position_options* o, int fixed_view) {
  if (B->num_pairs == 0) return "LUD positions: no view pair";
  if (fixed_view < 0 || fixed_view >= B->num_views) return "LUD positions: fixed_view out of range";
  for (const double x : {o->rho, o->alpha, o->absolute_tolerance, o->relative_tolerance})
    if (!(x > 0.0) || !std::isfinite(x)) return "LUD positions: rho, alpha or a tolerance that is not positive and finite";
  if (o->max_num_iterations < 1) return "LUD positions: max_num_iterations < 1 (the reference CHECK_GTs it)";
  return nullptr;
}
}  // namespace
extern "C" {

void tmi_ba_lud_position_options_init(tmi_ba_lud_position_options* o) {
  if (!o) return;
  o->max_num_iterations = 1000;  // math/constrained_l1_solver.h:64-74
  o->rho = 10.0;
  o->alpha = 1.2;
  o->absolute_tolerance = 1e-4;
  o->relative_tolerance = 1e-2;
}

int32_t tmi_ba_estimate_global_positions_lud(const tmi_ba_view_pair_batch* Bh, const tmi_ba_lud_position_options* opt,
                                             int32_t fixed_view, int32_t device, double* view_position,
                                             double* pair_scale, double* pair_residual, double* admm_r_norm,
                                             double* admm_s_norm, tmi_ba_lud_position_summary* sum) {
  if (!Bh || !opt || !view_position || !sum)
    return bad_argument("LUD positions: null batch, options, view_position or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is touched
  if (const char* why = check_view_pair_batch(Bh, false, Bh->pair_position2)) return bad_argument(why);
  if (const char* why = check_lud_arguments(Bh, opt, fixed_view)) return bad_argument(why);
  const int V = Bh->num_views, E = Bh->num_pairs, n = V - 1;
  // the cap before anything of the views' size is allocated, the union-find included
  if ((int64_t)3 * n > rotation_order_cap()) {
    g_last_error = "LUD positions: 3 (num_views - 1) exceeds the dense solver's cap (see the header)";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  const int N = 3 * n;  // (<= the cap)
  if (!view_components(V, E, Bh->pair_view1, Bh->pair_view2).all_reach(fixed_view))
    return bad_argument("LUD positions: a view is not connected to fixed_view");
  const EdgeRows rows = build_edge_rows(V, E, Bh->pair_view1, Bh->pair_view2, fixed_view);
  const int max_it = opt->max_num_iterations;
  const double rho = opt->rho, alpha = opt->alpha;
  std::vector<double> r_trace, s_trace;
  return one_shot_batch(device, "LUD positions: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    int rc;
    double *d_pos, *d_t, *d_rot = nullptr, *d_qs, *d_z, *d_u, *d_dz, *d_scale, *d_ax, *d_rhs, *d_p, *d_part;
    TMI_HIP(s->upload(&d_pos, Bh->pair_position2, (size_t)3 * E));
    d_t = d_pos;
    if (Bh->view_rotation) {
      TMI_HIP(s->upload(&d_rot, Bh->view_rotation, (size_t)3 * V));
      TMI_HIP(s->alloc(&d_t, (size_t)3 * E));
    }
    PoseGraphDevice graph;
    if ((rc = graph.upload(s, V, fixed_view, rows, E, Bh->pair_view1, Bh->pair_view2, d_t))) return rc;
    const PoseGraph& G = graph.G;
    const std::vector<double> ones((size_t)E, 1.0);  // the scale entries of A^T b
    TMI_HIP(s->upload(&d_qs, ones.data(), ones.size()));
    TMI_HIP(s->alloc(&d_z, (size_t)4 * E));
    TMI_HIP(s->alloc(&d_u, (size_t)4 * E));
    TMI_HIP(s->alloc(&d_dz, (size_t)4 * E));
    TMI_HIP(s->alloc(&d_scale, (size_t)E));
    TMI_HIP(s->alloc(&d_ax, (size_t)3 * E));
    TMI_HIP(s->alloc(&d_rhs, (size_t)N));
    TMI_HIP(s->alloc(&d_p, (size_t)N));
    const int nbE = (E + 255) / 256, nbV = (n + 255) / 256;
    // the blocks' parts: |A x - z - b|^2, |A x|^2, |z|^2 [nbE each], then |rho A^T dz|^2 and |rho A^T u|^2, each the
    // edges' parts [nbE] followed by the views' [nbV] and reduced as one quantity
    TMI_HIP(s->alloc(&d_part, (size_t)5 * nbE + (size_t)2 * nbV));
    double *p_r = d_part, *p_ax = p_r + nbE, *p_z = p_ax + nbE, *p_s = p_z + nbE, *p_t = p_s + nbE + nbV;
    DenseSpd S;  // order N, one right-hand side
    if ((rc = S.alloc(s, N, 1, &sum->num_factorizations))) return rc;
    ScalarFetch F;  // the ADMM norms
    if ((rc = F.alloc(s, S.flag))) return rc;
    F.set(0, p_r, nbE);
    F.set(1, p_ax, nbE);
    F.set(2, p_z, nbE);
    F.set(3, p_s, nbE + nbV);
    F.set(4, p_t, nbE + nbV);
    hipStream_t st = s->stream;
    const dim3 edge_grid(nbE), view_grid(nbV), block(256);
    TMI_HIP(hipMemsetAsync(d_z, 0, (size_t)4 * E * sizeof(double), st));
    TMI_HIP(hipMemsetAsync(d_u, 0, (size_t)4 * E * sizeof(double), st));
    TMI_HIP(hipMemsetAsync(d_dz, 0, (size_t)4 * E * sizeof(double), st));
    ClassSeconds T(st);
    TMI_HIP(T.status());

    // ---- the directions, S and its factor, and the right-hand side of the first solve: A^T b ----
    TMI_HIP(T.begin(T.kFactor));
    if (Bh->view_rotation)
      hipLaunchKernelGGL(lud_direction_kernel, edge_grid, block, 0, st, E, d_rot, G.pair_view1, d_pos, d_t);
    hipLaunchKernelGGL(lud_assemble_kernel, dim3(n), block, 0, st, G, N, S.A);
    S.factor(st);
    TMI_HIP(T.begin(T.kGraph));
    hipLaunchKernelGGL(lud_view_kernel, view_grid, block, 0, st, G, n, rho, d_qs, d_z, d_u, d_dz, d_rhs, p_s + nbE,
                       p_t + nbE);
    if ((rc = F.fetch(s, &T, 0))) return rc;  // (no sum yet: the pivot flag alone)
    if (F.flag()) {
      s->error = "LUD positions: a pivot of the Cholesky factorisation of S is not positive";
      return TMI_BA_ERR_LINEAR_SOLVER;
    }

    // ---- ConstrainedL1Solver::Solve (:112-170) ----
    const double rhs_norm = std::sqrt((double)E);  // |b|
    const double primal_abs = std::sqrt(4.0 * (double)E) * opt->absolute_tolerance;
    const double dual_abs = std::sqrt(3.0 * (double)n + (double)E) * opt->absolute_tolerance;
    for (int it = 0; it < max_it; ++it) {
      TMI_HIP(T.begin(T.kSubstitution));
      S.substitute<1>(st, d_rhs, d_p);
      TMI_HIP(T.begin(T.kGraph));
      hipLaunchKernelGGL(lud_edge_kernel, edge_grid, block, 0, st, G, rho, alpha, d_p, d_qs, d_z, d_u, d_dz, d_scale,
                         d_ax, p_r, p_ax, p_z, p_s, p_t);
      hipLaunchKernelGGL(lud_view_kernel, view_grid, block, 0, st, G, n, rho, d_qs, d_z, d_u, d_dz, d_rhs, p_s + nbE,
                         p_t + nbE);
      if ((rc = F.fetch(s, &T, 5))) return rc;
      sum->num_admm_iterations++;
      const AdmmNorms norms = admm_converged(F.h_norms, rhs_norm, primal_abs, dual_abs, opt->relative_tolerance);
      r_trace.push_back(norms.r_norm);
      s_trace.push_back(norms.s_norm);
      if (norms.converged) {
        sum->converged = 1;
        break;
      }
    }

    // the results, only now: a failure above leaves the caller's arrays as they were
    std::vector<double> p_h((size_t)N), scale_h(pair_scale ? (size_t)E : 0), ax_h(pair_residual ? (size_t)3 * E : 0);
    TMI_HIP(s->download(p_h.data(), d_p, p_h.size()));
    TMI_HIP(s->download(scale_h.data(), d_scale, scale_h.size()));
    TMI_HIP(s->download(ax_h.data(), d_ax, ax_h.size()));
    TMI_HIP(hipStreamSynchronize(st));
    scatter_free(V, fixed_view, nullptr, p_h.data(), view_position);
    std::fill(view_position + (size_t)3 * fixed_view, view_position + (size_t)3 * fixed_view + 3, 0.0);
    if (pair_scale) std::copy(scale_h.begin(), scale_h.end(), pair_scale);
    if (pair_residual) std::copy(ax_h.begin(), ax_h.end(), pair_residual);
    if (admm_r_norm) std::copy(r_trace.begin(), r_trace.end(), admm_r_norm);
    if (admm_s_norm) std::copy(s_trace.begin(), s_trace.end(), admm_s_norm);
    sum->num_views = V;
    sum->num_pairs = E;
    T.write(sum);
    return TMI_BA_OK;
  });
}
}  // extern "C"

// ---- NonlinearPositionEstimator (position_nonlinear_kernels.h) ----------------------------------
namespace {
// The device memory of the Levenberg-Marquardt loop on dense normal equations of order N over E edges that the nonlinear
// position and rotation estimators share (normal_lm_solve), and the traces it leaves.
struct NormalLm {
  int N = 0, nbE = 0, nbN = 0;
  double *x, *cand, *step, *y, *rhs, *scale, *diag, *g, *gabs, *M, *part;
  DenseSpd damped;  // the damped copy of M, overwritten by the factor
  ScalarFetch F;    // cost, model cost change, |step|^2, |candidate|^2, max |gradient|
  double *p_cost, *p_mcc, *p_step, *p_x;  // the blocks' parts: cost and model cost change [nbE], |step|^2, |x|^2 [nbN]
  std::vector<double> cost_trace, radius_trace;
  std::vector<int32_t> outcome_trace;
  int alloc(OneShot* s, int N_, int E, int32_t* factorizations) {
    N = N_;
    nbE = (E + 255) / 256;
    nbN = (N + 255) / 256;
    TMI_HIP(s->alloc(&x, (size_t)N));
    const std::vector<double> ones((size_t)N, 1.0);  // the scales without jacobi_scaling
    TMI_HIP(s->upload(&scale, ones.data(), ones.size()));
    TMI_HIP(hipStreamSynchronize(s->stream));  // (ones goes out of scope)
    TMI_HIP(s->alloc(&cand, (size_t)N));
    TMI_HIP(s->alloc(&step, (size_t)N));
    TMI_HIP(s->alloc(&y, (size_t)N));
    TMI_HIP(s->alloc(&rhs, (size_t)N));
    TMI_HIP(s->alloc(&diag, (size_t)N));
    TMI_HIP(s->alloc(&g, (size_t)N));
    TMI_HIP(s->alloc(&gabs, (size_t)N));
    TMI_HIP(s->alloc(&M, (size_t)N * N));  // the assembled normal matrix, kept across rejected steps
    TMI_HIP(s->alloc(&part, (size_t)2 * nbE + (size_t)2 * nbN));
    int rc;
    if ((rc = damped.alloc(s, N, 1, factorizations))) return rc;
    if ((rc = F.alloc(s, damped.flag))) return rc;
    p_cost = part;
    p_mcc = p_cost + nbE;
    p_step = p_mcc + nbE;
    p_x = p_step + nbN;
    F.set(0, p_cost, nbE);
    F.set(1, p_mcc, nbE);
    F.set(2, p_step, nbN);
    F.set(3, p_x, nbN);
    F.absmax = gabs;
    F.absmax_n = N;
    return TMI_BA_OK;
  }
};

// Ceres 1.14's TrustRegionMinimizer with the Levenberg-Marquardt strategy on the dense normal equations, the rules of
// tmi_ba_solver_solve (steps 6 and 7 of tmi_ba_estimate_global_positions_nonlinear).  x_h [N] is the start and receives
// the last accepted point.  linearize(first_scaled) queues, at L.x: the records, the residuals and the cost parts
// (L.p_cost), the Jacobi scales into L.scale where first_scaled, then L.M, L.diag, L.g and L.gabs.  candidate() queues, at
// L.cand with L.step: the cost parts and the parts of the model cost change (L.p_mcc).  Opt has the trust-region fields of
// tmi_ba_nonlinear_position_options; Sum the counters and times of tmi_ba_nonlinear_position_summary.
// Device time: an iteration's damped copy and factorisation, its substitution, then the step, the candidate and the
// reductions; a linearisation with its assembly is read after the next synchronisation (ClassSeconds' deferred marks).
template <class Opt, class Sum, class Linearize, class Candidate>
int normal_lm_solve(OneShot* s, const Opt* opt, Sum* sum, NormalLm& L, std::vector<double>& x_h, Linearize linearize_at,
                    Candidate candidate_at) {
  const int N = L.N, nbE = L.nbE, nbN = L.nbN, max_it = opt->max_num_iterations;
  double*& d_x = L.x;
  double*& d_cand = L.cand;
  double *d_step = L.step, *d_y = L.y, *d_rhs = L.rhs, *d_scale = L.scale, *d_diag = L.diag, *d_g = L.g, *d_M = L.M;
  double *p_mcc = L.p_mcc, *p_step = L.p_step, *p_x = L.p_x;
  DenseSpd& damped = L.damped;
  ScalarFetch& F = L.F;
  const double* h_norms = F.h_norms;
  std::vector<double>&cost_trace = L.cost_trace, &radius_trace = L.radius_trace;
  std::vector<int32_t>& outcome_trace = L.outcome_trace;
  hipStream_t st = s->stream;
  const dim3 entry_grid(nbN), block(256);
  TMI_HIP(hipMemcpyAsync(d_x, x_h.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
  TMI_HIP(hipMemsetAsync(d_y, 0, (size_t)N * sizeof(double), st));
  ClassSeconds T(st);
  TMI_HIP(T.status());
  // records, residuals and the cost parts at d_x, then M, its diagonal and the gradient
  bool scaled = !opt->jacobi_scaling;
  auto linearize = [&]() -> int {
    TMI_HIP(T.begin_deferred());
    linearize_at(!scaled);
    scaled = true;
    TMI_HIP(T.end_deferred());
    return TMI_BA_OK;
  };
  int rc;

  // ---- the first linearisation, its cost and |x| (the step kernel on y = 0) ----
  if ((rc = linearize())) return rc;
  hipLaunchKernelGGL(nlp_step_kernel, entry_grid, block, 0, st, N, d_x, d_scale, d_y, d_step, d_cand, p_step, p_x);
  TMI_HIP(hipMemsetAsync(p_mcc, 0, (size_t)nbE * sizeof(double), st));
  if ((rc = F.fetch(s, &T, 4))) return rc;
  double cost = h_norms[0], x_norm = std::sqrt(h_norms[3]);
  sum->initial_cost = cost;

  double radius = opt->initial_trust_region_radius, decrease_factor = 2.0;
  int invalid_run = 0, iter = 0, termination = 1;
  bool need_gradient_check = true;
  cost_trace.push_back(cost);
  radius_trace.push_back(radius);
  outcome_trace.push_back(1);
  auto record = [&](int outcome) {
    cost_trace.push_back(cost);
    radius_trace.push_back(radius);
    outcome_trace.push_back(outcome);
  };
  for (;;) {
    if (iter >= max_it) break;
    ++iter;
    TMI_HIP(T.begin(T.kFactor));
    hipLaunchKernelGGL(nlp_copy_lower_kernel, dim3(N), block, 0, st, N, d_M, damped.A);
    hipLaunchKernelGGL(nlp_lm_diagonal_kernel, entry_grid, block, 0, st, N, d_diag, opt->min_lm_diagonal,
                       opt->max_lm_diagonal, radius, damped.A);
    damped.factor(st);
    TMI_HIP(T.begin(T.kSubstitution));
    TMI_HIP(hipMemcpyAsync(d_rhs, d_g, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
    damped.substitute<1>(st, d_rhs, d_y);
    TMI_HIP(T.begin(T.kGraph));
    hipLaunchKernelGGL(nlp_step_kernel, entry_grid, block, 0, st, N, d_x, d_scale, d_y, d_step, d_cand, p_step, p_x);
    candidate_at();
    if ((rc = F.fetch(s, &T, 4))) return rc;
    bool usable = true;
    if (F.flag()) {  // a non-positive pivot: the linear solve failed, an invalid step as in Ceres
      usable = false;
      TMI_HIP(F.clear_flag(st));
    }
    if (need_gradient_check) {
      need_gradient_check = false;
      if (!(h_norms[4] > opt->gradient_tolerance)) {
        termination = 0;
        --iter;
        break;
      }
    }
    const double cand_cost = h_norms[0], model_cost_change = h_norms[1], step_sq = h_norms[2], cand_x_sq = h_norms[3];
    if (!(model_cost_change > 0.0)) usable = false;
    if (!usable) {
      // HandleInvalidStep
      sum->num_unsuccessful_steps++;
      if (++invalid_run >= opt->max_num_consecutive_invalid_steps) {
        record(-1);
        termination = 2;
        break;
      }
      radius /= decrease_factor;
      decrease_factor *= 2.0;
      record(-1);
      if (radius < opt->min_trust_region_radius) {
        termination = 0;
        break;
      }
      continue;
    }
    invalid_run = 0;
    if (std::sqrt(step_sq) <= opt->parameter_tolerance * (x_norm + opt->parameter_tolerance)) {
      record(2);
      termination = 0;
      break;
    }
    const double cost_change = cost - cand_cost;
    if (std::fabs(cost_change) <= opt->function_tolerance * cost) {
      record(3);
      termination = 0;
      break;
    }
    const double relative_decrease = cost_change / model_cost_change;
    if (relative_decrease > opt->min_relative_decrease) {  // IsStepSuccessful
      std::swap(d_x, d_cand);
      cost = cand_cost;
      x_norm = std::sqrt(cand_x_sq);
      sum->num_successful_steps++;
      radius = radius / std::fmax(1.0 / 3.0, 1.0 - std::pow(2.0 * relative_decrease - 1.0, 3));
      radius = std::fmin(opt->max_trust_region_radius, radius);
      decrease_factor = 2.0;
      if ((rc = linearize())) return rc;
      need_gradient_check = true;
      record(1);
    } else {
      sum->num_unsuccessful_steps++;
      radius /= decrease_factor;
      decrease_factor *= 2.0;
      record(0);
    }
    if (radius < opt->min_trust_region_radius) {
      termination = 0;
      break;
    }
  }

  TMI_HIP(s->download(x_h.data(), d_x, (size_t)N));
  TMI_HIP(hipStreamSynchronize(st));
  T.collect();
  sum->num_iterations = iter;
  sum->termination = termination;
  sum->usable = termination != 2;
  sum->final_cost = cost;
  T.write(sum);
  return TMI_BA_OK;
}

// What the nonlinear position estimator asks of its arguments beyond check_view_pair_batch, the connection to fixed_view
// apart; empty: fine.  Nothing is allocated here.
std::string check_nonlinear_position_arguments(const tmi_ba_view_pair_batch* B,
                                               const tmi_ba_nonlinear_position_options* o, int fixed_view,
                                               const double* view_position) {
  if (B->num_pairs == 0) return "nonlinear positions: no view pair";
  if (fixed_view < 0 || fixed_view >= B->num_views) return "nonlinear positions: fixed_view out of range";
  const std::string why = trust_region_options_error(o, "nonlinear positions", " (the reference CHECK_GTs it)");
  if (!why.empty()) return why;
  if (o->positions_given && !all_finite(view_position, (size_t)3 * B->num_views))
    return "nonlinear positions: positions_given with a non-finite position";
  return std::string();
}

// Component k of view v of the random start: 100 (2 u - 1), u from word 3 v + k of the splitmix64 stream of `seed`.
double nonlinear_position_start(uint64_t seed, int v, int k) {
  uint64_t z = seed + ((uint64_t)3 * (uint64_t)v + (uint64_t)k + 1) * 0x9e3779b97f4a7c15ULL;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  z ^= z >> 31;
  const double u = ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  const double centred = 2.0 * u - 1.0;
  return 100.0 * centred;
}
}  // namespace
extern "C" {

void tmi_ba_nonlinear_position_options_init(tmi_ba_nonlinear_position_options* o) {
  if (!o) return;
  set_trust_region_options(o, ceres_default_lm_args(400, TMI_BA_LOSS_HUBER, 0.1));  // nonlinear_position_estimator.h:70-72
  o->positions_given = 0;
  o->seed = 0;
}

int32_t tmi_ba_estimate_global_positions_nonlinear(const tmi_ba_view_pair_batch* Bh,
                                                   const tmi_ba_nonlinear_position_options* opt, int32_t fixed_view,
                                                   int32_t device, double* view_position, double* initial_position,
                                                   double* iteration_cost, double* iteration_radius,
                                                   int32_t* iteration_step_accepted, double* pair_residual,
                                                   tmi_ba_nonlinear_position_summary* sum) {
  if (!Bh || !opt || !view_position || !sum)
    return bad_argument("nonlinear positions: null batch, options, view_position or summary");
  memset(sum, 0, sizeof(*sum));
  sum->termination = 2;
  const double t0 = now_s();
  // argument errors before the device is touched
  if (const char* why = check_view_pair_batch(Bh, false, Bh->pair_position2)) return bad_argument(why);
  const std::string why = check_nonlinear_position_arguments(Bh, opt, fixed_view, view_position);
  if (!why.empty()) return bad_argument(why.c_str());
  const int V = Bh->num_views, E = Bh->num_pairs, n = V - 1;
  // the cap before anything of the views' size is allocated, the union-find included
  if ((int64_t)3 * n > rotation_order_cap()) {
    g_last_error = "nonlinear positions: 3 (num_views - 1) exceeds the dense solver's cap (see the header)";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  const int N = 3 * n;  // (<= the cap)
  if (!view_components(V, E, Bh->pair_view1, Bh->pair_view2).all_reach(fixed_view))
    return bad_argument("nonlinear positions: a view is not connected to fixed_view");
  const EdgeRows rows = build_edge_rows(V, E, Bh->pair_view1, Bh->pair_view2, fixed_view);
  // the start: x [n][3] over the free views
  std::vector<double> start((size_t)3 * V);
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < 3; ++k)
      start[(size_t)3 * v + k] = v == fixed_view ? 0.0
                                 : opt->positions_given ? view_position[(size_t)3 * v + k]
                                                        : nonlinear_position_start(opt->seed, v, k);
  std::vector<double> x_h((size_t)N);
  gather_free(V, fixed_view, nullptr, start.data(), x_h.data());
  const double width = opt->robust_loss_width;
  return one_shot_batch(device, "nonlinear positions: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    int rc;
    double *d_pos, *d_t, *d_rot = nullptr, *d_rec, *d_res;
    TMI_HIP(s->upload(&d_pos, Bh->pair_position2, (size_t)3 * E));
    d_t = d_pos;
    if (Bh->view_rotation) {
      TMI_HIP(s->upload(&d_rot, Bh->view_rotation, (size_t)3 * V));
      TMI_HIP(s->alloc(&d_t, (size_t)3 * E));
    }
    PoseGraphDevice graph;
    if ((rc = graph.upload(s, V, fixed_view, rows, E, Bh->pair_view1, Bh->pair_view2, d_t))) return rc;
    const PoseGraph& G = graph.G;
    TMI_HIP(s->alloc(&d_rec, (size_t)9 * E));
    TMI_HIP(s->alloc(&d_res, (size_t)3 * E));
    NormalLm L;
    if ((rc = L.alloc(s, N, E, &sum->num_factorizations))) return rc;
    hipStream_t st = s->stream;
    const dim3 edge_grid(L.nbE), view_grid((n + 255) / 256), block(256);
    // the directions, then the loop
    if (Bh->view_rotation)
      hipLaunchKernelGGL(lud_direction_kernel, edge_grid, block, 0, st, E, d_rot, G.pair_view1, d_pos, d_t);
    rc = normal_lm_solve(
        s, opt, sum, L, x_h,
        [&](bool first_scaled) {
          hipLaunchKernelGGL(nlp_edge_kernel<true>, edge_grid, block, 0, st, G, width, L.x, nullptr, d_rec, d_res,
                             L.p_cost, nullptr);
          if (first_scaled)
            hipLaunchKernelGGL(nlp_scale_kernel<nlp::PositionBlocks>, view_grid, block, 0, st, G, n, d_rec, L.scale);
          hipLaunchKernelGGL(nlp_assemble_kernel<nlp::PositionBlocks>, dim3(n), block, 0, st, G, N, d_rec, L.scale, L.M,
                             L.diag, L.g, L.gabs);
        },
        [&]() {
          hipLaunchKernelGGL(nlp_edge_kernel<false>, edge_grid, block, 0, st, G, width, L.cand, L.step, d_rec, nullptr,
                             L.p_cost, L.p_mcc);
        });
    if (rc) return rc;
    std::vector<double> res_h(pair_residual ? (size_t)3 * E : 0);
    if (pair_residual) {
      TMI_HIP(s->download(res_h.data(), d_res, res_h.size()));
      TMI_HIP(hipStreamSynchronize(st));
    }
    // the results, only now: a failure above leaves the caller's arrays as they were
    scatter_free(V, fixed_view, nullptr, x_h.data(), view_position);
    std::fill(view_position + (size_t)3 * fixed_view, view_position + (size_t)3 * fixed_view + 3, 0.0);
    if (initial_position) std::copy(start.begin(), start.end(), initial_position);
    if (pair_residual) std::copy(res_h.begin(), res_h.end(), pair_residual);
    if (iteration_cost) std::copy(L.cost_trace.begin(), L.cost_trace.end(), iteration_cost);
    if (iteration_radius) std::copy(L.radius_trace.begin(), L.radius_trace.end(), iteration_radius);
    if (iteration_step_accepted) std::copy(L.outcome_trace.begin(), L.outcome_trace.end(), iteration_step_accepted);
    sum->num_views = V;
    sum->num_pairs = E;
    return TMI_BA_OK;
  });
}

// ---- NonlinearRotationEstimator (rotation_nonlinear_kernels.h) ----------------------------------
void tmi_ba_nonlinear_rotation_options_init(tmi_ba_nonlinear_rotation_options* o) {
  if (!o) return;
  // nonlinear_rotation_estimator.h (width 0.1), nonlinear_rotation_estimator.cc:94 (200 iterations)
  set_trust_region_options(o, ceres_default_lm_args(200, TMI_BA_LOSS_SOFTLONE, 0.1));
  o->fixed_view = -1;
}

int32_t tmi_ba_estimate_global_rotations_nonlinear(const tmi_ba_view_pair_batch* Bh,
                                                   const tmi_ba_nonlinear_rotation_options* opt,
                                                   const uint8_t* view_given, int32_t device, double* view_rotation,
                                                   double* iteration_cost, double* iteration_radius,
                                                   int32_t* iteration_step_accepted, double* pair_residual,
                                                   tmi_ba_nonlinear_rotation_summary* sum) {
  if (!Bh || !opt || !view_rotation || !sum)
    return bad_argument("nonlinear rotations: null batch, options, view_rotation or summary");
  memset(sum, 0, sizeof(*sum));
  sum->termination = 2;
  const double t0 = now_s();
  // argument errors before the device is touched; the batch's own view_rotation is not this call's
  tmi_ba_view_pair_batch checked = *Bh;
  checked.view_rotation = nullptr;
  if (const char* why = check_view_pair_batch(&checked, false, Bh->pair_rotation2)) return bad_argument(why);
  const int V = Bh->num_views, E_all = Bh->num_pairs, fixed_view = opt->fixed_view;
  // the reference's two refusals (nonlinear_rotation_estimator.cc:53-62)
  if (E_all == 0) return bad_argument("nonlinear rotations: no relative rotation constraint");
  int num_given = 0;
  for (int v = 0; v < V; ++v) num_given += !view_given || view_given[v];
  if (num_given == 0) return bad_argument("nonlinear rotations: no view has an initialisation");
  if (fixed_view < -1 || fixed_view >= V) return bad_argument("nonlinear rotations: fixed_view out of range");
  if (fixed_view >= 0 && view_given && !view_given[fixed_view])
    return bad_argument("nonlinear rotations: fixed_view has no initialisation");
  const std::string why = trust_region_options_error(opt, "nonlinear rotations", "");
  if (!why.empty()) return bad_argument(why.c_str());
  for (int v = 0; v < V; ++v)
    if ((!view_given || view_given[v]) && !all_finite(view_rotation + (size_t)3 * v, 3))
      return bad_argument("nonlinear rotations: a marked view with a non-finite rotation");
  // the problem: the edges between marked views in the caller's order, and the marked views with such an edge
  const ViewSubset P = build_view_subset(V, E_all, Bh->pair_view1, Bh->pair_view2, view_given);
  const int E = (int)P.edge_of.size(), Vp = (int)P.view_of.size();
  // the held view's index in the problem; Vp: no view is held
  const int held = fixed_view >= 0 && P.view_index[fixed_view] >= 0 ? P.view_index[fixed_view] : Vp;
  const int n = held < Vp ? Vp - 1 : Vp;
  // the cap before anything of the views' size is allocated
  if ((int64_t)3 * n > rotation_order_cap()) {
    g_last_error = "nonlinear rotations: 3 (free views) exceeds the dense solver's cap (see the header)";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  const int N = 3 * n;  // (<= the cap)
  std::vector<double> rel((size_t)3 * E), x_h((size_t)N), held_h(3, 0.0);
  for (int e = 0; e < E; ++e)
    std::copy(Bh->pair_rotation2 + (size_t)3 * P.edge_of[e], Bh->pair_rotation2 + (size_t)3 * P.edge_of[e] + 3,
              rel.begin() + (size_t)3 * e);
  gather_free(Vp, held, P.view_of.data(), view_rotation, x_h.data());
  if (held < Vp) std::copy(view_rotation + (size_t)3 * P.view_of[held], view_rotation + (size_t)3 * P.view_of[held] + 3,
                           held_h.begin());
  const EdgeRows rows = build_edge_rows(Vp, E, P.v1.data(), P.v2.data(), held);
  const double width = opt->robust_loss_width;
  if (E == 0) {  // an empty problem: solved
    sum->termination = 0;
    sum->usable = 1;
  }
  return one_shot_batch(device, "nonlinear rotations: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    int rc;  // (an edge has two views, so n >= 1)
    double *d_rel, *d_held, *d_rec, *d_res;
    TMI_HIP(s->upload(&d_rel, rel.data(), rel.size()));
    TMI_HIP(s->upload(&d_held, held_h.data(), held_h.size()));
    PoseGraphDevice graph;
    if ((rc = graph.upload(s, Vp, held, rows, E, P.v1.data(), P.v2.data(), d_rel))) return rc;
    const PoseGraph& G = graph.G;
    TMI_HIP(s->alloc(&d_rec, (size_t)nlr::kRecordPlanes * E));
    TMI_HIP(s->alloc(&d_res, (size_t)3 * E));
    NormalLm L;
    if ((rc = L.alloc(s, N, E, &sum->num_factorizations))) return rc;
    hipStream_t st = s->stream;
    const dim3 edge_grid(L.nbE), view_grid((n + 255) / 256), block(256);
    rc = normal_lm_solve(
        s, opt, sum, L, x_h,
        [&](bool first_scaled) {
          hipLaunchKernelGGL(nlr_edge_kernel<true>, edge_grid, block, 0, st, G, width, L.x, nullptr, d_held, d_rec,
                             d_res, L.p_cost, nullptr);
          if (first_scaled)
            hipLaunchKernelGGL(nlp_scale_kernel<nlr::RotationBlocks>, view_grid, block, 0, st, G, n, d_rec, L.scale);
          hipLaunchKernelGGL(nlp_assemble_kernel<nlr::RotationBlocks>, dim3(n), block, 0, st, G, N, d_rec, L.scale, L.M,
                             L.diag, L.g, L.gabs);
        },
        [&]() {
          hipLaunchKernelGGL(nlr_edge_kernel<false>, edge_grid, block, 0, st, G, width, L.cand, L.step, d_held, d_rec,
                             nullptr, L.p_cost, L.p_mcc);
        });
    if (rc) return rc;
    std::vector<double> res_h(pair_residual ? (size_t)3 * E : 0);
    if (pair_residual) {
      TMI_HIP(s->download(res_h.data(), d_res, res_h.size()));
      TMI_HIP(hipStreamSynchronize(st));
    }
    // the results, only now: a failure above leaves the caller's arrays as they were (the held view's is not written)
    scatter_free(Vp, held, P.view_of.data(), x_h.data(), view_rotation);
    if (pair_residual) {
      std::fill(pair_residual, pair_residual + (size_t)3 * E_all, 0.0);
      for (int e = 0; e < E; ++e)
        std::copy(res_h.begin() + (size_t)3 * e, res_h.begin() + (size_t)3 * e + 3, pair_residual + (size_t)3 * P.edge_of[e]);
    }
    if (iteration_cost) std::copy(L.cost_trace.begin(), L.cost_trace.end(), iteration_cost);
    if (iteration_radius) std::copy(L.radius_trace.begin(), L.radius_trace.end(), iteration_radius);
    if (iteration_step_accepted) std::copy(L.outcome_trace.begin(), L.outcome_trace.end(), iteration_step_accepted);
    sum->num_views = Vp;
    sum->num_pairs = E;
    return TMI_BA_OK;
  });
}

// ---- LinearRotationEstimator (rotation_linear_kernels.h) -----------------------------------------
void tmi_ba_linear_rotation_options_init(tmi_ba_linear_rotation_options* o) {
  if (!o) return;
  o->max_iterations = 1000;  // Spectra's maxit and tol, which linear_rotation_estimator.cc:173-177 leaves alone
  o->tolerance = 1e-10;
  o->relative_shift = 1e-9;  // 200 x the factorisation's rounding n eps 2 at the order cap
  o->seed = 0;
}

int32_t tmi_ba_estimate_global_rotations_linear(const tmi_ba_view_pair_batch* Bh,
                                                const tmi_ba_linear_rotation_options* opt, int32_t device,
                                                double* view_rotation, tmi_ba_linear_rotation_summary* sum) {
  if (!Bh || !opt || !view_rotation || !sum)
    return bad_argument("linear rotations: null batch, options, view_rotation or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is touched; the batch's own view_rotation is not this call's
  tmi_ba_view_pair_batch checked = *Bh;
  checked.view_rotation = nullptr;
  if (const char* why = check_view_pair_batch(&checked, false, Bh->pair_rotation2)) return bad_argument(why);
  const int V = Bh->num_views, E = Bh->num_pairs;
  if (E == 0) return bad_argument("linear rotations: no relative rotation constraint (the reference CHECK_GTs them)");
  if (opt->max_iterations <= 0) return bad_argument("linear rotations: max_iterations is not positive");
  if (!(opt->tolerance > 0.0) || !std::isfinite(opt->tolerance))
    return bad_argument("linear rotations: tolerance is not positive and finite");
  if (!(opt->relative_shift >= 0.0) || !std::isfinite(opt->relative_shift))
    return bad_argument("linear rotations: relative_shift is negative or not finite");
  // the views of the problem: those with an edge, in ascending index
  const ViewSubset P = build_view_subset(V, E, Bh->pair_view1, Bh->pair_view2, nullptr);
  const int Vp = (int)P.view_of.size();
  // the cap before anything of the matrix's size is allocated
  if ((int64_t)3 * Vp > rotation_order_cap()) {
    g_last_error = "linear rotations: 3 (views with an edge) exceeds the dense solver's cap (see the header)";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  const int n = 3 * Vp;  // (<= the cap)
  if (view_components(Vp, E, P.v1.data(), P.v2.data()).count != 1)
    return bad_argument("linear rotations: the view pairs are not connected (with c components the null space has 3 c "
                        "dimensions; RemoveDisconnectedViewPairs comes first)");
  const EdgeRows rows = build_edge_rows(Vp, E, P.v1.data(), P.v2.data(), Vp);
  int max_degree = 0;
  for (int p = 0; p < Vp; ++p) max_degree = std::max(max_degree, rows.row_ptr[(size_t)p + 1] - rows.row_ptr[p]);
  const double lambda_bound = 2.0 * (double)max_degree;  // Gershgorin
  const double mu = opt->relative_shift * (double)max_degree;
  const double threshold = opt->tolerance * lambda_bound;
  return one_shot_batch(device, "linear rotations: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    int rc;
    hipStream_t st = s->stream;
    const int nb = (n + 255) / 256;
    const size_t block_words = (size_t)n * lin::kBlock;
    int* d_refl;
    double *d_rel, *d_R, *d_Q, *d_Y, *d_Z, *d_W, *d_mgs[2], *d_gram, *d_res[3], *d_rot;
    TMI_HIP(s->upload(&d_rel, Bh->pair_rotation2, (size_t)3 * E));
    TMI_HIP(s->alloc(&d_R, (size_t)9 * E));
    PoseGraphDevice graph;  // no view is held
    if ((rc = graph.upload(s, Vp, Vp, rows, E, P.v1.data(), P.v2.data(), d_R))) return rc;
    const PoseGraph& G = graph.G;
    TMI_HIP(s->alloc(&d_Q, block_words));
    TMI_HIP(s->alloc(&d_Y, block_words));
    TMI_HIP(s->alloc(&d_Z, block_words));
    TMI_HIP(s->alloc(&d_W, block_words));
    for (double*& p : d_mgs) TMI_HIP(s->alloc(&p, (size_t)nb * lin::kBlock));
    TMI_HIP(s->alloc(&d_gram, (size_t)nb * lin::kGram));
    for (double*& p : d_res) TMI_HIP(s->alloc(&p, (size_t)nb));
    TMI_HIP(s->alloc(&d_rot, (size_t)3 * Vp));
    TMI_HIP(s->alloc(&d_refl, (size_t)Vp));
    DenseSpd shifted;  // M + mu I, overwritten by its factor; kBlock right-hand sides
    if ((rc = shifted.alloc(s, n, lin::kBlock, nullptr))) return rc;
    ScalarFetch F;  // the small block: its last three words are the sums of the residuals' parts
    if ((rc = F.alloc(s, shifted.flag, lin::kSmallWords))) return rc;
    for (int q = 0; q < 3; ++q) F.set(q, d_res[q], nb);
    double* d_small = F.d_norms;
    const double* h_small = F.h_norms;
    const dim3 block(256), rows_grid(nb);
    sum->num_views = Vp;
    sum->num_pairs = E;
    sum->order = n;
    ClassSeconds T(st);
    TMI_HIP(T.status());

    // ---- the matrix, its factor and the start block ----
    TMI_HIP(T.begin(T.kGraph));
    hipLaunchKernelGGL(lin_edge_matrix_kernel, dim3((E + 255) / 256), block, 0, st, E, d_rel, d_R);
    hipLaunchKernelGGL(lin_assemble_kernel, dim3(Vp), block, 0, st, G, n, mu, shifted.A);
    TMI_HIP(T.begin(T.kFactor));
    shifted.factor(st);
    TMI_HIP(T.begin(T.kGraph));
    hipLaunchKernelGGL(lin_start_kernel, dim3(((int)block_words + 255) / 256), block, 0, st, n, (unsigned long long)opt->seed,
                       d_Q);
    if ((rc = F.fetch(s, &T, 0))) return rc;  // (no sum yet: the pivot flag alone)
    if (F.flag()) {  // a pivot of M + mu I that is not positive: nothing is written
      T.write(sum);
      return TMI_BA_OK;
    }
    sum->usable = 1;

    // ---- subspace iteration with Rayleigh-Ritz ----
    int iter = 0, launches = 0;
    bool converged = false;
    while (iter < opt->max_iterations && !converged) {
      ++iter;
      TMI_HIP(T.begin(T.kSubstitution));
      TMI_HIP(hipMemcpyAsync(d_W, d_Q, block_words * sizeof(double), hipMemcpyDeviceToDevice, st));
      shifted.substitute<lin::kBlock>(st, d_W, d_Y);
      TMI_HIP(T.begin(T.kGraph));
      for (int pass = 0; pass < 2; ++pass)
        for (int j = 0; j <= lin::kBlock; ++j, ++launches)
          hipLaunchKernelGGL(lin_mgs_kernel, rows_grid, block, 0, st, n, j, d_Y, d_mgs[(launches + 1) & 1],
                             d_mgs[launches & 1]);
      hipLaunchKernelGGL(lin_apply_kernel, dim3((Vp * lin::kBlock + 255) / 256), block, 0, st, G, d_Y, d_Z);
      hipLaunchKernelGGL(lin_gram_kernel, rows_grid, block, 0, st, n, d_Y, d_Z, d_gram);
      hipLaunchKernelGGL(lin_ritz_kernel, dim3(1), dim3(64), 0, st, d_gram, nb, d_small);
      hipLaunchKernelGGL(lin_rotate_kernel, rows_grid, block, 0, st, n, d_small, d_Y, d_Z, d_Q, d_res[0], d_res[1],
                         d_res[2]);
      // the whole small block, without the flag: the factor is not touched again
      if ((rc = F.fetch(s, &T, 3, lin::kSmallResidual, lin::kSmallWords, /*with_flag=*/false))) return rc;
      converged = true;
      for (int j = 0; j < 3; ++j) {
        sum->residual[j] = std::sqrt(h_small[lin::kSmallResidual + j]);
        converged = converged && sum->residual[j] <= threshold;
      }
    }
    for (int j = 0; j < 4; ++j) sum->eigenvalue[j] = h_small[lin::kSmallTheta + j];
    sum->num_iterations = iter;
    sum->converged = converged;

    // ---- the projection of the last Ritz vectors ----
    std::vector<double> rot_h((size_t)3 * Vp);
    std::vector<int> refl_h((size_t)Vp);
    TMI_HIP(T.begin(T.kGraph));
    hipLaunchKernelGGL(lin_project_kernel, dim3((Vp + 255) / 256), block, 0, st, Vp, d_Q, d_rot, d_refl);
    TMI_HIP(T.end());
    TMI_HIP(s->download(rot_h.data(), d_rot, rot_h.size()));
    TMI_HIP(s->download(refl_h.data(), d_refl, refl_h.size()));
    ReadBack rb(st);  // (the launch error is taken after the copies here)
    TMI_HIP(rb.finish());
    T.collect();
    T.write(sum);
    // the results, only now: a failure above leaves the caller's array as it was
    for (int p = 0; p < Vp; ++p) {
      std::copy(rot_h.begin() + (size_t)3 * p, rot_h.begin() + (size_t)3 * p + 3, view_rotation + (size_t)3 * P.view_of[p]);
      sum->num_reflected += refl_h[p];
    }
    return TMI_BA_OK;
  });
}
}  // extern "C"

// ---- LinearPositionEstimator (position_linear_kernels.h) ------------------------------------------
namespace {
// What the linear position estimator asks of its batch and options; null: fine.
const char* check_linear_position_arguments(const tmi_ba_view_pair_batch* B, const tmi_ba_linear_position_options* o) {
  const int V = B->num_views, E = B->num_pairs;
  if (V < 0 || E < 0) return "linear positions: negative size";
  if (E == 0) return "linear positions: no view pair";
  if (!B->pair_view1 || !B->pair_view2 || !B->pair_rotation2 || !B->pair_position2 || !B->view_rotation)
    return "linear positions: missing array";
  if (E > (1 << 30)) return "linear positions: more than 2^30 pairs";
  std::vector<uint64_t> keys((size_t)E);
  std::vector<uint8_t> has_edge((size_t)V, 0);
  for (int e = 0; e < E; ++e) {
    const int a = B->pair_view1[e], b = B->pair_view2[e];
    if (a < 0 || a >= V || b < 0 || b >= V) return "linear positions: view index out of range";
    if (a >= b) return "linear positions: pair_view1 >= pair_view2 (the reference's ViewIdPair keys are ordered)";
    keys[e] = ((uint64_t)a << 32) | (uint64_t)b;
    has_edge[a] = has_edge[b] = 1;
  }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return "linear positions: a pair appears twice";
  if (!all_finite(B->pair_rotation2, (size_t)3 * E) || !all_finite(B->pair_position2, (size_t)3 * E))
    return "linear positions: non-finite rotation_2 or position_2";
  for (int v = 0; v < V; ++v)
    if (has_edge[v] && !all_finite(B->view_rotation + (size_t)3 * v, 3))
      return "linear positions: non-finite orientation of a view with an edge";
  if (o->max_iterations <= 0) return "linear positions: max_iterations is not positive";
  if (!(o->tolerance > 0.0) || !std::isfinite(o->tolerance)) return "linear positions: tolerance is not positive and finite";
  if (!(o->relative_shift >= 0.0) || !std::isfinite(o->relative_shift))
    return "linear positions: relative_shift is negative or not finite";
  if (!(o->min_triangulation_angle_degrees > 0.0) || !(o->min_triangulation_angle_degrees < 180.0))
    return "linear positions: min_triangulation_angle_degrees outside (0, 180)";
  return nullptr;
}
}  // namespace
extern "C" {

void tmi_ba_linear_position_options_init(tmi_ba_linear_position_options* o) {
  if (!o) return;
  o->max_iterations = 1000;  // Spectra's maxit and tol, which linear_position_estimator.cc:200-205 leaves alone
  o->tolerance = 1e-10;
  o->relative_shift = 1e-9;  // as tmi_ba_linear_rotation_options
  o->seed = 0;
  o->min_triangulation_angle_degrees = 2.0;  // compute_triplet_baseline_ratios.cc:60
}

int32_t tmi_ba_estimate_global_positions_linear(const tmi_ba_problem* P, const tmi_ba_view_pair_batch* Bh,
                                                const tmi_ba_linear_position_options* opt, int32_t device,
                                                double* view_position, uint8_t* view_estimated,
                                                int32_t triplet_capacity, int32_t* triplet_view, int32_t* triplet_pair,
                                                double* triplet_baseline, int32_t* triplet_num_common,
                                                int32_t* triplet_num_used, int32_t* triplet_component,
                                                tmi_ba_linear_position_summary* sum) {
  if (!P || !Bh || !opt || !view_position || !view_estimated || !sum)
    return bad_argument("linear positions: null problem, batch, options, view_position, view_estimated or summary");
  memset(sum, 0, sizeof(*sum));
  const double t0 = now_s();
  // argument errors before the device is looked for
  if (const char* why = check_linear_position_arguments(Bh, opt)) return bad_argument(why);
  if (triplet_capacity < 0) return bad_argument("linear positions: negative triplet_capacity");
  const int V = Bh->num_views, E = Bh->num_pairs, G = P->num_groups;
  const int64_t No = P->num_observations;
  if (P->num_cameras != V) return bad_argument("linear positions: num_cameras differs from the batch's num_views");
  if (G < 0 || No < 0) return bad_argument("linear positions: negative size");
  if (!P->camera_group || (G && (!P->group_model || !P->group_offset)) || (No && (!P->obs_camera || !P->obs_point || !P->obs_xy)))
    return bad_argument("linear positions: missing array");
  if (No >= (int64_t)0x7fffffffLL) return bad_argument("linear positions: more than 2^31 observations");
  const int n_intr = G ? P->group_offset[G] : 0;
  if (n_intr && !P->intrinsics) return bad_argument("linear positions: missing intrinsics");
  for (int g = 0; g < G; ++g) {
    const int o = P->group_offset[g], nk = P->group_offset[g + 1] - o;
    if (P->group_model[g] < 0 || P->group_model[g] > 4 || nk != tmi_ba_intrinsics_size(P->group_model[g]) || o < 0)
      return bad_argument("linear positions: bad intrinsics group");
  }
  std::vector<int4> cam((size_t)V);
  for (int c = 0; c < V; ++c) {
    const int g = P->camera_group[c];
    if (g < 0 || g >= G) return bad_argument("linear positions: bad camera group");
    cam[c] = make_int4(P->group_model[g], P->group_offset[g], P->group_offset[g + 1] - P->group_offset[g], 0);
  }
  for (int64_t i = 0; i < No; ++i)
    if (P->obs_camera[i] < 0 || P->obs_camera[i] >= V || P->obs_point[i] < 0)
      return bad_argument("linear positions: bad observation index");
  const ViewTracks tracks = build_view_tracks(V, No, P->obs_camera, P->obs_point);
  if (tracks.repeated) return bad_argument("linear positions: a view observes a track twice");
  const SortedAdjacency adjacency = build_sorted_adjacency(V, E, Bh->pair_view1, Bh->pair_view2);
  std::vector<int> slot_cam((size_t)No);
  std::vector<double> slot_xy((size_t)2 * No);
  for (int v = 0; v < V; ++v)
    for (int r = tracks.ptr[v]; r < tracks.ptr[(size_t)v + 1]; ++r) {
      slot_cam[r] = v;
      slot_xy[(size_t)2 * r] = P->obs_xy[2 * tracks.obs[r]];
      slot_xy[(size_t)2 * r + 1] = P->obs_xy[2 * tracks.obs[r] + 1];
    }
  const double cos_min = std::cos(opt->min_triangulation_angle_degrees * (M_PI / 180.0));
  const int order_cap = rotation_order_cap();
  sum->num_views = V;
  sum->num_pairs = E;
  return one_shot_batch(device, "linear positions: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    int rc;
    hipStream_t st = s->stream;
    const dim3 block(256);
    auto grid = [](long long n) { return dim3((unsigned)std::max(1LL, (n + 255) / 256)); };
    const int slots = 2 * E;
    int *d_adj_ptr, *d_owner, *d_track_ptr, *d_track, *d_slot_cam, *d_count, *d_offset, *d_v1, *d_v2;
    int2* d_adj;
    int4* d_cam;
    double *d_slot_xy, *d_intr, *d_feature, *d_rot2, *d_pos2, *d_orient;
    unsigned long long *d_counters, *d_total;
    TMI_HIP(s->upload(&d_adj_ptr, adjacency.ptr.data(), adjacency.ptr.size()));
    TMI_HIP(s->upload(&d_adj, adjacency.adj.data(), adjacency.adj.size()));
    TMI_HIP(s->upload(&d_owner, adjacency.owner.data(), adjacency.owner.size()));
    TMI_HIP(s->upload(&d_track_ptr, tracks.ptr.data(), tracks.ptr.size()));
    TMI_HIP(s->upload(&d_track, tracks.track.data(), tracks.track.size()));
    TMI_HIP(s->upload(&d_slot_cam, slot_cam.data(), slot_cam.size()));
    TMI_HIP(s->upload(&d_slot_xy, slot_xy.data(), slot_xy.size()));
    TMI_HIP(s->upload(&d_cam, cam.data(), cam.size()));
    TMI_HIP(s->upload(&d_intr, (const double*)P->intrinsics, (size_t)n_intr));
    TMI_HIP(s->upload(&d_rot2, Bh->pair_rotation2, (size_t)3 * E));
    TMI_HIP(s->upload(&d_pos2, Bh->pair_position2, (size_t)3 * E));
    TMI_HIP(s->upload(&d_orient, Bh->view_rotation, (size_t)3 * V));
    TMI_HIP(s->upload(&d_v1, (const int*)Bh->pair_view1, (size_t)E));
    TMI_HIP(s->upload(&d_v2, (const int*)Bh->pair_view2, (size_t)E));
    TMI_HIP(s->alloc(&d_count, (size_t)slots));
    TMI_HIP(s->alloc(&d_offset, (size_t)slots + 1));
    TMI_HIP(s->alloc(&d_feature, (size_t)3 * No));
    TMI_HIP(s->alloc_filled(&d_counters, (size_t)lpos::kCounters, 0));
    TMI_HIP(s->alloc(&d_total, 2));
    StreamTimer triplet_timer(st, 4), baseline_timer(st, 2), component_timer(st, 2);
    TMI_HIP(triplet_timer.status);
    TMI_HIP(baseline_timer.status);
    TMI_HIP(component_timer.status);
    unsigned long long total_h[2] = {0, 0};

    // ---- step 1: the triangles, counted, scanned, filled ----
    TMI_HIP(triplet_timer.mark());
    hipLaunchKernelGGL(lpos_triplet_kernel<false>, dim3((slots + 3) / 4), block, 0, st, slots, d_adj_ptr, d_adj, d_owner,
                       d_track_ptr, d_count, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(lpos_scan_kernel, dim3(1), block, 0, st, d_count, slots, -1, d_offset, d_total);
    TMI_HIP(triplet_timer.mark());
    {
      ReadBack rb(st);
      rb.add(total_h, d_total, 1);
      TMI_HIP(rb.finish());
    }
    if (total_h[0] > (1ull << 30)) {
      s->error = "linear positions: more than 2^30 triplets";
      return TMI_BA_ERR_UNSUPPORTED;
    }
    const int T = (int)total_h[0];
    sum->num_triplets = T;
    sum->triplet_seconds = triplet_timer.seconds(0, 1);
    sum->kernel_seconds = sum->triplet_seconds;
    if (T == 0) return TMI_BA_OK;  // (usable = 0: nothing is written)
    int *d_tview, *d_tpair, *d_shortest, *d_scratch_at, *d_common, *d_used;
    unsigned *d_first, *d_link, *d_parent, *d_label, *d_size;
    double *d_baseline, *d_scratch;
    TMI_HIP(s->alloc(&d_tview, (size_t)3 * T));
    TMI_HIP(s->alloc(&d_tpair, (size_t)3 * T));
    TMI_HIP(s->alloc(&d_shortest, (size_t)T));
    TMI_HIP(s->alloc(&d_scratch_at, (size_t)T + 1));
    TMI_HIP(triplet_timer.mark());
    hipLaunchKernelGGL(lpos_triplet_kernel<true>, dim3((slots + 3) / 4), block, 0, st, slots, d_adj_ptr, d_adj, d_owner,
                       d_track_ptr, nullptr, d_offset, d_tview, d_tpair, d_shortest);
    hipLaunchKernelGGL(lpos_scan_kernel, dim3(1), block, 0, st, d_shortest, T, (int)lpos::kSelectCap, d_scratch_at,
                       d_total + 1);
    TMI_HIP(triplet_timer.mark());
    {
      ReadBack rb(st);
      rb.add(total_h + 1, d_total + 1, 1);
      TMI_HIP(rb.finish());
    }
    if (total_h[1] > (1ull << 30)) {
      s->error = "linear positions: the selection scratch of the triplets exceeds 2^30 ratios";
      return TMI_BA_ERR_UNSUPPORTED;
    }
    sum->triplet_seconds += triplet_timer.seconds(2, 3);

    // ---- steps 2 to 4: features, baselines, the components of the survivors ----
    TMI_HIP(s->alloc(&d_scratch, (size_t)total_h[1]));
    TMI_HIP(s->alloc(&d_baseline, (size_t)3 * T));
    TMI_HIP(s->alloc(&d_common, (size_t)T));
    TMI_HIP(s->alloc(&d_used, (size_t)T));
    TMI_HIP(s->alloc_filled(&d_first, (size_t)E, 0xff));
    TMI_HIP(s->alloc(&d_link, (size_t)6 * T));
    TMI_HIP(s->alloc(&d_parent, (size_t)T));
    TMI_HIP(s->alloc(&d_label, (size_t)T));
    TMI_HIP(s->alloc_filled(&d_size, (size_t)T, 0));
    TMI_HIP(baseline_timer.mark());
    hipLaunchKernelGGL(lpos_feature_kernel, grid(No), block, 0, st, (int)No, d_slot_cam, d_slot_xy, d_cam, d_intr, d_feature);
    hipLaunchKernelGGL(lpos_baseline_kernel, dim3(T), block, 0, st, d_tview, d_tpair, d_track_ptr, d_track, d_feature,
                       d_rot2, d_pos2, cos_min, d_shortest, d_scratch_at, d_scratch, d_baseline, d_common, d_used,
                       d_counters);
    TMI_HIP(baseline_timer.mark());
    TMI_HIP(component_timer.mark());
    hipLaunchKernelGGL(lpos_first_kernel, grid(T), block, 0, st, T, d_tpair, d_used, d_first);
    hipLaunchKernelGGL(lpos_link_kernel, grid(T), block, 0, st, T, d_tpair, d_used, d_first, d_link);
    hipLaunchKernelGGL(tb_iota_kernel, grid(T), block, 0, st, d_parent, (unsigned)T);
    hipLaunchKernelGGL(tb_union_kernel, grid((long long)3 * T), block, 0, st, d_link, (long long)3 * T, (unsigned)T,
                       d_parent, d_counters);
    hipLaunchKernelGGL(tb_flatten_kernel, grid(T), block, 0, st, d_parent, (unsigned)T, d_label, d_counters);
    hipLaunchKernelGGL(tb_sizes_kernel, grid(T), block, 0, st, d_label, (unsigned)T, d_size);
    hipLaunchKernelGGL(lpos_component_stats_kernel, grid(T), block, 0, st, T, d_used, d_label, d_size, d_counters);
    TMI_HIP(component_timer.mark());
    std::vector<int> tview_h((size_t)3 * T), tpair_h((size_t)3 * T), common_h((size_t)T), used_h((size_t)T);
    std::vector<unsigned> label_h((size_t)T);
    std::vector<double> baseline_h((size_t)3 * T);
    unsigned long long counters_h[lpos::kCounters];
    {
      ReadBack rb(st);
      rb.add(tview_h.data(), d_tview, tview_h.size());
      rb.add(tpair_h.data(), d_tpair, tpair_h.size());
      rb.add(common_h.data(), d_common, common_h.size());
      rb.add(used_h.data(), d_used, used_h.size());
      rb.add(label_h.data(), d_label, label_h.size());
      rb.add(baseline_h.data(), d_baseline, baseline_h.size());
      rb.add(counters_h, d_counters, (size_t)lpos::kCounters);
      TMI_HIP(rb.finish());
    }
    if (counters_h[lpos::kError]) {
      s->error = "linear positions: a device loop reached its bound";
      return TMI_BA_ERR_DEVICE;
    }
    sum->baseline_seconds = baseline_timer.seconds();
    double graph_before = component_timer.seconds();
    sum->graph_seconds = graph_before;
    sum->kernel_seconds = sum->triplet_seconds + sum->baseline_seconds + sum->graph_seconds;
    sum->num_dropped_ratios = (int64_t)counters_h[lpos::kDroppedRatios];
    sum->num_triplet_components = (int32_t)counters_h[lpos::kComponents];
    for (int t = 0; t < T; ++t) sum->num_triplets_with_baseline += used_h[t] > 0;
    if (!counters_h[lpos::kBest]) return TMI_BA_OK;  // no triplet survived: usable = 0, nothing is written
    const unsigned chosen_label = 0xffffffffu - (unsigned)counters_h[lpos::kBest];
    std::vector<int> chosen, cview, cpair;
    std::vector<double> cbase;
    for (int t = 0; t < T; ++t)
      if (used_h[t] > 0 && label_h[t] == chosen_label) {
        chosen.push_back(t);
        for (int k = 0; k < 3; ++k) {
          cview.push_back(tview_h[(size_t)3 * t + k]);
          cpair.push_back(tpair_h[(size_t)3 * t + k]);
          cbase.push_back(baseline_h[(size_t)3 * t + k]);
        }
      }
    const int C = (int)chosen.size();
    if ((unsigned long long)C != (counters_h[lpos::kBest] >> 32)) {
      s->error = "linear positions: the device reported impossible totals";
      return TMI_BA_ERR_DEVICE;
    }
    const TripletRows rows = build_triplet_rows(V, C, cview.data());
    const int Vc = (int)rows.views.size(), columns = Vc - 1;
    sum->num_chosen_triplets = C;
    sum->num_chosen_views = Vc;
    // the cap before anything of the matrix's size is allocated
    if ((int64_t)3 * columns > order_cap) {
      s->error = "linear positions: 3 (estimated views - 1) exceeds the dense solver's cap (see the header)";
      return TMI_BA_ERR_UNSUPPORTED;
    }
    const int n = 3 * columns;  // (<= the cap; >= 6: a triplet has three views)
    sum->order = n;

    // ---- step 5: the records and M = A^T A ----
    const int nb = (n + 255) / 256, B = (int)rows.block_pq.size();
    const size_t block_words = (size_t)n * lin::kBlock;
    int *d_cview, *d_cpair, *d_view_count, *d_column, *d_view_ptr, *d_block_ptr, *d_view_column;
    int2 *d_view_entry, *d_block_pq, *d_block_entry;
    double *d_cbase, *d_record, *d_rowsum, *d_diag, *d_scal, *d_Q, *d_Y, *d_Z, *d_W, *d_U, *d_mgs[2], *d_gram, *d_res[3],
        *d_position;
    TMI_HIP(s->upload(&d_cview, cview.data(), cview.size()));
    TMI_HIP(s->upload(&d_cpair, cpair.data(), cpair.size()));
    TMI_HIP(s->upload(&d_cbase, cbase.data(), cbase.size()));
    TMI_HIP(s->upload(&d_view_count, rows.view_count.data(), rows.view_count.size()));
    TMI_HIP(s->upload(&d_view_column, rows.view_column.data(), rows.view_column.size()));
    TMI_HIP(s->upload(&d_column, rows.column.data(), rows.column.size()));
    TMI_HIP(s->upload(&d_view_ptr, rows.view_ptr.data(), rows.view_ptr.size()));
    TMI_HIP(s->upload(&d_view_entry, rows.view_entry.data(), rows.view_entry.size()));
    TMI_HIP(s->upload(&d_block_ptr, rows.block_ptr.data(), rows.block_ptr.size()));
    TMI_HIP(s->upload(&d_block_pq, rows.block_pq.data(), rows.block_pq.size()));
    TMI_HIP(s->upload(&d_block_entry, rows.block_entry.data(), rows.block_entry.size()));
    TMI_HIP(s->alloc(&d_record, (size_t)lpos::kRecord * C));
    TMI_HIP(s->alloc(&d_rowsum, (size_t)n));
    TMI_HIP(s->alloc(&d_diag, (size_t)n));
    TMI_HIP(s->alloc(&d_scal, 2));
    TMI_HIP(s->alloc(&d_Q, block_words));
    TMI_HIP(s->alloc(&d_Y, block_words));
    TMI_HIP(s->alloc(&d_Z, block_words));
    TMI_HIP(s->alloc(&d_W, block_words));
    TMI_HIP(s->alloc(&d_U, (size_t)9 * C * lin::kBlock));
    for (double*& p : d_mgs) TMI_HIP(s->alloc(&p, (size_t)nb * lin::kBlock));
    TMI_HIP(s->alloc(&d_gram, (size_t)nb * lin::kGram));
    for (double*& p : d_res) TMI_HIP(s->alloc(&p, (size_t)nb));
    TMI_HIP(s->alloc(&d_position, (size_t)3 * V));
    DenseSpd shifted;  // M + mu I, overwritten by its factor; kBlock right-hand sides
    if ((rc = shifted.alloc(s, n, lin::kBlock, nullptr))) return rc;
    ScalarFetch F;  // the small block: its last three words are the sums of the residuals' parts
    if ((rc = F.alloc(s, shifted.flag, lin::kSmallWords))) return rc;
    for (int q = 0; q < 3; ++q) F.set(q, d_res[q], nb);
    double* d_small = F.d_norms;
    const double* h_small = F.h_norms;
    const dim3 rows_grid(nb);
    ClassSeconds T3(st);
    TMI_HIP(T3.status());
    auto write_times = [&]() {
      T3.write(sum);
      sum->graph_seconds += graph_before;
      sum->kernel_seconds += graph_before + sum->triplet_seconds + sum->baseline_seconds;
    };
    double scal_h[2] = {0.0, 0.0};
    TMI_HIP(T3.begin(T3.kGraph));
    hipLaunchKernelGGL(lpos_record_kernel, grid(C), block, 0, st, C, d_cview, d_cpair, d_cbase, d_view_count, d_orient,
                       d_pos2, d_record);
    TMI_HIP(hipMemsetAsync(shifted.A, 0, (size_t)n * n * sizeof(double), st));
    hipLaunchKernelGGL(lpos_assemble_kernel, grid((long long)9 * B), block, 0, st, B, d_block_ptr, d_block_pq,
                       d_block_entry, d_record, n, shifted.A);
    hipLaunchKernelGGL(lpos_rowsum_kernel, dim3(n), block, 0, st, n, shifted.A, d_rowsum, d_diag);
    hipLaunchKernelGGL(lpos_scalars_kernel, dim3(1), block, 0, st, n, d_rowsum, d_diag, d_scal);
    hipLaunchKernelGGL(lpos_shift_kernel, rows_grid, block, 0, st, n, opt->relative_shift, d_scal, shifted.A);
    TMI_HIP(T3.begin(T3.kFactor));
    shifted.factor(st);
    TMI_HIP(T3.begin(T3.kGraph));
    hipLaunchKernelGGL(lin_start_kernel, dim3(((int)block_words + 255) / 256), block, 0, st, n, (unsigned long long)opt->seed,
                       d_Q);
    TMI_HIP(s->download(scal_h, d_scal, 2));
    if ((rc = F.fetch(s, &T3, 0))) return rc;  // (no sum yet: the pivot flag alone)
    sum->matrix_norm = scal_h[1];
    if (F.flag()) {  // a pivot of M + mu I that is not positive: nothing is written
      write_times();
      return TMI_BA_OK;
    }
    const double threshold = opt->tolerance * scal_h[1];

    // ---- step 6: subspace iteration with Rayleigh-Ritz ----
    int iter = 0, launches = 0;
    bool converged = false;
    while (iter < opt->max_iterations && !converged) {
      ++iter;
      TMI_HIP(T3.begin(T3.kSubstitution));
      TMI_HIP(hipMemcpyAsync(d_W, d_Q, block_words * sizeof(double), hipMemcpyDeviceToDevice, st));
      shifted.substitute<lin::kBlock>(st, d_W, d_Y);
      TMI_HIP(T3.begin(T3.kGraph));
      for (int pass = 0; pass < 2; ++pass)
        for (int j = 0; j <= lin::kBlock; ++j, ++launches)
          hipLaunchKernelGGL(lin_mgs_kernel, rows_grid, block, 0, st, n, j, d_Y, d_mgs[(launches + 1) & 1],
                             d_mgs[launches & 1]);
      hipLaunchKernelGGL(lpos_apply_rows_kernel, grid((long long)C * lin::kBlock), block, 0, st, C, d_column, d_record,
                         d_Y, d_U);
      hipLaunchKernelGGL(lpos_apply_cols_kernel, grid((long long)columns * lin::kBlock), block, 0, st, columns, d_view_ptr,
                         d_view_entry, d_record, d_U, d_Z);
      hipLaunchKernelGGL(lin_gram_kernel, rows_grid, block, 0, st, n, d_Y, d_Z, d_gram);
      hipLaunchKernelGGL(lin_ritz_kernel, dim3(1), dim3(64), 0, st, d_gram, nb, d_small);
      hipLaunchKernelGGL(lin_rotate_kernel, rows_grid, block, 0, st, n, d_small, d_Y, d_Z, d_Q, d_res[0], d_res[1],
                         d_res[2]);
      if ((rc = F.fetch(s, &T3, 3, lin::kSmallResidual, lin::kSmallWords, /*with_flag=*/false))) return rc;
      sum->residual = std::sqrt(h_small[lin::kSmallResidual]);
      converged = sum->residual <= threshold;
    }
    sum->eigenvalue[0] = h_small[lin::kSmallTheta];
    sum->eigenvalue[1] = h_small[lin::kSmallTheta + 1];
    sum->num_iterations = iter;
    sum->converged = converged;

    // ---- step 7: the positions and the sign vote ----
    std::vector<double> position_h((size_t)3 * V);
    TMI_HIP(T3.begin(T3.kGraph));
    hipLaunchKernelGGL(lpos_position_kernel, grid(V), block, 0, st, V, d_view_column, d_Q, d_position);
    hipLaunchKernelGGL(lpos_vote_kernel, grid(E), block, 0, st, E, d_v1, d_v2, d_view_column, d_position, d_orient, d_pos2,
                       d_counters);
    TMI_HIP(T3.end());
    {
      ReadBack rb(st);
      rb.add(position_h.data(), d_position, position_h.size());
      rb.add(counters_h, d_counters, (size_t)lpos::kCounters);
      TMI_HIP(rb.finish());
    }
    T3.collect();
    write_times();
    sum->sign_votes = (int32_t)((long long)counters_h[lpos::kVotesFor] - (long long)counters_h[lpos::kVotesAgainst]);
    sum->flipped = sum->sign_votes < 0;
    sum->usable = 1;
    // the results, only now: a failure above leaves the caller's arrays as they were
    for (int v = 0; v < V; ++v) {
      view_estimated[v] = rows.view_column[v] > -2;
      if (rows.view_column[v] > -2)
        for (int k = 0; k < 3; ++k) {
          const double x = position_h[(size_t)3 * v + k];
          view_position[(size_t)3 * v + k] = sum->flipped ? -x : x;
        }
    }
    if (triplet_capacity >= T) {
      sum->triplets_written = 1;
      if (triplet_view) std::copy(tview_h.begin(), tview_h.end(), triplet_view);
      if (triplet_pair) std::copy(tpair_h.begin(), tpair_h.end(), triplet_pair);
      if (triplet_baseline) std::copy(baseline_h.begin(), baseline_h.end(), triplet_baseline);
      if (triplet_num_common) std::copy(common_h.begin(), common_h.end(), triplet_num_common);
      if (triplet_num_used) std::copy(used_h.begin(), used_h.end(), triplet_num_used);
      if (triplet_component)
        for (int t = 0; t < T; ++t) triplet_component[t] = used_h[t] > 0 ? (int32_t)label_h[t] : -1;
    }
    return TMI_BA_OK;
  });
}

// ---- ExtractMaximallyParallelRigidSubgraph (rigid_subgraph_kernels.h) ------------------------------
void tmi_ba_rigid_subgraph_options_init(tmi_ba_rigid_subgraph_options* o) {
  if (!o) return;
  o->relative_shift = 1e-9;  // DESIGN 8.21 (and 8.17): well above the factorisation's rounding n eps |L| at the order cap
  o->null_tolerance = 1e-9;
  o->max_null_dimension = rsg::kMaxWidth;
  o->max_iterations = 100;
  o->device = -1;
}

int32_t tmi_ba_extract_parallel_rigid_subgraph(const tmi_ba_view_pair_batch* Bh, const uint8_t* view_mask,
                                               const tmi_ba_rigid_subgraph_options* opt, uint8_t* keep,
                                               int32_t* component_size, double* null_space,
                                               tmi_ba_rigid_subgraph_summary* sum) {
  if (!Bh || !opt || !keep || !sum) return bad_argument("rigid subgraph: null batch, options, keep or summary");
  memset(sum, 0, sizeof(*sum));
  sum->fixed_view = -1;
  const double t0 = now_s();
  if (const char* why = check_view_pair_batch(Bh, true, Bh->pair_position2)) return bad_argument(why);
  if (!(opt->relative_shift >= 0.0) || !std::isfinite(opt->relative_shift))
    return bad_argument("rigid subgraph: relative_shift is negative or not finite");
  if (!(opt->null_tolerance > 0.0) || !std::isfinite(opt->null_tolerance))
    return bad_argument("rigid subgraph: null_tolerance is not positive and finite");
  if (opt->max_null_dimension < 1 || opt->max_null_dimension > rsg::kMaxWidth)
    return bad_argument("rigid subgraph: max_null_dimension is not in [1, 128]");
  if (opt->max_iterations <= 0) return bad_argument("rigid subgraph: max_iterations is not positive");
  const int V = Bh->num_views;
  // the views of the problem: those with an edge between two views of the mask, in ascending index
  const ViewSubset P = build_view_subset(V, Bh->num_pairs, Bh->pair_view1, Bh->pair_view2, view_mask);
  const int Vp = (int)P.view_of.size(), E = (int)P.edge_of.size();
  if ((int64_t)3 * Vp > rotation_order_cap()) {
    g_last_error = "rigid subgraph: 3 (views with an edge) exceeds the dense solver's cap (see the header)";
    return TMI_BA_ERR_UNSUPPORTED;
  }
  const int n = 3 * Vp;  // (<= the cap)
  std::vector<double> orient_h((size_t)3 * Vp), pos_h((size_t)3 * E);
  for (int p = 0; p < Vp; ++p)
    std::copy(Bh->view_rotation + (size_t)3 * P.view_of[p], Bh->view_rotation + (size_t)3 * P.view_of[p] + 3,
              orient_h.begin() + (size_t)3 * p);
  for (int e = 0; e < E; ++e)
    std::copy(Bh->pair_position2 + (size_t)3 * P.edge_of[e], Bh->pair_position2 + (size_t)3 * P.edge_of[e] + 3,
              pos_h.begin() + (size_t)3 * e);
  const EdgeRows rows = build_edge_rows(Vp, E, P.v1.data(), P.v2.data(), Vp);
  std::vector<uint8_t> keep_h;
  std::vector<int> size_h;
  std::vector<double> null_h;
  const int rc = one_shot_batch(opt->device, "rigid subgraph: no such device", E, t0, &sum->seconds, [&](OneShot* s) -> int {
    int rc;
    hipStream_t st = s->stream;
    const int nb = (n + 255) / 256;
    const int W = rsg::kMaxWidth;
    double *d_orient, *d_pos, *d_S, *d_D, *d_Q, *d_Y, *d_Z, *d_W, *d_mgs[2], *d_gram, *d_res, *d_small;
    TMI_HIP(s->upload(&d_orient, orient_h.data(), orient_h.size()));
    TMI_HIP(s->upload(&d_pos, pos_h.data(), pos_h.size()));
    TMI_HIP(s->alloc(&d_S, (size_t)6 * E));
    PoseGraphDevice graph;  // no view is held
    if ((rc = graph.upload(s, Vp, Vp, rows, E, P.v1.data(), P.v2.data(), d_S))) return rc;
    const PoseGraph& G = graph.G;
    TMI_HIP(s->alloc(&d_D, (size_t)6 * Vp));
    for (double** p : {&d_Q, &d_Y, &d_Z, &d_W}) TMI_HIP(s->alloc(p, (size_t)n * W));
    for (double*& p : d_mgs) TMI_HIP(s->alloc(&p, (size_t)nb * W));
    TMI_HIP(s->alloc(&d_gram, (size_t)nb * W * W));
    TMI_HIP(s->alloc(&d_res, (size_t)nb * W));
    TMI_HIP(s->alloc(&d_small, (size_t)2 * W * W + 2 * W + 2));  // (the last words: the largest diagonal entry)
    double* d_scale = d_small + (size_t)2 * W * W + 2 * W;
    DenseSpd shifted;  // L + mu I, overwritten by its factor; kChunk right-hand sides at a time
    if ((rc = shifted.alloc(s, n, rsg::kChunk, nullptr))) return rc;
    Pinned<double> pinned;
    TMI_HIP(pinned.alloc((size_t)2 * W + 2));
    double* h_small = pinned.get();
    int* h_flag = reinterpret_cast<int*>(h_small + 2 * W + 1);
    static bool attr_set = false;
    if (!attr_set) {
      TMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&rsg_ritz_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)rsg::ritz_lds_bytes(W)));
      attr_set = true;
    }
    const dim3 block(256), rows_grid(nb);
    sum->num_views = Vp;
    sum->num_pairs = E;
    sum->order = n;
    ClassSeconds T(st);
    TMI_HIP(T.status());

    // ---- the matrix and its factor ----
    TMI_HIP(T.begin(T.kGraph));
    hipLaunchKernelGGL(rsg_edge_kernel, dim3((E + 255) / 256), block, 0, st, E, d_orient, G.pair_view1, d_pos, d_S);
    hipLaunchKernelGGL(rsg_diag_kernel, dim3((6 * Vp + 255) / 256), block, 0, st, G, d_D);
    hipLaunchKernelGGL(rsg_scale_kernel, dim3(1), block, 0, st, Vp, d_D, d_scale);
    hipLaunchKernelGGL(rsg_assemble_kernel, dim3(Vp), block, 0, st, G, n, d_D, d_scale, opt->relative_shift, shifted.A);
    TMI_HIP(T.begin(T.kFactor));
    shifted.factor(st);
    TMI_HIP(T.end());
    {
      ReadBack rb(st);
      rb.add(h_small, d_scale, 1);
      rb.add(h_flag, shifted.flag, 1);
      TMI_HIP(rb.finish());
    }
    T.collect();
    const double scale = h_small[0];
    sum->largest_diagonal = scale;
    if (*h_flag || !(scale > 0.0)) {  // a pivot of L + mu I that is not positive, or no direction at all
      T.write(sum);
      s->error = "rigid subgraph: L + mu I could not be factored (every position_2 zero, or relative_shift too small)";
      return TMI_BA_ERR_LINEAR_SOLVER;
    }
    const double null_threshold = opt->null_tolerance * scale;
    const double stop_tolerance = 1e-3 * null_threshold;
    sum->stop_tolerance = stop_tolerance;

    // ---- the null space: block inverse iteration with Rayleigh-Ritz, the block doubled while all of it is null ----
    int m = rsg::kStartWidth, k = -1, iter = 0;
    for (;;) {
      const int me = std::min(m, n);  // the columns from me on are zero and stay zero: the block cannot outgrow R^n
      const size_t block_words = (size_t)n * m;
      const int chunks = m / rsg::kChunk;
      TMI_HIP(hipMemsetAsync(d_Q, 0, block_words * sizeof(double), st));
      hipLaunchKernelGGL(rsg_start_kernel, dim3((n * me + 255) / 256), block, 0, st, n, me, d_Q);
      int previous = -1, stable = 0, launches = 0;
      bool all_null = false;
      k = -1;
      while (k < 0 && !all_null) {
        if (iter >= opt->max_iterations) {
          sum->block_width = m;
          sum->iterations = iter;
          T.write(sum);
          s->error = "rigid subgraph: the null space did not settle within max_iterations";
          return TMI_BA_ERR_NOT_CONVERGED;
        }
        ++iter;
        TMI_HIP(T.begin(T.kSubstitution));
        TMI_HIP(hipMemcpyAsync(d_W, d_Q, block_words * sizeof(double), hipMemcpyDeviceToDevice, st));
        for (int c = 0; c < chunks; ++c)
          shifted.substitute<rsg::kChunk>(st, d_W + (size_t)c * n * rsg::kChunk, d_Y + (size_t)c * n * rsg::kChunk);
        TMI_HIP(T.begin(T.kGraph));
        for (int pass = 0; pass < 2; ++pass)
          for (int j = 0; j <= m; ++j, ++launches)
            hipLaunchKernelGGL(rsg_mgs_kernel, rows_grid, block, 0, st, n, m, j, d_Y, d_mgs[(launches + 1) & 1],
                               d_mgs[launches & 1]);
        hipLaunchKernelGGL(rsg_apply_kernel, dim3((Vp * m + 255) / 256), block, 0, st, G, m, d_Y, d_Z);
        hipLaunchKernelGGL(rsg_gram_kernel, dim3(nb, m), dim3(128), 0, st, n, m, d_Y, d_Z, d_gram);
        hipLaunchKernelGGL(rsg_ritz_kernel, dim3(1), block, rsg::ritz_lds_bytes(m), st, d_gram, nb, m, me, d_small);
        hipLaunchKernelGGL(rsg_rotate_kernel, dim3(nb, chunks), block, 0, st, n, m, d_small, d_Y, d_Z, d_Q, d_res);
        hipLaunchKernelGGL(rsg_residual_kernel, dim3(1), dim3(128), 0, st, d_res, nb, m, d_small);
        TMI_HIP(T.end());
        {
          ReadBack rb(st);  // theta [m], residual^2 [m]
          rb.add(h_small, d_small + (size_t)2 * m * m, (size_t)2 * m);
          TMI_HIP(rb.finish());
        }
        T.collect();
        int count = 0;
        while (count < me && h_small[count] <= null_threshold) ++count;
        double worst = 0.0;
        for (int j = 0; j < count; ++j) worst = std::max(worst, std::sqrt(h_small[m + j]));
        if (count == me && me < n) {
          all_null = true;
        } else {
          stable = (count == previous && worst <= stop_tolerance) ? stable + 1 : (worst <= stop_tolerance ? 1 : 0);
          previous = count;
          if (stable >= 2) {
            k = count;
            sum->max_residual = worst;
            sum->largest_null_value = count > 0 ? h_small[count - 1] : 0.0;
            sum->smallest_other_value = count < me ? h_small[count] : 0.0;
          }
        }
      }
      sum->block_width = m;
      sum->iterations = iter;
      if (k >= 0) break;
      if (m >= opt->max_null_dimension || 2 * m > rsg::kMaxWidth) {
        k = rsg::kMaxWidth + 1;  // at least m dimensions, and no wider block is allowed
        break;
      }
      m *= 2;
    }
    if (k > opt->max_null_dimension) {
      T.write(sum);
      s->error = "rigid subgraph: the null space has more dimensions than max_null_dimension";
      return TMI_BA_ERR_NULL_SPACE_TOO_LARGE;
    }
    sum->null_dimension = k;

    // ---- the search ----
    double *d_N, *d_Mt, *d_norms;
    unsigned char* d_flag;
    int *d_size, *d_pick;
    const int kk = std::max(k, 1);  // (k = 0: no null direction, every row of M is zero and every view a zero view)
    const size_t per_fixed = (size_t)3 * kk * Vp;
    const int batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)Vp, ((size_t)256 << 20) / (per_fixed * sizeof(double))));
    TMI_HIP(s->alloc_filled(&d_N, (size_t)n * kk, 0));
    TMI_HIP(s->alloc(&d_Mt, per_fixed * batch));
    TMI_HIP(s->alloc(&d_norms, (size_t)3 * Vp * batch));
    TMI_HIP(s->alloc(&d_flag, (size_t)Vp * Vp));
    TMI_HIP(s->alloc(&d_size, (size_t)Vp));
    TMI_HIP(s->alloc(&d_pick, 2));
    StreamTimer search(st);
    TMI_HIP(search.status);
    TMI_HIP(search.mark());
    if (k > 0) hipLaunchKernelGGL(rsg_null_kernel, dim3((n * k + 255) / 256), block, 0, st, n, k, d_Q, d_N);
    for (int f0 = 0; f0 < Vp; f0 += batch) {
      const int F = std::min(batch, Vp - f0);
      const long long threads = (long long)F * 3 * Vp;
      hipLaunchKernelGGL(rsg_rows_kernel, dim3((unsigned)((threads + 255) / 256)), block, 0, st, Vp, kk, f0, F, d_N, d_Mt,
                         d_norms);
      hipLaunchKernelGGL(rsg_component_kernel, dim3((Vp + 255) / 256, F), block, rsg::component_lds_bytes(kk), st, Vp, kk,
                         f0, d_Mt, d_norms, d_flag);
    }
    hipLaunchKernelGGL(rsg_count_kernel, dim3(Vp), block, 0, st, Vp, d_flag, d_size);
    hipLaunchKernelGGL(rsg_pick_kernel, dim3(1), block, 0, st, Vp, d_size, d_pick);
    TMI_HIP(search.mark());
    int pick_h[2] = {0, 0};
    size_h.resize((size_t)Vp);
    if (null_space) null_h.resize((size_t)n * k);
    {
      ReadBack rb(st);
      rb.add(pick_h, d_pick, 2);
      rb.add(size_h.data(), d_size, size_h.size());
      rb.add(null_h.data(), d_N, null_h.size());
      TMI_HIP(rb.finish());
    }
    keep_h.resize((size_t)Vp);
    {
      ReadBack rb(st);  // the flags of the picked view
      rb.add(keep_h.data(), (const uint8_t*)d_flag + (size_t)pick_h[0] * Vp, keep_h.size());
      TMI_HIP(rb.finish());
    }
    T.write(sum);
    sum->search_seconds = search.seconds();
    sum->kernel_seconds += sum->search_seconds;
    sum->fixed_view = P.view_of[pick_h[0]];
    sum->num_kept = pick_h[1];
    return TMI_BA_OK;
  });
  if (rc != TMI_BA_OK) return rc;
  // the results, only now: a failure above leaves the caller's arrays as they were
  std::fill(keep, keep + V, (uint8_t)0);
  if (component_size) std::fill(component_size, component_size + V, 0);
  for (size_t p = 0; p < keep_h.size(); ++p) {
    keep[P.view_of[p]] = keep_h[p];
    if (component_size) component_size[P.view_of[p]] = size_h[p];
  }
  if (null_space) {
    // the sign rule: the entry of largest magnitude of each column, the first of equals, is positive
    const int k = sum->null_dimension;
    for (int c = 0; c < k; ++c) {
      double big = 0.0;
      bool negative = false;
      for (int i = 0; i < n; ++i)
        if (std::fabs(null_h[(size_t)i * k + c]) > big) {
          big = std::fabs(null_h[(size_t)i * k + c]);
          negative = null_h[(size_t)i * k + c] < 0.0;
        }
      for (int i = 0; i < n; ++i) null_space[(size_t)i * k + c] = negative ? -null_h[(size_t)i * k + c] : null_h[(size_t)i * k + c];
    }
  }
  return TMI_BA_OK;
}

}  // extern "C"
