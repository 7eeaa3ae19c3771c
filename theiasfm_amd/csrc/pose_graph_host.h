// The host side of what the global pose estimators share (pose_graph_calls.h): the rows of PoseGraph (pose_graph.h)
// from a view table and an edge list, the graph's components, the views of a problem, the [n][3] vector of the free
// views, the ADMM stopping test and the trust-region options.  Host only: no HIP runtime call, int2 the only HIP type,
// so that tests/cpp/pose_graph_host_check.cc runs it under the host's sanitizers.
#pragma once
#include <hip/hip_vector_types.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace tmi {

// The CSR of the undirected graph in ascending edge index -- row: (neighbour, edge << 1 | (this view is the edge's
// view2)) -- and per free view (column c = v - (v > fixed_view)) the entries with a free neighbour sorted by
// (neighbour's column, edge), for the matrix assembly of the rotation and the position estimators.
struct EdgeRows {
  std::vector<int> row_ptr;   // [V + 1]
  std::vector<int2> row;      // [2 E]
  std::vector<int> lap_ptr;   // [n + 1]
  std::vector<int2> lap_row;  // [<= 2 E]
};

// fixed_view = V: no view is fixed and every view has a column (the nonlinear rotation estimator's gauge-free problem).
inline EdgeRows build_edge_rows(int V, int E, const int32_t* view1, const int32_t* view2, int fixed_view) {
  const int n = fixed_view < V ? V - 1 : V;
  EdgeRows rows;
  std::vector<int>& row_ptr = rows.row_ptr;
  std::vector<int>& lap_ptr = rows.lap_ptr;
  std::vector<int2>& row = rows.row;
  std::vector<int2>& lap_row = rows.lap_row;
  auto column_of = [&](int v) { return v == fixed_view ? -1 : v - (v > fixed_view); };
  row_ptr.assign((size_t)V + 1, 0);
  lap_ptr.assign((size_t)n + 1, 0);
  row.resize((size_t)2 * E);
  for (int e = 0; e < E; ++e) {
    row_ptr[(size_t)view1[e] + 1]++;
    row_ptr[(size_t)view2[e] + 1]++;
  }
  for (int v = 0; v < V; ++v) row_ptr[(size_t)v + 1] += row_ptr[v];
  std::vector<int> fill(row_ptr.begin(), row_ptr.end() - 1);
  for (int e = 0; e < E; ++e) {
    const int a = view1[e], b = view2[e];
    row[(size_t)fill[a]++] = make_int2(b, e << 1);
    row[(size_t)fill[b]++] = make_int2(a, (e << 1) | 1);
  }
  lap_row.reserve((size_t)2 * E);
  for (int c = 0; c < n; ++c) {
    const int v = c + (c >= fixed_view);
    const size_t first = lap_row.size();
    for (int r = row_ptr[v]; r < row_ptr[(size_t)v + 1]; ++r) {
      const int nc = column_of(row[r].x);
      if (nc >= 0) lap_row.push_back(make_int2(nc, row[r].y >> 1));
    }
    std::sort(lap_row.begin() + first, lap_row.end(),
              [](const int2& p, const int2& q) { return p.x != q.x ? p.x < q.x : p.y < q.y; });
    lap_ptr[(size_t)c + 1] = (int)lap_row.size();
  }
  return rows;
}

// The connected components of the (checked) edges by union-find, the smaller root kept: root[v] is the smallest view of
// v's component.
struct ViewComponents {
  int count = 0;
  std::vector<int> root;  // [V]
  bool all_reach(int v) const {  // does every view reach v?
    for (const int r : root)
      if (r != root[v]) return false;
    return true;
  }
};

inline ViewComponents view_components(int V, int E, const int32_t* view1, const int32_t* view2) {
  ViewComponents c;
  std::vector<int>& parent = c.root;
  parent.resize((size_t)V);
  for (int v = 0; v < V; ++v) parent[v] = v;
  auto find = [&](int v) {
    while (parent[v] != v) v = parent[v] = parent[parent[v]];
    return v;
  };
  c.count = V;
  for (int e = 0; e < E; ++e) {
    const int ra = find(view1[e]), rb = find(view2[e]);
    if (ra != rb) {
      parent[std::max(ra, rb)] = std::min(ra, rb);
      --c.count;
    }
  }
  for (int v = 0; v < V; ++v) parent[v] = find(v);
  return c;
}

// The problem of an estimator that leaves views out: the edges whose two views are marked (mask null: every edge) in
// the caller's order, and the views with such an edge in ascending index.
struct ViewSubset {
  std::vector<int> view_index;  // [V] the view's index in the problem, -1: not part of it
  std::vector<int> view_of;     // [Vp] the caller's index of view p of the problem
  std::vector<int> edge_of;     // [Ep] the caller's index of edge e of the problem
  std::vector<int32_t> v1, v2;  // [Ep] the edges on the problem's views
};

inline ViewSubset build_view_subset(int V, int E, const int32_t* view1, const int32_t* view2, const uint8_t* mask) {
  ViewSubset S;
  S.view_index.assign((size_t)V, -1);
  for (int e = 0; e < E; ++e) {
    const int a = view1[e], b = view2[e];
    if (mask && (!mask[a] || !mask[b])) continue;
    S.edge_of.push_back(e);
    S.view_index[a] = S.view_index[b] = 0;
  }
  for (int v = 0; v < V; ++v)
    if (S.view_index[v] == 0) {
      S.view_index[v] = (int)S.view_of.size();
      S.view_of.push_back(v);
    }
  S.v1.resize(S.edge_of.size());
  S.v2.resize(S.edge_of.size());
  for (size_t e = 0; e < S.edge_of.size(); ++e) {
    S.v1[e] = S.view_index[view1[S.edge_of[e]]];
    S.v2[e] = S.view_index[view2[S.edge_of[e]]];
  }
  return S;
}

// x [n][3], the free views' columns (view p has column p - (p > held); held = V: every view has one), from and to the
// rows view_of[p] (null: p) of full.  scatter_free leaves the held view's row to the caller.
inline void gather_free(int V, int held, const int* view_of, const double* full, double* x) {
  for (int p = 0; p < V; ++p)
    if (p != held) std::copy(full + (size_t)3 * (view_of ? view_of[p] : p), full + (size_t)3 * (view_of ? view_of[p] : p) + 3,
                             x + (size_t)3 * (p - (p > held)));
}

inline void scatter_free(int V, int held, const int* view_of, const double* x, double* full) {
  for (int p = 0; p < V; ++p)
    if (p != held) std::copy(x + (size_t)3 * (p - (p > held)), x + (size_t)3 * (p - (p > held)) + 3,
                             full + (size_t)3 * (view_of ? view_of[p] : p));
}

// ---- the linear position estimator's rows (position_linear_kernels.h) ---------------------------------------------
// The adjacency rows of the (checked: no pair twice) edges with every row in ascending neighbour: adj (neighbour, edge),
// owner the row's view per slot.  The triangle finder intersects two such rows.
struct SortedAdjacency {
  std::vector<int> ptr;    // [V + 1]
  std::vector<int2> adj;   // [2 E]
  std::vector<int> owner;  // [2 E]
};

inline SortedAdjacency build_sorted_adjacency(int V, int E, const int32_t* view1, const int32_t* view2) {
  SortedAdjacency S;
  S.ptr.assign((size_t)V + 1, 0);
  S.adj.resize((size_t)2 * E);
  S.owner.resize((size_t)2 * E);
  for (int e = 0; e < E; ++e) {
    S.ptr[(size_t)view1[e] + 1]++;
    S.ptr[(size_t)view2[e] + 1]++;
  }
  for (int v = 0; v < V; ++v) S.ptr[(size_t)v + 1] += S.ptr[v];
  std::vector<int> fill(S.ptr.begin(), S.ptr.end() - 1);
  for (int e = 0; e < E; ++e) {
    S.adj[(size_t)fill[view1[e]]++] = make_int2(view2[e], e);
    S.adj[(size_t)fill[view2[e]]++] = make_int2(view1[e], e);
  }
  for (int v = 0; v < V; ++v) {
    std::sort(S.adj.begin() + S.ptr[v], S.adj.begin() + S.ptr[(size_t)v + 1],
              [](const int2& p, const int2& q) { return p.x < q.x; });
    std::fill(S.owner.begin() + S.ptr[v], S.owner.begin() + S.ptr[(size_t)v + 1], v);
  }
  return S;
}

// The (checked: indices in range) observations in view-major order, a view's in ascending track: track and obs (the
// caller's observation) per slot.  repeated: some view observes a track twice.
struct ViewTracks {
  std::vector<int> ptr;      // [V + 1]
  std::vector<int> track;    // [No]
  std::vector<int64_t> obs;  // [No]
  bool repeated = false;
};

inline ViewTracks build_view_tracks(int V, int64_t num_obs, const int32_t* obs_view, const int32_t* obs_track) {
  ViewTracks T;
  T.ptr.assign((size_t)V + 1, 0);
  for (int64_t i = 0; i < num_obs; ++i) T.ptr[(size_t)obs_view[i] + 1]++;
  for (int v = 0; v < V; ++v) T.ptr[(size_t)v + 1] += T.ptr[v];
  std::vector<std::pair<int, int64_t>> slot((size_t)num_obs);
  std::vector<int> fill(T.ptr.begin(), T.ptr.end() - 1);
  for (int64_t i = 0; i < num_obs; ++i) slot[(size_t)fill[obs_view[i]]++] = {obs_track[i], i};
  T.track.resize((size_t)num_obs);
  T.obs.resize((size_t)num_obs);
  for (int v = 0; v < V; ++v) {
    std::sort(slot.begin() + T.ptr[v], slot.begin() + T.ptr[(size_t)v + 1]);
    for (int r = T.ptr[v]; r < T.ptr[(size_t)v + 1]; ++r) {
      T.track[r] = slot[r].first;
      T.obs[r] = slot[r].second;
      if (r > T.ptr[v] && slot[r].first == slot[(size_t)r - 1].first) T.repeated = true;
    }
  }
  return T;
}

// The unknowns and the rows of A^T A over C chosen triplets (view [3 C], ascending triplet number): the views of the
// triplets in ascending index, the first of them held (column -1), every other with a column; per free column its
// triplets (view_entry: triplet, slot) and per 3 x 3 block (row column, column column) of the matrix the triplets that
// hold both views (block_entry: triplet, 3 x the row's slot + the column's), all in ascending triplet.
struct TripletRows {
  std::vector<int> views;         // [V'] the estimated views, ascending; views[0] is held
  std::vector<int> view_column;   // [V] >= 0: the column, -1: the held view, -2: not estimated
  std::vector<int> view_count;    // [V] chosen triplets of the view
  std::vector<int> column;        // [3 C] the slots' columns
  std::vector<int> view_ptr;      // [V']  (V' - 1 columns)
  std::vector<int2> view_entry;
  std::vector<int> block_ptr;     // [B + 1]
  std::vector<int2> block_pq;     // [B]
  std::vector<int2> block_entry;
};

inline TripletRows build_triplet_rows(int V, int C, const int* view) {
  TripletRows R;
  R.view_column.assign((size_t)V, -2);
  R.view_count.assign((size_t)V, 0);
  for (size_t i = 0; i < (size_t)3 * C; ++i) R.view_count[view[i]]++;
  for (int v = 0; v < V; ++v)
    if (R.view_count[v] > 0) {
      R.view_column[v] = (int)R.views.size() - 1;
      R.views.push_back(v);
    }
  const int columns = std::max(0, (int)R.views.size() - 1);
  R.column.resize((size_t)3 * C);
  R.view_ptr.assign((size_t)columns + 1, 0);
  for (size_t i = 0; i < (size_t)3 * C; ++i) {
    R.column[i] = R.view_column[view[i]];
    if (R.column[i] >= 0) R.view_ptr[(size_t)R.column[i] + 1]++;
  }
  for (int p = 0; p < columns; ++p) R.view_ptr[(size_t)p + 1] += R.view_ptr[p];
  R.view_entry.resize((size_t)R.view_ptr[columns]);
  std::vector<int> fill(R.view_ptr.begin(), R.view_ptr.end() - 1);
  for (int c = 0; c < C; ++c)
    for (int s = 0; s < 3; ++s) {
      const int p = R.column[(size_t)3 * c + s];
      if (p >= 0) R.view_entry[(size_t)fill[p]++] = make_int2(c, s);
    }
  R.block_ptr.push_back(0);
  std::vector<std::pair<int, int2>> row;  // (column column, entry) of one row column
  for (int p = 0; p < columns; ++p) {
    row.clear();
    for (int r = R.view_ptr[p]; r < R.view_ptr[(size_t)p + 1]; ++r) {
      const int2 ent = R.view_entry[r];
      for (int s = 0; s < 3; ++s) {
        const int q = R.column[(size_t)3 * ent.x + s];
        if (q >= 0) row.push_back({q, make_int2(ent.x, 3 * ent.y + s)});
      }
    }
    std::stable_sort(row.begin(), row.end(),
                     [](const std::pair<int, int2>& a, const std::pair<int, int2>& b) { return a.first < b.first; });
    for (size_t i = 0; i < row.size(); ++i) {
      if (i == 0 || row[i].first != row[i - 1].first) {
        if (i > 0) R.block_ptr.push_back((int)R.block_entry.size());
        R.block_pq.push_back(make_int2(p, row[i].first));
      }
      R.block_entry.push_back(row[i].second);
    }
    if (!row.empty()) R.block_ptr.push_back((int)R.block_entry.size());
  }
  return R;
}

// The stopping test of the two ADMM loops (l1_solver.h:157-170, constrained_l1_solver.cc:152-164) on the five squared
// norms of an iteration: |A x - z - b|^2, |A x|^2, |z|^2, |rho A^T dz|^2, |rho A^T u|^2.
struct AdmmNorms {
  double r_norm, s_norm;
  bool converged;
};

inline AdmmNorms admm_converged(const double* h_norms, double rhs_norm, double primal_abs, double dual_abs, double rel_tol) {
  const double r_norm = std::sqrt(h_norms[0]), s_norm = std::sqrt(h_norms[3]);
  const double max_norm = std::max({std::sqrt(h_norms[1]), std::sqrt(h_norms[2]), rhs_norm});
  const double primal_eps = primal_abs + rel_tol * max_norm;
  const double dual_eps = dual_abs + rel_tol * std::sqrt(h_norms[4]);
  return {r_norm, s_norm, r_norm < primal_eps && s_norm < dual_eps};
}

// What the two nonlinear estimators ask of the loss width and the trust-region fields of their options, as
// "<call>: <what>" (empty: fine).  width_note: what the call adds to the loss width's message.
template <class Options>
std::string trust_region_options_error(const Options* o, const char* call, const char* width_note) {
  const std::string prefix = std::string(call) + ": ";
  if (!(o->robust_loss_width > 0.0) || !std::isfinite(o->robust_loss_width))
    return prefix + "robust_loss_width is not positive and finite" + width_note;
  if (o->max_num_iterations < 0) return prefix + "max_num_iterations < 0";
  for (const double x : {o->function_tolerance, o->gradient_tolerance, o->parameter_tolerance,
                         o->initial_trust_region_radius, o->max_trust_region_radius, o->min_trust_region_radius,
                         o->min_relative_decrease, o->min_lm_diagonal, o->max_lm_diagonal})
    if (!(x >= 0.0)) return prefix + "a radius, tolerance or LM diagonal bound that is negative or NaN";
  if (!(o->initial_trust_region_radius > 0.0)) return prefix + "initial_trust_region_radius is 0";
  return std::string();
}

// The loss width and the trust-region fields of either options struct from the solver's defaults (Args: SmallLmArgs).
template <class Options, class Args>
void set_trust_region_options(Options* o, const Args& A) {
  o->max_num_iterations = A.max_num_iterations;
  o->robust_loss_width = A.loss_width;
  o->jacobi_scaling = A.jacobi_scaling;
  o->max_num_consecutive_invalid_steps = A.max_num_consecutive_invalid_steps;
  o->function_tolerance = A.function_tolerance;
  o->gradient_tolerance = A.gradient_tolerance;
  o->parameter_tolerance = A.parameter_tolerance;
  o->initial_trust_region_radius = A.initial_radius;
  o->max_trust_region_radius = A.max_radius;
  o->min_trust_region_radius = A.min_radius;
  o->min_relative_decrease = A.min_relative_decrease;
  o->min_lm_diagonal = A.lm_lo;
  o->max_lm_diagonal = A.lm_hi;
}

}  // namespace tmi
