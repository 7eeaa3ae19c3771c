// The host pieces of the global pose estimators (theiasfm_amd/csrc/pose_graph_host.h) on their own, so that
// tests/test_pose_graph_host_cpu.py can compare them with a few lines of numpy and run them under the host's
// sanitizers.  Compiled as HIP for the host only; no device is touched.
//
// stdin: one command per graph,
//   "graph V E fixed  a_0 b_0 ... a_{E-1} b_{E-1}  m_0 .. m_{V-1}"   (fixed = V: no view is held; m: the view mask)
// or "options": the option check on both options structs, each field in turn at -1 and at NaN.
// stdout, per graph, one line each:
//   row_ptr, row (x y pairs), lap_ptr, lap_row (x y pairs)                      build_edge_rows(V, E, a, b, fixed)
//   components: count, root[V], all_reach(v) for every v                        view_components
//   subset with the mask: view_index[V] | view_of | edge_of | v1 | v2            build_view_subset
//   subset without one: the same
//   round trip: gather_free of the table 100 v + k, then scatter_free of it into a table of -1; then the same through
//   the masked subset's view_of with its first view held
// per "options": "<struct> <field> <value>: <text>" lines.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/theia_mi355_ba.h"
#include "pose_graph_host.h"

template <class T>
static void print(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (const T& x : v) std::printf(" %d", (int)x);
  std::printf("\n");
}

static void print(const char* name, const std::vector<int2>& v) {
  std::printf("%s", name);
  for (const int2& x : v) std::printf(" %d %d", x.x, x.y);
  std::printf("\n");
}

static void print_subset(const char* name, const tmi::ViewSubset& S) {
  std::printf("%s", name);
  for (int x : S.view_index) std::printf(" %d", x);
  std::printf(" |");
  for (int x : S.view_of) std::printf(" %d", x);
  std::printf(" |");
  for (int x : S.edge_of) std::printf(" %d", x);
  std::printf(" |");
  for (int x : S.v1) std::printf(" %d", x);
  std::printf(" |");
  for (int x : S.v2) std::printf(" %d", x);
  std::printf("\n");
}

// the trust-region fields by name; the same list for both structs
#define TR_FIELDS(X)                                                                                                  \
  X(robust_loss_width) X(max_num_iterations) X(function_tolerance) X(gradient_tolerance) X(parameter_tolerance)       \
  X(initial_trust_region_radius) X(max_trust_region_radius) X(min_trust_region_radius) X(min_relative_decrease)       \
  X(min_lm_diagonal) X(max_lm_diagonal)

template <class Options>
static Options good_options() {
  Options o{};
  o.max_num_iterations = 10;
  o.robust_loss_width = 0.1;
  o.function_tolerance = 1e-6;
  o.gradient_tolerance = 1e-10;
  o.parameter_tolerance = 1e-8;
  o.initial_trust_region_radius = 1e4;
  o.max_trust_region_radius = 1e16;
  o.min_trust_region_radius = 1e-32;
  o.min_relative_decrease = 1e-3;
  o.min_lm_diagonal = 1e-6;
  o.max_lm_diagonal = 1e32;
  return o;
}

template <class Options>
static void check_options(const char* name, const char* call, const char* width_note) {
  const Options good = good_options<Options>();
  std::printf("%s none 0: %s\n", name, tmi::trust_region_options_error(&good, call, width_note).c_str());
  Options zero = good;
  zero.initial_trust_region_radius = 0.0;
  std::printf("%s initial_trust_region_radius 0: %s\n", name, tmi::trust_region_options_error(&zero, call, width_note).c_str());
  for (const double value : {-1.0, (double)NAN}) {
#define X(field)                                                                                                      \
  {                                                                                                                   \
    Options o = good;                                                                                                 \
    if (std::isnan(value) && sizeof(o.field) == sizeof(int32_t)) {                                                    \
    } else {                                                                                                          \
      o.field = (decltype(o.field))value;                                                                             \
      std::printf("%s " #field " %s: %s\n", name, std::isnan(value) ? "nan" : "-1",                                   \
                  tmi::trust_region_options_error(&o, call, width_note).c_str());                                     \
    }                                                                                                                 \
  }
    TR_FIELDS(X)
#undef X
  }
}

int main() {
  char word[16];
  int graphs = 0;
  while (std::scanf("%15s", word) == 1) {
    if (word[0] == 'o') {
      check_options<tmi_ba_nonlinear_position_options>("position", "nonlinear positions", " (the reference CHECK_GTs it)");
      check_options<tmi_ba_nonlinear_rotation_options>("rotation", "nonlinear rotations", "");
      continue;
    }
    int V, E, fixed;
    if (std::scanf("%d %d %d", &V, &E, &fixed) != 3) return 2;
    std::vector<int32_t> a((size_t)E), b((size_t)E);
    std::vector<uint8_t> mask((size_t)V);
    for (int e = 0; e < E; ++e)
      if (std::scanf("%d %d", &a[e], &b[e]) != 2) return 2;
    for (int v = 0; v < V; ++v) {
      int m;
      if (std::scanf("%d", &m) != 1) return 2;
      mask[v] = (uint8_t)m;
    }
    const tmi::EdgeRows rows = tmi::build_edge_rows(V, E, a.data(), b.data(), fixed);
    print("row_ptr", rows.row_ptr);
    print("row", rows.row);
    print("lap_ptr", rows.lap_ptr);
    print("lap_row", rows.lap_row);
    const tmi::ViewComponents comp = tmi::view_components(V, E, a.data(), b.data());
    std::printf("components %d", comp.count);
    for (int r : comp.root) std::printf(" %d", r);
    for (int v = 0; v < V; ++v) std::printf(" %d", (int)comp.all_reach(v));
    std::printf("\n");
    print_subset("masked", tmi::build_view_subset(V, E, a.data(), b.data(), mask.data()));
    print_subset("unmasked", tmi::build_view_subset(V, E, a.data(), b.data(), nullptr));
    const int n = fixed < V ? V - 1 : V;
    std::vector<double> table((size_t)3 * V), x((size_t)3 * n), back((size_t)3 * V, -1.0);
    for (int i = 0; i < 3 * V; ++i) table[i] = 100.0 * (i / 3) + i % 3;
    tmi::gather_free(V, fixed, nullptr, table.data(), x.data());
    tmi::scatter_free(V, fixed, nullptr, x.data(), back.data());
    print("gathered", x);
    print("scattered", back);
    // through the masked subset's view_of, its first view held
    const tmi::ViewSubset S = tmi::build_view_subset(V, E, a.data(), b.data(), mask.data());
    const int Vp = (int)S.view_of.size();
    std::vector<double> xs((size_t)3 * (Vp > 0 ? Vp - 1 : 0)), back_s((size_t)3 * V, -1.0);
    tmi::gather_free(Vp, 0, S.view_of.data(), table.data(), xs.data());
    tmi::scatter_free(Vp, 0, S.view_of.data(), xs.data(), back_s.data());
    print("gathered_subset", xs);
    print("scattered_subset", back_s);
    ++graphs;
  }
  std::fprintf(stderr, "pose graph host check: %d graphs\n", graphs);
  return 0;
}
