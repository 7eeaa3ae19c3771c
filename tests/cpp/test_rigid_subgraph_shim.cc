// tests/test_rigid_subgraph_cpu.py and tests/test_gpu_rigid_subgraph.py: the shim of
// theia::ExtractMaximallyParallelRigidSubgraph (theiasfm_amd/host/rigid_subgraph_ops.cc).
//   -DRSG_STUB_ABI    the C ABI call is replaced by a recorder that hands back a programmed keep: the flattening order
//                     (views in ascending ViewId, edges in ascending ViewIdPair, position_2 per edge, the orientations
//                     in view order), a graph untouched when a view with an edge has no orientation or when the call
//                     fails, and the removal of exactly the views that are not kept.  Needs no device.
//   otherwise         without a device: false, the graph unchanged.  With one: the reference's scene (a skeletal chain
//                     and random further pairs: no view removed) and a rigid core with leaves on scattered ids (the
//                     leaves removed), against the C ABI called on the graph flattened independently of the shim.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <unordered_map>
#include <vector>

#include "theia/sfm/extract_maximally_parallel_rigid_subgraph.h"
#include "theia/sfm/view_graph/view_graph.h"
#include "theia_mi355_ba.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      return 1;                                                            \
    }                                                                      \
  } while (0)

using theia::TwoViewInfo;
using theia::ViewGraph;
using theia::ViewId;
using theia::ViewIdPair;
typedef std::unordered_map<ViewId, Eigen::Vector3d> OrientationMap;

namespace {
struct Lcg {
  unsigned long long s;
  double next() {  // uniform in [-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(s >> 11) / 4503599627370496.0 - 1.0;
  }
};

std::vector<ViewIdPair> SortedEdges(const ViewGraph& g) {
  std::vector<ViewIdPair> e;
  for (const auto& edge : g.GetAllEdges()) e.push_back(edge.first);
  std::sort(e.begin(), e.end());
  return e;
}

// R p with R the rotation of the angle-axis vector aa (Rodrigues)
Eigen::Vector3d Rotate(const Eigen::Vector3d& aa, const Eigen::Vector3d& p) {
  const double theta = std::sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
  if (theta < 1e-12) return p;
  const double w[3] = {aa[0] / theta, aa[1] / theta, aa[2] / theta};
  const double c = std::cos(theta), s = std::sin(theta);
  const double dot = w[0] * p[0] + w[1] * p[1] + w[2] * p[2];
  const double cross[3] = {w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]};
  Eigen::Vector3d r;
  for (int a = 0; a < 3; ++a) r[a] = c * p[a] + s * cross[a] + (1.0 - c) * dot * w[a];
  return r;
}

struct Scene {
  ViewGraph graph;
  OrientationMap orientations;
  std::map<ViewId, Eigen::Vector3d> positions;
};

void AddView(Scene* sc, Lcg* rng, ViewId id) {
  Eigen::Vector3d o, c;
  for (int a = 0; a < 3; ++a) {
    o[a] = rng->next();
    c[a] = rng->next();
  }
  sc->orientations[id] = o;
  sc->positions[id] = c;
}

// position_2 = R1 (c2 - c1) / |c2 - c1|
void AddValidEdge(Scene* sc, ViewId a, ViewId b) {
  const ViewId first = std::min(a, b), second = std::max(a, b);
  Eigen::Vector3d t;
  double norm = 0.0;
  for (int k = 0; k < 3; ++k) {
    t[k] = sc->positions[second][k] - sc->positions[first][k];
    norm += t[k] * t[k];
  }
  for (int k = 0; k < 3; ++k) t[k] /= std::sqrt(norm);
  TwoViewInfo info;
  info.position_2 = Rotate(sc->orientations[first], t);
  sc->graph.AddEdge(first, second, info);
}

// extract_maximally_parallel_rigid_subgraph_test.cc:95-124 on scattered ids: a skeletal chain and random further pairs
Scene ReferenceScene(const std::vector<ViewId>& ids, int num_pairs, unsigned long long seed) {
  Scene sc;
  Lcg rng{seed};
  for (const ViewId id : ids) AddView(&sc, &rng, id);
  for (size_t i = 1; i < ids.size(); ++i) AddValidEdge(&sc, ids[i - 1], ids[i]);
  while (sc.graph.NumEdges() < num_pairs) {
    const size_t a = static_cast<size_t>((rng.next() + 1.0) * 0.5 * ids.size()) % ids.size();
    const size_t b = static_cast<size_t>((rng.next() + 1.0) * 0.5 * ids.size()) % ids.size();
    if (a == b || sc.graph.HasEdge(ids[a], ids[b])) continue;
    AddValidEdge(&sc, ids[a], ids[b]);
  }
  return sc;
}

#ifdef RSG_STUB_ABI
// what the stub saw and what it answers
struct Recorded {
  int calls = 0;
  int32_t num_views = 0, device = 0;
  std::vector<int32_t> v1, v2;
  std::vector<double> orientation, position2;
  bool mask_null = false, rotation2_null = false;
  std::vector<uint8_t> keep;  // programmed
  int32_t rc = TMI_BA_OK;
} g_rec;
#endif
}  // namespace

#ifdef RSG_STUB_ABI
extern "C" {
void tmi_ba_rigid_subgraph_options_init(tmi_ba_rigid_subgraph_options* o) {
  o->relative_shift = 1e-9;
  o->null_tolerance = 1e-9;
  o->max_null_dimension = 128;
  o->max_iterations = 100;
  o->device = -1;
}
int32_t tmi_ba_extract_parallel_rigid_subgraph(const tmi_ba_view_pair_batch* B, const uint8_t* view_mask,
                                               const tmi_ba_rigid_subgraph_options* options, uint8_t* keep,
                                               int32_t* component_size, double* null_space,
                                               tmi_ba_rigid_subgraph_summary* summary) {
  (void)component_size;
  (void)null_space;
  ++g_rec.calls;
  g_rec.num_views = B->num_views;
  g_rec.device = options->device;
  g_rec.v1.assign(B->pair_view1, B->pair_view1 + B->num_pairs);
  g_rec.v2.assign(B->pair_view2, B->pair_view2 + B->num_pairs);
  g_rec.orientation.assign(B->view_rotation, B->view_rotation + 3 * B->num_views);
  g_rec.position2.assign(B->pair_position2, B->pair_position2 + 3 * B->num_pairs);
  g_rec.mask_null = view_mask == nullptr;
  g_rec.rotation2_null = B->pair_rotation2 == nullptr;
  std::memset(summary, 0, sizeof(*summary));
  if (g_rec.rc != TMI_BA_OK) return g_rec.rc;
  std::copy(g_rec.keep.begin(), g_rec.keep.end(), keep);
  return TMI_BA_OK;
}
}

int main() {
  // ids out of order and far apart; view 900 has no edge
  const std::vector<ViewId> ids = {40, 7, 300, 12, 5};
  Scene sc = ReferenceScene(ids, 7, 99);
  const std::vector<ViewIdPair> all = SortedEdges(sc.graph);
  const std::vector<ViewId> sorted = {5, 7, 12, 40, 300};

  {  // the flattening order and the removal of exactly the views that are not kept
    ViewGraph g = sc.graph;
    g_rec = Recorded();
    g_rec.keep = {1, 0, 1, 1, 0};  // 7 and 300 go
    CHECK(theia::ExtractMaximallyParallelRigidSubgraphOrReport(sc.orientations, &g, 3));
    CHECK(g_rec.calls == 1 && g_rec.num_views == 5 && g_rec.device == 3 && g_rec.mask_null && g_rec.rotation2_null);
    CHECK(g_rec.v1.size() == all.size());
    for (size_t e = 0; e < all.size(); ++e) {
      CHECK(sorted[g_rec.v1[e]] == all[e].first && sorted[g_rec.v2[e]] == all[e].second);
      const TwoViewInfo* info = sc.graph.GetEdge(all[e].first, all[e].second);
      for (int a = 0; a < 3; ++a) CHECK(g_rec.position2[3 * e + a] == info->position_2[a]);
    }
    for (size_t v = 0; v < sorted.size(); ++v)
      for (int a = 0; a < 3; ++a) CHECK(g_rec.orientation[3 * v + a] == sc.orientations[sorted[v]][a]);
    CHECK(g.NumViews() == 3 && g.HasView(5) && g.HasView(12) && g.HasView(40) && !g.HasView(7) && !g.HasView(300));
    for (const ViewIdPair& p : all) {
      const bool both = p.first != 7 && p.first != 300 && p.second != 7 && p.second != 300;
      CHECK(g.HasEdge(p.first, p.second) == both);
    }
  }
  {  // the reference's signature does the same on the current device
    ViewGraph g = sc.graph;
    g_rec = Recorded();
    g_rec.keep = {1, 1, 1, 1, 1};
    theia::ExtractMaximallyParallelRigidSubgraph(sc.orientations, &g);
    CHECK(g_rec.calls == 1 && g_rec.device == -1 && SortedEdges(g) == all && g.NumViews() == 5);
  }
  {  // an orientation more than the graph has views is not sent; a view with an edge and no orientation: untouched
    ViewGraph g = sc.graph;
    OrientationMap more = sc.orientations;
    more[900] = Eigen::Vector3d(0.1, 0.2, 0.3);
    g_rec = Recorded();
    g_rec.keep = {1, 1, 1, 1, 1};
    CHECK(theia::ExtractMaximallyParallelRigidSubgraphOrReport(more, &g) && g_rec.num_views == 5);
    OrientationMap fewer = sc.orientations;
    fewer.erase(12);
    g_rec = Recorded();
    g_rec.keep = {0, 0, 0, 0, 0};
    CHECK(!theia::ExtractMaximallyParallelRigidSubgraphOrReport(fewer, &g));
    CHECK(g_rec.calls == 0 && SortedEdges(g) == all && g.NumViews() == 5);
  }
  {  // a failed call: untouched
    ViewGraph g = sc.graph;
    g_rec = Recorded();
    g_rec.keep = {0, 0, 0, 0, 0};
    g_rec.rc = TMI_BA_ERR_NULL_SPACE_TOO_LARGE;
    CHECK(!theia::ExtractMaximallyParallelRigidSubgraphOrReport(sc.orientations, &g));
    CHECK(g_rec.calls == 1 && SortedEdges(g) == all && g.NumViews() == 5);
  }
  {  // no graph, no edges
    g_rec = Recorded();
    CHECK(!theia::ExtractMaximallyParallelRigidSubgraphOrReport(sc.orientations, nullptr));
    ViewGraph empty;
    CHECK(theia::ExtractMaximallyParallelRigidSubgraphOrReport(sc.orientations, &empty) && g_rec.calls == 0);
  }
  std::printf("rigid subgraph shim (stubbed call): OK\n");
  return 0;
}
#else

namespace {
// The dense batch of the graph, built independently of the shim.
struct Dense {
  std::vector<ViewId> ids;
  std::vector<int32_t> v1, v2;
  std::vector<double> orientation, position2;
  tmi_ba_view_pair_batch B;
};

void MakeDense(const Scene& sc, Dense* d) {
  const std::vector<ViewIdPair> pairs = SortedEdges(sc.graph);
  std::map<ViewId, int> index;
  for (const ViewIdPair& p : pairs) index[p.first] = index[p.second] = 0;
  for (auto& entry : index) {
    entry.second = static_cast<int>(d->ids.size());
    d->ids.push_back(entry.first);
    for (int a = 0; a < 3; ++a) d->orientation.push_back(sc.orientations.at(entry.first)[a]);
  }
  for (const ViewIdPair& p : pairs) {
    d->v1.push_back(index[p.first]);
    d->v2.push_back(index[p.second]);
    for (int a = 0; a < 3; ++a) d->position2.push_back(sc.graph.GetEdge(p.first, p.second)->position_2[a]);
  }
  std::memset(&d->B, 0, sizeof(d->B));
  d->B.num_views = static_cast<int32_t>(d->ids.size());
  d->B.view_rotation = d->orientation.data();
  d->B.num_pairs = static_cast<int32_t>(pairs.size());
  d->B.pair_view1 = d->v1.data();
  d->B.pair_view2 = d->v2.data();
  d->B.pair_position2 = d->position2.data();
}

// the shim against the C ABI on the same flattened input; *kept: the views the call keeps
int CompareWithAbi(const Scene& sc, std::vector<ViewId>* kept, int* null_dimension) {
  Dense d;
  MakeDense(sc, &d);
  tmi_ba_rigid_subgraph_options options;
  tmi_ba_rigid_subgraph_options_init(&options);
  std::vector<uint8_t> keep(d.ids.size(), 9);
  tmi_ba_rigid_subgraph_summary summary;
  CHECK(tmi_ba_extract_parallel_rigid_subgraph(&d.B, nullptr, &options, keep.data(), nullptr, nullptr, &summary) == TMI_BA_OK);
  *null_dimension = summary.null_dimension;
  ViewGraph g = sc.graph;
  CHECK(theia::ExtractMaximallyParallelRigidSubgraphOrReport(sc.orientations, &g));
  kept->clear();
  for (size_t v = 0; v < d.ids.size(); ++v) {
    CHECK(keep[v] == 0 || keep[v] == 1);
    CHECK(g.HasView(d.ids[v]) == (keep[v] == 1));
    if (keep[v]) kept->push_back(d.ids[v]);
  }
  CHECK(static_cast<int>(kept->size()) == summary.num_kept && g.NumViews() == summary.num_kept);
  for (const ViewIdPair& p : SortedEdges(sc.graph))
    CHECK(g.HasEdge(p.first, p.second) == (g.HasView(p.first) && g.HasView(p.second)));
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  const bool have_device = tmi_ba_device_count() > 0;
  if (need_device) CHECK(have_device);
  std::vector<ViewId> ids;
  for (ViewId i = 0; i < 10; ++i) ids.push_back(3 + 17 * ((i * 7) % 10));  // scattered, out of order
  const Scene reference = ReferenceScene(ids, 30, 57);

  if (!have_device) {
    ViewGraph g = reference.graph;
    CHECK(!theia::ExtractMaximallyParallelRigidSubgraphOrReport(reference.orientations, &g));
    theia::ExtractMaximallyParallelRigidSubgraph(reference.orientations, &g);
    CHECK(SortedEdges(g) == SortedEdges(reference.graph) && g.NumViews() == reference.graph.NumViews());
    std::printf("rigid subgraph shim (no device): OK\n");
    return 0;
  }

  std::vector<ViewId> kept;
  int k = 0;
  // (a) extract_maximally_parallel_rigid_subgraph_test.cc:169-170: no view removed, every valid edge left
  if (CompareWithAbi(reference, &kept, &k)) return 1;
  CHECK(kept.size() == ids.size() && k == 4);
  {
    ViewGraph g = reference.graph;
    theia::ExtractMaximallyParallelRigidSubgraph(reference.orientations, &g);
    CHECK(g.NumViews() == 10 && g.NumEdges() >= 30);
  }
  // (b) a rigid core of 12 and 3 leaves on one edge each: k = 7, the leaves go
  std::vector<ViewId> core;
  for (ViewId i = 0; i < 12; ++i) core.push_back(100 + 11 * ((i * 5) % 12));
  Scene leaves = ReferenceScene(core, 36, 11);
  Lcg rng{5};
  const ViewId leaf_ids[3] = {2, 150, 999};
  for (int l = 0; l < 3; ++l) {
    AddView(&leaves, &rng, leaf_ids[l]);
    AddValidEdge(&leaves, core[static_cast<size_t>(3 * l + 1)], leaf_ids[l]);
  }
  if (CompareWithAbi(leaves, &kept, &k)) return 1;
  std::sort(core.begin(), core.end());
  CHECK(k == 7 && kept == core);
  std::printf("rigid subgraph shim: OK\n");
  return 0;
}
#endif
