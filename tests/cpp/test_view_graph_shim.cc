// tests/test_host_shim_view_graph.py: theia::ViewGraph (include/theia/sfm/view_graph/view_graph.h) and the view-graph
// shim (theiasfm_amd/host/view_graph_ops.cc).
//   always:           the ViewGraph semantics of the reference's view_graph_test.cc.
//   without a device: RemoveDisconnectedViewPairs returns the empty set, OrientationsFromMaximumSpanningTree returns
//                     false, the ViewGraph forms of the two filters remove nothing; graph and map are unchanged.
//   with a device:    both functions equal the C ABI called on the graph with the views in ascending ViewId order and
//                     the edges in ascending ViewIdPair order; the ViewGraph forms of the filters equal the vector
//                     forms.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "theia/sfm/filter_view_pairs_from_orientation.h"
#include "theia/sfm/filter_view_pairs_from_relative_translation.h"
#include "theia/sfm/view_graph/orientations_from_maximum_spanning_tree.h"
#include "theia/sfm/view_graph/remove_disconnected_view_pairs.h"
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

// view_graph_test.cc
int TestViewGraphSemantics() {
  ViewGraph g;
  CHECK(g.NumViews() == 0 && g.NumEdges() == 0);
  TwoViewInfo info1, info2;
  info1.num_verified_matches = 1;
  info2.num_verified_matches = 2;
  g.AddEdge(0, 1, info1);
  g.AddEdge(2, 0, info2);
  g.AddEdge(3, 3, info2);  // ignored
  CHECK(g.NumViews() == 3 && g.NumEdges() == 2);
  CHECK(g.HasView(0) && g.HasView(1) && g.HasView(2) && !g.HasView(3));
  CHECK(g.HasEdge(0, 1) && g.HasEdge(1, 0) && g.HasEdge(0, 2) && g.HasEdge(2, 0) && !g.HasEdge(1, 2));
  CHECK(g.GetEdge(1, 0) != nullptr && g.GetEdge(1, 0)->num_verified_matches == 1);
  CHECK(g.GetEdge(0, 2) == g.GetEdge(2, 0) && g.GetEdge(2, 0)->num_verified_matches == 2);
  CHECK(g.GetEdge(1, 2) == nullptr && g.GetMutableEdge(1, 2) == nullptr);
  CHECK(g.GetAllEdges().count(ViewIdPair(0, 2)) == 1 && g.GetAllEdges().count(ViewIdPair(2, 0)) == 0);
  g.GetMutableEdge(0, 1)->num_verified_matches = 7;
  CHECK(g.GetEdge(0, 1)->num_verified_matches == 7);
  g.AddEdge(1, 0, info2);  // an existing edge gets the new value
  CHECK(g.NumEdges() == 2 && g.GetEdge(0, 1)->num_verified_matches == 2);
  const auto* n0 = g.GetNeighborIdsForView(0);
  CHECK(n0 != nullptr && n0->size() == 2 && n0->count(1) && n0->count(2));
  CHECK(g.GetNeighborIdsForView(5) == nullptr);
  CHECK(g.ViewIds() == (std::unordered_set<ViewId>{0, 1, 2}));
  // RemoveEdge
  CHECK(!g.RemoveEdge(1, 2) && !g.RemoveEdge(0, 9));
  CHECK(g.RemoveEdge(1, 0) && g.NumEdges() == 1 && !g.HasEdge(0, 1) && g.HasView(1));
  CHECK(g.GetNeighborIdsForView(1)->empty() && g.GetNeighborIdsForView(0)->size() == 1);
  // RemoveView
  g.AddEdge(0, 1, info1);
  g.AddEdge(1, 2, info1);
  CHECK(!g.RemoveView(9));
  CHECK(g.RemoveView(0) && g.NumViews() == 2 && g.NumEdges() == 1 && g.HasEdge(1, 2) && !g.HasView(0));
  CHECK(g.GetNeighborIdsForView(1)->size() == 1 && g.GetNeighborIdsForView(2)->count(0) == 0);
  // ExtractSubgraph
  ViewGraph h, sub;
  for (ViewId i = 0; i < 5; ++i)
    for (ViewId j = i + 1; j < 5; ++j) h.AddEdge(i, j, info1);
  h.ExtractSubgraph({1, 3, 4, 8}, &sub);
  CHECK(sub.NumViews() == 3 && sub.NumEdges() == 3 && sub.HasEdge(1, 3) && sub.HasEdge(1, 4) && sub.HasEdge(3, 4));
  // GetLargestConnectedComponentIds: {10, 11, 12} against {1, 2} and, of the same size, {4, 5, 6}: the smallest id
  ViewGraph c;
  c.AddEdge(10, 11, info1);
  c.AddEdge(11, 12, info1);
  c.AddEdge(1, 2, info1);
  std::unordered_set<ViewId> cc;
  c.GetLargestConnectedComponentIds(&cc);
  CHECK(cc == (std::unordered_set<ViewId>{10, 11, 12}));
  c.AddEdge(5, 4, info1);
  c.AddEdge(6, 5, info1);
  c.GetLargestConnectedComponentIds(&cc);
  CHECK(cc == (std::unordered_set<ViewId>{4, 5, 6}));
  return 0;
}

// Scattered ids; two components with an edge ({3, 7, 9, 12, 50, 77, 300} and {20, 21, 1000}); rotation_2 random,
// position_2 a unit vector, distinct and tied match counts.
struct Scene {
  ViewGraph graph;
  std::unordered_map<ViewId, Eigen::Vector3d> filter_orientations;
};

Scene MakeScene() {
  Scene sc;
  Lcg rng{4242};
  const ViewId pairs[][2] = {{50, 7}, {300, 7}, {300, 12}, {9, 12}, {9, 77}, {3, 77}, {3, 50}, {50, 9},
                             {12, 7}, {1000, 20}, {21, 20}, {21, 1000}, {77, 300}};
  const int matches[] = {40, 90, 90, 35, 90, 12, 61, 40, 40, 500, 400, 300, 35};
  for (size_t e = 0; e < sizeof(pairs) / sizeof(pairs[0]); ++e) {
    TwoViewInfo info;
    double norm = 0.0;
    for (int a = 0; a < 3; ++a) {
      info.rotation_2[a] = (e % 3 ? 0.7 : 0.02) * rng.next();
      info.position_2[a] = rng.next();
      norm += info.position_2[a] * info.position_2[a];
    }
    for (int a = 0; a < 3; ++a) info.position_2[a] /= std::sqrt(norm);
    info.num_verified_matches = matches[e];
    sc.graph.AddEdge(pairs[e][0], pairs[e][1], info);
  }
  for (const ViewId id : sc.graph.ViewIds()) {
    Eigen::Vector3d r;
    for (int a = 0; a < 3; ++a) r[a] = 0.05 * rng.next();
    sc.filter_orientations[id] = r;
  }
  return sc;
}

// The dense batch of the graph, built independently of the shim.
struct Dense {
  std::vector<ViewId> ids;
  std::vector<ViewIdPair> pairs;
  std::vector<int32_t> v1, v2, matches;
  std::vector<double> rotation2;
  tmi_ba_view_pair_batch B;
};

void MakeDense(const ViewGraph& g, Dense* d) {
  d->pairs = SortedEdges(g);
  std::map<ViewId, int> index;
  for (const ViewIdPair& p : d->pairs) {
    index[p.first] = 0;
    index[p.second] = 0;
  }
  for (auto& entry : index) {
    entry.second = static_cast<int>(d->ids.size());
    d->ids.push_back(entry.first);
  }
  for (const ViewIdPair& p : d->pairs) {
    const TwoViewInfo* info = g.GetEdge(p.first, p.second);
    d->v1.push_back(index[p.first]);
    d->v2.push_back(index[p.second]);
    d->matches.push_back(info->num_verified_matches);
    for (int a = 0; a < 3; ++a) d->rotation2.push_back(info->rotation_2[a]);
  }
  std::memset(&d->B, 0, sizeof(d->B));
  d->B.num_views = static_cast<int32_t>(d->ids.size());
  d->B.num_pairs = static_cast<int32_t>(d->pairs.size());
  d->B.pair_view1 = d->v1.data();
  d->B.pair_view2 = d->v2.data();
  d->B.pair_rotation2 = d->rotation2.data();
}
}  // namespace

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  if (TestViewGraphSemantics()) return 1;
  const bool have_device = tmi_ba_device_count() > 0;
  if (need_device) CHECK(have_device);
  const Scene sc = MakeScene();
  const std::vector<ViewIdPair> all = SortedEdges(sc.graph);

  if (!have_device) {
    ViewGraph g = sc.graph;
    CHECK(theia::RemoveDisconnectedViewPairs(&g).empty() && SortedEdges(g) == all && g.NumViews() == sc.graph.NumViews());
    std::unordered_map<ViewId, Eigen::Vector3d> o;
    o[5][0] = 1.5;
    CHECK(!theia::OrientationsFromMaximumSpanningTree(g, &o) && o.size() == 1 && o[5][0] == 1.5);
    theia::FilterViewPairsFromOrientation(sc.filter_orientations, 5.0, &g);
    theia::FilterViewPairsFromRelativeTranslation(theia::FilterViewPairsFromRelativeTranslationOptions(),
                                                  sc.filter_orientations, &g);
    CHECK(SortedEdges(g) == all);
    CHECK(theia::RemoveDisconnectedViewPairs(nullptr).empty());
    std::printf("view-graph shim (no device): OK\n");
    return 0;
  }

  Dense d;
  MakeDense(sc.graph, &d);
  {  // RemoveDisconnectedViewPairs against the C ABI
    std::vector<uint8_t> in_largest(d.ids.size()), keep(d.pairs.size());
    tmi_ba_view_graph_component_summary cs;
    CHECK(tmi_ba_largest_connected_component(&d.B, nullptr, -1, nullptr, in_largest.data(), keep.data(), &cs) == TMI_BA_OK);
    CHECK(cs.num_components == 2 && cs.largest_num_views == 7 && d.ids[cs.largest_label] == 3 && cs.num_views_removed == 3);
    ViewGraph g = sc.graph;
    const std::unordered_set<ViewId> removed = theia::RemoveDisconnectedViewPairs(&g);
    CHECK(removed == (std::unordered_set<ViewId>{20, 21, 1000}));
    CHECK(static_cast<int>(removed.size()) == cs.num_views_removed && g.NumEdges() == cs.num_pairs_kept);
    std::vector<ViewIdPair> want;
    for (size_t e = 0; e < d.pairs.size(); ++e)
      if (keep[e]) want.push_back(d.pairs[e]);
    CHECK(SortedEdges(g) == want);
    for (size_t v = 0; v < d.ids.size(); ++v) CHECK(g.HasView(d.ids[v]) == (in_largest[v] != 0));
    CHECK(theia::RemoveDisconnectedViewPairs(&g).empty() && SortedEdges(g) == want);  // one component: nothing to do
    ViewGraph empty;
    CHECK(theia::RemoveDisconnectedViewPairs(&empty).empty());
  }
  {  // OrientationsFromMaximumSpanningTree against the C ABI
    std::vector<double> orientation(3 * d.ids.size(), -9.0);
    std::vector<int32_t> depth(d.ids.size());
    tmi_ba_spanning_tree_summary ts;
    CHECK(tmi_ba_orientations_from_maximum_spanning_tree(&d.B, d.matches.data(), nullptr, -1, -1, orientation.data(),
                                                         nullptr, nullptr, depth.data(), nullptr, &ts) == TMI_BA_OK);
    CHECK(ts.usable == 1 && ts.num_tree_pairs == 6 && d.ids[ts.root_view] == 3);
    std::unordered_map<ViewId, Eigen::Vector3d> o;
    o[20][0] = 1.5;  // outside the largest component: left as it is
    CHECK(theia::OrientationsFromMaximumSpanningTree(sc.graph, &o));
    CHECK(o.size() == 8 && o[20][0] == 1.5 && o.count(21) == 0 && o.count(1000) == 0);
    for (size_t v = 0; v < d.ids.size(); ++v) {
      if (depth[v] < 0) continue;
      CHECK(o.count(d.ids[v]) == 1);
      for (int a = 0; a < 3; ++a) CHECK(o[d.ids[v]][a] == orientation[3 * v + a]);  // the same call: the same bits
    }
    for (int a = 0; a < 3; ++a) CHECK(o[3][a] == 0.0);
    ViewGraph empty;
    CHECK(!theia::OrientationsFromMaximumSpanningTree(empty, &o) && o.size() == 8);
  }
  {  // the ViewGraph forms of the filters against the vector forms
    for (int which = 0; which < 2; ++which) {
      ViewGraph g = sc.graph, h = sc.graph;
      std::vector<std::pair<ViewIdPair, TwoViewInfo*>> edges;
      for (const ViewIdPair& p : all) edges.emplace_back(p, h.GetMutableEdge(p.first, p.second));
      theia::FilterViewPairsFromRelativeTranslationOptions options;
      options.seed = 5;
      int removed;
      if (which == 0) {
        // the five edges with a small rotation_2 are at most 0.21 rad = 12 degrees from the orientations' relative
        // rotation and stay; the others draw rotation_2 from [-0.7, 0.7]^3
        removed = theia::FilterViewPairsFromOrientation(sc.filter_orientations, 15.0, &edges);
        theia::FilterViewPairsFromOrientation(sc.filter_orientations, 15.0, &g);
      } else {
        removed = theia::FilterViewPairsFromRelativeTranslation(options, sc.filter_orientations, &edges);
        theia::FilterViewPairsFromRelativeTranslation(options, sc.filter_orientations, &g);
      }
      std::vector<ViewIdPair> want;
      for (const auto& e : edges) want.push_back(e.first);
      CHECK(SortedEdges(g) == want && g.NumEdges() + removed == static_cast<int>(all.size()));
      CHECK(g.NumViews() == sc.graph.NumViews());  // RemoveEdge keeps the views
      if (which == 0) CHECK(removed > 0 && removed <= static_cast<int>(all.size()) - 5);
    }
  }
  std::printf("view-graph shim: OK\n");
  return 0;
}
