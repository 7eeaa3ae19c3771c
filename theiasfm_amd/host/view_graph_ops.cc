// Host shim of theia::RemoveDisconnectedViewPairs (reference view_graph/remove_disconnected_view_pairs.cc:48-95) and
// theia::OrientationsFromMaximumSpanningTree (view_graph/orientations_from_maximum_spanning_tree.cc:109-180) on the C
// ABI, and the ViewGraph forms of the two edge filters.  The graph is flattened into one tmi_ba_view_pair_batch -- the
// views with an edge numbered in ascending ViewId order, the edges in ascending ViewIdPair order -- and handled in one
// device call.
#include <cstdio>
#include <vector>

#include "flat_view_graph.h"
#include "theia/sfm/filter_view_pairs_from_orientation.h"
#include "theia/sfm/filter_view_pairs_from_relative_translation.h"
#include "theia/sfm/view_graph/orientations_from_maximum_spanning_tree.h"
#include "theia/sfm/view_graph/remove_disconnected_view_pairs.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
using flat_view_graph::FlatViewGraph;

// The views with an edge get a row; every edge is sent, with its rotation_2 and its num_verified_matches.
FlatViewGraph Flatten(const ViewGraph& graph) {
  std::vector<std::pair<ViewIdPair, const TwoViewInfo*>> edges;
  for (const auto& edge : graph.GetAllEdges()) edges.emplace_back(edge.first, &edge.second);
  flat_view_graph::SortByPair(&edges);
  FlatViewGraph flat;
  flat.views.AddEnds(edges);
  flat.views.Finish();
  for (const auto& edge : edges) {
    flat.AddPair(edge.first, &edge.second->rotation_2, nullptr);
    flat.matches.push_back(edge.second->num_verified_matches);
  }
  return flat;
}

// The graph's edges in ascending ViewIdPair order, as the vector forms of the filters take them.
std::vector<std::pair<ViewIdPair, TwoViewInfo*>> EdgeList(ViewGraph* graph) {
  std::vector<std::pair<ViewIdPair, TwoViewInfo*>> edges;
  for (const auto& edge : graph->GetAllEdges())
    edges.emplace_back(edge.first, graph->GetMutableEdge(edge.first.first, edge.first.second));
  flat_view_graph::SortByPair(&edges);
  return edges;
}

// Removes from the graph every edge of `before` that is not in `after` (a subsequence of `before`).
void RemoveMissingEdges(const std::vector<std::pair<ViewIdPair, TwoViewInfo*>>& before,
                        const std::vector<std::pair<ViewIdPair, TwoViewInfo*>>& after, ViewGraph* graph) {
  size_t k = 0;
  for (const auto& edge : before) {
    if (k < after.size() && after[k].first == edge.first) {
      ++k;
      continue;
    }
    graph->RemoveEdge(edge.first.first, edge.first.second);
  }
}
}  // namespace

std::unordered_set<ViewId> RemoveDisconnectedViewPairs(ViewGraph* view_graph, int device) {
  std::unordered_set<ViewId> removed_views;
  if (view_graph == nullptr || view_graph->NumEdges() == 0) return removed_views;
  const FlatViewGraph flat = Flatten(*view_graph);
  const tmi_ba_view_pair_batch B = flat.Batch(nullptr);
  std::vector<uint8_t> in_largest(flat.views.size(), 0);
  tmi_ba_view_graph_component_summary cs;
  const int rc = tmi_ba_largest_connected_component(&B, nullptr, device, nullptr, in_largest.data(), nullptr, &cs);
  if (flat_view_graph::DeviceCallFailed("[theia::RemoveDisconnectedViewPairs]", rc)) return removed_views;
  // :71-86 (every view sent has an edge, so each one outside the largest component is in another component)
  for (size_t v = 0; v < flat.views.size(); ++v) {
    if (in_largest[v]) continue;
    view_graph->RemoveView(flat.views.id(v));
    removed_views.insert(flat.views.id(v));
  }
  return removed_views;
}

bool OrientationsFromMaximumSpanningTree(const ViewGraph& view_graph,
                                         std::unordered_map<ViewId, Eigen::Vector3d>* orientations, int device) {
  if (orientations == nullptr || view_graph.NumEdges() == 0) return false;
  const FlatViewGraph flat = Flatten(view_graph);
  const tmi_ba_view_pair_batch B = flat.Batch(nullptr);
  std::vector<double> orientation(3 * flat.views.size(), 0.0);
  std::vector<int32_t> depth(flat.views.size(), -1);
  tmi_ba_spanning_tree_summary ts;
  const int rc = tmi_ba_orientations_from_maximum_spanning_tree(&B, flat.matches.data(), nullptr, -1, device,
                                                                orientation.data(), nullptr, nullptr, depth.data(),
                                                                nullptr, &ts);
  if (flat_view_graph::DeviceCallFailed("[theia::OrientationsFromMaximumSpanningTree]", rc)) return false;
  if (!ts.usable) return false;
  // only the views of the tree
  flat.views.Scatter(orientation, orientations, [&depth](const size_t v) { return depth[v] >= 0; });
  return true;
}

void FilterViewPairsFromOrientation(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                    double max_relative_rotation_difference_degrees, ViewGraph* view_graph,
                                    int device) {
  if (view_graph == nullptr) return;
  const std::vector<std::pair<ViewIdPair, TwoViewInfo*>> before = EdgeList(view_graph);
  std::vector<std::pair<ViewIdPair, TwoViewInfo*>> after = before;
  FilterViewPairsFromOrientation(orientations, max_relative_rotation_difference_degrees, &after, device);
  RemoveMissingEdges(before, after, view_graph);
}

void FilterViewPairsFromRelativeTranslation(const FilterViewPairsFromRelativeTranslationOptions& options,
                                            const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                            ViewGraph* view_graph, int device) {
  if (view_graph == nullptr) return;
  const std::vector<std::pair<ViewIdPair, TwoViewInfo*>> before = EdgeList(view_graph);
  std::vector<std::pair<ViewIdPair, TwoViewInfo*>> after = before;
  FilterViewPairsFromRelativeTranslation(options, orientations, &after, device);
  RemoveMissingEdges(before, after, view_graph);
}
}  // namespace theia
