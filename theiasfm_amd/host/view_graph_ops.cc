// Host shim of theia::RemoveDisconnectedViewPairs (reference view_graph/remove_disconnected_view_pairs.cc:48-95) and
// theia::OrientationsFromMaximumSpanningTree (view_graph/orientations_from_maximum_spanning_tree.cc:109-180) on the C
// ABI, and the ViewGraph forms of the two edge filters.  The graph is flattened into one tmi_ba_view_pair_batch -- the
// views with an edge numbered in ascending ViewId order, the edges in ascending ViewIdPair order -- and handled in one
// device call.
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#include "theia/sfm/filter_view_pairs_from_orientation.h"
#include "theia/sfm/filter_view_pairs_from_relative_translation.h"
#include "theia/sfm/view_graph/orientations_from_maximum_spanning_tree.h"
#include "theia/sfm/view_graph/remove_disconnected_view_pairs.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
struct FlatGraph {
  std::vector<ViewId> view_id;  // dense index -> ViewId, ascending
  std::vector<ViewIdPair> pair;  // ascending
  std::vector<int32_t> view1, view2, matches;
  std::vector<double> rotation2;
  tmi_ba_view_pair_batch Batch() const {
    tmi_ba_view_pair_batch B;
    B.num_views = static_cast<int32_t>(view_id.size());
    B.view_rotation = nullptr;
    B.num_pairs = static_cast<int32_t>(pair.size());
    B.pair_view1 = view1.data();
    B.pair_view2 = view2.data();
    B.pair_rotation2 = rotation2.data();
    B.pair_position2 = nullptr;
    return B;
  }
};

FlatGraph Flatten(const ViewGraph& graph) {
  FlatGraph flat;
  const auto& edges = graph.GetAllEdges();
  flat.pair.reserve(edges.size());
  for (const auto& edge : edges) flat.pair.push_back(edge.first);
  std::sort(flat.pair.begin(), flat.pair.end());
  std::map<ViewId, int> index;  // ascending ViewId -> dense index
  for (const ViewIdPair& p : flat.pair) {
    index[p.first] = 0;
    index[p.second] = 0;
  }
  for (auto& entry : index) {
    entry.second = static_cast<int>(flat.view_id.size());
    flat.view_id.push_back(entry.first);
  }
  for (const ViewIdPair& p : flat.pair) {
    const TwoViewInfo& info = edges.find(p)->second;
    flat.view1.push_back(index[p.first]);
    flat.view2.push_back(index[p.second]);
    flat.matches.push_back(info.num_verified_matches);
    for (int a = 0; a < 3; ++a) flat.rotation2.push_back(info.rotation_2[a]);
  }
  return flat;
}

// The graph's edges in ascending ViewIdPair order, as the vector forms of the filters take them.
std::vector<std::pair<ViewIdPair, TwoViewInfo*>> EdgeList(ViewGraph* graph) {
  std::vector<std::pair<ViewIdPair, TwoViewInfo*>> edges;
  for (const auto& edge : graph->GetAllEdges())
    edges.emplace_back(edge.first, graph->GetMutableEdge(edge.first.first, edge.first.second));
  std::sort(edges.begin(), edges.end());
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
  const FlatGraph flat = Flatten(*view_graph);
  const tmi_ba_view_pair_batch B = flat.Batch();
  std::vector<uint8_t> in_largest(flat.view_id.size(), 0);
  tmi_ba_view_graph_component_summary cs;
  const int rc = tmi_ba_largest_connected_component(&B, nullptr, device, nullptr, in_largest.data(), nullptr, &cs);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::RemoveDisconnectedViewPairs] device call failed: %s\n", tmi_ba_last_error());
    return removed_views;
  }
  // :71-86 (every view sent has an edge, so each one outside the largest component is in another component)
  for (size_t v = 0; v < flat.view_id.size(); ++v) {
    if (in_largest[v]) continue;
    view_graph->RemoveView(flat.view_id[v]);
    removed_views.insert(flat.view_id[v]);
  }
  return removed_views;
}

bool OrientationsFromMaximumSpanningTree(const ViewGraph& view_graph,
                                         std::unordered_map<ViewId, Eigen::Vector3d>* orientations, int device) {
  if (orientations == nullptr || view_graph.NumEdges() == 0) return false;
  const FlatGraph flat = Flatten(view_graph);
  const tmi_ba_view_pair_batch B = flat.Batch();
  std::vector<double> orientation(3 * flat.view_id.size(), 0.0);
  std::vector<int32_t> depth(flat.view_id.size(), -1);
  tmi_ba_spanning_tree_summary ts;
  const int rc = tmi_ba_orientations_from_maximum_spanning_tree(&B, flat.matches.data(), nullptr, -1, device,
                                                                orientation.data(), nullptr, nullptr, depth.data(),
                                                                nullptr, &ts);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::OrientationsFromMaximumSpanningTree] device call failed: %s\n", tmi_ba_last_error());
    return false;
  }
  if (!ts.usable) return false;
  for (size_t v = 0; v < flat.view_id.size(); ++v) {
    if (depth[v] < 0) continue;
    Eigen::Vector3d o;
    for (int a = 0; a < 3; ++a) o[a] = orientation[3 * v + a];
    (*orientations)[flat.view_id[v]] = o;
  }
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
