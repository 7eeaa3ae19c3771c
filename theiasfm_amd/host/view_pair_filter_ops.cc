// Host shim of theia::FilterViewPairsFromRelativeTranslation (reference
// filter_view_pairs_from_relative_translation.cc:256-308) and theia::FilterViewPairsFromOrientation
// (filter_view_pairs_from_orientation.cc:72-122) on the C ABI: the edge list is flattened into one
// tmi_ba_view_pair_batch -- a rotation per view, numbered in ascending ViewId order, and the TwoViewInfo of every
// edge -- and filtered in one device call.
#include <cstdio>
#include <vector>

#include "flat_view_graph.h"
#include "theia/sfm/filter_view_pairs_from_orientation.h"
#include "theia/sfm/filter_view_pairs_from_relative_translation.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
using EdgeList = std::vector<std::pair<ViewIdPair, TwoViewInfo*>>;

// The edges that go to the device (`sent`: their places in the caller's vector) on dense view indices.
struct FlatEdges {
  flat_view_graph::FlatViewGraph graph;
  std::vector<double> rotation;
  std::vector<size_t> sent;
  tmi_ba_view_pair_batch Batch() const { return graph.Batch(rotation.data()); }
};

// usable[e] != 0: edge e has an info and both orientations.  The views of the usable edges get a row; the usable edges
// are sent in the caller's order.
FlatEdges Flatten(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations, const EdgeList& edges,
                  const std::vector<char>& usable) {
  FlatEdges flat;
  for (size_t e = 0; e < edges.size(); ++e)
    if (usable[e]) flat.graph.views.Add(edges[e].first);
  flat.graph.views.Finish();
  flat.rotation = flat.graph.views.Gather(orientations);
  for (size_t e = 0; e < edges.size(); ++e) {
    if (!usable[e]) continue;
    flat.graph.AddPair(edges[e].first, &edges[e].second->rotation_2, &edges[e].second->position_2);
    flat.sent.push_back(e);
  }
  return flat;
}

std::vector<char> UsableEdges(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations, const EdgeList& edges) {
  std::vector<char> usable(edges.size(), 0);
  for (size_t e = 0; e < edges.size(); ++e)
    usable[e] = edges[e].second != nullptr && orientations.count(edges[e].first.first) != 0 &&
                orientations.count(edges[e].first.second) != 0;
  return usable;
}

int EraseMarked(const std::vector<char>& remove, EdgeList* edges) {
  size_t kept = 0;
  for (size_t e = 0; e < edges->size(); ++e)
    if (!remove[e]) (*edges)[kept++] = (*edges)[e];
  const int removed = static_cast<int>(edges->size() - kept);
  edges->resize(kept);
  return removed;
}
}  // namespace

int FilterViewPairsFromRelativeTranslation(const FilterViewPairsFromRelativeTranslationOptions& options,
                                           const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                           EdgeList* edges, int device) {
  if (edges == nullptr || edges->empty()) return 0;
  const std::vector<char> usable = UsableEdges(orientations, *edges);
  for (const char u : usable) {
    if (u) continue;
    std::fprintf(stderr, "[theia::FilterViewPairsFromRelativeTranslation] an edge without a TwoViewInfo or without "
                         "an orientation of both views: nothing filtered\n");
    return 0;
  }
  const FlatEdges flat = Flatten(orientations, *edges, usable);
  const tmi_ba_view_pair_batch B = flat.Batch();
  tmi_ba_translation_filter_options o;
  tmi_ba_translation_filter_options_init(&o);
  o.num_iterations = options.num_iterations;
  o.translation_projection_tolerance = options.translation_projection_tolerance;
  o.seed = options.seed;
  std::vector<double> axes;
  if (!options.axes.empty()) {
    if (static_cast<int>(options.axes.size()) != options.num_iterations) {
      std::fprintf(stderr, "[theia::FilterViewPairsFromRelativeTranslation] options.axes must hold num_iterations "
                           "axes: nothing filtered\n");
      return 0;
    }
    for (const Eigen::Vector3d& a : options.axes) flat_view_graph::Append(a, &axes);
  }
  std::vector<uint8_t> flag(flat.sent.size(), 0);
  tmi_ba_view_pair_filter_summary fs;
  const int rc = tmi_ba_filter_view_pairs_from_relative_translation(
      &B, &o, axes.empty() ? nullptr : axes.data(), axes.empty() ? 0 : 1, device, flag.data(), nullptr, nullptr,
      nullptr, &fs);
  if (flat_view_graph::DeviceCallFailed("[theia::FilterViewPairsFromRelativeTranslation]", rc)) return 0;
  std::vector<char> remove(edges->size(), 0);
  for (size_t p = 0; p < flat.sent.size(); ++p) remove[flat.sent[p]] = flag[p] != 0;
  return EraseMarked(remove, edges);
}

int FilterViewPairsFromOrientation(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                   double max_relative_rotation_difference_degrees, EdgeList* edges, int device) {
  if (edges == nullptr || edges->empty()) return 0;
  if (!(max_relative_rotation_difference_degrees >= 0.0)) {
    std::fprintf(stderr, "[theia::FilterViewPairsFromOrientation] negative threshold: nothing filtered\n");
    return 0;
  }
  const std::vector<char> usable = UsableEdges(orientations, *edges);
  const FlatEdges flat = Flatten(orientations, *edges, usable);
  std::vector<uint8_t> flag(flat.sent.size(), 0);
  if (!flat.sent.empty()) {
    const tmi_ba_view_pair_batch B = flat.Batch();
    tmi_ba_view_pair_filter_summary fs;
    const int rc = tmi_ba_filter_view_pairs_from_orientation(&B, max_relative_rotation_difference_degrees, device,
                                                             flag.data(), nullptr, &fs);
    if (flat_view_graph::DeviceCallFailed("[theia::FilterViewPairsFromOrientation]", rc)) return 0;
  }
  // :94-103: an edge with a view that has no orientation is removed
  std::vector<char> remove(edges->size(), 0);
  for (size_t e = 0; e < edges->size(); ++e) remove[e] = !usable[e];
  for (size_t p = 0; p < flat.sent.size(); ++p) remove[flat.sent[p]] = flag[p] != 0;
  return EraseMarked(remove, edges);
}
}  // namespace theia
