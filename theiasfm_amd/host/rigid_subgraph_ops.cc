// Host shim of theia::ExtractMaximallyParallelRigidSubgraph (reference extract_maximally_parallel_rigid_subgraph.cc:172-228)
// on the C ABI.  The graph is flattened into one tmi_ba_view_pair_batch -- the views with an edge numbered in ascending
// ViewId order, the edges in ascending ViewIdPair order with their position_2 -- and handled in one device call; the
// views that come back with keep = 0 are removed.
#include <cstdio>
#include <vector>

#include "flat_view_graph.h"
#include "theia/sfm/extract_maximally_parallel_rigid_subgraph.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
using flat_view_graph::FlatViewGraph;

// The views with an edge get a row; every edge is sent with its position_2.
FlatViewGraph Flatten(const ViewGraph& graph) {
  std::vector<std::pair<ViewIdPair, const TwoViewInfo*>> edges;
  for (const auto& edge : graph.GetAllEdges()) edges.emplace_back(edge.first, &edge.second);
  flat_view_graph::SortByPair(&edges);
  FlatViewGraph flat;
  flat.views.AddEnds(edges);
  flat.views.Finish();
  for (const auto& edge : edges) flat.AddPair(edge.first, nullptr, &edge.second->position_2);
  return flat;
}
}  // namespace

bool ExtractMaximallyParallelRigidSubgraphOrReport(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                                   ViewGraph* view_graph, int device) {
  if (view_graph == nullptr) return false;
  if (view_graph->NumEdges() == 0) return true;
  const FlatViewGraph flat = Flatten(*view_graph);
  std::vector<uint8_t> given;
  const std::vector<double> orientation = flat.views.Gather(orientations, &given);
  for (size_t v = 0; v < flat.views.size(); ++v)
    if (!given[v]) {  // :68 FindOrDie
      std::fprintf(stderr, "[theia::ExtractMaximallyParallelRigidSubgraph] view %u has an edge and no orientation; "
                           "the graph is left as it is\n", static_cast<unsigned>(flat.views.id(v)));
      return false;
    }
  const tmi_ba_view_pair_batch B = flat.Batch(orientation.data());
  tmi_ba_rigid_subgraph_options options;
  tmi_ba_rigid_subgraph_options_init(&options);
  options.device = device;
  std::vector<uint8_t> keep(flat.views.size(), 0);
  tmi_ba_rigid_subgraph_summary summary;
  const int rc = tmi_ba_extract_parallel_rigid_subgraph(&B, nullptr, &options, keep.data(), nullptr, nullptr, &summary);
  if (flat_view_graph::DeviceCallFailed("[theia::ExtractMaximallyParallelRigidSubgraph]", rc)) return false;
  // :217-227
  for (size_t v = 0; v < flat.views.size(); ++v)
    if (!keep[v]) view_graph->RemoveView(flat.views.id(v));
  return true;
}

void ExtractMaximallyParallelRigidSubgraph(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                           ViewGraph* view_graph) {
  ExtractMaximallyParallelRigidSubgraphOrReport(orientations, view_graph, -1);
}
}  // namespace theia
