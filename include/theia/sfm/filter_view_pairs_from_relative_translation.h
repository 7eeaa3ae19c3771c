// reference: src/theia/sfm/filter_view_pairs_from_relative_translation.h:48-80 (declaration) and .cc:68-304
// (semantics): the 1DSfM filter of Wilson and Snavely (ECCV 2014).  The relative translations are projected onto
// (semi) random axes; for every axis the views are ordered by a greedy minimum-feedback-arc-set heuristic, and an
// edge whose projection contradicts the order collects the projection's size as "bad weight".  Edges whose weight
// over all axes exceeds translation_projection_tolerance * num_iterations are removed.
// Implemented on the C ABI (tmi_ba_filter_view_pairs_from_relative_translation): one workgroup per axis, all axes
// in one device launch, where the reference runs one axis per task on a CPU thread pool.  The orders the
// reference's hash maps leave open are fixed there (include/theia_mi355_ba.h).
#ifndef THEIA_MI355_FILTER_VIEW_PAIRS_FROM_RELATIVE_TRANSLATION_H_
#define THEIA_MI355_FILTER_VIEW_PAIRS_FROM_RELATIVE_TRANSLATION_H_
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>

#include "theia/sfm/twoview_info.h"
#include "theia/sfm/types.h"
#include "theia/sfm/view_graph/view_graph.h"
#include "theia/util/eigen_lite.h"

namespace theia {
struct FilterViewPairsFromRelativeTranslationOptions {
  // In place of the reference's rng: the seed of the engine's own axis generator (documented at the C ABI; it
  // is deterministic in the seed and does not equal the reference's generator) ...
  std::uint64_t seed = 0;
  // ... or the projection axes themselves, num_iterations of them, used as they are when not empty.
  std::vector<Eigen::Vector3d> axes;

  // Accepted and unused: every iteration is a workgroup of one launch.
  int num_threads = 1;

  // The projection will be performed for the given number of iterations (the reference recommends > 40).
  int num_iterations = 48;

  // tau in the paper.
  double translation_projection_tolerance = 0.08;
};

// The reference's call with the edge list in place of the ViewGraph (fill it from view_graph->GetAllEdges() /
// GetMutableEdge), as RefineRelativeTranslationsWithKnownRotations takes it.  The views of the
// edges are numbered in ascending ViewId order and the edges go to the device in the vector's order.  Removed
// edges are erased from *edges (the order of the others is kept); returns the number removed (call
// view_graph->RemoveEdge for the ids that left).  An edge with a null info or a view missing from `orientations`
// (the reference dies in FindOrDie), or a failed device call (no device: the message goes to stderr), leaves *edges
// unchanged and returns 0.
int FilterViewPairsFromRelativeTranslation(const FilterViewPairsFromRelativeTranslationOptions& options,
                                           const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                           std::vector<std::pair<ViewIdPair, TwoViewInfo*>>* edges, int device = -1);

// The reference's signature (filter_view_pairs_from_relative_translation.h:75-78): the call above on the graph's edges
// in ascending ViewIdPair order, the flagged edges removed from the graph (theiasfm_amd/host/view_graph_ops.cc).
void FilterViewPairsFromRelativeTranslation(const FilterViewPairsFromRelativeTranslationOptions& options,
                                            const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                            ViewGraph* view_graph, int device = -1);
}  // namespace theia
#endif
