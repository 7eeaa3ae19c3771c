// reference: src/theia/sfm/filter_view_pairs_from_orientation.h:59-62 (declaration) and .cc:55-122 (semantics):
// a view pair is kept only if the relative rotation of its match (TwoViewInfo::rotation_2) and the relative
// rotation of the two orientation estimates differ by at most the threshold, as an angle.
// Implemented on the C ABI (tmi_ba_filter_view_pairs_from_orientation): one thread per edge, one launch.
#ifndef THEIA_MI355_FILTER_VIEW_PAIRS_FROM_ORIENTATION_H_
#define THEIA_MI355_FILTER_VIEW_PAIRS_FROM_ORIENTATION_H_
#include <unordered_map>
#include <utility>
#include <vector>

#include "theia/sfm/twoview_info.h"
#include "theia/sfm/types.h"
#include "theia/sfm/view_graph/view_graph.h"
#include "theia/util/eigen_lite.h"

namespace theia {
// The reference's call with the edge list in place of the ViewGraph.  An edge with a view that has
// no entry in `orientations` is removed without being sent to the device (:94-103); so is an edge with a null info.
// The views of the other edges are numbered in ascending ViewId order.  Removed edges are erased from *edges (the
// order of the others is kept); returns the number removed.  A failed device call (no device: the message goes to
// stderr) or a negative threshold (the reference CHECK-fails) leaves *edges unchanged and returns 0.
int FilterViewPairsFromOrientation(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                   double max_relative_rotation_difference_degrees,
                                   std::vector<std::pair<ViewIdPair, TwoViewInfo*>>* edges, int device = -1);

// The reference's signature (filter_view_pairs_from_orientation.h:59-62): the call above on the graph's edges in
// ascending ViewIdPair order, the flagged edges removed from the graph (theiasfm_amd/host/view_graph_ops.cc).
void FilterViewPairsFromOrientation(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                    double max_relative_rotation_difference_degrees, ViewGraph* view_graph,
                                    int device = -1);
}  // namespace theia
#endif
