// reference: src/theia/sfm/view_graph/orientations_from_maximum_spanning_tree.h:47-57 (declaration) and .cc:109-180
// (semantics): the maximum spanning tree of the largest connected component by num_verified_matches, the relative
// rotations chained along it from a root with the identity orientation.  Implemented on the C ABI
// (tmi_ba_orientations_from_maximum_spanning_tree): Boruvka rounds on the ranks of the reference's sort order, then one
// workgroup walks the tree level by level.
#ifndef THEIA_MI355_ORIENTATIONS_FROM_MAXIMUM_SPANNING_TREE_H_
#define THEIA_MI355_ORIENTATIONS_FROM_MAXIMUM_SPANNING_TREE_H_
#include <unordered_map>

#include "theia/sfm/types.h"
#include "theia/sfm/view_graph/view_graph.h"
#include "theia/util/eigen_lite.h"

namespace theia {
// The views with an edge are numbered in ascending ViewId order and the edges go to the device in ascending ViewIdPair
// order; the root is the smallest ViewId of the largest component (the reference: the first entry of a hash set).
// Writes an orientation for every view of the largest component and returns true.  A graph without edges (the
// reference returns false too) or a failed device call (no device: the message goes to stderr) returns false and
// leaves *orientations as it was.
bool OrientationsFromMaximumSpanningTree(const ViewGraph& view_graph,
                                         std::unordered_map<ViewId, Eigen::Vector3d>* orientations, int device = -1);
}  // namespace theia
#endif
