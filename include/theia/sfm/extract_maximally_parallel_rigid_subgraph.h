// reference: src/theia/sfm/extract_maximally_parallel_rigid_subgraph.h (declaration) and .cc:53-228 (semantics): the
// views outside the largest maximally parallel rigid component (Kennedy et al., IROS 2012) are removed from the graph
// with their edges.  Implemented on the C ABI (tmi_ba_extract_parallel_rigid_subgraph, whose header comment is the
// numbered specification).
#ifndef THEIA_MI355_EXTRACT_MAXIMALLY_PARALLEL_RIGID_SUBGRAPH_H_
#define THEIA_MI355_EXTRACT_MAXIMALLY_PARALLEL_RIGID_SUBGRAPH_H_
#include <unordered_map>

#include "theia/sfm/types.h"
#include "theia/sfm/view_graph/view_graph.h"
#include "theia/util/eigen_lite.h"

namespace theia {
// The views with an edge are numbered in ascending ViewId order and the edges go to the device in ascending ViewIdPair
// order, each with its position_2.  Every view that was sent and is not kept is removed with RemoveView; a view of the
// graph without an edge is not part of the system (DEVIATION, see the C header) and stays as it is.
// A view of the graph that has an edge and no orientation makes the reference abort (FindOrDie); here the graph is left
// untouched and the fact is reported on stderr.  So is a failed device call (no device, a null space beyond the cap).
// The bool form says which: true when the graph was handled (also: a null graph pointer is false, a graph without
// edges is true and unchanged).
bool ExtractMaximallyParallelRigidSubgraphOrReport(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                                   ViewGraph* view_graph, int device = -1);

// The reference's signature.
void ExtractMaximallyParallelRigidSubgraph(const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                           ViewGraph* view_graph);
}  // namespace theia
#endif
