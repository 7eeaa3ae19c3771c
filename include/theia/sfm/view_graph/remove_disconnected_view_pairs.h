// reference: src/theia/sfm/view_graph/remove_disconnected_view_pairs.h:47-51 (declaration) and .cc:48-95 (semantics):
// every view outside the largest connected component is removed from the graph with its edges; the removed views are
// returned.  Implemented on the C ABI (tmi_ba_largest_connected_component): a union-find over the edges on the device.
#ifndef THEIA_MI355_REMOVE_DISCONNECTED_VIEW_PAIRS_H_
#define THEIA_MI355_REMOVE_DISCONNECTED_VIEW_PAIRS_H_
#include <unordered_set>

#include "theia/sfm/types.h"
#include "theia/sfm/view_graph/view_graph.h"

namespace theia {
// The views with an edge are numbered in ascending ViewId order and the edges go to the device in ascending ViewIdPair
// order.  Among components of equal size the one with the smallest ViewId is kept (the reference: the first its hash
// map yields).  A view without an edge is in no component and stays in the graph, as in the reference.  A null graph,
// a graph without edges or a failed device call (no device: the message goes to stderr) changes nothing and returns
// the empty set.
std::unordered_set<ViewId> RemoveDisconnectedViewPairs(ViewGraph* view_graph, int device = -1);
}  // namespace theia
#endif
