// reference: src/theia/sfm/view_graph/view_graph.h:59-138 and view_graph.cc:85-265 -- the undirected graph of the
// views of a reconstruction: ViewIds at the vertices, a TwoViewInfo per edge, each edge stored once under the
// ViewIdPair with the smaller id first.  The reference's members and semantics except disk I/O and serialization.
// GetLargestConnectedComponentIds runs on the host (a breadth-first search); among components of equal size it takes
// the one with the smallest ViewId, where the reference takes the first its hash map yields -- the rule of
// tmi_ba_largest_connected_component, which RemoveDisconnectedViewPairs and OrientationsFromMaximumSpanningTree use.
#ifndef THEIA_MI355_VIEW_GRAPH_H_
#define THEIA_MI355_VIEW_GRAPH_H_
#include <algorithm>
#include <cstddef>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "theia/sfm/twoview_info.h"
#include "theia/sfm/types.h"
#include "theia/util/hash.h"

namespace theia {
class ViewGraph {
 public:
  ViewGraph() {}

  int NumViews() const { return static_cast<int>(vertices_.size()); }
  int NumEdges() const { return static_cast<int>(edges_.size()); }
  bool HasView(const ViewId view_id) const { return vertices_.count(view_id) != 0; }
  bool HasEdge(const ViewId view_id_1, const ViewId view_id_2) const {
    return edges_.count(Ordered(view_id_1, view_id_2)) != 0;
  }

  std::unordered_set<ViewId> ViewIds() const {
    std::unordered_set<ViewId> view_ids;
    view_ids.reserve(vertices_.size());
    for (const auto& vertex : vertices_) view_ids.insert(vertex.first);
    return view_ids;
  }

  // Removes the view and every edge at it; false if the view is not in the graph.  (As in the reference a neighbour
  // that loses its last edge stays a view of the graph.)
  bool RemoveView(const ViewId view_id) {
    const auto it = vertices_.find(view_id);
    if (it == vertices_.end()) return false;
    for (const ViewId neighbor_id : it->second) {
      vertices_[neighbor_id].erase(view_id);
      edges_.erase(Ordered(view_id, neighbor_id));
    }
    vertices_.erase(view_id);
    return true;
  }

  // New vertices are added as needed; an existing edge gets the new value.  An edge from a view to itself is ignored.
  void AddEdge(const ViewId view_id_1, const ViewId view_id_2, const TwoViewInfo& two_view_info) {
    if (view_id_1 == view_id_2) return;
    vertices_[view_id_1].insert(view_id_2);
    vertices_[view_id_2].insert(view_id_1);
    edges_[Ordered(view_id_1, view_id_2)] = two_view_info;
  }

  bool RemoveEdge(const ViewId view_id_1, const ViewId view_id_2) {
    const ViewIdPair view_id_pair = Ordered(view_id_1, view_id_2);
    if (edges_.count(view_id_pair) == 0) return false;
    return vertices_[view_id_1].erase(view_id_2) != 0 && vertices_[view_id_2].erase(view_id_1) != 0 &&
           edges_.erase(view_id_pair) != 0;
  }

  const std::unordered_set<ViewId>* GetNeighborIdsForView(const ViewId view_id) const {
    const auto it = vertices_.find(view_id);
    return it == vertices_.end() ? nullptr : &it->second;
  }

  const TwoViewInfo* GetEdge(const ViewId view_id_1, const ViewId view_id_2) const {
    const auto it = edges_.find(Ordered(view_id_1, view_id_2));
    return it == edges_.end() ? nullptr : &it->second;
  }

  TwoViewInfo* GetMutableEdge(const ViewId view_id_1, const ViewId view_id_2) {
    const auto it = edges_.find(Ordered(view_id_1, view_id_2));
    return it == edges_.end() ? nullptr : &it->second;
  }

  // Every edge exactly once, under (view id 1, view id 2) with view id 1 < view id 2.
  const std::unordered_map<ViewIdPair, TwoViewInfo>& GetAllEdges() const { return edges_; }

  // The edges between the given views (a view without such an edge does not enter the subgraph, as in the reference).
  void ExtractSubgraph(const std::unordered_set<ViewId>& views_in_subgraph, ViewGraph* subgraph) const {
    for (const auto& vertex : vertices_) {
      if (views_in_subgraph.count(vertex.first) == 0) continue;
      for (const ViewId second_vertex : vertex.second) {
        if (views_in_subgraph.count(second_vertex) == 0 || second_vertex < vertex.first) continue;
        subgraph->AddEdge(vertex.first, second_vertex, edges_.find(ViewIdPair(vertex.first, second_vertex))->second);
      }
    }
  }

  // The views of the largest connected component (over the views with at least one edge; empty without edges, where
  // the reference CHECK-fails).  Ties: the component with the smallest ViewId.
  void GetLargestConnectedComponentIds(std::unordered_set<ViewId>* largest_cc) const {
    largest_cc->clear();
    std::vector<ViewId> ids;
    for (const auto& vertex : vertices_)
      if (!vertex.second.empty()) ids.push_back(vertex.first);
    std::sort(ids.begin(), ids.end());
    std::unordered_set<ViewId> seen;
    std::vector<ViewId> best, component;
    for (const ViewId start : ids) {  // ascending: a tie keeps the component found first, the one with the smallest id
      if (!seen.insert(start).second) continue;
      component.assign(1, start);
      for (std::size_t head = 0; head < component.size(); ++head)
        for (const ViewId neighbor_id : vertices_.find(component[head])->second)
          if (seen.insert(neighbor_id).second) component.push_back(neighbor_id);
      if (component.size() > best.size()) best.swap(component);
    }
    largest_cc->insert(best.begin(), best.end());
  }

 private:
  static ViewIdPair Ordered(const ViewId a, const ViewId b) { return a < b ? ViewIdPair(a, b) : ViewIdPair(b, a); }

  std::unordered_map<ViewId, std::unordered_set<ViewId>> vertices_;
  std::unordered_map<ViewIdPair, TwoViewInfo> edges_;
};
}  // namespace theia
#endif
