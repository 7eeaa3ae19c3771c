// What the view-graph host shims share (rotation_ops.cc, nonlinear_rotation_ops.cc, linear_rotation_ops.cc,
// position_ops.cc, nonlinear_position_ops.cc, view_graph_ops.cc, view_pair_filter_ops.cc): the dense view table in
// ascending ViewId order, the edge order, the flat pair arrays behind tmi_ba_view_pair_batch and
// tmi_ba_relative_rotation_batch, the gather / scatter between ViewId -> Vector3d maps and [3 n] doubles, and the report
// of a failed device call.  Host only.  Which views get a row, which edges are sent and what is written back is each
// shim's own rule and stays in its file.
#ifndef THEIA_MI355_FLAT_VIEW_GRAPH_H_
#define THEIA_MI355_FLAT_VIEW_GRAPH_H_
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <utility>
#include <vector>

#include "theia/sfm/types.h"
#include "theia/util/eigen_lite.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace flat_view_graph {
using Vector3dMap = std::unordered_map<ViewId, Eigen::Vector3d>;

inline void Append(const Eigen::Vector3d& v, std::vector<double>* values) {
  values->insert(values->end(), v.data(), v.data() + 3);
}

// Ascending ViewIdPair order; equal pairs keep the order they were added in.  (A hash map's order is unspecified: this
// order makes a call reproducible.)
template <typename Payload>
void SortByPair(std::vector<std::pair<ViewIdPair, Payload>>* edges) {
  std::stable_sort(edges->begin(), edges->end(),
                   [](const std::pair<ViewIdPair, Payload>& a, const std::pair<ViewIdPair, Payload>& b) {
                     return a.first < b.first;
                   });
}

// The dense view table: Add / AddKeys / AddEnds in any mix, then Finish; row r is the r-th smallest id.
class ViewTable {
 public:
  void Add(const ViewIdPair& pair) {
    ids_.push_back(pair.first);
    ids_.push_back(pair.second);
  }
  void AddKeys(const Vector3dMap& map) {
    for (const auto& entry : map) ids_.push_back(entry.first);
  }
  template <typename Payload>
  void AddEnds(const std::vector<std::pair<ViewIdPair, Payload>>& edges) {
    for (const auto& edge : edges) Add(edge.first);
  }
  void Finish() {
    std::sort(ids_.begin(), ids_.end());
    ids_.erase(std::unique(ids_.begin(), ids_.end()), ids_.end());
  }

  size_t size() const { return ids_.size(); }
  ViewId id(const size_t row) const { return ids_[row]; }
  int32_t index(const ViewId id) const {  // the row, or -1
    const auto it = std::lower_bound(ids_.begin(), ids_.end(), id);
    return it == ids_.end() || *it != id ? -1 : static_cast<int32_t>(it - ids_.begin());
  }

  // [3 size()] in table order; a row whose id the map lacks is 0, and 0 in *given where that is asked for.
  std::vector<double> Gather(const Vector3dMap& map, std::vector<uint8_t>* given = nullptr) const {
    std::vector<double> values(3 * ids_.size(), 0.0);
    if (given != nullptr) given->assign(ids_.size(), 0);
    for (size_t row = 0; row < ids_.size(); ++row) {
      const auto it = map.find(ids_[row]);
      if (it == map.end()) continue;
      if (given != nullptr) (*given)[row] = 1;
      std::copy(it->second.data(), it->second.data() + 3, values.begin() + 3 * row);
    }
    return values;
  }

  // (*map)[id(row)] = row of `values`, for the rows where keep(row) holds.
  template <typename Keep>
  void Scatter(const std::vector<double>& values, Vector3dMap* map, const Keep& keep) const {
    for (size_t row = 0; row < ids_.size(); ++row)
      if (keep(row)) (*map)[ids_[row]] = Eigen::Vector3d(values[3 * row], values[3 * row + 1], values[3 * row + 2]);
  }
  void Scatter(const std::vector<double>& values, Vector3dMap* map) const {
    Scatter(values, map, [](size_t) { return true; });
  }
  void Scatter(const std::vector<double>& values, const std::vector<uint8_t>& given, Vector3dMap* map) const {
    Scatter(values, map, [&given](const size_t row) { return given[row] != 0; });
  }

 private:
  std::vector<ViewId> ids_;
};

enum class PairValue { kRotation2, kPosition2 };

// The table and the flat per-pair arrays on its rows.  rotation2, position2 and matches are optional: an array that was
// never appended to goes into the batch as NULL.
struct FlatViewGraph {
  ViewTable views;
  std::vector<int32_t> view1, view2, matches;
  std::vector<double> rotation2, position2;

  FlatViewGraph() {}
  // The table of the edges' ends and of the keys of *more_views, and the edges in their order with `value` as their
  // rotation2 or position2.
  FlatViewGraph(const std::vector<std::pair<ViewIdPair, Eigen::Vector3d>>& edges, const PairValue value,
                const Vector3dMap* more_views = nullptr) {
    views.AddEnds(edges);
    if (more_views != nullptr) views.AddKeys(*more_views);
    views.Finish();
    for (const auto& edge : edges)
      AddPair(edge.first, value == PairValue::kRotation2 ? &edge.second : nullptr,
              value == PairValue::kPosition2 ? &edge.second : nullptr);
  }

  // Both views must have a row.
  void AddPair(const ViewIdPair& pair, const Eigen::Vector3d* rotation, const Eigen::Vector3d* position) {
    view1.push_back(views.index(pair.first));
    view2.push_back(views.index(pair.second));
    if (rotation != nullptr) Append(*rotation, &rotation2);
    if (position != nullptr) Append(*position, &position2);
  }

  tmi_ba_view_pair_batch Batch(const double* view_rotation) const {
    tmi_ba_view_pair_batch B;
    B.num_views = static_cast<int32_t>(views.size());
    B.view_rotation = view_rotation;
    B.num_pairs = static_cast<int32_t>(view1.size());
    B.pair_view1 = view1.data();
    B.pair_view2 = view2.data();
    B.pair_rotation2 = rotation2.empty() ? nullptr : rotation2.data();
    B.pair_position2 = position2.empty() ? nullptr : position2.data();
    return B;
  }

  tmi_ba_relative_rotation_batch RotationBatch() const {
    tmi_ba_relative_rotation_batch B;
    B.num_views = static_cast<int32_t>(views.size());
    B.num_pairs = static_cast<int32_t>(view1.size());
    B.pair_view1 = view1.data();
    B.pair_view2 = view2.data();
    B.pair_rotation = rotation2.data();
    return B;
  }
};

// True, with the one report on stderr, unless rc is TMI_BA_OK.
inline bool DeviceCallFailed(const char* tag, const int32_t rc) {
  if (rc == TMI_BA_OK) return false;
  std::fprintf(stderr, "%s device call failed: %s\n", tag, tmi_ba_last_error());
  return true;
}
}  // namespace flat_view_graph
}  // namespace theia
#endif
