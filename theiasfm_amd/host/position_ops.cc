// Host shim of theia::LeastUnsquaredDeviationPositionEstimator (reference
// least_unsquared_deviation_position_estimator.cc:67-152) on the C ABI: the view pairs whose two views have an
// orientation are flattened into one tmi_ba_view_pair_batch on a dense view table -- the views numbered in ascending
// ViewId order, the smallest id fixed, the pairs in ascending ViewIdPair order -- and estimated in one device call.
#include <cstdio>
#include <vector>

#include "flat_view_graph.h"
#include "theia/sfm/global_pose_estimation/least_unsquared_deviation_position_estimator.h"
#include "theia_mi355_ba.h"

namespace theia {
bool LeastUnsquaredDeviationPositionEstimator::EstimatePositions(
    const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
    const std::unordered_map<ViewId, Eigen::Vector3d>& orientation,
    std::unordered_map<ViewId, Eigen::Vector3d>* positions) {
  const char* const tag = "[theia::LeastUnsquaredDeviationPositionEstimator]";
  if (positions == nullptr) {
    std::fprintf(stderr, "%s null positions\n", tag);
    return false;
  }
  if (options_.max_num_iterations <= 0 || options_.max_num_reweighted_iterations <= 0) {  // :71-72
    std::fprintf(stderr, "%s max_num_iterations and max_num_reweighted_iterations must be positive\n", tag);
    return false;
  }
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted;
  for (const auto& view_pair : view_pairs) {
    const ViewIdPair& pair = view_pair.first;
    if (orientation.count(pair.first) == 0 || orientation.count(pair.second) == 0) continue;  // :127-133
    sorted.emplace_back(pair, view_pair.second.position_2);
  }
  if (sorted.empty()) {
    std::fprintf(stderr, "%s no view pair between oriented views\n", tag);
    return false;
  }
  // (the map's order is unspecified: ascending (view1, view2) makes the call reproducible)
  flat_view_graph::SortByPair(&sorted);
  // the views of the kept pairs get a row
  const flat_view_graph::FlatViewGraph flat(sorted, flat_view_graph::PairValue::kPosition2);
  const std::vector<double> rotation = flat.views.Gather(orientation);
  const tmi_ba_view_pair_batch B = flat.Batch(rotation.data());
  tmi_ba_lud_position_options o;
  tmi_ba_lud_position_options_init(&o);  // (the reference's solver runs on these, not on options_)
  tmi_ba_lud_position_summary summary;
  std::vector<double> position(3 * flat.views.size());
  const int rc = tmi_ba_estimate_global_positions_lud(&B, &o, /*fixed_view=*/0, options_.device, position.data(),
                                                      nullptr, nullptr, nullptr, nullptr, &summary);
  if (flat_view_graph::DeviceCallFailed(tag, rc)) return false;
  positions->clear();
  flat.views.Scatter(position, positions);
  return true;
}
}  // namespace theia
