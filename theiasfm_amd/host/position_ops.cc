// Host shim of theia::LeastUnsquaredDeviationPositionEstimator (reference
// least_unsquared_deviation_position_estimator.cc:67-152) on the C ABI: the view pairs whose two views have an
// orientation are flattened into one tmi_ba_view_pair_batch on a dense view table -- the views numbered in ascending
// ViewId order, the smallest id fixed, the pairs in ascending ViewIdPair order -- and estimated in one device call.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "theia/sfm/global_pose_estimation/least_unsquared_deviation_position_estimator.h"
#include "theia_mi355_ba.h"

namespace theia {

bool LeastUnsquaredDeviationPositionEstimator::EstimatePositions(
    const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
    const std::unordered_map<ViewId, Eigen::Vector3d>& orientation,
    std::unordered_map<ViewId, Eigen::Vector3d>* positions) {
  if (positions == nullptr) {
    std::fprintf(stderr, "[theia::LeastUnsquaredDeviationPositionEstimator] null positions\n");
    return false;
  }
  if (options_.max_num_iterations <= 0 || options_.max_num_reweighted_iterations <= 0) {  // :71-72
    std::fprintf(stderr, "[theia::LeastUnsquaredDeviationPositionEstimator] max_num_iterations and "
                         "max_num_reweighted_iterations must be positive\n");
    return false;
  }
  // (the map's order is unspecified: ascending (view1, view2) makes the call reproducible)
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted;
  std::vector<ViewId> ids;
  for (const auto& view_pair : view_pairs) {
    const ViewIdPair& pair = view_pair.first;
    if (orientation.count(pair.first) == 0 || orientation.count(pair.second) == 0) continue;  // :127-133
    sorted.emplace_back(pair, view_pair.second.position_2);
    ids.push_back(pair.first);
    ids.push_back(pair.second);
  }
  if (sorted.empty()) {
    std::fprintf(stderr, "[theia::LeastUnsquaredDeviationPositionEstimator] no view pair between oriented views\n");
    return false;
  }
  std::sort(sorted.begin(), sorted.end(),
            [](const std::pair<ViewIdPair, Eigen::Vector3d>& a, const std::pair<ViewIdPair, Eigen::Vector3d>& b) {
              return a.first < b.first;
            });
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  std::vector<double> rotation, position2;
  rotation.reserve(3 * ids.size());
  for (const ViewId id : ids) {
    const Eigen::Vector3d& r = orientation.find(id)->second;
    for (int a = 0; a < 3; ++a) rotation.push_back(r[a]);
  }
  std::vector<int32_t> view1, view2;
  for (const auto& edge : sorted) {
    view1.push_back(static_cast<int32_t>(std::lower_bound(ids.begin(), ids.end(), edge.first.first) - ids.begin()));
    view2.push_back(static_cast<int32_t>(std::lower_bound(ids.begin(), ids.end(), edge.first.second) - ids.begin()));
    for (int a = 0; a < 3; ++a) position2.push_back(edge.second[a]);
  }
  tmi_ba_view_pair_batch B;
  B.num_views = static_cast<int32_t>(ids.size());
  B.view_rotation = rotation.data();
  B.num_pairs = static_cast<int32_t>(view1.size());
  B.pair_view1 = view1.data();
  B.pair_view2 = view2.data();
  B.pair_rotation2 = nullptr;
  B.pair_position2 = position2.data();
  tmi_ba_lud_position_options o;
  tmi_ba_lud_position_options_init(&o);  // (the reference's solver runs on these, not on options_)
  tmi_ba_lud_position_summary summary;
  std::vector<double> position(3 * ids.size());
  const int rc = tmi_ba_estimate_global_positions_lud(&B, &o, /*fixed_view=*/0, options_.device, position.data(),
                                                      nullptr, nullptr, nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::LeastUnsquaredDeviationPositionEstimator] device call failed: %s\n",
                 tmi_ba_last_error());
    return false;
  }
  positions->clear();
  for (size_t i = 0; i < ids.size(); ++i) {
    Eigen::Vector3d& p = (*positions)[ids[i]];
    for (int a = 0; a < 3; ++a) p[a] = position[3 * i + a];
  }
  return true;
}
}  // namespace theia
