// Host shim of theia::NonlinearPositionEstimator (reference nonlinear_position_estimator.cc:86-214) on the C ABI: the
// view pairs whose two views have an orientation are flattened into one tmi_ba_view_pair_batch on a dense view table --
// the views numbered in ascending ViewId order, the smallest id fixed, the pairs in ascending ViewIdPair order -- and
// estimated in one device call.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "theia/sfm/global_pose_estimation/nonlinear_position_estimator.h"
#include "theia_mi355_ba.h"

namespace theia {

bool NonlinearPositionEstimator::EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                   const std::unordered_map<ViewId, Eigen::Vector3d>& orientation,
                                                   std::unordered_map<ViewId, Eigen::Vector3d>* positions) {
  const char* const tag = "[theia::NonlinearPositionEstimator]";
  if (positions == nullptr) {
    std::fprintf(stderr, "%s null positions\n", tag);
    return false;
  }
  if (view_pairs.empty() || orientation.empty()) {  // :107-111
    std::fprintf(stderr, "%s number of view pairs = %zu, number of orientations = %zu\n", tag, view_pairs.size(),
                 orientation.size());
    return false;
  }
  if (options_.num_threads <= 0 || options_.min_num_points_per_view < 0 || !(options_.point_to_camera_weight > 0.0) ||
      !(options_.robust_loss_width > 0.0)) {  // :90-93
    std::fprintf(stderr, "%s num_threads, point_to_camera_weight and robust_loss_width must be positive and "
                         "min_num_points_per_view must not be negative\n", tag);
    return false;
  }
  if (options_.min_num_points_per_view > 0) {
    std::fprintf(stderr, "%s min_num_points_per_view > 0: the point-to-camera constraints are not provided\n", tag);
    return false;
  }
  // (the map's order is unspecified: ascending (view1, view2) makes the call reproducible)
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted;
  std::vector<ViewId> ids;
  for (const auto& view_pair : view_pairs) {
    const ViewIdPair& pair = view_pair.first;
    if (orientation.count(pair.first) == 0 || orientation.count(pair.second) == 0) continue;  // :188-194
    sorted.emplace_back(pair, view_pair.second.position_2);
    ids.push_back(pair.first);
    ids.push_back(pair.second);
  }
  if (sorted.empty()) {
    std::fprintf(stderr, "%s no view pair between oriented views\n", tag);
    return false;
  }
  std::sort(sorted.begin(), sorted.end(),
            [](const std::pair<ViewIdPair, Eigen::Vector3d>& a, const std::pair<ViewIdPair, Eigen::Vector3d>& b) {
              return a.first < b.first;
            });
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  std::vector<double> rotation, position2, position(3 * ids.size(), 0.0);
  rotation.reserve(3 * ids.size());
  for (size_t i = 0; i < ids.size(); ++i) {
    const Eigen::Vector3d& r = orientation.find(ids[i])->second;
    for (int a = 0; a < 3; ++a) rotation.push_back(r[a]);
    if (options_.initial_positions != nullptr) {
      const auto it = options_.initial_positions->find(ids[i]);
      if (it == options_.initial_positions->end()) {
        std::fprintf(stderr, "%s initial_positions lacks view %u\n", tag, static_cast<unsigned>(ids[i]));
        return false;
      }
      for (int a = 0; a < 3; ++a) position[3 * i + a] = it->second[a];
    }
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
  tmi_ba_nonlinear_position_options o;
  tmi_ba_nonlinear_position_options_init(&o);
  o.max_num_iterations = options_.max_num_iterations;
  o.robust_loss_width = options_.robust_loss_width;
  o.seed = options_.seed;
  o.positions_given = options_.initial_positions != nullptr ? 1 : 0;
  tmi_ba_nonlinear_position_summary summary;
  const int rc = tmi_ba_estimate_global_positions_nonlinear(&B, &o, /*fixed_view=*/0, options_.device, position.data(),
                                                            nullptr, nullptr, nullptr, nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "%s device call failed: %s\n", tag, tmi_ba_last_error());
    return false;
  }
  if (!summary.usable) {  // :161
    std::fprintf(stderr, "%s the solve ended in FAILURE after %d iterations: the solution is not usable\n", tag,
                 summary.num_iterations);
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
