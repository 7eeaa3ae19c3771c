// Host shim of theia::NonlinearPositionEstimator (reference nonlinear_position_estimator.cc:86-214) on the C ABI: the
// view pairs whose two views have an orientation are flattened into one tmi_ba_view_pair_batch on a dense view table --
// the views numbered in ascending ViewId order, the smallest id fixed, the pairs in ascending ViewIdPair order -- and
// estimated in one device call.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "flat_view_graph.h"
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
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted;
  for (const auto& view_pair : view_pairs) {
    const ViewIdPair& pair = view_pair.first;
    if (orientation.count(pair.first) == 0 || orientation.count(pair.second) == 0) continue;  // :188-194
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
  std::vector<double> position(3 * flat.views.size(), 0.0);
  if (options_.initial_positions != nullptr) {
    std::vector<uint8_t> given;
    position = flat.views.Gather(*options_.initial_positions, &given);
    const size_t lacking = std::find(given.begin(), given.end(), 0) - given.begin();
    if (lacking < given.size()) {
      std::fprintf(stderr, "%s initial_positions lacks view %u\n", tag, static_cast<unsigned>(flat.views.id(lacking)));
      return false;
    }
  }
  const tmi_ba_view_pair_batch B = flat.Batch(rotation.data());
  tmi_ba_nonlinear_position_options o;
  tmi_ba_nonlinear_position_options_init(&o);
  o.max_num_iterations = options_.max_num_iterations;
  o.robust_loss_width = options_.robust_loss_width;
  o.seed = options_.seed;
  o.positions_given = options_.initial_positions != nullptr ? 1 : 0;
  tmi_ba_nonlinear_position_summary summary;
  const int rc = tmi_ba_estimate_global_positions_nonlinear(&B, &o, /*fixed_view=*/0, options_.device, position.data(),
                                                            nullptr, nullptr, nullptr, nullptr, nullptr, &summary);
  if (flat_view_graph::DeviceCallFailed(tag, rc)) return false;
  if (!summary.usable) {  // :161
    std::fprintf(stderr, "%s the solve ended in FAILURE after %d iterations: the solution is not usable\n", tag,
                 summary.num_iterations);
    return false;
  }
  positions->clear();
  flat.views.Scatter(position, positions);
  return true;
}
}  // namespace theia
