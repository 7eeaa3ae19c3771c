// Host shim of theia::LinearPositionEstimator (reference linear_position_estimator.cc:163-470) on the C ABI: the view
// pairs whose two views have an orientation and are in the reconstruction are flattened into one tmi_ba_view_pair_batch
// on a dense view table -- the views numbered in ascending ViewId order, the pairs in ascending ViewIdPair order -- the
// cameras and features of those views into one tmi_ba_problem whose camera index is the table's row (a group per view,
// a view's features in ascending TrackId, the tracks numbered in the order they are met), and estimated in one device
// call.
#include <algorithm>
#include <cstdio>
#include <unordered_map>
#include <vector>

#include "flat_view_graph.h"
#include "theia/sfm/global_pose_estimation/linear_position_estimator.h"
#include "theia_mi355_ba.h"

namespace theia {
bool LinearPositionEstimator::EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                const std::unordered_map<ViewId, Eigen::Vector3d>& orientation,
                                                std::unordered_map<ViewId, Eigen::Vector3d>* positions) {
  const char* const tag = "[theia::LinearPositionEstimator]";
  if (positions == nullptr) {
    std::fprintf(stderr, "%s null positions\n", tag);
    return false;
  }
  if (view_pairs.empty() || orientation.empty()) {
    std::fprintf(stderr, "%s number of view pairs = %zu, number of orientations = %zu\n", tag, view_pairs.size(),
                 orientation.size());
    return false;
  }
  if (options_.num_threads <= 0 || options_.max_power_iterations <= 0 || !(options_.eigensolver_threshold > 0.0)) {  // :160
    std::fprintf(stderr, "%s num_threads, max_power_iterations and eigensolver_threshold must be positive\n", tag);
    return false;
  }
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted;  // position_2; rotation_2 follows below in the same order
  for (const auto& view_pair : view_pairs) {
    const ViewIdPair& pair = view_pair.first;
    if (!(pair.first < pair.second)) {  // the reference's look-ups for a sorted triplet rely on ordered keys
      std::fprintf(stderr, "%s view pair (%u, %u): the first id is not below the second\n", tag,
                   static_cast<unsigned>(pair.first), static_cast<unsigned>(pair.second));
      return false;
    }
    if (orientation.count(pair.first) == 0 || orientation.count(pair.second) == 0) continue;
    if (reconstruction_.View(pair.first) == nullptr || reconstruction_.View(pair.second) == nullptr) continue;
    sorted.emplace_back(pair, view_pair.second.position_2);
  }
  if (sorted.empty()) {
    std::fprintf(stderr, "%s no view pair between oriented views of the reconstruction\n", tag);
    return false;
  }
  // (the map's order is unspecified: ascending (view1, view2) makes the call reproducible)
  flat_view_graph::SortByPair(&sorted);
  flat_view_graph::FlatViewGraph flat(sorted, flat_view_graph::PairValue::kPosition2);
  for (const auto& edge : sorted) flat_view_graph::Append(view_pairs.at(edge.first).rotation_2, &flat.rotation2);
  const std::vector<double> rotation = flat.views.Gather(orientation);
  const tmi_ba_view_pair_batch B = flat.Batch(rotation.data());

  // the cameras and the features of the table's views
  const int num_views = static_cast<int>(flat.views.size());
  std::vector<double> extrinsics(6 * static_cast<size_t>(num_views), 0.0), intrinsics, obs_xy;
  std::vector<int32_t> camera_group(num_views), group_model, group_offset(1, 0), obs_camera, obs_point;
  std::unordered_map<TrackId, int32_t> point_of_track;
  for (int row = 0; row < num_views; ++row) {
    const View* view = reconstruction_.View(flat.views.id(row));
    const CameraIntrinsicsModel& model = *view->Camera().CameraIntrinsics();
    camera_group[row] = row;
    group_model.push_back(static_cast<int32_t>(model.Type()));
    intrinsics.insert(intrinsics.end(), model.parameters(), model.parameters() + model.NumParameters());
    group_offset.push_back(static_cast<int32_t>(intrinsics.size()));
    std::vector<TrackId> tracks;
    for (const auto& feature : view->Features()) tracks.push_back(feature.first);  // (estimated or not: not consulted)
    std::sort(tracks.begin(), tracks.end());
    for (const TrackId t : tracks) {
      const auto it = point_of_track.emplace(t, static_cast<int32_t>(point_of_track.size())).first;
      const Feature& f = *view->GetFeature(t);
      obs_camera.push_back(row);
      obs_point.push_back(it->second);
      obs_xy.push_back(f[0]);
      obs_xy.push_back(f[1]);
    }
  }
  std::vector<double> points(4 * std::max<size_t>(point_of_track.size(), 1), 0.0);
  std::vector<uint8_t> intrinsics_constant(intrinsics.size(), 1);
  tmi_ba_problem P = {};
  P.num_cameras = num_views;
  P.extrinsics = extrinsics.data();
  P.camera_group = camera_group.data();
  P.num_groups = num_views;
  P.group_model = group_model.data();
  P.group_offset = group_offset.data();
  P.intrinsics = intrinsics.data();
  P.intrinsics_constant = intrinsics_constant.data();
  P.num_points = static_cast<int32_t>(point_of_track.size());
  P.points = points.data();
  P.num_observations = static_cast<int64_t>(obs_camera.size());
  P.obs_camera = obs_camera.data();
  P.obs_point = obs_point.data();
  P.obs_xy = obs_xy.data();

  tmi_ba_linear_position_options o;
  tmi_ba_linear_position_options_init(&o);
  o.max_iterations = options_.max_power_iterations;
  tmi_ba_linear_position_summary summary;
  std::vector<double> position(3 * static_cast<size_t>(num_views), 0.0);
  std::vector<uint8_t> estimated(num_views, 0);
  const int rc = tmi_ba_estimate_global_positions_linear(&P, &B, &o, options_.device, position.data(), estimated.data(),
                                                         0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &summary);
  if (flat_view_graph::DeviceCallFailed(tag, rc)) return false;
  if (!summary.usable) {
    std::fprintf(stderr, "%s %d triplets, %d with a baseline: no triplet to solve from, or the shifted matrix has a pivot "
                         "that is not positive; the solution is not usable\n", tag, summary.num_triplets,
                 summary.num_triplets_with_baseline);
    return false;
  }
  positions->clear();
  flat.views.Scatter(position, estimated, positions);
  return true;
}
}  // namespace theia
