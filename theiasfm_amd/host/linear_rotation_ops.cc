// Host shim of theia::LinearRotationEstimator (reference linear_rotation_estimator.cc:78-203) on the C ABI: the
// constraints are flattened into one tmi_ba_view_pair_batch on a dense view table -- the views they name numbered in
// ascending ViewId order, the constraints in ascending ViewIdPair order -- and estimated in one device call.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "theia/sfm/global_pose_estimation/linear_rotation_estimator.h"
#include "theia_mi355_ba.h"

namespace theia {

bool LinearRotationEstimator::EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  for (const auto& view_pair : view_pairs) AddRelativeRotationConstraint(view_pair.first, view_pair.second.rotation_2);
  return EstimateRotations(global_orientations);
}

void LinearRotationEstimator::AddRelativeRotationConstraint(const ViewIdPair& view_id_pair,
                                                            const Eigen::Vector3d& relative_rotation) {
  constraints_.emplace_back(view_id_pair, relative_rotation);
}

bool LinearRotationEstimator::EstimateRotations(std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  const char* const tag = "[theia::LinearRotationEstimator]";
  if (global_orientations == nullptr || constraints_.empty()) {  // (:160-161 CHECK both)
    std::fprintf(stderr, "%s skipping: no relative rotation constraints, or no map to write to\n", tag);
    return false;
  }
  // (ascending (view1, view2) makes the call reproducible; stable, so that a pair added twice stays adjacent)
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted = constraints_;
  std::stable_sort(sorted.begin(), sorted.end(),
                   [](const std::pair<ViewIdPair, Eigen::Vector3d>& a, const std::pair<ViewIdPair, Eigen::Vector3d>& b) {
                     return a.first < b.first;
                   });
  std::vector<ViewId> ids;
  for (const auto& edge : sorted) {
    ids.push_back(edge.first.first);
    ids.push_back(edge.first.second);
  }
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  std::vector<int32_t> view1, view2;
  std::vector<double> relative, rotation(3 * ids.size(), 0.0);
  for (const auto& edge : sorted) {
    view1.push_back(static_cast<int32_t>(std::lower_bound(ids.begin(), ids.end(), edge.first.first) - ids.begin()));
    view2.push_back(static_cast<int32_t>(std::lower_bound(ids.begin(), ids.end(), edge.first.second) - ids.begin()));
    for (int a = 0; a < 3; ++a) relative.push_back(edge.second[a]);
  }
  tmi_ba_view_pair_batch B;
  B.num_views = static_cast<int32_t>(ids.size());
  B.view_rotation = nullptr;
  B.num_pairs = static_cast<int32_t>(view1.size());
  B.pair_view1 = view1.data();
  B.pair_view2 = view2.data();
  B.pair_rotation2 = relative.data();
  B.pair_position2 = nullptr;
  tmi_ba_linear_rotation_options o;
  tmi_ba_linear_rotation_options_init(&o);
  tmi_ba_linear_rotation_summary summary;
  // (a pair added twice, in either direction, is the C call's repeated unordered pair)
  const int rc = tmi_ba_estimate_global_rotations_linear(&B, &o, device, rotation.data(), &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "%s device call failed: %s\n", tag, tmi_ba_last_error());
    return false;
  }
  if (!summary.usable) {
    std::fprintf(stderr, "%s the shifted constraint matrix could not be factored\n", tag);
    return false;
  }
  if (!summary.converged)
    std::fprintf(stderr, "%s warning: not converged after %d iterations (residuals %g %g %g)\n", tag,
                 summary.num_iterations, summary.residual[0], summary.residual[1], summary.residual[2]);
  global_orientations->reserve(global_orientations->size() + ids.size());
  for (size_t i = 0; i < ids.size(); ++i)
    global_orientations->emplace(ids[i], Eigen::Vector3d(rotation[3 * i], rotation[3 * i + 1], rotation[3 * i + 2]));
  return true;
}
}  // namespace theia
