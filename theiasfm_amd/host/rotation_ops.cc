// Host shim of theia::RobustRotationEstimator (reference robust_rotation_estimator.cc:51-98) on the C ABI: the
// constraints are flattened into one tmi_ba_relative_rotation_batch on a dense view table -- the views of
// global_orientations numbered in ascending ViewId order, the smallest id fixed -- and estimated in one device call.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "theia/sfm/global_pose_estimation/robust_rotation_estimator.h"
#include "theia_mi355_ba.h"

namespace theia {

bool RobustRotationEstimator::EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  // (the map's order is unspecified: ascending (view1, view2) makes the call reproducible)
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted;
  sorted.reserve(view_pairs.size());
  for (const auto& view_pair : view_pairs) sorted.emplace_back(view_pair.first, view_pair.second.rotation_2);
  std::sort(sorted.begin(), sorted.end(),
            [](const std::pair<ViewIdPair, Eigen::Vector3d>& a, const std::pair<ViewIdPair, Eigen::Vector3d>& b) {
              return a.first < b.first;
            });
  for (const auto& constraint : sorted) AddRelativeRotationConstraint(constraint.first, constraint.second);
  return EstimateRotations(global_orientations);
}

void RobustRotationEstimator::AddRelativeRotationConstraint(const ViewIdPair& view_id_pair,
                                                            const Eigen::Vector3d& relative_rotation) {
  relative_rotations_.emplace_back(view_id_pair, relative_rotation);
}

bool RobustRotationEstimator::EstimateRotations(std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  if (global_orientations == nullptr || global_orientations->empty() || relative_rotations_.empty()) {
    std::fprintf(stderr, "[theia::RobustRotationEstimator] no orientations or no relative rotation constraints\n");
    return false;
  }
  std::vector<ViewId> ids;
  ids.reserve(global_orientations->size());
  for (const auto& orientation : *global_orientations) ids.push_back(orientation.first);
  std::sort(ids.begin(), ids.end());
  std::vector<double> rotation;
  rotation.reserve(3 * ids.size());
  for (const ViewId id : ids) {
    const Eigen::Vector3d& r = global_orientations->find(id)->second;
    for (int a = 0; a < 3; ++a) rotation.push_back(r[a]);
  }
  std::vector<int32_t> view1, view2;
  std::vector<double> relative;
  for (const auto& constraint : relative_rotations_) {
    const ViewId pair[2] = {constraint.first.first, constraint.first.second};
    int32_t index[2];
    for (int k = 0; k < 2; ++k) {
      const auto it = std::lower_bound(ids.begin(), ids.end(), pair[k]);
      if (it == ids.end() || *it != pair[k]) {
        std::fprintf(stderr, "[theia::RobustRotationEstimator] view %u of a constraint has no initial orientation\n",
                     static_cast<unsigned>(pair[k]));
        return false;
      }
      index[k] = static_cast<int32_t>(it - ids.begin());
    }
    view1.push_back(index[0]);
    view2.push_back(index[1]);
    for (int a = 0; a < 3; ++a) relative.push_back(constraint.second[a]);
  }
  tmi_ba_relative_rotation_batch B;
  B.num_views = static_cast<int32_t>(ids.size());
  B.num_pairs = static_cast<int32_t>(view1.size());
  B.pair_view1 = view1.data();
  B.pair_view2 = view2.data();
  B.pair_rotation = relative.data();
  tmi_ba_robust_rotation_options o;
  tmi_ba_robust_rotation_options_init(&o);
  o.max_num_l1_iterations = options_.max_num_l1_iterations;
  o.l1_step_convergence_threshold = options_.l1_step_convergence_threshold;
  o.max_num_irls_iterations = options_.max_num_irls_iterations;
  o.irls_step_convergence_threshold = options_.irls_step_convergence_threshold;
  o.irls_loss_parameter_sigma = options_.irls_loss_parameter_sigma;
  tmi_ba_robust_rotation_summary summary;
  const int rc = tmi_ba_estimate_global_rotations_robust(&B, &o, /*fixed_view=*/0, options_.device, rotation.data(),
                                                         nullptr, nullptr, nullptr, nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::RobustRotationEstimator] device call failed: %s\n", tmi_ba_last_error());
    return false;
  }
  for (size_t i = 0; i < ids.size(); ++i) {
    Eigen::Vector3d& r = (*global_orientations)[ids[i]];
    for (int a = 0; a < 3; ++a) r[a] = rotation[3 * i + a];
  }
  return true;
}
}  // namespace theia
