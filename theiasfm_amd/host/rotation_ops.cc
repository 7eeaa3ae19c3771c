// Host shim of theia::RobustRotationEstimator (reference robust_rotation_estimator.cc:51-98) on the C ABI: the
// constraints are flattened into one tmi_ba_relative_rotation_batch on a dense view table -- the views of
// global_orientations numbered in ascending ViewId order, the smallest id fixed -- and estimated in one device call.
#include <cstdio>
#include <vector>

#include "flat_view_graph.h"
#include "theia/sfm/global_pose_estimation/robust_rotation_estimator.h"
#include "theia_mi355_ba.h"

namespace theia {
using flat_view_graph::FlatViewGraph;

bool RobustRotationEstimator::EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  // (the map's order is unspecified: ascending (view1, view2) makes the call reproducible)
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted;
  sorted.reserve(view_pairs.size());
  for (const auto& view_pair : view_pairs) sorted.emplace_back(view_pair.first, view_pair.second.rotation_2);
  flat_view_graph::SortByPair(&sorted);
  for (const auto& constraint : sorted) AddRelativeRotationConstraint(constraint.first, constraint.second);
  return EstimateRotations(global_orientations);
}

void RobustRotationEstimator::AddRelativeRotationConstraint(const ViewIdPair& view_id_pair,
                                                            const Eigen::Vector3d& relative_rotation) {
  relative_rotations_.emplace_back(view_id_pair, relative_rotation);
}

bool RobustRotationEstimator::EstimateRotations(std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  const char* const tag = "[theia::RobustRotationEstimator]";
  if (global_orientations == nullptr || global_orientations->empty() || relative_rotations_.empty()) {
    std::fprintf(stderr, "%s no orientations or no relative rotation constraints\n", tag);
    return false;
  }
  // the views of the map get a row; the constraints go in the order they were added
  FlatViewGraph flat;
  flat.views.AddKeys(*global_orientations);
  flat.views.Finish();
  for (const auto& constraint : relative_rotations_) {
    for (const ViewId id : {constraint.first.first, constraint.first.second}) {
      if (flat.views.index(id) >= 0) continue;
      std::fprintf(stderr, "%s view %u of a constraint has no initial orientation\n", tag, static_cast<unsigned>(id));
      return false;
    }
    flat.AddPair(constraint.first, &constraint.second, nullptr);
  }
  std::vector<double> rotation = flat.views.Gather(*global_orientations);
  const tmi_ba_relative_rotation_batch B = flat.RotationBatch();
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
  if (flat_view_graph::DeviceCallFailed(tag, rc)) return false;
  flat.views.Scatter(rotation, global_orientations);
  return true;
}
}  // namespace theia
