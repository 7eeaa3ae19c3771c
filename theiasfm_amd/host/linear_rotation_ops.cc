// Host shim of theia::LinearRotationEstimator (reference linear_rotation_estimator.cc:78-203) on the C ABI: the
// constraints are flattened into one tmi_ba_view_pair_batch on a dense view table -- the views they name numbered in
// ascending ViewId order, the constraints in ascending ViewIdPair order -- and estimated in one device call.
#include <cstdio>
#include <vector>

#include "flat_view_graph.h"
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
  flat_view_graph::SortByPair(&sorted);
  // the views the constraints name get a row
  const flat_view_graph::FlatViewGraph flat(sorted, flat_view_graph::PairValue::kRotation2);
  const tmi_ba_view_pair_batch B = flat.Batch(nullptr);
  std::vector<double> rotation(3 * flat.views.size(), 0.0);
  tmi_ba_linear_rotation_options o;
  tmi_ba_linear_rotation_options_init(&o);
  tmi_ba_linear_rotation_summary summary;
  // (a pair added twice, in either direction, is the C call's repeated unordered pair)
  const int rc = tmi_ba_estimate_global_rotations_linear(&B, &o, device, rotation.data(), &summary);
  if (flat_view_graph::DeviceCallFailed(tag, rc)) return false;
  if (!summary.usable) {
    std::fprintf(stderr, "%s the shifted constraint matrix could not be factored\n", tag);
    return false;
  }
  if (!summary.converged)
    std::fprintf(stderr, "%s warning: not converged after %d iterations (residuals %g %g %g)\n", tag,
                 summary.num_iterations, summary.residual[0], summary.residual[1], summary.residual[2]);
  // emplaced: a key the map already holds keeps its value (:199)
  global_orientations->reserve(global_orientations->size() + flat.views.size());
  flat.views.Scatter(rotation, global_orientations,
                     [&](const size_t row) { return global_orientations->count(flat.views.id(row)) == 0; });
  return true;
}
}  // namespace theia
