// Host shim of theia::NonlinearRotationEstimator (reference nonlinear_rotation_estimator.cc:49-100) on the C ABI: the
// view pairs are flattened into one tmi_ba_view_pair_batch on a dense view table -- the views of the map and of the pairs
// numbered in ascending ViewId order, those the map lacks unmarked, the pairs in ascending ViewIdPair order -- and
// estimated in one device call with no view held.
#include <cstdio>
#include <vector>

#include "flat_view_graph.h"
#include "theia/sfm/global_pose_estimation/nonlinear_rotation_estimator.h"
#include "theia_mi355_ba.h"

namespace theia {
bool NonlinearRotationEstimator::EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                                   std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) {
  const char* const tag = "[theia::NonlinearRotationEstimator]";
  if (global_orientations == nullptr || global_orientations->empty()) {  // :53-57
    std::fprintf(stderr, "%s skipping: no initialisation was provided\n", tag);
    return false;
  }
  if (view_pairs.empty()) {  // :58-62
    std::fprintf(stderr, "%s skipping: no relative rotation constraints were provided\n", tag);
    return false;
  }
  // (the map's order is unspecified: ascending (view1, view2) makes the call reproducible)
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> sorted;
  sorted.reserve(view_pairs.size());
  for (const auto& view_pair : view_pairs) sorted.emplace_back(view_pair.first, view_pair.second.rotation_2);
  flat_view_graph::SortByPair(&sorted);
  // the views of the pairs and of the map get a row; those the map lacks are not given
  const flat_view_graph::FlatViewGraph flat(sorted, flat_view_graph::PairValue::kRotation2, global_orientations);
  std::vector<uint8_t> given;
  std::vector<double> rotation = flat.views.Gather(*global_orientations, &given);
  const tmi_ba_view_pair_batch B = flat.Batch(nullptr);
  tmi_ba_nonlinear_rotation_options o;
  tmi_ba_nonlinear_rotation_options_init(&o);
  o.robust_loss_width = robust_loss_width_;
  tmi_ba_nonlinear_rotation_summary summary;
  const int rc = tmi_ba_estimate_global_rotations_nonlinear(&B, &o, given.data(), device, rotation.data(), nullptr,
                                                            nullptr, nullptr, nullptr, &summary);
  if (flat_view_graph::DeviceCallFailed(tag, rc)) return false;
  flat.views.Scatter(rotation, given, global_orientations);
  return true;
}
}  // namespace theia
