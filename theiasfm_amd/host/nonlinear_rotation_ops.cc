// Host shim of theia::NonlinearRotationEstimator (reference nonlinear_rotation_estimator.cc:49-100) on the C ABI: the
// view pairs are flattened into one tmi_ba_view_pair_batch on a dense view table -- the views of the map and of the pairs
// numbered in ascending ViewId order, those the map lacks unmarked, the pairs in ascending ViewIdPair order -- and
// estimated in one device call with no view held.
#include <algorithm>
#include <cstdio>
#include <vector>

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
  std::vector<ViewId> ids;
  sorted.reserve(view_pairs.size());
  for (const auto& view_pair : view_pairs) {
    sorted.emplace_back(view_pair.first, view_pair.second.rotation_2);
    ids.push_back(view_pair.first.first);
    ids.push_back(view_pair.first.second);
  }
  std::sort(sorted.begin(), sorted.end(),
            [](const std::pair<ViewIdPair, Eigen::Vector3d>& a, const std::pair<ViewIdPair, Eigen::Vector3d>& b) {
              return a.first < b.first;
            });
  for (const auto& orientation : *global_orientations) ids.push_back(orientation.first);
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  std::vector<double> rotation(3 * ids.size(), 0.0), relative;
  std::vector<uint8_t> given(ids.size(), 0);
  for (size_t i = 0; i < ids.size(); ++i) {
    const auto it = global_orientations->find(ids[i]);
    if (it == global_orientations->end()) continue;
    given[i] = 1;
    for (int a = 0; a < 3; ++a) rotation[3 * i + a] = it->second[a];
  }
  std::vector<int32_t> view1, view2;
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
  tmi_ba_nonlinear_rotation_options o;
  tmi_ba_nonlinear_rotation_options_init(&o);
  o.robust_loss_width = robust_loss_width_;
  tmi_ba_nonlinear_rotation_summary summary;
  const int rc = tmi_ba_estimate_global_rotations_nonlinear(&B, &o, given.data(), device, rotation.data(), nullptr,
                                                            nullptr, nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "%s device call failed: %s\n", tag, tmi_ba_last_error());
    return false;
  }
  for (size_t i = 0; i < ids.size(); ++i) {
    if (!given[i]) continue;
    Eigen::Vector3d& r = (*global_orientations)[ids[i]];
    for (int a = 0; a < 3; ++a) r[a] = rotation[3 * i + a];
  }
  return true;
}
}  // namespace theia
