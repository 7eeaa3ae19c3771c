// Host shim of the batched BundleAdjustView (bundle_adjustment.cc:83-93, called per newly localised view from
// localize_view_to_reconstruction.cc:248-252): the estimated views of the set are flattened in ascending ViewId
// order with the estimated tracks they observe held constant -- the residual set BundleAdjuster::AddView builds
// (bundle_adjuster.cc:102-135) for each of them -- and handed to tmi_ba_adjust_views, whose result equals one
// BundleAdjustView call per view in that order.
#include <algorithm>
#include <vector>

#include "theia/sfm/bundle_adjustment/bundle_adjuster.h"
#include "theia/sfm/bundle_adjustment/bundle_adjustment.h"
#include "theia/sfm/reconstruction.h"

namespace theia {

std::unordered_map<ViewId, BundleAdjustmentSummary> BundleAdjustViews(const BundleAdjustmentOptions& options,
                                                                      const std::unordered_set<ViewId>& view_ids,
                                                                      Reconstruction* reconstruction) {
  std::unordered_map<ViewId, BundleAdjustmentSummary> result;
  if (reconstruction == nullptr) return result;
  std::vector<ViewId> views;
  for (const ViewId v : view_ids) {
    const View* view = reconstruction->View(v);
    if (view != nullptr && view->IsEstimated()) views.push_back(v);
  }
  std::sort(views.begin(), views.end());
  if (views.empty()) return result;
  BundleAdjustmentOptions ba_options = options;
  ba_options.linear_solver_type = ceres::DENSE_QR;  // bundle_adjustment.cc:86-87
  ba_options.use_inner_iterations = false;
  FlattenedBundleAdjustmentProblem flat;
  {
    BundleAdjuster adjuster(ba_options, reconstruction);
    adjuster.AddViews(views);
    if (!adjuster.Flatten(&flat)) return result;
  }
  const size_t n = flat.view_ids.size();
  std::vector<int8_t> termination(n, -1);
  std::vector<double> initial_cost(n, 0.0), final_cost(n, 0.0);
  tmi_ba_view_batch_summary vs = {};
  int rc = TMI_BA_OK;
  if (n > 0 && !flat.obs_camera.empty()) {
    tmi_ba_options o;
    ToDeviceOptions(ba_options, &o);
    tmi_ba_problem p = flat.AsC();
    rc = tmi_ba_adjust_views(&p, &o, nullptr, termination.data(), nullptr, initial_cost.data(), final_cost.data(), &vs);
  }
  const double share = vs.num_views > 0 ? 1.0 / static_cast<double>(vs.num_views) : 0.0;
  std::vector<ViewId> not_adjusted;  // no estimated track, or nothing free: the per-view path's own answer
  std::vector<uint8_t> group_moved(flat.group_ids.size(), 0);
  for (size_t c = 0; c < n; ++c) {
    if (rc == TMI_BA_OK && termination[c] < 0) {
      not_adjusted.push_back(flat.view_ids[c]);
      continue;
    }
    BundleAdjustmentSummary& s = result[flat.view_ids[c]];
    s.success = rc == TMI_BA_OK && (termination[c] == 0 || termination[c] == 1);
    s.initial_cost = initial_cost[c];
    s.final_cost = final_cost[c];
    s.solve_time_in_seconds = vs.kernel_seconds * share;
    s.setup_time_in_seconds = (vs.seconds - vs.kernel_seconds) * share;
    if (!s.success) continue;
    Camera* camera = reconstruction->MutableView(flat.view_ids[c])->MutableCamera();
    std::copy(flat.extrinsics.begin() + 6 * c, flat.extrinsics.begin() + 6 * c + 6, camera->mutable_extrinsics());
    group_moved[flat.camera_group[c]] = 1;
  }
  // the groups' intrinsics through the group's representative view, as BundleAdjuster::Optimize writes them
  // (GetIntrinsicsForCameraIntrinsicsGroup, bundle_adjuster.cc:289-302)
  for (size_t g = 0; g < flat.group_ids.size(); ++g) {
    if (!group_moved[g]) continue;
    const auto members = reconstruction->GetViewsInCameraIntrinsicGroup(flat.group_ids[g]);
    if (members.empty()) continue;
    double* K = reconstruction->MutableView(*members.begin())->MutableCamera()->MutableCameraIntrinsics()->mutable_parameters();
    std::copy(flat.intrinsics.begin() + flat.group_offset[g], flat.intrinsics.begin() + flat.group_offset[g + 1], K);
  }
  // views the flattening left out have no residual either
  for (const ViewId v : views)
    if (!std::binary_search(flat.view_ids.begin(), flat.view_ids.end(), v)) not_adjusted.push_back(v);
  std::sort(not_adjusted.begin(), not_adjusted.end());
  for (const ViewId v : not_adjusted) result[v] = BundleAdjustView(options, v, reconstruction);
  return result;
}

}  // namespace theia
