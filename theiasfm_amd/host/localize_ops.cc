// Host shim of theia::LocalizeViewToReconstruction (reference localize_view_to_reconstruction.cc:47-257) on the C ABI:
// the candidate views' observations of estimated tracks are flattened into one tmi_ba_problem whose camera index IS
// the ViewId (so that a view's sample stream does not depend on the batch it is in), RANSAC runs for all of them in one
// tmi_ba_localize_views call, the poses are written back, and the localised views are adjusted by BundleAdjustViews.
#include <algorithm>
#include <cstdio>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "theia/sfm/bundle_adjustment/bundle_adjuster.h"
#include "theia/sfm/localize_view_to_reconstruction.h"
#include "theia_mi355_ba.h"

namespace theia {

double ComputeResolutionScaledThreshold(const double threshold_pixels, const int image_width, const int image_height) {
  if (image_width == 0 && image_height == 0) return threshold_pixels;
  return threshold_pixels * static_cast<double>(std::max(image_width, image_height)) / 1024.0;
}

namespace {
// localize_view_to_reconstruction.cc:51-76, as the reference writes it: inside the loop over the intrinsics group it
// looks at the view itself, not at the view that shares the intrinsics.
bool DoesViewHaveKnownIntrinsics(const Reconstruction& reconstruction, const ViewId view_id) {
  const View* view = reconstruction.View(view_id);
  if (view->CameraIntrinsicsPrior().focal_length.is_set) return true;
  const CameraIntrinsicsGroupId group = reconstruction.CameraIntrinsicsGroupIdFromViewId(view_id);
  for (const ViewId shared : reconstruction.GetViewsInCameraIntrinsicGroup(group)) {
    const View* same_view = reconstruction.View(view_id);
    if (same_view->IsEstimated() && view_id != shared) return true;
  }
  return false;
}

const char* Unsupported(const LocalizeViewToReconstructionOptions& options, const Reconstruction& reconstruction,
                        const ViewId id) {
  if (reconstruction.View(id) == nullptr) return "no such view";
  if (options.assume_known_orientation) return "assume_known_orientation (the position-only solver) is not provided";
  if (options.ransac_params.use_mle) return "ransac_params.use_mle is not provided";
  if (options.ransac_params.use_Tdd_test) return "ransac_params.use_Tdd_test is not provided";
  if (!DoesViewHaveKnownIntrinsics(reconstruction, id)) return "unknown intrinsics (P4Pf) are not provided";
  return nullptr;
}
}  // namespace

std::vector<bool> LocalizeViewsToReconstruction(const std::vector<ViewId>& view_ids,
                                                const LocalizeViewToReconstructionOptions& options,
                                                Reconstruction* reconstruction, std::vector<RansacSummary>* summaries) {
  std::vector<bool> success(view_ids.size(), false);
  if (summaries != nullptr) summaries->assign(view_ids.size(), RansacSummary());
  if (reconstruction == nullptr || view_ids.empty()) return success;
  // the supported candidates, once each
  std::vector<ViewId> candidates;
  ViewId max_id = 0;
  for (const ViewId id : view_ids) {
    if (const char* why = Unsupported(options, *reconstruction, id)) {
      std::fprintf(stderr, "[theia::LocalizeViewToReconstruction] view %u is unsupported and left alone: %s\n", id, why);
      continue;
    }
    if (std::find(candidates.begin(), candidates.end(), id) == candidates.end()) candidates.push_back(id);
    max_id = std::max(max_id, id);
  }
  if (candidates.empty()) return success;
  // cameras indexed by ViewId; group 0 is a placeholder for the ids that are no candidates, group 1 + k is candidate k's
  const int num_cameras = static_cast<int>(max_id) + 1;
  std::vector<double> extrinsics(6 * static_cast<size_t>(num_cameras), 0.0), threshold(num_cameras, 1.0);
  std::vector<int32_t> camera_group(num_cameras, 0), group_model(1, 0), group_offset(2, 0);
  std::vector<double> intrinsics(tmi_ba_intrinsics_size(0), 0.0);
  intrinsics[0] = intrinsics[1] = 1.0;
  group_offset[1] = static_cast<int32_t>(intrinsics.size());
  std::vector<uint8_t> mask(num_cameras, 0);
  std::vector<double> points, obs_xy;
  std::vector<int32_t> obs_camera, obs_point;
  std::unordered_map<TrackId, int32_t> point_of_track;
  std::unordered_map<ViewId, int64_t> first_obs;  // of a candidate, in obs_*
  std::unordered_map<ViewId, int> num_obs;
  for (const ViewId id : candidates) {
    const View* view = reconstruction->View(id);
    const Camera& camera = view->Camera();
    const CameraIntrinsicsModel& model = *camera.CameraIntrinsics();
    mask[id] = 1;
    camera_group[id] = static_cast<int32_t>(group_model.size());
    group_model.push_back(static_cast<int32_t>(model.Type()));
    intrinsics.insert(intrinsics.end(), model.parameters(), model.parameters() + model.NumParameters());
    group_offset.push_back(static_cast<int32_t>(intrinsics.size()));
    const double scaled = ComputeResolutionScaledThreshold(options.reprojection_error_threshold_pixels,
                                                           camera.ImageWidth(), camera.ImageHeight());
    threshold[id] = scaled * scaled / (camera.FocalLength() * camera.FocalLength());  // :188-191
    std::vector<TrackId> tracks;
    for (const auto& feature : view->Features()) {
      const Track* track = reconstruction->Track(feature.first);
      if (track != nullptr && track->IsEstimated()) tracks.push_back(feature.first);  // :92-96
    }
    std::sort(tracks.begin(), tracks.end());
    first_obs[id] = static_cast<int64_t>(obs_camera.size());
    num_obs[id] = static_cast<int>(tracks.size());
    for (const TrackId t : tracks) {
      auto it = point_of_track.find(t);
      if (it == point_of_track.end()) {
        it = point_of_track.emplace(t, static_cast<int32_t>(points.size() / 4)).first;
        const Eigen::Vector4d& X = reconstruction->Track(t)->Point();
        for (int a = 0; a < 4; ++a) points.push_back(X[a]);
      }
      const Feature& f = *view->GetFeature(t);
      obs_camera.push_back(static_cast<int32_t>(id));
      obs_point.push_back(it->second);
      obs_xy.push_back(f[0]);
      obs_xy.push_back(f[1]);
    }
  }
  std::vector<uint8_t> intrinsics_constant(intrinsics.size(), 1);
  tmi_ba_problem P = {};
  P.num_cameras = num_cameras;
  P.extrinsics = extrinsics.data();
  P.camera_group = camera_group.data();
  P.num_groups = static_cast<int32_t>(group_model.size());
  P.group_model = group_model.data();
  P.group_offset = group_offset.data();
  P.intrinsics = intrinsics.data();
  P.intrinsics_constant = intrinsics_constant.data();
  P.num_points = static_cast<int32_t>(points.size() / 4);
  P.points = points.data();
  P.num_observations = static_cast<int64_t>(obs_camera.size());
  P.obs_camera = obs_camera.data();
  P.obs_point = obs_point.data();
  P.obs_xy = obs_xy.data();
  tmi_ba_localization_options L;
  tmi_ba_localization_options_init(&L);
  const RansacParameters& rp = options.ransac_params;
  L.failure_probability = rp.failure_probability;
  L.min_inlier_ratio = rp.min_inlier_ratio;
  L.min_iterations = rp.min_iterations;
  L.max_iterations = std::min(rp.max_iterations, 1 << 20);
  L.min_num_inliers = options.min_num_inliers;
  L.bundle_adjust_view = 0;  // the adjustment goes through BundleAdjustViews below, on the reconstruction's own groups
  L.seed = rp.seed;
  tmi_ba_options O;
  ToDeviceOptions(options.ba_options, &O);
  std::vector<int8_t> status(num_cameras, -1);
  std::vector<int32_t> iterations(num_cameras, 0);
  std::vector<double> confidence(num_cameras, 0.0);
  std::vector<uint8_t> inlier(obs_camera.size(), 0);
  tmi_ba_localization_summary summary;
  const int rc = tmi_ba_localize_views(&P, &L, &O, mask.data(), threshold.data(), nullptr, 0, status.data(), nullptr,
                                       nullptr, iterations.data(), nullptr, nullptr, confidence.data(), inlier.data(),
                                       nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::LocalizeViewToReconstruction] device call failed: %s\n", tmi_ba_last_error());
    return success;
  }
  // statuses 0 (and, after the adjustment, 4): the pose and SetEstimated(true) (:196-197, :247)
  std::unordered_set<ViewId> localised;
  for (const ViewId id : candidates) {
    if (status[id] != 0) continue;
    View* view = reconstruction->MutableView(id);
    double* e = view->MutableCamera()->mutable_extrinsics();
    for (int a = 0; a < 6; ++a) e[a] = extrinsics[6 * static_cast<size_t>(id) + a];
    view->SetEstimated(true);
    localised.insert(id);
  }
  std::unordered_map<ViewId, BundleAdjustmentSummary> adjusted;
  if (options.bundle_adjust_view && !localised.empty())
    adjusted = BundleAdjustViews(options.ba_options, localised, reconstruction);
  for (size_t k = 0; k < view_ids.size(); ++k) {
    const ViewId id = view_ids[k];
    if (id >= static_cast<ViewId>(num_cameras) || !mask[id]) continue;
    if (summaries != nullptr) {
      RansacSummary& s = (*summaries)[k];
      s.num_input_data_points = num_obs[id];
      s.num_iterations = iterations[id];
      s.confidence = confidence[id];
      for (int j = 0; j < num_obs[id]; ++j)
        if (inlier[static_cast<size_t>(first_obs[id]) + j]) s.inliers.push_back(j);
    }
    bool ok = status[id] == 0;
    if (ok && options.bundle_adjust_view) {
      const auto it = adjusted.find(id);
      ok = it != adjusted.end() && it->second.success;  // :248-252
    }
    success[k] = ok;
  }
  return success;
}

bool LocalizeViewToReconstruction(const ViewId view_to_localize, const LocalizeViewToReconstructionOptions options,
                                  Reconstruction* reconstruction, RansacSummary* summary) {
  std::vector<RansacSummary> summaries;
  const std::vector<bool> ok = LocalizeViewsToReconstruction({view_to_localize}, options, reconstruction, &summaries);
  if (summary != nullptr && !summaries.empty()) *summary = summaries[0];
  return !ok.empty() && ok[0];
}

}  // namespace theia
