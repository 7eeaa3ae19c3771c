// Host shim of theia::TrackEstimator (estimate_track.cc:130-264).  The requested unestimated tracks and their
// observations in estimated views are flattened -- cameras held constant, ascending ViewId / TrackId order --
// and handed to tmi_ba_estimate_tracks, which runs EstimateTrack for all of them at once.  The statuses are then
// applied as the reference's sequence leaves the reconstruction: the point is written for statuses 0 (estimated),
// 3 (track BA failed) and 4 (bad reprojection), and status 0 marks the track estimated.
#include "theia/sfm/estimate_track.h"

#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#include "theia/sfm/bundle_adjustment/bundle_adjuster.h"
#include "theia/sfm/reconstruction.h"
#include "theia_mi355_ba.h"

namespace theia {

// estimate_track.cc:130-145
TrackEstimator::Summary TrackEstimator::EstimateAllTracks() {
  std::unordered_set<TrackId> tracks;
  for (const ViewId view_id : reconstruction_->ViewIds()) {
    const View* view = reconstruction_->View(view_id);
    if (view == nullptr || !view->IsEstimated()) continue;
    for (const auto& f : view->Features()) tracks.insert(f.first);
  }
  return EstimateTracks(tracks);
}

TrackEstimator::Summary TrackEstimator::EstimateTracks(const std::unordered_set<TrackId>& track_ids) {
  Summary summary;
  if (reconstruction_ == nullptr) return summary;
  std::vector<TrackId> tracks;
  for (const TrackId t : track_ids) {
    const Track* track = reconstruction_->Track(t);
    if (track == nullptr) continue;
    if (track->IsEstimated()) {
      ++summary.input_num_estimated_tracks;
    } else {
      tracks.push_back(t);
    }
  }
  summary.num_triangulation_attempts = static_cast<int>(tracks.size());
  if (tracks.empty()) return summary;
  std::sort(tracks.begin(), tracks.end());

  // the estimated views observing the tracks (GetObservationsFromTrackViews, estimate_track.cc:59-86)
  std::vector<ViewId> views;
  for (const TrackId t : tracks)
    for (const ViewId v : reconstruction_->Track(t)->ViewIds()) {
      const View* view = reconstruction_->View(v);
      if (view != nullptr && view->IsEstimated() && view->GetFeature(t) != nullptr) views.push_back(v);
    }
  std::sort(views.begin(), views.end());
  views.erase(std::unique(views.begin(), views.end()), views.end());
  if (views.empty()) return summary;  // every track has fewer than two observations
  std::map<ViewId, int> cam_index;
  std::map<CameraIntrinsicsGroupId, int> group_index;
  for (const ViewId v : views) {
    cam_index.emplace(v, static_cast<int>(cam_index.size()));
    group_index.emplace(reconstruction_->CameraIntrinsicsGroupIdFromViewId(v), 0);
  }
  std::vector<ViewId> group_view(group_index.size());
  {
    int g = 0;
    for (auto& e : group_index) e.second = g++;
  }
  const int nc = static_cast<int>(views.size()), ng = static_cast<int>(group_index.size());
  std::vector<double> extrinsics(6 * static_cast<size_t>(nc)), intrinsics;
  std::vector<int32_t> camera_group(nc), group_model(ng), group_offset(ng + 1, 0);
  std::vector<uint8_t> camera_flags(nc, TMI_BA_CAMERA_POSITION_CONSTANT | TMI_BA_CAMERA_ORIENTATION_CONSTANT);
  for (int c = 0; c < nc; ++c) {
    const Camera& camera = reconstruction_->View(views[c])->Camera();
    std::copy(camera.extrinsics(), camera.extrinsics() + 6, extrinsics.begin() + 6 * c);
    camera_group[c] = group_index[reconstruction_->CameraIntrinsicsGroupIdFromViewId(views[c])];
    group_view[camera_group[c]] = views[c];
  }
  for (int g = 0; g < ng; ++g) {
    const auto& intr = reconstruction_->View(group_view[g])->Camera().CameraIntrinsics();
    group_model[g] = static_cast<int32_t>(intr->Type());
    intrinsics.insert(intrinsics.end(), intr->parameters(), intr->parameters() + intr->NumParameters());
    group_offset[g + 1] = static_cast<int32_t>(intrinsics.size());
  }
  std::vector<uint8_t> intrinsics_constant(intrinsics.size(), 1);
  const int np = static_cast<int>(tracks.size());
  std::vector<double> points(4 * static_cast<size_t>(np));
  std::vector<uint8_t> point_constant(np, 0);
  std::vector<int32_t> obs_camera, obs_point;
  std::vector<double> obs_xy;
  for (int p = 0; p < np; ++p) {
    const Track* track = reconstruction_->Track(tracks[p]);
    std::copy(track->Point().data(), track->Point().data() + 4, points.begin() + 4 * p);
    std::vector<ViewId> seen;
    for (const ViewId v : track->ViewIds())
      if (cam_index.count(v) && reconstruction_->View(v)->GetFeature(tracks[p]) != nullptr) seen.push_back(v);
    std::sort(seen.begin(), seen.end());
    for (const ViewId v : seen) {
      const Feature& f = *reconstruction_->View(v)->GetFeature(tracks[p]);
      obs_camera.push_back(cam_index[v]);
      obs_point.push_back(p);
      obs_xy.push_back(f[0]);
      obs_xy.push_back(f[1]);
    }
  }
  tmi_ba_problem problem = {};
  problem.num_cameras = nc;
  problem.extrinsics = extrinsics.data();
  problem.camera_group = camera_group.data();
  problem.camera_flags = camera_flags.data();
  problem.num_groups = ng;
  problem.group_model = group_model.data();
  problem.group_offset = group_offset.data();
  problem.intrinsics = intrinsics.data();
  problem.intrinsics_constant = intrinsics_constant.data();
  problem.num_points = np;
  problem.points = points.data();
  problem.point_constant = point_constant.data();
  problem.num_observations = static_cast<int64_t>(obs_camera.size());
  problem.obs_camera = obs_camera.data();
  problem.obs_point = obs_point.data();
  problem.obs_xy = obs_xy.data();

  tmi_ba_track_estimator_options eo;
  tmi_ba_track_estimator_options_init(&eo);
  eo.max_acceptable_reprojection_error_pixels = options_.max_acceptable_reprojection_error_pixels;
  eo.min_triangulation_angle_degrees = options_.min_triangulation_angle_degrees;
  eo.bundle_adjustment = options_.bundle_adjustment ? 1 : 0;
  BundleAdjustmentOptions ba_options = options_.ba_options;
  ba_options.linear_solver_type = ceres::DENSE_QR;  // BundleAdjustTrack, bundle_adjustment.cc:100-101
  ba_options.use_inner_iterations = false;
  tmi_ba_options o;
  ToDeviceOptions(ba_options, &o);
  std::vector<int8_t> status(np, -1);
  tmi_ba_track_estimate_summary es;
  const int rc = tmi_ba_estimate_tracks(&problem, &eo, &o, nullptr, status.data(), &es);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::TrackEstimator] device track estimation failed: %s\n", tmi_ba_last_error());
    return summary;
  }
  for (int p = 0; p < np; ++p) {
    const int s = status[p];
    if (s != 0 && s != 3 && s != 4) continue;
    Track* track = reconstruction_->MutableTrack(tracks[p]);
    std::copy(points.begin() + 4 * p, points.begin() + 4 * p + 4, track->MutablePoint()->data());
    if (s == 0) {
      track->SetEstimated(true);
      summary.estimated_tracks.insert(tracks[p]);
    }
  }
  return summary;
}

}  // namespace theia
