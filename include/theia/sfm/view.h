// reference: src/theia/sfm/view.h:57-101
#ifndef THEIA_MI355_SFM_VIEW_H_
#define THEIA_MI355_SFM_VIEW_H_
#include <string>
#include <unordered_map>
#include <vector>
#include "theia/sfm/camera/camera.h"
#include "theia/sfm/feature.h"
#include "theia/sfm/types.h"
namespace theia {
// reference: sfm/camera_intrinsics_prior.h -- of the priors the focal length's, which DoesViewHaveKnownIntrinsics
// (localize_view_to_reconstruction.cc:55-58) and EstimateTwoViewInfo read, and the image size and the principal
// point, from which EstimateTwoViewInfo centres the pixels and scales its threshold.
struct CameraIntrinsicsPrior {
  int image_width = 0;
  int image_height = 0;
  struct FocalLength {
    bool is_set = false;
    double value[1] = {0.0};
  } focal_length;
  struct PrincipalPoint {
    bool is_set = false;
    double value[2] = {0.0, 0.0};
  } principal_point;
};
class View {
 public:
  View() : name_(""), is_estimated_(false) {}
  explicit View(const std::string& name) : name_(name), is_estimated_(false) {}
  const std::string& Name() const { return name_; }
  void SetEstimated(bool is_estimated) {
    if (is_estimated != is_estimated_) internal::BumpDataModelEpoch();
    is_estimated_ = is_estimated;
  }
  bool IsEstimated() const { return is_estimated_; }
  const class Camera& Camera() const { return camera_; }
  class Camera* MutableCamera() { return &camera_; }
  const struct CameraIntrinsicsPrior& CameraIntrinsicsPrior() const { return camera_intrinsics_prior_; }
  struct CameraIntrinsicsPrior* MutableCameraIntrinsicsPrior() { return &camera_intrinsics_prior_; }
  int NumFeatures() const { return static_cast<int>(features_.size()); }
  std::vector<TrackId> TrackIds() const {
    std::vector<TrackId> ids;
    ids.reserve(features_.size());
    for (const auto& f : features_) ids.push_back(f.first);
    return ids;
  }
  const Feature* GetFeature(const TrackId track_id) const {
    auto it = features_.find(track_id);
    return it == features_.end() ? nullptr : &it->second;
  }
  // Extension: the (track id -> feature) table itself, for callers that walk every feature
  // (the reference's TrackIds() + GetFeature() pair costs a copy and a look-up per feature).
  const std::unordered_map<TrackId, Feature>& Features() const { return features_; }
  void AddFeature(const TrackId track_id, const Feature& feature) {
    internal::BumpDataModelEpoch();
    features_[track_id] = feature;
  }
  bool RemoveFeature(const TrackId track_id) {
    internal::BumpDataModelEpoch();
    return features_.erase(track_id) > 0;
  }

 private:
  std::string name_;
  bool is_estimated_;
  class Camera camera_;
  struct CameraIntrinsicsPrior camera_intrinsics_prior_;
  std::unordered_map<TrackId, Feature> features_;
};
}  // namespace theia
#endif
