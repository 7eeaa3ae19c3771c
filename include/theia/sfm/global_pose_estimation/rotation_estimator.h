// reference: src/theia/sfm/global_pose_estimation/rotation_estimator.h:48-62 -- the interface of the global rotation
// estimators: orientations of all views from the relative rotations of the view pairs and an initial guess.
#ifndef THEIA_MI355_ROTATION_ESTIMATOR_H_
#define THEIA_MI355_ROTATION_ESTIMATOR_H_
#include <unordered_map>

#include "theia/sfm/twoview_info.h"
#include "theia/sfm/types.h"
#include "theia/util/eigen_lite.h"
#include "theia/util/hash.h"

namespace theia {
class RotationEstimator {
 public:
  RotationEstimator() {}
  virtual ~RotationEstimator() {}
  // Input: the view pairs (their relative rotations are used) and an initial orientation of every view.
  // Output: the orientations, in place.  Returns true on success.
  virtual bool EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                 std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) = 0;

 private:
  RotationEstimator(const RotationEstimator&) = delete;
  void operator=(const RotationEstimator&) = delete;
};
}  // namespace theia
#endif
