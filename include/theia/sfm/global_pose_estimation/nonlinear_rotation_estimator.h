// reference: src/theia/sfm/global_pose_estimation/nonlinear_rotation_estimator.h (declaration) and .cc:49-100
// (semantics): global orientations refined from an initialisation by a nonlinear solve on the relative rotation error
// with a SoftLOne loss; GlobalRotationEstimatorType::NONLINEAR.
// Implemented on the C ABI (tmi_ba_estimate_global_rotations_nonlinear): one device call per EstimateRotations.
#ifndef THEIA_MI355_NONLINEAR_ROTATION_ESTIMATOR_H_
#define THEIA_MI355_NONLINEAR_ROTATION_ESTIMATOR_H_
#include <unordered_map>

#include "theia/sfm/global_pose_estimation/rotation_estimator.h"

namespace theia {
class NonlinearRotationEstimator : public RotationEstimator {
 public:
  NonlinearRotationEstimator() : robust_loss_width_(0.1) {}
  explicit NonlinearRotationEstimator(const double robust_loss_width) : robust_loss_width_(robust_loss_width) {}

  // *global_orientations holds the initialisation and receives the result.  The views -- those of the map and those the
  // pairs name -- are numbered in ascending ViewId order; a view that the map lacks has no initialisation (view_given =
  // 0), its pairs are skipped (:76-80) and it stays absent.  The pairs go to the device in ascending ViewIdPair order, the
  // order RobustRotationEstimator's shim uses (DEVIATION: the reference adds its residual blocks in hash-map order).  No
  // view is held (fixed_view = -1, the reference's problem).  An empty map or no pairs (the reference's two refusals,
  // :53-62), no device or a failed device call return false, leave the map as it was and write the message to stderr.
  bool EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                         std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) override;

  int device = -1;  // extension: the HIP device (-1: the current one)

 private:
  const double robust_loss_width_;
};
}  // namespace theia
#endif
