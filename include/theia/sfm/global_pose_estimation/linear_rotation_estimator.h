// reference: src/theia/sfm/global_pose_estimation/linear_rotation_estimator.h (declaration) and .cc:78-203
// (semantics): global orientations as the three eigenvectors of the smallest eigenvalues of the matrix of
// sum |R_j - R_ij R_i|_F^2, projected to SO(3); GlobalRotationEstimatorType::LINEAR.  Needs no initialisation.
// Implemented on the C ABI (tmi_ba_estimate_global_rotations_linear): one device call per EstimateRotations.
#ifndef THEIA_MI355_LINEAR_ROTATION_ESTIMATOR_H_
#define THEIA_MI355_LINEAR_ROTATION_ESTIMATOR_H_
#include <unordered_map>
#include <utility>
#include <vector>

#include "theia/sfm/global_pose_estimation/rotation_estimator.h"

namespace theia {
class LinearRotationEstimator : public RotationEstimator {
 public:
  LinearRotationEstimator() {}

  // Adds every pair's rotation_2 as a constraint, then estimates (:78-85).
  bool EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                         std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) override;

  // An alternative interface: add the constraints one by one, then call the one-argument EstimateRotations.
  void AddRelativeRotationConstraint(const ViewIdPair& view_id_pair, const Eigen::Vector3d& relative_rotation);

  // The views the constraints name are numbered in ascending ViewId order and the constraints go to the device in
  // ascending ViewIdPair order (DEVIATION: the reference numbers the views as its constraints arrive and walks hash
  // maps).  The results are emplaced: a key the map already holds keeps its value (:199).  Not converged within the
  // iteration limit: a warning and true, as the reference, which ignores Spectra's status.  No constraints (the
  // reference CHECK-fails), a pair added twice, constraints that are not connected or otherwise refused by the C call, no
  // device, a failed device call or a matrix that could not be factored return false, leave the map as it was and write
  // the message to stderr.
  bool EstimateRotations(std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations);

  int device = -1;  // extension: the HIP device (-1: the current one)

 private:
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> constraints_;
};
}  // namespace theia
#endif
