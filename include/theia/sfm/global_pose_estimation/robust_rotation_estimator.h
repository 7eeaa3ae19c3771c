// reference: src/theia/sfm/global_pose_estimation/robust_rotation_estimator.h:61-162 (declaration) and .cc:51-282
// (semantics): global orientations from relative rotations by L1 minimisation followed by iteratively reweighted least
// squares (Chatterjee and Govindu, ICCV 2013).
// Implemented on the C ABI (tmi_ba_estimate_global_rotations_robust): one device call per EstimateRotations.
#ifndef THEIA_MI355_ROBUST_ROTATION_ESTIMATOR_H_
#define THEIA_MI355_ROBUST_ROTATION_ESTIMATOR_H_
#include <unordered_map>
#include <utility>
#include <vector>

#include "theia/sfm/global_pose_estimation/rotation_estimator.h"

namespace theia {
class RobustRotationEstimator : public RotationEstimator {
 public:
  struct Options {
    int max_num_l1_iterations = 5;
    double l1_step_convergence_threshold = 0.001;
    int max_num_irls_iterations = 100;
    double irls_step_convergence_threshold = 0.001;
    double irls_loss_parameter_sigma = 5.0 * 3.14159265358979323846 / 180.0;  // DegToRad(5.0)
    int device = -1;  // extension: the HIP device (-1: the current one)
  };

  explicit RobustRotationEstimator(const Options& options) : options_(options) {}

  // Adds the relative rotation of every view pair, then estimates.  The views of global_orientations are numbered in
  // ascending ViewId order and the smallest id is held fixed (the reference holds whichever its hash map yields first).
  // An edge with a view that has no initial orientation is an error (the reference dies in FindOrDie).  A failed device
  // call (no device, a view that the edges do not connect to the fixed one, ...) returns false, leaves
  // *global_orientations unchanged and writes the message to stderr.
  bool EstimateRotations(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                         std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations) override;

  // The alternative interface (:93-110): constraints one by one -- the same pair may be added more than once and in
  // either direction -- then EstimateRotations on the orientations alone.  Edges go to the device in the order added.
  void AddRelativeRotationConstraint(const ViewIdPair& view_id_pair, const Eigen::Vector3d& relative_rotation);
  bool EstimateRotations(std::unordered_map<ViewId, Eigen::Vector3d>* global_orientations);

 private:
  const Options options_;
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> relative_rotations_;
};
}  // namespace theia
#endif
