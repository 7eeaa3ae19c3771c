// reference: src/theia/sfm/global_pose_estimation/linear_position_estimator.h:59-80 (declaration) and .cc:163-470
// (semantics): camera positions from global orientations, relative translation directions and the tracks the views of a
// triplet share, as the eigenvector of the smallest eigenvalue of the triplets' constraints (Jiang, Cui and Tan, ICCV
// 2013); GlobalPositionEstimatorType::LINEAR_TRIPLET.
// Implemented on the C ABI (tmi_ba_estimate_global_positions_linear): one device call per EstimatePositions.
#ifndef THEIA_MI355_LINEAR_POSITION_ESTIMATOR_H_
#define THEIA_MI355_LINEAR_POSITION_ESTIMATOR_H_
#include <unordered_map>

#include "theia/sfm/global_pose_estimation/position_estimator.h"
#include "theia/sfm/reconstruction.h"

namespace theia {
class LinearPositionEstimator : public PositionEstimator {
 public:
  struct Options {
    int num_threads = 1;              // accepted and ignored: the solve is one device call
    int max_power_iterations = 1000;  // the bound on the subspace iterations
    // Declared by the reference and never read by it (Spectra runs on its own defaults); accepted and not forwarded:
    // the device's stop rule keeps its own tolerance (theia_mi355_ba.h).
    double eigensolver_threshold = 1e-8;
    int device = -1;  // extension: the HIP device (-1: the current one)
  };

  // The reconstruction supplies every view's camera model and features; it is read during EstimatePositions and must
  // outlive the estimator.
  LinearPositionEstimator(const Options& options, const Reconstruction& reconstruction)
      : options_(options), reconstruction_(reconstruction) {}

  // View pairs with a view that has no orientation or is not in the reconstruction are dropped.  The views of the
  // remaining pairs are numbered in ascending ViewId order, the pairs go to the device in ascending ViewIdPair order, a
  // view's features in ascending TrackId.  *positions is cleared and receives an entry for exactly the estimated views:
  // those of the largest component of triplets; the smallest id among them is at the origin before the
  // sign vote.  A failed call (empty inputs, an option that is not positive, a pair whose first id is not below its
  // second, no pair left, no device, no triplet with a baseline or a solve that is not usable) returns false, leaves
  // *positions unchanged and writes the message to stderr.
  bool EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                         const std::unordered_map<ViewId, Eigen::Vector3d>& orientation,
                         std::unordered_map<ViewId, Eigen::Vector3d>* positions) override;

 private:
  const Options options_;
  const Reconstruction& reconstruction_;
};
}  // namespace theia
#endif
