// reference: src/theia/sfm/global_pose_estimation/least_unsquared_deviation_position_estimator.h:58-102 (declaration)
// and .cc:67-212 (semantics): camera positions from global orientations and relative translation directions by least
// unsquared deviations (Ozyesil and Singer, CVPR 2015).
// Implemented on the C ABI (tmi_ba_estimate_global_positions_lud): one device call per EstimatePositions.
#ifndef THEIA_MI355_LEAST_UNSQUARED_DEVIATION_POSITION_ESTIMATOR_H_
#define THEIA_MI355_LEAST_UNSQUARED_DEVIATION_POSITION_ESTIMATOR_H_
#include <unordered_map>

#include "theia/sfm/global_pose_estimation/position_estimator.h"

namespace theia {
class LeastUnsquaredDeviationPositionEstimator : public PositionEstimator {
 public:
  // The reference only CHECKs the first two (> 0) and reads none of the three: the solver runs on the defaults of
  // ConstrainedL1Solver::Options (1000 iterations, rho 10, alpha 1.2, tolerances 1e-4 and 1e-2).  So does this one.
  struct Options {
    int max_num_iterations = 400;
    int max_num_reweighted_iterations = 10;
    double convergence_criterion = 1e-4;
    int device = -1;  // extension: the HIP device (-1: the current one)
  };

  explicit LeastUnsquaredDeviationPositionEstimator(const Options& options) : options_(options) {}

  // View pairs with a view that has no orientation are dropped (InitializeIndexMapping, :123-152).  The views of the
  // remaining pairs are numbered in ascending ViewId order and the smallest id is held at the origin (the reference
  // holds whichever its hash map yields first); the pairs go to the device in ascending ViewIdPair order.  *positions is
  // cleared and filled on success.  A failed call (an option the reference CHECKs, no pair left, no device, views that
  // the pairs do not connect, ...) returns false, leaves *positions unchanged and writes the message to stderr.
  bool EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                         const std::unordered_map<ViewId, Eigen::Vector3d>& orientation,
                         std::unordered_map<ViewId, Eigen::Vector3d>* positions) override;

 private:
  const Options options_;
};
}  // namespace theia
#endif
