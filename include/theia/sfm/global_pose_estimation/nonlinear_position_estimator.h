// reference: src/theia/sfm/global_pose_estimation/nonlinear_position_estimator.h:61-94 (declaration) and .cc:86-214
// (semantics): camera positions from global orientations and relative translation directions by a nonlinear solve with
// a robust loss (Wilson and Snavely, ECCV 2014); GlobalPositionEstimatorType::NONLINEAR, the default of
// ReconstructionEstimatorOptions.
// Implemented on the C ABI (tmi_ba_estimate_global_positions_nonlinear): one device call per EstimatePositions.
#ifndef THEIA_MI355_NONLINEAR_POSITION_ESTIMATOR_H_
#define THEIA_MI355_NONLINEAR_POSITION_ESTIMATOR_H_
#include <cstdint>
#include <unordered_map>

#include "theia/sfm/global_pose_estimation/position_estimator.h"
#include "theia/sfm/reconstruction.h"

namespace theia {
class NonlinearPositionEstimator : public PositionEstimator {
 public:
  struct Options {
    // The reference's `rng` is a seed here: the start is component k of view i (in ascending ViewId order)
    // = 100 (2 u - 1) with u from word 3 i + k of the splitmix64 stream of `seed` (theia_mi355_ba.h).
    uint64_t seed = 0;
    int num_threads = 1;  // accepted and ignored: the solve is one device call
    int max_num_iterations = 400;
    double robust_loss_width = 0.1;
    // Point-to-camera constraints are not provided: any value above 0 makes EstimatePositions return false.
    int min_num_points_per_view = 0;
    double point_to_camera_weight = 0.5;
    int device = -1;  // extension: the HIP device (-1: the current one)
    // extension: where given (not null), the positions to start from instead of the random start; it must hold every
    // view that receives a position.  Not owned.
    const std::unordered_map<ViewId, Eigen::Vector3d>* initial_positions = nullptr;
  };

  // The reconstruction is only read by the point-to-camera constraints, which are not provided.
  NonlinearPositionEstimator(const Options& options, const Reconstruction& reconstruction) : options_(options) {
    (void)reconstruction;
  }

  // View pairs with a view that has no orientation are dropped (:188-194).  The views of the remaining pairs -- only
  // they receive a position (:169-179) -- are numbered in ascending ViewId order and the smallest id is held at the
  // origin (the reference holds whichever its hash map yields first); the pairs go to the device in ascending ViewIdPair
  // order.  *positions is cleared and filled on success.  A failed call (empty inputs, an option the reference CHECKs,
  // min_num_points_per_view > 0, no pair left, views that the pairs do not connect, no device, a solve that is not
  // usable) returns false, leaves *positions unchanged and writes the message to stderr.
  bool EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                         const std::unordered_map<ViewId, Eigen::Vector3d>& orientation,
                         std::unordered_map<ViewId, Eigen::Vector3d>* positions) override;

 private:
  const Options options_;
};
}  // namespace theia
#endif
