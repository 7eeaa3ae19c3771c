// reference: src/theia/sfm/global_pose_estimation/position_estimator.h:48-66 -- the interface of the global position
// estimators: positions of all views from the relative translations of the view pairs and the global orientations.
#ifndef THEIA_MI355_POSITION_ESTIMATOR_H_
#define THEIA_MI355_POSITION_ESTIMATOR_H_
#include <unordered_map>

#include "theia/sfm/twoview_info.h"
#include "theia/sfm/types.h"
#include "theia/util/eigen_lite.h"
#include "theia/util/hash.h"

namespace theia {
class PositionEstimator {
 public:
  PositionEstimator() {}
  virtual ~PositionEstimator() {}
  // Input: the view pairs (their relative translations are used) and the global orientation of every view.
  // Output: the positions.  Returns true on success.
  virtual bool EstimatePositions(const std::unordered_map<ViewIdPair, TwoViewInfo>& view_pairs,
                                 const std::unordered_map<ViewId, Eigen::Vector3d>& orientation,
                                 std::unordered_map<ViewId, Eigen::Vector3d>* positions) = 0;

 private:
  PositionEstimator(const PositionEstimator&) = delete;
  void operator=(const PositionEstimator&) = delete;
};
}  // namespace theia
#endif
