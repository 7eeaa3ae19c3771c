// reference: src/theia/sfm/estimators/estimate_relative_pose_with_known_orientation.h:49-59
// EstimateRelativePoseWithKnownOrientation on tmi_ba_estimate_relative_positions_known_orientation (theia_mi355_ba.h,
// where the steps are listed line by line): RANSAC over RelativePoseFromTwoPointsWithKnownRotation with inlier-count or
// MLESAC scoring.  Implemented in theiasfm_amd/host/known_orientation_ops.cc.
//
// As in the reference the correspondences of this signature are ALREADY ROTATED into one frame by the caller
// (rf = hnormalize(R^t K^-1 [u v 1]^t)); the device call is given zero rotations, which pass the features through bit
// for bit.  The batched extension below can take the two views' orientations and have the device rotate.
// *relative_camera2_position is the unit direction +-(c2 - c1) / |c2 - c1|: ITS SIGN IS NOT PART OF THE ESTIMATE (the
// reference's is whatever FullPivLU::kernel() leaves; here that of the cross product of the two sampled epipolar rows).
//
// ransac_params.use_mle IS honoured.  NOT provided -- the call returns false, leaves its outputs alone and says so on
// stderr: a ransac_type other than RansacType::RANSAC and ransac_params.use_Tdd_test.  Fewer than two correspondences,
// no model in any iteration and a failed device call return false as well.
// ransac_params.rng is ignored: the samples come from ransac_params.seed, an extension field; max_iterations above 2^20
// is taken as 2^20.
#ifndef THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_RELATIVE_POSE_WITH_KNOWN_ORIENTATION_H_
#define THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_RELATIVE_POSE_WITH_KNOWN_ORIENTATION_H_
#include <cstdint>
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/create_and_initialize_ransac_variant.h"
#include "theia/sfm/localize_view_to_reconstruction.h"  // RansacParameters, RansacSummary
#include "theia/util/eigen_lite.h"
#include "theia_mi355_ba.h"

namespace theia {
bool EstimateRelativePoseWithKnownOrientation(const RansacParameters& ransac_params, const RansacType& ransac_type,
                                              const std::vector<FeatureCorrespondence>& rotated_correspondences,
                                              Eigen::Vector3d* relative_camera2_position,
                                              RansacSummary* ransac_summary);

// Extension of the MI355X path: every view pair in ONE device call.  orientation1 / orientation2 (angle-axis, world to
// camera) rotate feature1 / feature2 on the device; leave both zero for correspondences that are already rotated.  The
// other fields are those of KnownOrientationAbsoluteProblem.
struct KnownOrientationRelativeProblem {
  Eigen::Vector3d orientation1, orientation2;
  const std::vector<FeatureCorrespondence>* correspondences = nullptr;
  double error_thresh = 0.0;
  Eigen::Vector3d* relative_camera2_position = nullptr;  // out, written only when the pair's result is true
  RansacSummary* ransac_summary = nullptr;               // out (optional), written for every attempted pair
  std::uint32_t stream_id = 0;
};
std::vector<bool> EstimateRelativePosesWithKnownOrientation(const RansacParameters& ransac_params,
                                                            const RansacType& ransac_type,
                                                            const std::vector<KnownOrientationRelativeProblem>& problems,
                                                            int device = -1);
}  // namespace theia
#endif
