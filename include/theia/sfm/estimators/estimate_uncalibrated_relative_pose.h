// reference: src/theia/sfm/estimators/estimate_uncalibrated_relative_pose.h:51-73
// EstimateUncalibratedRelativePose on tmi_ba_estimate_uncalibrated_relative_poses (theia_mi355_ba.h, where the steps are
// listed line by line): RANSAC over the normalised eight-point fundamental matrix, the focal lengths from it, the pose
// from the essential matrix.  Implemented in theiasfm_amd/host/two_view_ransac_ops.cc.
//
// NOT provided -- the call returns false and leaves its outputs alone: a ransac_type other than RansacType::RANSAC,
// ransac_params.use_mle and ransac_params.use_Tdd_test.  Fewer than eight correspondences, no model in any iteration
// and a failed device call return false as well.
// ransac_params.rng cannot be honoured (the device draws its samples from a stateless stream of its own): the samples
// come from ransac_params.seed, an extension field.  Sample sequences are not the reference's.
// ransac_params.max_iterations above 2^20 (the reference's default is INT_MAX) is taken as 2^20, the C ABI's limit.
#ifndef THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_UNCALIBRATED_RELATIVE_POSE_H_
#define THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_UNCALIBRATED_RELATIVE_POSE_H_
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/create_and_initialize_ransac_variant.h"
#include "theia/sfm/localize_view_to_reconstruction.h"  // RansacParameters, RansacSummary
#include "theia/util/eigen_lite.h"

namespace theia {
struct UncalibratedRelativePose {
  Eigen::Matrix3d fundamental_matrix;
  double focal_length1;
  double focal_length2;
  Eigen::Matrix3d rotation;
  Eigen::Vector3d position;
};

// centered_correspondences: pixels with the principal point removed.  ransac_params.error_thresh: the squared
// Sampson threshold in pixels^2.
bool EstimateUncalibratedRelativePose(const RansacParameters& ransac_params, const RansacType& ransac_type,
                                      const std::vector<FeatureCorrespondence>& centered_correspondences,
                                      UncalibratedRelativePose* relative_pose, RansacSummary* ransac_summary);
}  // namespace theia
#endif
