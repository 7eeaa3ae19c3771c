// reference: src/theia/sfm/estimators/estimate_relative_pose.h:49-65
// EstimateRelativePose on tmi_ba_estimate_calibrated_relative_poses (theia_mi355_ba.h, where the steps are listed line
// by line): RANSAC over the minimal five-point essential matrix, the pose from it.  Implemented in
// theiasfm_amd/host/two_view_ransac_ops.cc.
//
// NOT provided -- the call returns false and leaves its outputs alone: a ransac_type other than RansacType::RANSAC,
// ransac_params.use_mle (MLESAC scoring) and ransac_params.use_Tdd_test.  Fewer than five correspondences, no model in
// any iteration and a failed device call return false as well.
// ransac_params.rng cannot be honoured (the device draws its samples from a stateless stream of its own): the samples
// come from ransac_params.seed, an extension field.  Sample sequences are not the reference's.
// ransac_params.max_iterations above 2^20 (the reference's default is INT_MAX) is taken as 2^20, the C ABI's limit.
// relative_pose->essential_matrix has unit Frobenius norm (the reference leaves the solver's scale).
#ifndef THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_RELATIVE_POSE_H_
#define THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_RELATIVE_POSE_H_
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/create_and_initialize_ransac_variant.h"
#include "theia/sfm/localize_view_to_reconstruction.h"  // RansacParameters, RansacSummary
#include "theia/util/eigen_lite.h"

namespace theia {
struct RelativePose {
  Eigen::Matrix3d essential_matrix;
  Eigen::Matrix3d rotation;
  Eigen::Vector3d position;
};

// normalized_correspondences: the principal point removed and divided by the focal length.
// ransac_params.error_thresh: the squared Sampson threshold in those units.
bool EstimateRelativePose(const RansacParameters& ransac_params, const RansacType& ransac_type,
                          const std::vector<FeatureCorrespondence>& normalized_correspondences,
                          RelativePose* relative_pose, RansacSummary* ransac_summary);
}  // namespace theia
#endif
