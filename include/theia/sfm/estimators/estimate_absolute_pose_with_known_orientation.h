// reference: src/theia/sfm/estimators/estimate_absolute_pose_with_known_orientation.h:50-62
// EstimateAbsolutePoseWithKnownOrientation on tmi_ba_estimate_positions_known_orientation (theia_mi355_ba.h, where the
// steps are listed line by line): the correspondences are rotated by the camera's orientation ON THE DEVICE, then RANSAC
// over PositionFromTwoRays with inlier-count or MLESAC scoring.  Implemented in
// theiasfm_amd/host/known_orientation_ops.cc.
//
// ransac_params.use_mle IS honoured (MLEQualityMeasurement).  NOT provided -- the call returns false, leaves its outputs
// alone and says so on stderr: a ransac_type other than RansacType::RANSAC and ransac_params.use_Tdd_test.  Fewer than
// two correspondences, no model in any iteration and a failed device call return false as well.
// The assume_known_orientation branch of LocalizeViewToReconstruction stays refused (localize_view_to_reconstruction.h);
// this is the estimator that branch would call.
// ransac_params.rng cannot be honoured (the device draws its samples from a stateless stream of its own): the samples
// come from ransac_params.seed, an extension field.  Sample sequences are not the reference's.
// ransac_params.max_iterations above 2^20 (the reference's default is INT_MAX) is taken as 2^20, the C ABI's limit.
#ifndef THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_ABSOLUTE_POSE_WITH_KNOWN_ORIENTATION_H_
#define THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_ABSOLUTE_POSE_WITH_KNOWN_ORIENTATION_H_
#include <cstdint>
#include <vector>

#include "theia/sfm/create_and_initialize_ransac_variant.h"
#include "theia/sfm/estimators/feature_correspondence_2d_3d.h"
#include "theia/sfm/localize_view_to_reconstruction.h"  // RansacParameters, RansacSummary
#include "theia/util/eigen_lite.h"
#include "theia_mi355_ba.h"

namespace theia {
// The 2D features are normalised by the camera intrinsics and NOT rotated; camera_orientation is the angle-axis of the
// world-to-camera rotation; ransac_params.error_thresh is in normalised units squared.
bool EstimateAbsolutePoseWithKnownOrientation(const RansacParameters& ransac_params, const RansacType& ransac_type,
                                              const Eigen::Vector3d& camera_orientation,
                                              const std::vector<FeatureCorrespondence2D3D>& normalized_correspondences,
                                              Eigen::Vector3d* camera_position, RansacSummary* ransac_summary);

// Extension of the MI355X path: every view in ONE device call.  One entry per view; every pointer must stay valid for
// the call.  A view's sample stream depends only on (ransac_params.seed, stream_id) -- 0 unless the caller sets it -- so
// the batched call equals one EstimateAbsolutePoseWithKnownOrientation per view.  error_thresh <= 0:
// ransac_params.error_thresh.
struct KnownOrientationAbsoluteProblem {
  Eigen::Vector3d camera_orientation;
  const std::vector<FeatureCorrespondence2D3D>* normalized_correspondences = nullptr;
  double error_thresh = 0.0;
  Eigen::Vector3d* camera_position = nullptr;  // out, written only when the view's result is true
  RansacSummary* ransac_summary = nullptr;     // out (optional), written for every attempted view
  std::uint32_t stream_id = 0;
};
std::vector<bool> EstimateAbsolutePosesWithKnownOrientation(const RansacParameters& ransac_params,
                                                            const RansacType& ransac_type,
                                                            const std::vector<KnownOrientationAbsoluteProblem>& problems,
                                                            int device = -1);
}  // namespace theia
#endif
