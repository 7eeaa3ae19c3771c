// reference: src/theia/sfm/estimators/estimate_homography.h:45-63 and
// src/theia/sfm/two_view_match_geometric_verification.cc:326-363 (CountHomographyInliers)
// EstimateHomography on tmi_ba_estimate_homographies (theia_mi355_ba.h, where the steps are listed line by line): RANSAC
// over the normalised four-point homography with inlier-count or MLESAC scoring, and the homography inlier count that
// TwoViewMatchGeometricVerification::VerifyMatches writes to TwoViewInfo::num_homography_inliers before anything else.
// Implemented in theiasfm_amd/host/homography_ops.cc (link it with localize_ops.cc, which owns
// ComputeResolutionScaledThreshold).
//
// ransac_params.use_mle IS honoured (MLEQualityMeasurement).  NOT provided -- the call returns false (the count: -1) and
// leaves its outputs alone: a ransac_type other than RansacType::RANSAC and ransac_params.use_Tdd_test.  Fewer than
// four correspondences, no model in any iteration and a failed device call return false as well.
// DEVIATION: a sample whose 8x9 constraint matrix has a rank other than 8 (three collinear points, a repeated point)
// gives no model; the reference scores whatever vector its SVD leaves.
// ransac_params.rng cannot be honoured (the device draws its samples from a stateless stream of its own): the samples
// come from ransac_params.seed, an extension field.  Sample sequences are not the reference's.
// ransac_params.max_iterations above 2^20 (the reference's default is INT_MAX) is taken as 2^20, the C ABI's limit.
#ifndef THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_HOMOGRAPHY_H_
#define THEIA_MI355_SFM_ESTIMATORS_ESTIMATE_HOMOGRAPHY_H_
#include <cstdint>
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/create_and_initialize_ransac_variant.h"
#include "theia/sfm/estimate_twoview_info.h"             // EstimateTwoViewInfoOptions
#include "theia/sfm/localize_view_to_reconstruction.h"  // RansacParameters, RansacSummary
#include "theia/sfm/twoview_info.h"
#include "theia/util/eigen_lite.h"
#include "theia_mi355_ba.h"

namespace theia {
// The correspondences are in whatever units the caller uses; ransac_params.error_thresh is in those units squared.
// *homography maps feature1 to feature2, as estimated (no scale is imposed).
bool EstimateHomography(const RansacParameters& ransac_params, const RansacType& ransac_type,
                        const std::vector<FeatureCorrespondence>& correspondences, Eigen::Matrix3d* homography,
                        RansacSummary* ransac_summary);

// Extension of the MI355X path: every pair in ONE device call.  One entry per view pair; every pointer must stay valid
// for the call.  A pair's sample stream depends only on (ransac_params.seed, stream_id) -- 0 unless the caller sets it
// -- so the batched call equals one EstimateHomography per pair.  error_thresh <= 0: ransac_params.error_thresh.
struct HomographyProblem {
  const std::vector<FeatureCorrespondence>* correspondences = nullptr;
  double error_thresh = 0.0;
  Eigen::Matrix3d* homography = nullptr;    // out, written only when the pair's result is true
  RansacSummary* ransac_summary = nullptr;  // out (optional), written for every attempted pair
  std::uint32_t stream_id = 0;
};
std::vector<bool> EstimateHomographies(const RansacParameters& ransac_params, const RansacType& ransac_type,
                                       const std::vector<HomographyProblem>& problems, int device = -1);

// TwoViewMatchGeometricVerification::CountHomographyInliers (:326-363) without the class around it: the image sizes are
// those of the two cameras (camera1_.ImageWidth() ..), the correspondences are what
// CreateCorrespondencesFromIndexedMatches leaves (pixels).  The threshold is the product of the two resolution-scaled
// options.max_sampson_error_pixels (:334-346); min / max_ransac_iterations, 1 - expected_ransac_confidence and use_mle
// are passed on.  Returns the number of inliers (0 where no homography was found, as the reference's empty summary
// gives), or -1 where the call is refused (ransac_type) or the device call failed.
int CountHomographyInliers(const EstimateTwoViewInfoOptions& options, int image_width1, int image_height1,
                           int image_width2, int image_height2,
                           const std::vector<FeatureCorrespondence>& correspondences);

// Extension: the counts of many pairs in ONE device call, written to info->num_homography_inliers.  One result per
// problem: false where nothing was written (a refused call, a failed device call, a null pointer).
struct HomographyCountProblem {
  int image_width1 = 0, image_height1 = 0, image_width2 = 0, image_height2 = 0;
  const std::vector<FeatureCorrespondence>* correspondences = nullptr;  // pixels
  TwoViewInfo* info = nullptr;  // out: num_homography_inliers
  std::uint32_t stream_id = 0;
};
std::vector<bool> CountHomographyInliersBatch(const EstimateTwoViewInfoOptions& options,
                                              const std::vector<HomographyCountProblem>& problems);

// The two host-only builders of the calls above (no device is touched).
// :334-346: the squared threshold of CountHomographyInliers for two image sizes.
double HomographyCountThreshold(const EstimateTwoViewInfoOptions& options, int image_width1, int image_height1,
                                int image_width2, int image_height2);
// RansacParameters -> the C ABI's options (max_iterations clamped to 2^20, use_mle passed on).
void HomographyDeviceOptions(const RansacParameters& ransac_params, int device, tmi_ba_homography_ransac_options* options);
// :348-352: the RansacParameters CountHomographyInliers builds from EstimateTwoViewInfoOptions.
RansacParameters HomographyCountRansacParameters(const EstimateTwoViewInfoOptions& options, double error_thresh);
}  // namespace theia
#endif
