// reference: src/theia/sfm/estimate_twoview_info.h:50-98, estimate_twoview_info.cc:60-285
// EstimateTwoViewInfo on tmi_ba_estimate_uncalibrated_relative_poses (the UNCALIBRATED branch, :191-248: a focal prior
// is missing) and tmi_ba_estimate_calibrated_relative_poses (the CALIBRATED branch, :131-189: both focal priors are set).
// Implemented in theiasfm_amd/host/two_view_ransac_ops.cc.
//
// What is and is not provided:
//  * The CALIBRATED branch exists for INLIER-COUNT scoring only: it is taken when both focal priors are set AND
//    options.use_mle == false.  The pixels are centred and divided by the focal prior, the threshold is
//    t1 t2 / (f1 f2) (:152-162), focal_length_1 / focal_length_2 are the priors.  The reference passes use_mle on to
//    MLESAC scoring, which this project provides nowhere: with both priors set and use_mle == true (THE DEFAULT)
//    EstimateTwoViewInfo returns false and leaves *twoview_info and *inlier_indices exactly as they were (the reference
//    clears the indices on entry; here they are untouched so that the gap is visible).  MLE is the remaining gap; there
//    is NO silent fall-back to inlier-count scoring or to the uncalibrated branch.
//  * A ransac_type other than RansacType::RANSAC returns false.  The uncalibrated branch does not read
//    options.use_mle: the reference's never passes it on (:213-221); EstimateUncalibratedRelativePose itself refuses
//    ransac_params.use_mle.
//  * Of CameraIntrinsicsPrior only the image size, the focal length's is_set and the principal point are read: the
//    pixels are centred on the principal point prior or, without one, on (image_width / 2, image_height / 2), as a
//    PINHOLE camera set from the priors centres them (pinhole_camera_model.cc:85-90) -- no distortion priors.
// twoview_info->visibility_score is 0, as in the reference: it computes the score from *inlier_indices BEFORE assigning
// them, after clearing them on entry (estimate_twoview_info.cc:243-245, :260).  num_homography_inliers is not written
// here, as in the reference: CountHomographyInliers (theia/sfm/estimators/estimate_homography.h) is what sets it.
// options.rng cannot be honoured; the samples come from options.seed, an extension field.
#ifndef THEIA_MI355_SFM_ESTIMATE_TWOVIEW_INFO_H_
#define THEIA_MI355_SFM_ESTIMATE_TWOVIEW_INFO_H_
#include <cstdint>
#include <memory>
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/create_and_initialize_ransac_variant.h"
#include "theia/sfm/twoview_info.h"
#include "theia/sfm/view.h"  // CameraIntrinsicsPrior

namespace theia {
class RandomNumberGenerator;  // (never dereferenced here)

struct EstimateTwoViewInfoOptions {
  std::shared_ptr<RandomNumberGenerator> rng;  // ignored: see above
  RansacType ransac_type = RansacType::RANSAC;
  double max_sampson_error_pixels = 6.0;  // w.r.t. an image 1024 pixels wide (ComputeResolutionScaledThreshold)
  double expected_ransac_confidence = 0.9999;
  int min_ransac_iterations = 10;
  int max_ransac_iterations = 1000;
  bool use_mle = true;  // calibrated pairs are estimated only with false (see above); not read by the uncalibrated branch
  // extensions of the MI355X path
  std::uint64_t seed = 0;  // of the device's sample stream
  int device = -1;         // -1 = the current device
};

bool EstimateTwoViewInfo(const EstimateTwoViewInfoOptions& options, const CameraIntrinsicsPrior& intrinsics1,
                         const CameraIntrinsicsPrior& intrinsics2,
                         const std::vector<FeatureCorrespondence>& correspondences, TwoViewInfo* twoview_info,
                         std::vector<int>* inlier_indices);

// Extension of the MI355X path: every pair in ONE device call.  One entry per view pair; every pointer must stay
// valid for the call.  A pair's sample stream depends only on (options.seed, stream_id) -- 0 unless the caller sets
// it -- so the batched call equals one EstimateTwoViewInfo per pair.  A batch that mixes calibrated and uncalibrated
// pairs makes one device call per kind.
struct TwoViewInfoProblem {
  const CameraIntrinsicsPrior* intrinsics1 = nullptr;
  const CameraIntrinsicsPrior* intrinsics2 = nullptr;
  const std::vector<FeatureCorrespondence>* correspondences = nullptr;  // pixels
  TwoViewInfo* twoview_info = nullptr;         // out, written only when the pair's result is true
  std::vector<int>* inlier_indices = nullptr;  // out: cleared on entry (attempted pairs), the inliers in order
  std::uint32_t stream_id = 0;
};
std::vector<bool> EstimateTwoViewInfos(const EstimateTwoViewInfoOptions& options,
                                       const std::vector<TwoViewInfoProblem>& problems);
}  // namespace theia
#endif
