// reference: src/theia/sfm/localize_view_to_reconstruction.h:45-83, src/theia/solvers/sample_consensus_estimator.h:57-129
// LocalizeViewToReconstruction on tmi_ba_localize_views: the calibrated path (P3P RANSAC), then the batched
// BundleAdjustView.  Implemented in theiasfm_amd/host/localize_ops.cc.
//
// NOT provided -- such a view is reported on stderr as unsupported, left exactly as it was, and false is returned for
// it: a view without known intrinsics (the reference runs P4Pf), assume_known_orientation (the position-only solver),
// ransac_params.use_mle and ransac_params.use_Tdd_test.
// ransac_params.rng cannot be honoured (the device draws its samples from a stateless stream of its own): the samples
// come from ransac_params.seed, an extension field, and the ViewId.  Sample sequences are not the reference's.
// ransac_params.max_iterations above 2^20 (the reference's default is INT_MAX) is taken as 2^20, the C ABI's limit.
// A view's correspondences are numbered in ascending TrackId over its estimated tracks (the reference walks its hash
// map); RansacSummary::inliers holds those numbers.
#ifndef THEIA_MI355_SFM_LOCALIZE_VIEW_TO_RECONSTRUCTION_H_
#define THEIA_MI355_SFM_LOCALIZE_VIEW_TO_RECONSTRUCTION_H_
#include <cstdint>
#include <limits>
#include <memory>
#include <vector>

#include "theia/sfm/bundle_adjustment/bundle_adjustment.h"
#include "theia/sfm/reconstruction.h"
#include "theia/sfm/types.h"

namespace theia {
class RandomNumberGenerator;  // (never dereferenced here)

struct RansacParameters {
  std::shared_ptr<RandomNumberGenerator> rng;  // ignored: see above
  double error_thresh = -1;                    // overwritten per view from reprojection_error_threshold_pixels
  double failure_probability = 0.01;
  double min_inlier_ratio = 0;
  int min_iterations = 100;
  int max_iterations = std::numeric_limits<int>::max();
  bool use_mle = false;
  bool use_Tdd_test = false;
  std::uint64_t seed = 0;  // extension: the seed of the device's sample stream
};

struct RansacSummary {
  std::vector<int> inliers;
  int num_input_data_points = 0;
  int num_iterations = 0;
  double confidence = 0.0;
};

struct LocalizeViewToReconstructionOptions {
  double reprojection_error_threshold_pixels = 4.0;
  bool assume_known_orientation = false;
  RansacParameters ransac_params;
  bool bundle_adjust_view = true;
  BundleAdjustmentOptions ba_options;  // ba_options.device: the HIP device of the whole call
  int min_num_inliers = 30;
};

// reference: reconstruction_estimator_utils.cc:95-107
double ComputeResolutionScaledThreshold(double threshold_pixels, int image_width, int image_height);

// As the reference: true when the view was localised (and, with bundle_adjust_view, its adjustment was usable).  The
// pose is written and SetEstimated(true) is called once RANSAC found min_num_inliers inliers -- also where the
// adjustment then fails and false is returned (localize_view_to_reconstruction.cc:247-252).  Every other view is left
// as it was.
bool LocalizeViewToReconstruction(const ViewId view_to_localize, const LocalizeViewToReconstructionOptions options,
                                  Reconstruction* reconstruction, RansacSummary* summary);

// Extension: every view of view_ids in ONE device call; returns success per entry and fills summaries (resized).  A
// view's sample stream depends only on (ransac_params.seed, ViewId) and its RANSAC only on the estimated tracks, so
// "try the candidates in order until the first success" over this result equals calling the single-view form in that
// order -- up to what a view adjustment with free SHARED intrinsics changes for later views of its group.
std::vector<bool> LocalizeViewsToReconstruction(const std::vector<ViewId>& view_ids,
                                                const LocalizeViewToReconstructionOptions& options,
                                                Reconstruction* reconstruction, std::vector<RansacSummary>* summaries);
}  // namespace theia
#endif
