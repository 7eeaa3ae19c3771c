// Host shim of theia::EstimateHomography (reference estimators/estimate_homography.cc:101-116) and of
// TwoViewMatchGeometricVerification::CountHomographyInliers (two_view_match_geometric_verification.cc:326-363) on the C
// ABI: all pairs of a call go through ONE tmi_ba_estimate_homographies and the results are written back.
// ComputeResolutionScaledThreshold is localize_ops.cc's.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "theia/sfm/estimators/estimate_homography.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
bool Supported(const char* who, const RansacType& ransac_type, bool use_Tdd_test) {
  if (ransac_type == RansacType::RANSAC && !use_Tdd_test) return true;
  std::fprintf(stderr, "[theia::%s] unsupported: only RansacType::RANSAC without use_Tdd_test is provided\n", who);
  return false;
}

struct PairResult {
  bool ok = false;
  Eigen::Matrix3d homography;
  RansacSummary summary;
};

// All pairs in one device call; thresholds: squared, in the correspondences' units.
bool RunBatch(const char* who, const std::vector<const std::vector<FeatureCorrespondence>*>& pairs,
              const std::vector<double>& thresholds, const std::vector<uint32_t>& streams,
              const tmi_ba_homography_ransac_options& options, std::vector<PairResult>* results) {
  const int P = static_cast<int>(pairs.size());
  results->assign(P, PairResult());
  std::vector<int64_t> offset(P + 1, 0);
  for (int p = 0; p < P; ++p) offset[p + 1] = offset[p] + static_cast<int64_t>(pairs[p]->size());
  std::vector<double> f1(2 * static_cast<size_t>(offset[P]) + 2), f2(f1.size());
  for (int p = 0; p < P; ++p)
    for (size_t k = 0; k < pairs[p]->size(); ++k) {
      const FeatureCorrespondence& c = (*pairs[p])[k];
      const size_t o = 2 * (static_cast<size_t>(offset[p]) + k);
      f1[o] = c.feature1.x();
      f1[o + 1] = c.feature1.y();
      f2[o] = c.feature2.x();
      f2[o + 1] = c.feature2.y();
    }
  std::vector<int8_t> status(P + 1, -1);
  std::vector<int32_t> iterations(P + 1, 0);
  std::vector<double> confidence(P + 1, 0.0), H(9 * static_cast<size_t>(P) + 1);
  std::vector<uint8_t> inlier(static_cast<size_t>(offset[P]) + 1, 0);
  tmi_ba_two_view_ransac_summary summary;
  const int rc = tmi_ba_estimate_homographies(&options, P, offset.data(), f1.data(), f2.data(), thresholds.data(),
                                              nullptr, streams.data(), nullptr, 0, status.data(), nullptr, nullptr,
                                              iterations.data(), nullptr, confidence.data(), H.data(), inlier.data(),
                                              nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::%s] device call failed: %s\n", who, tmi_ba_last_error());
    return false;
  }
  for (int p = 0; p < P; ++p) {
    PairResult& r = (*results)[p];
    const int n = static_cast<int>(pairs[p]->size());
    r.summary.num_input_data_points = n;
    r.summary.num_iterations = iterations[p];
    r.summary.confidence = confidence[p];
    for (int k = 0; k < n; ++k)
      if (inlier[static_cast<size_t>(offset[p]) + k]) r.summary.inliers.push_back(k);
    r.ok = status[p] == 0;
    if (r.ok)
      for (int i = 0; i < 9; ++i) r.homography.data()[i] = H[9 * static_cast<size_t>(p) + i];
  }
  return true;
}
}  // namespace

double HomographyCountThreshold(const EstimateTwoViewInfoOptions& options, int image_width1, int image_height1,
                                int image_width2, int image_height2) {
  const double t1 = ComputeResolutionScaledThreshold(options.max_sampson_error_pixels, image_width1, image_height1);
  const double t2 = ComputeResolutionScaledThreshold(options.max_sampson_error_pixels, image_width2, image_height2);
  return t1 * t2;
}

void HomographyDeviceOptions(const RansacParameters& ransac_params, int device,
                             tmi_ba_homography_ransac_options* options) {
  tmi_ba_homography_ransac_options_init(options);
  options->failure_probability = ransac_params.failure_probability;
  options->min_inlier_ratio = ransac_params.min_inlier_ratio;
  options->min_iterations = ransac_params.min_iterations;
  options->max_iterations = std::min(ransac_params.max_iterations, 1 << 20);
  options->seed = ransac_params.seed;
  options->device = device;
  options->use_mle = ransac_params.use_mle ? 1 : 0;
}

RansacParameters HomographyCountRansacParameters(const EstimateTwoViewInfoOptions& options, double error_thresh) {
  RansacParameters params;
  params.error_thresh = error_thresh;
  params.max_iterations = options.max_ransac_iterations;
  params.min_iterations = options.min_ransac_iterations;
  params.use_mle = options.use_mle;
  params.failure_probability = 1.0 - options.expected_ransac_confidence;
  params.seed = options.seed;
  return params;
}

std::vector<bool> EstimateHomographies(const RansacParameters& ransac_params, const RansacType& ransac_type,
                                       const std::vector<HomographyProblem>& problems, int device) {
  std::vector<bool> success(problems.size(), false);
  if (!Supported("EstimateHomography", ransac_type, ransac_params.use_Tdd_test)) return success;
  std::vector<size_t> which;
  std::vector<const std::vector<FeatureCorrespondence>*> pairs;
  std::vector<double> thresholds;
  std::vector<uint32_t> streams;
  for (size_t k = 0; k < problems.size(); ++k) {
    const HomographyProblem& q = problems[k];
    if (q.correspondences == nullptr || q.homography == nullptr) continue;
    which.push_back(k);
    pairs.push_back(q.correspondences);
    thresholds.push_back(q.error_thresh > 0.0 ? q.error_thresh : ransac_params.error_thresh);
    streams.push_back(q.stream_id);
  }
  if (which.empty()) return success;
  tmi_ba_homography_ransac_options o;
  HomographyDeviceOptions(ransac_params, device, &o);
  std::vector<PairResult> results;
  if (!RunBatch("EstimateHomography", pairs, thresholds, streams, o, &results)) return success;
  for (size_t j = 0; j < which.size(); ++j) {
    const HomographyProblem& q = problems[which[j]];
    if (q.ransac_summary != nullptr) *q.ransac_summary = results[j].summary;
    if (!results[j].ok) continue;
    *q.homography = results[j].homography;
    success[which[j]] = true;
  }
  return success;
}

bool EstimateHomography(const RansacParameters& ransac_params, const RansacType& ransac_type,
                        const std::vector<FeatureCorrespondence>& correspondences, Eigen::Matrix3d* homography,
                        RansacSummary* ransac_summary) {
  HomographyProblem q;
  q.correspondences = &correspondences;
  q.homography = homography;
  q.ransac_summary = ransac_summary;
  return EstimateHomographies(ransac_params, ransac_type, {q})[0];
}

std::vector<bool> CountHomographyInliersBatch(const EstimateTwoViewInfoOptions& options,
                                              const std::vector<HomographyCountProblem>& problems) {
  std::vector<bool> success(problems.size(), false);
  if (!Supported("CountHomographyInliers", options.ransac_type, false)) return success;
  std::vector<size_t> which;
  std::vector<const std::vector<FeatureCorrespondence>*> pairs;
  std::vector<double> thresholds;
  std::vector<uint32_t> streams;
  for (size_t k = 0; k < problems.size(); ++k) {
    const HomographyCountProblem& q = problems[k];
    if (q.correspondences == nullptr || q.info == nullptr) continue;
    which.push_back(k);
    pairs.push_back(q.correspondences);
    thresholds.push_back(
        HomographyCountThreshold(options, q.image_width1, q.image_height1, q.image_width2, q.image_height2));
    streams.push_back(q.stream_id);
  }
  if (which.empty()) return success;
  tmi_ba_homography_ransac_options o;
  HomographyDeviceOptions(HomographyCountRansacParameters(options, 0.0), options.device, &o);
  std::vector<PairResult> results;
  if (!RunBatch("CountHomographyInliers", pairs, thresholds, streams, o, &results)) return success;
  for (size_t j = 0; j < which.size(); ++j) {
    // (:362: the size of the summary's inliers, empty where Estimate found nothing)
    problems[which[j]].info->num_homography_inliers = static_cast<int>(results[j].summary.inliers.size());
    success[which[j]] = true;
  }
  return success;
}

int CountHomographyInliers(const EstimateTwoViewInfoOptions& options, int image_width1, int image_height1,
                           int image_width2, int image_height2,
                           const std::vector<FeatureCorrespondence>& correspondences) {
  TwoViewInfo info;
  HomographyCountProblem q;
  q.image_width1 = image_width1;
  q.image_height1 = image_height1;
  q.image_width2 = image_width2;
  q.image_height2 = image_height2;
  q.correspondences = &correspondences;
  q.info = &info;
  if (!CountHomographyInliersBatch(options, {q})[0]) return -1;
  return info.num_homography_inliers;
}

}  // namespace theia
