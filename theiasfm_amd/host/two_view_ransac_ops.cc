// Host shim of theia::EstimateUncalibratedRelativePose, theia::EstimateRelativePose and theia::EstimateTwoViewInfo
// (reference estimate_uncalibrated_relative_pose.cc:153-170, estimate_relative_pose.cc:129-144,
// estimate_twoview_info.cc:67-285) on the C ABI: the pairs' pixels are centred (and, for a calibrated pair, divided by
// the focal priors), the squared threshold is computed per pair, RANSAC runs for all pairs of a kind in one
// tmi_ba_estimate_uncalibrated_relative_poses / tmi_ba_estimate_calibrated_relative_poses call and the results are
// written back.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "theia/sfm/estimate_twoview_info.h"
#include "theia/sfm/estimators/estimate_relative_pose.h"
#include "theia/sfm/estimators/estimate_uncalibrated_relative_pose.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
// reconstruction_estimator_utils.cc:95-107 (ComputeResolutionScaledThreshold; the shim's own copy lives with the
// localisation call, which this file does not need to be linked with)
double ResolutionScaledThreshold(const double threshold_pixels, const int image_width, const int image_height) {
  if (image_width == 0 && image_height == 0) return threshold_pixels;
  return threshold_pixels * static_cast<double>(std::max(image_width, image_height)) / 1024.0;
}

void PrincipalPoint(const CameraIntrinsicsPrior& prior, double pp[2]) {
  pp[0] = pp[1] = 0.0;
  if (prior.principal_point.is_set) {
    pp[0] = prior.principal_point.value[0];
    pp[1] = prior.principal_point.value[1];
  } else if (prior.image_width != 0 && prior.image_height != 0) {
    pp[0] = prior.image_width / 2.0;
    pp[1] = prior.image_height / 2.0;
  }
}

// Eigen's AngleAxisd(angle, axis).toRotationMatrix() for the angle-axis vector aa
void RotationMatrix(const double aa[3], Eigen::Matrix3d* R) {
  const double theta = std::sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) (*R)(r, c) = r == c ? 1.0 : 0.0;
  if (!(theta > 0.0)) return;
  const double k[3] = {aa[0] / theta, aa[1] / theta, aa[2] / theta};
  const double s = std::sin(theta), c1 = 1.0 - std::cos(theta);
  const double K[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double kk = 0.0;
      for (int j = 0; j < 3; ++j) kk += K[r][j] * K[j][c];
      (*R)(r, c) += s * K[r][c] + c1 * kk;
    }
}

struct PairResult {
  bool ok = false;
  UncalibratedRelativePose pose;  // fundamental_matrix holds E for a calibrated pair (focal lengths 0)
  double rotation_angle_axis[3] = {0, 0, 0};
  RansacSummary summary;
};

// All pairs of one kind in one device call.  centred[p]: the pair's centred (calibrated: normalised) correspondences;
// thresholds: squared, in the correspondences' units.
bool RunBatch(bool calibrated, const std::vector<const std::vector<FeatureCorrespondence>*>& centred,
              const std::vector<double>& thresholds, const std::vector<uint32_t>& streams,
              const tmi_ba_two_view_ransac_options& options, std::vector<PairResult>* results) {
  const int P = static_cast<int>(centred.size());
  results->assign(P, PairResult());
  std::vector<int64_t> offset(P + 1, 0);
  for (int p = 0; p < P; ++p) offset[p + 1] = offset[p] + static_cast<int64_t>(centred[p]->size());
  std::vector<double> f1(2 * static_cast<size_t>(offset[P]) + 2), f2(f1.size());
  for (int p = 0; p < P; ++p)
    for (size_t k = 0; k < centred[p]->size(); ++k) {
      const FeatureCorrespondence& c = (*centred[p])[k];
      const size_t o = 2 * (static_cast<size_t>(offset[p]) + k);
      f1[o] = c.feature1.x();
      f1[o + 1] = c.feature1.y();
      f2[o] = c.feature2.x();
      f2[o + 1] = c.feature2.y();
    }
  std::vector<int8_t> status(P, -1);
  std::vector<int32_t> iterations(P, 0);
  std::vector<double> confidence(P, 0.0), F(9 * static_cast<size_t>(P) + 1), fl1(P + 1), fl2(P + 1),
      rot(3 * static_cast<size_t>(P) + 1), pos(3 * static_cast<size_t>(P) + 1);
  std::vector<uint8_t> inlier(static_cast<size_t>(offset[P]) + 1, 0);
  tmi_ba_two_view_ransac_summary summary;
  const int rc =
      calibrated
          ? tmi_ba_estimate_calibrated_relative_poses(
                &options, P, offset.data(), f1.data(), f2.data(), thresholds.data(), nullptr, streams.data(), nullptr, 0,
                status.data(), nullptr, nullptr, iterations.data(), nullptr, nullptr, confidence.data(), F.data(),
                rot.data(), pos.data(), inlier.data(), nullptr, &summary)
          : tmi_ba_estimate_uncalibrated_relative_poses(
                &options, P, offset.data(), f1.data(), f2.data(), thresholds.data(), nullptr, streams.data(), nullptr, 0,
                status.data(), nullptr, nullptr, iterations.data(), nullptr, confidence.data(), F.data(), fl1.data(),
                fl2.data(), rot.data(), pos.data(), inlier.data(), nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::%s] device call failed: %s\n",
                 calibrated ? "EstimateRelativePose" : "EstimateUncalibratedRelativePose", tmi_ba_last_error());
    return false;
  }
  for (int p = 0; p < P; ++p) {
    PairResult& r = (*results)[p];
    const int n = static_cast<int>(centred[p]->size());
    r.summary.num_input_data_points = n;
    r.summary.num_iterations = iterations[p];
    r.summary.confidence = confidence[p];
    for (int k = 0; k < n; ++k)
      if (inlier[static_cast<size_t>(offset[p]) + k]) r.summary.inliers.push_back(k);
    r.ok = status[p] == 0;
    if (!r.ok) continue;
    for (int i = 0; i < 9; ++i) r.pose.fundamental_matrix.data()[i] = F[9 * static_cast<size_t>(p) + i];
    r.pose.focal_length1 = fl1[p];
    r.pose.focal_length2 = fl2[p];
    for (int i = 0; i < 3; ++i) {
      r.rotation_angle_axis[i] = rot[3 * static_cast<size_t>(p) + i];
      r.pose.position[i] = pos[3 * static_cast<size_t>(p) + i];
    }
    RotationMatrix(r.rotation_angle_axis, &r.pose.rotation);
  }
  return true;
}

void DeviceOptions(double failure_probability, double min_inlier_ratio, int min_iterations, int max_iterations,
                   uint64_t seed, int device, tmi_ba_two_view_ransac_options* o) {
  tmi_ba_two_view_ransac_options_init(o);
  o->failure_probability = failure_probability;
  o->min_inlier_ratio = min_inlier_ratio;
  o->min_iterations = min_iterations;
  o->max_iterations = std::min(max_iterations, 1 << 20);
  o->seed = seed;
  o->device = device;
}
}  // namespace

bool EstimateUncalibratedRelativePose(const RansacParameters& ransac_params, const RansacType& ransac_type,
                                      const std::vector<FeatureCorrespondence>& centered_correspondences,
                                      UncalibratedRelativePose* relative_pose, RansacSummary* ransac_summary) {
  if (ransac_type != RansacType::RANSAC || ransac_params.use_mle || ransac_params.use_Tdd_test) {
    std::fprintf(stderr, "[theia::EstimateUncalibratedRelativePose] unsupported: only RansacType::RANSAC without "
                         "use_mle and use_Tdd_test is provided\n");
    return false;
  }
  if (relative_pose == nullptr) return false;
  tmi_ba_two_view_ransac_options o;
  DeviceOptions(ransac_params.failure_probability, ransac_params.min_inlier_ratio, ransac_params.min_iterations,
                ransac_params.max_iterations, ransac_params.seed, -1, &o);
  std::vector<PairResult> results;
  if (!RunBatch(false, {&centered_correspondences}, {ransac_params.error_thresh}, {0u}, o, &results)) return false;
  if (ransac_summary != nullptr) *ransac_summary = results[0].summary;
  if (!results[0].ok) return false;
  *relative_pose = results[0].pose;
  return true;
}

bool EstimateRelativePose(const RansacParameters& ransac_params, const RansacType& ransac_type,
                          const std::vector<FeatureCorrespondence>& normalized_correspondences,
                          RelativePose* relative_pose, RansacSummary* ransac_summary) {
  if (ransac_type != RansacType::RANSAC || ransac_params.use_mle || ransac_params.use_Tdd_test) {
    std::fprintf(stderr, "[theia::EstimateRelativePose] unsupported: only RansacType::RANSAC without use_mle and "
                         "use_Tdd_test is provided\n");
    return false;
  }
  if (relative_pose == nullptr) return false;
  tmi_ba_two_view_ransac_options o;
  DeviceOptions(ransac_params.failure_probability, ransac_params.min_inlier_ratio, ransac_params.min_iterations,
                ransac_params.max_iterations, ransac_params.seed, -1, &o);
  std::vector<PairResult> results;
  if (!RunBatch(true, {&normalized_correspondences}, {ransac_params.error_thresh}, {0u}, o, &results)) return false;
  if (ransac_summary != nullptr) *ransac_summary = results[0].summary;
  if (!results[0].ok) return false;
  relative_pose->essential_matrix = results[0].pose.fundamental_matrix;
  relative_pose->rotation = results[0].pose.rotation;
  relative_pose->position = results[0].pose.position;
  return true;
}

std::vector<bool> EstimateTwoViewInfos(const EstimateTwoViewInfoOptions& options,
                                       const std::vector<TwoViewInfoProblem>& problems) {
  std::vector<bool> success(problems.size(), false);
  if (options.ransac_type != RansacType::RANSAC) {
    std::fprintf(stderr, "[theia::EstimateTwoViewInfo] unsupported: only RansacType::RANSAC is provided\n");
    return success;
  }
  // one device call per kind of pair: [0] uncalibrated (eight-point), [1] calibrated (five-point)
  std::vector<size_t> which[2];
  std::vector<std::vector<FeatureCorrespondence>> centred[2];
  std::vector<double> thresholds[2];
  std::vector<uint32_t> streams[2];
  for (size_t k = 0; k < problems.size(); ++k) {
    const TwoViewInfoProblem& q = problems[k];
    if (q.intrinsics1 == nullptr || q.intrinsics2 == nullptr || q.correspondences == nullptr ||
        q.twoview_info == nullptr || q.inlier_indices == nullptr)
      continue;
    const bool calibrated = q.intrinsics1->focal_length.is_set && q.intrinsics2->focal_length.is_set;
    if (calibrated && options.use_mle) {
      std::fprintf(stderr, "[theia::EstimateTwoViewInfo] pair %zu: both focal lengths are known and options.use_mle is "
                           "set; MLESAC scoring is not provided (set use_mle = false for inlier-count scoring), the "
                           "pair is left alone\n", k);
      continue;
    }
    q.inlier_indices->clear();  // estimate_twoview_info.cc:260
    double pp1[2], pp2[2];
    PrincipalPoint(*q.intrinsics1, pp1);
    PrincipalPoint(*q.intrinsics2, pp2);
    // NormalizeFeatures (:67-100) for a PINHOLE camera set from the priors: the focal division only with both priors
    const double fl1 = calibrated ? q.intrinsics1->focal_length.value[0] : 1.0;
    const double fl2 = calibrated ? q.intrinsics2->focal_length.value[0] : 1.0;
    std::vector<FeatureCorrespondence> c(q.correspondences->size());
    for (size_t i = 0; i < c.size(); ++i) {
      const FeatureCorrespondence& in = (*q.correspondences)[i];
      c[i].feature1 = Feature((in.feature1.x() - pp1[0]) / fl1, (in.feature1.y() - pp1[1]) / fl1);
      c[i].feature2 = Feature((in.feature2.x() - pp2[0]) / fl2, (in.feature2.y() - pp2[1]) / fl2);
    }
    centred[calibrated].push_back(std::move(c));
    const double t1 = ResolutionScaledThreshold(options.max_sampson_error_pixels, q.intrinsics1->image_width,
                                                q.intrinsics1->image_height);
    const double t2 = ResolutionScaledThreshold(options.max_sampson_error_pixels, q.intrinsics2->image_width,
                                                q.intrinsics2->image_height);
    thresholds[calibrated].push_back(calibrated ? t1 * t2 / (fl1 * fl2) : t1 * t2);  // :160-162, :220-221
    streams[calibrated].push_back(q.stream_id);
    which[calibrated].push_back(k);
  }
  tmi_ba_two_view_ransac_options o;
  DeviceOptions(1.0 - options.expected_ransac_confidence, 0.0, options.min_ransac_iterations,
                options.max_ransac_iterations, options.seed, options.device, &o);
  for (int calibrated = 0; calibrated < 2; ++calibrated) {
    if (which[calibrated].empty()) continue;
    std::vector<const std::vector<FeatureCorrespondence>*> ptrs;
    for (const auto& c : centred[calibrated]) ptrs.push_back(&c);
    std::vector<PairResult> results;
    if (!RunBatch(calibrated != 0, ptrs, thresholds[calibrated], streams[calibrated], o, &results)) continue;
    for (size_t j = 0; j < which[calibrated].size(); ++j) {
      const PairResult& r = results[j];
      if (!r.ok) continue;
      const TwoViewInfoProblem& q = problems[which[calibrated][j]];
      TwoViewInfo* info = q.twoview_info;
      for (int i = 0; i < 3; ++i) {
        info->rotation_2[i] = r.rotation_angle_axis[i];
        info->position_2[i] = r.pose.position[i];
      }
      info->focal_length_1 = calibrated ? q.intrinsics1->focal_length.value[0] : r.pose.focal_length1;  // :180-181
      info->focal_length_2 = calibrated ? q.intrinsics2->focal_length.value[0] : r.pose.focal_length2;
      info->num_verified_matches = static_cast<int>(r.summary.inliers.size());
      info->visibility_score = 0;  // of the (still empty) *inlier_indices: :183-186, :243-245
      *q.inlier_indices = r.summary.inliers;
      success[which[calibrated][j]] = true;
    }
  }
  return success;
}

bool EstimateTwoViewInfo(const EstimateTwoViewInfoOptions& options, const CameraIntrinsicsPrior& intrinsics1,
                         const CameraIntrinsicsPrior& intrinsics2,
                         const std::vector<FeatureCorrespondence>& correspondences, TwoViewInfo* twoview_info,
                         std::vector<int>* inlier_indices) {
  TwoViewInfoProblem q;
  q.intrinsics1 = &intrinsics1;
  q.intrinsics2 = &intrinsics2;
  q.correspondences = &correspondences;
  q.twoview_info = twoview_info;
  q.inlier_indices = inlier_indices;
  return EstimateTwoViewInfos(options, {q})[0];
}

}  // namespace theia
