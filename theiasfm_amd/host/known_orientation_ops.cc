// Host shim of theia::EstimateAbsolutePoseWithKnownOrientation (reference
// estimators/estimate_absolute_pose_with_known_orientation.cc:126-150) and theia::EstimateRelativePoseWithKnownOrientation
// (estimators/estimate_relative_pose_with_known_orientation.cc:66-82) on the C ABI: all items of a call go through ONE
// tmi_ba_estimate_positions_known_orientation / tmi_ba_estimate_relative_positions_known_orientation and the results are
// written back.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "theia/sfm/estimators/estimate_absolute_pose_with_known_orientation.h"
#include "theia/sfm/estimators/estimate_relative_pose_with_known_orientation.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
bool Supported(const char* who, const RansacType& ransac_type, bool use_Tdd_test) {
  if (ransac_type == RansacType::RANSAC && !use_Tdd_test) return true;
  std::fprintf(stderr, "[theia::%s] unsupported: only RansacType::RANSAC without use_Tdd_test is provided\n", who);
  return false;
}

void DeviceOptions(const RansacParameters& ransac_params, int device, tmi_ba_homography_ransac_options* options) {
  tmi_ba_homography_ransac_options_init(options);
  options->failure_probability = ransac_params.failure_probability;
  options->min_inlier_ratio = ransac_params.min_inlier_ratio;
  options->min_iterations = ransac_params.min_iterations;
  options->max_iterations = std::min(ransac_params.max_iterations, 1 << 20);
  options->seed = ransac_params.seed;
  options->device = device;
  options->use_mle = ransac_params.use_mle ? 1 : 0;
}

struct ItemResult {
  bool ok = false;
  Eigen::Vector3d position;
  RansacSummary summary;
};

// What the device call left for N items of offset[]: the shared read-out of the two calls.
void ReadOut(const std::vector<int64_t>& offset, const std::vector<int8_t>& status,
             const std::vector<int32_t>& iterations, const std::vector<double>& confidence,
             const std::vector<double>& position, const std::vector<uint8_t>& inlier,
             std::vector<ItemResult>* results) {
  const int N = static_cast<int>(offset.size()) - 1;
  results->assign(N, ItemResult());
  for (int p = 0; p < N; ++p) {
    ItemResult& r = (*results)[p];
    const int n = static_cast<int>(offset[p + 1] - offset[p]);
    r.summary.num_input_data_points = n;
    r.summary.num_iterations = iterations[p];
    r.summary.confidence = confidence[p];
    for (int k = 0; k < n; ++k)
      if (inlier[static_cast<size_t>(offset[p]) + k]) r.summary.inliers.push_back(k);
    r.ok = status[p] == 0;
    if (r.ok) r.position = Eigen::Vector3d(position[3 * p], position[3 * p + 1], position[3 * p + 2]);
  }
}
}  // namespace

std::vector<bool> EstimateAbsolutePosesWithKnownOrientation(const RansacParameters& ransac_params,
                                                            const RansacType& ransac_type,
                                                            const std::vector<KnownOrientationAbsoluteProblem>& problems,
                                                            int device) {
  const char* who = "EstimateAbsolutePoseWithKnownOrientation";
  std::vector<bool> success(problems.size(), false);
  if (!Supported(who, ransac_type, ransac_params.use_Tdd_test)) return success;
  std::vector<size_t> which;
  for (size_t k = 0; k < problems.size(); ++k)
    if (problems[k].normalized_correspondences != nullptr && problems[k].camera_position != nullptr) which.push_back(k);
  if (which.empty()) return success;
  const int N = static_cast<int>(which.size());
  std::vector<int64_t> offset(N + 1, 0);
  for (int p = 0; p < N; ++p)
    offset[p + 1] = offset[p] + static_cast<int64_t>(problems[which[p]].normalized_correspondences->size());
  const size_t total = static_cast<size_t>(offset[N]);
  std::vector<double> feature(2 * total + 2), point(3 * total + 3), orientation(3 * static_cast<size_t>(N)), thresholds(N);
  std::vector<uint32_t> streams(N);
  for (int p = 0; p < N; ++p) {
    const KnownOrientationAbsoluteProblem& q = problems[which[p]];
    for (size_t k = 0; k < q.normalized_correspondences->size(); ++k) {
      const FeatureCorrespondence2D3D& c = (*q.normalized_correspondences)[k];
      const size_t o = static_cast<size_t>(offset[p]) + k;
      feature[2 * o] = c.feature.x();
      feature[2 * o + 1] = c.feature.y();
      for (int i = 0; i < 3; ++i) point[3 * o + i] = c.world_point[i];
    }
    for (int i = 0; i < 3; ++i) orientation[3 * static_cast<size_t>(p) + i] = q.camera_orientation[i];
    thresholds[p] = q.error_thresh > 0.0 ? q.error_thresh : ransac_params.error_thresh;
    streams[p] = q.stream_id;
  }
  tmi_ba_homography_ransac_options o;
  DeviceOptions(ransac_params, device, &o);
  std::vector<int8_t> status(N, -1);
  std::vector<int32_t> iterations(N, 0);
  std::vector<double> confidence(N, 0.0), position(3 * static_cast<size_t>(N));
  std::vector<uint8_t> inlier(total + 1, 0);
  tmi_ba_two_view_ransac_summary summary;
  const int rc = tmi_ba_estimate_positions_known_orientation(
      &o, N, offset.data(), feature.data(), point.data(), orientation.data(), thresholds.data(), nullptr,
      streams.data(), nullptr, 0, status.data(), nullptr, nullptr, iterations.data(), nullptr, confidence.data(),
      position.data(), inlier.data(), nullptr, nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::%s] device call failed: %s\n", who, tmi_ba_last_error());
    return success;
  }
  std::vector<ItemResult> results;
  ReadOut(offset, status, iterations, confidence, position, inlier, &results);
  for (int p = 0; p < N; ++p) {
    const KnownOrientationAbsoluteProblem& q = problems[which[p]];
    if (q.ransac_summary != nullptr) *q.ransac_summary = results[p].summary;
    if (!results[p].ok) continue;
    *q.camera_position = results[p].position;
    success[which[p]] = true;
  }
  return success;
}

bool EstimateAbsolutePoseWithKnownOrientation(const RansacParameters& ransac_params, const RansacType& ransac_type,
                                              const Eigen::Vector3d& camera_orientation,
                                              const std::vector<FeatureCorrespondence2D3D>& normalized_correspondences,
                                              Eigen::Vector3d* camera_position, RansacSummary* ransac_summary) {
  KnownOrientationAbsoluteProblem q;
  q.camera_orientation = camera_orientation;
  q.normalized_correspondences = &normalized_correspondences;
  q.camera_position = camera_position;
  q.ransac_summary = ransac_summary;
  return EstimateAbsolutePosesWithKnownOrientation(ransac_params, ransac_type, {q})[0];
}

std::vector<bool> EstimateRelativePosesWithKnownOrientation(const RansacParameters& ransac_params,
                                                            const RansacType& ransac_type,
                                                            const std::vector<KnownOrientationRelativeProblem>& problems,
                                                            int device) {
  const char* who = "EstimateRelativePoseWithKnownOrientation";
  std::vector<bool> success(problems.size(), false);
  if (!Supported(who, ransac_type, ransac_params.use_Tdd_test)) return success;
  std::vector<size_t> which;
  for (size_t k = 0; k < problems.size(); ++k)
    if (problems[k].correspondences != nullptr && problems[k].relative_camera2_position != nullptr) which.push_back(k);
  if (which.empty()) return success;
  const int N = static_cast<int>(which.size());
  std::vector<int64_t> offset(N + 1, 0);
  for (int p = 0; p < N; ++p) offset[p + 1] = offset[p] + static_cast<int64_t>(problems[which[p]].correspondences->size());
  const size_t total = static_cast<size_t>(offset[N]);
  std::vector<double> f1(2 * total + 2), f2(2 * total + 2), o1(3 * static_cast<size_t>(N)), o2(o1.size()), thresholds(N);
  std::vector<uint32_t> streams(N);
  for (int p = 0; p < N; ++p) {
    const KnownOrientationRelativeProblem& q = problems[which[p]];
    for (size_t k = 0; k < q.correspondences->size(); ++k) {
      const FeatureCorrespondence& c = (*q.correspondences)[k];
      const size_t o = 2 * (static_cast<size_t>(offset[p]) + k);
      f1[o] = c.feature1.x();
      f1[o + 1] = c.feature1.y();
      f2[o] = c.feature2.x();
      f2[o + 1] = c.feature2.y();
    }
    for (int i = 0; i < 3; ++i) {
      o1[3 * static_cast<size_t>(p) + i] = q.orientation1[i];
      o2[3 * static_cast<size_t>(p) + i] = q.orientation2[i];
    }
    thresholds[p] = q.error_thresh > 0.0 ? q.error_thresh : ransac_params.error_thresh;
    streams[p] = q.stream_id;
  }
  tmi_ba_homography_ransac_options o;
  DeviceOptions(ransac_params, device, &o);
  std::vector<int8_t> status(N, -1);
  std::vector<int32_t> iterations(N, 0);
  std::vector<double> confidence(N, 0.0), position(3 * static_cast<size_t>(N));
  std::vector<uint8_t> inlier(total + 1, 0);
  tmi_ba_two_view_ransac_summary summary;
  const int rc = tmi_ba_estimate_relative_positions_known_orientation(
      &o, N, offset.data(), f1.data(), f2.data(), o1.data(), o2.data(), thresholds.data(), nullptr, streams.data(),
      nullptr, 0, status.data(), nullptr, nullptr, iterations.data(), nullptr, confidence.data(), position.data(),
      inlier.data(), nullptr, nullptr, nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::%s] device call failed: %s\n", who, tmi_ba_last_error());
    return success;
  }
  std::vector<ItemResult> results;
  ReadOut(offset, status, iterations, confidence, position, inlier, &results);
  for (int p = 0; p < N; ++p) {
    const KnownOrientationRelativeProblem& q = problems[which[p]];
    if (q.ransac_summary != nullptr) *q.ransac_summary = results[p].summary;
    if (!results[p].ok) continue;
    *q.relative_camera2_position = results[p].position;
    success[which[p]] = true;
  }
  return success;
}

bool EstimateRelativePoseWithKnownOrientation(const RansacParameters& ransac_params, const RansacType& ransac_type,
                                              const std::vector<FeatureCorrespondence>& rotated_correspondences,
                                              Eigen::Vector3d* relative_camera2_position,
                                              RansacSummary* ransac_summary) {
  KnownOrientationRelativeProblem q;  // (zero orientations: the correspondences are already rotated)
  q.correspondences = &rotated_correspondences;
  q.relative_camera2_position = relative_camera2_position;
  q.ransac_summary = ransac_summary;
  return EstimateRelativePosesWithKnownOrientation(ransac_params, ransac_type, {q})[0];
}

}  // namespace theia
