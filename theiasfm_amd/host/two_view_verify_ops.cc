// Host shim of TwoViewMatchGeometricVerification::BundleAdjustRelativePose (reference
// two_view_match_geometric_verification.cc:256-324) on the C ABI: the pairs are flattened into one
// tmi_ba_two_view_batch, verified in one tmi_ba_verify_two_views call and written back for the pairs of status 0 or 4.
#include <cmath>
#include <cstdio>
#include <vector>

#include "theia/sfm/two_view_match_geometric_verification.h"
#include "theia_mi355_ba.h"

namespace theia {

std::vector<bool> BundleAdjustRelativePoseBatch(const TwoViewMatchGeometricVerificationOptions& options,
                                                std::vector<TwoViewVerificationProblem>* problems) {
  std::vector<bool> out;
  if (problems == nullptr || problems->empty()) return out;
  const size_t P = problems->size();
  out.assign(P, false);
  std::vector<double> e1(6 * P, 0.0), e2(6 * P, 0.0), k1(10 * P, 0.0), k2(10 * P, 0.0), f1, f2;
  std::vector<int32_t> m1(P, 0), m2(P, 0);
  std::vector<uint8_t> c1(P, 1), c2(P, 1);
  std::vector<int64_t> ptr(P + 1, 0);
  std::vector<char> valid(P, 0);
  for (size_t p = 0; p < P; ++p) {
    const TwoViewVerificationProblem& q = (*problems)[p];
    ptr[p + 1] = ptr[p];
    // the reference CHECK-fails on null arguments; the shim reports failure (an empty pair: status 1)
    if (!q.camera1 || !q.camera2 || !q.correspondences || !q.info) continue;
    valid[p] = 1;
    for (int a = 0; a < 6; ++a) {
      e1[6 * p + a] = q.camera1->extrinsics()[a];
      e2[6 * p + a] = q.camera2->extrinsics()[a];
    }
    m1[p] = static_cast<int32_t>(q.camera1->GetCameraIntrinsicsModelType());
    m2[p] = static_cast<int32_t>(q.camera2->GetCameraIntrinsicsModelType());
    for (int a = 0; a < q.camera1->CameraIntrinsics()->NumParameters(); ++a) k1[10 * p + a] = q.camera1->intrinsics()[a];
    for (int a = 0; a < q.camera2->CameraIntrinsics()->NumParameters(); ++a) k2[10 * p + a] = q.camera2->intrinsics()[a];
    c1[p] = q.constant_camera1_intrinsics ? 1 : 0;
    c2[p] = q.constant_camera2_intrinsics ? 1 : 0;
    for (const FeatureCorrespondence& m : *q.correspondences) {
      f1.push_back(m.feature1.x());
      f1.push_back(m.feature1.y());
      f2.push_back(m.feature2.x());
      f2.push_back(m.feature2.y());
    }
    ptr[p + 1] = ptr[p] + static_cast<int64_t>(q.correspondences->size());
  }
  std::vector<double> pts(4 * static_cast<size_t>(ptr[P]), 0.0);
  tmi_ba_two_view_batch B;
  B.num_pairs = static_cast<int32_t>(P);
  B.extrinsics1 = e1.data();
  B.extrinsics2 = e2.data();
  B.model1 = m1.data();
  B.model2 = m2.data();
  B.intrinsics1 = k1.data();
  B.intrinsics2 = k2.data();
  B.constant_intrinsics1 = c1.data();
  B.constant_intrinsics2 = c2.data();
  B.correspondence_ptr = ptr.data();
  B.features1 = f1.data();
  B.features2 = f2.data();
  B.points = pts.data();
  tmi_ba_two_view_verification_options vo;
  tmi_ba_two_view_verification_options_init(&vo);
  vo.min_num_inlier_matches = options.min_num_inlier_matches;
  vo.triangulation_max_reprojection_error = options.triangulation_max_reprojection_error;
  vo.min_triangulation_angle_degrees = options.min_triangulation_angle_degrees;
  vo.final_max_reprojection_error = options.final_max_reprojection_error;
  vo.bundle_adjustment = options.bundle_adjustment ? 1 : 0;
  std::vector<int8_t> cst(static_cast<size_t>(ptr[P]) + 1, -1), pst(P, 1);
  tmi_ba_two_view_verification_summary vs;
  const int rc = tmi_ba_verify_two_views(&B, &vo, options.point_dof, /*max_num_iterations=*/200, options.device,
                                         cst.data(), pst.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &vs);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::BundleAdjustRelativePose] device batch failed: %s\n", tmi_ba_last_error());
    return out;  // false everywhere
  }
  for (size_t p = 0; p < P; ++p) {
    if (!valid[p]) continue;
    // BundleAdjustRelativePose returns true once the adjustment succeeded, whatever the last filter leaves (:323);
    // without the adjustment (the extension) the triangulation's own gate decides
    const bool ok = options.bundle_adjustment ? (pst[p] == 0 || pst[p] == 4) : pst[p] == 0;
    if (!ok) continue;
    out[p] = true;
    TwoViewVerificationProblem& q = (*problems)[p];
    if (options.bundle_adjustment) {
      for (int a = 0; a < 6; ++a) q.camera2->mutable_extrinsics()[a] = e2[6 * p + a];
      q.camera1->mutable_intrinsics()[0] = k1[10 * p];
      q.camera2->mutable_intrinsics()[0] = k2[10 * p];
    }
    // :316-321
    double n2 = 0.0;
    for (int a = 0; a < 3; ++a) {
      q.info->rotation_2[a] = e2[6 * p + 3 + a];
      q.info->position_2[a] = e2[6 * p + a];
      n2 += e2[6 * p + a] * e2[6 * p + a];
    }
    if (n2 > 0.0) {
      const double n = std::sqrt(n2);
      for (int a = 0; a < 3; ++a) q.info->position_2[a] /= n;
    }
    q.info->focal_length_1 = k1[10 * p];
    q.info->focal_length_2 = k2[10 * p];
    if (q.inlier_indices) {
      q.inlier_indices->clear();
      for (int64_t i = ptr[p]; i < ptr[p + 1]; ++i)
        if (cst[static_cast<size_t>(i)] == 0) q.inlier_indices->push_back(static_cast<int>(i - ptr[p]));
    }
  }
  return out;
}

bool BundleAdjustRelativePose(const TwoViewMatchGeometricVerificationOptions& options,
                              const TwoViewVerificationProblem& problem) {
  std::vector<TwoViewVerificationProblem> one(1, problem);
  const std::vector<bool> r = BundleAdjustRelativePoseBatch(options, &one);
  return !r.empty() && r[0];
}

}  // namespace theia
