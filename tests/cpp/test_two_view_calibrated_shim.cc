// The calibrated side of the two-view RANSAC shim (theiasfm_amd/host/two_view_ransac_ops.cc): the signatures and
// defaults against the reference's, use_mle == true / PROSAC / LMED refused with the outputs untouched, without a device
// false with the outputs untouched, and with one (--need-device) calibrated pairs estimated with use_mle = false, the
// focal lengths equal to the priors, batched == one-by-one and a batch that mixes calibrated and uncalibrated pairs.
// Stand-alone: its own main.
#include <cmath>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "theia/sfm/estimate_twoview_info.h"
#include "theia/sfm/estimators/estimate_relative_pose.h"
#include "theia_mi355_ba.h"

using namespace theia;  // NOLINT

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

// the reference's signature (estimators/estimate_relative_pose.h:49-65)
static_assert(std::is_same<decltype(&EstimateRelativePose),
                           bool (*)(const RansacParameters&, const RansacType&, const std::vector<FeatureCorrespondence>&,
                                    RelativePose*, RansacSummary*)>::value, "signature");
static_assert(std::is_same<decltype(RelativePose::essential_matrix), Eigen::Matrix3d>::value &&
              std::is_same<decltype(RelativePose::rotation), Eigen::Matrix3d>::value &&
              std::is_same<decltype(RelativePose::position), Eigen::Vector3d>::value, "RelativePose");

static unsigned long long g_state = 12345;
static double Uniform(double lo, double hi) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (static_cast<double>(g_state >> 11) / 9007199254740992.0);
}

// A noise-free pair in pixels of 1024 x 768 images: view 2 turned about y by `angle` and moved; focal lengths f1, f2.
static std::vector<FeatureCorrespondence> MakePair(int n, double f1, double f2, double angle, int outliers) {
  std::vector<FeatureCorrespondence> out;
  const double c = std::cos(angle), s = std::sin(angle);
  const double pos[3] = {1.0, 0.4, -0.2};
  while (static_cast<int>(out.size()) < n) {
    const double z = Uniform(4, 9), x = Uniform(-0.3, 0.3) * z, y = Uniform(-0.25, 0.25) * z;
    const double d[3] = {x - pos[0], y - pos[1], z - pos[2]};
    const double q[3] = {c * d[0] + s * d[2], d[1] * std::cos(0.1) - (-s * d[0] + c * d[2]) * std::sin(0.1),
                         d[1] * std::sin(0.1) + (-s * d[0] + c * d[2]) * std::cos(0.1)};
    if (q[2] < 1.0) continue;
    FeatureCorrespondence fc(Feature(512 + f1 * x / z, 384 + f1 * y / z), Feature(512 + f2 * q[0] / q[2], 384 + f2 * q[1] / q[2]));
    if (std::fabs(fc.feature2.x() - 512) > 512 || std::fabs(fc.feature2.y() - 384) > 384) continue;
    if (static_cast<int>(out.size()) < outliers)
      fc.feature2 = Feature(Uniform(0, 1024), Uniform(0, 768));
    out.push_back(fc);
  }
  return out;
}

static CameraIntrinsicsPrior Prior(double focal, bool set) {
  CameraIntrinsicsPrior k;
  k.image_width = 1024;
  k.image_height = 768;
  k.focal_length.is_set = set;
  k.focal_length.value[0] = focal;
  return k;
}

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::string(argv[1]) == "--need-device";
  EstimateTwoViewInfoOptions options;
  CHECK(options.use_mle == true && options.ransac_type == RansacType::RANSAC);  // estimate_twoview_info.h:55-72
  EstimateTwoViewInfoOptions count = options;
  count.use_mle = false;
  const CameraIntrinsicsPrior a1 = Prior(900.0, true), a2 = Prior(1250.0, true);
  const CameraIntrinsicsPrior b1 = Prior(1100.0, true), b2 = Prior(820.0, true);
  const CameraIntrinsicsPrior u1 = Prior(0.0, false), u2 = Prior(0.0, false);
  const std::vector<FeatureCorrespondence> pairA = MakePair(120, 900.0, 1250.0, 0.25, 20);
  const std::vector<FeatureCorrespondence> pairB = MakePair(70, 1100.0, 820.0, -0.3, 0);
  std::vector<FeatureCorrespondence> normB = pairB;
  for (auto& c : normB) {
    c.feature1 = Feature((c.feature1.x() - 512) / 1100.0, (c.feature1.y() - 384) / 1100.0);
    c.feature2 = Feature((c.feature2.x() - 512) / 820.0, (c.feature2.y() - 384) / 820.0);
  }
  RansacParameters rp;
  rp.error_thresh = 36.0 / (1100.0 * 820.0);
  rp.failure_probability = 1.0 - 0.9999;
  rp.min_iterations = 10;
  rp.max_iterations = 1000;

  // the refusals: nothing is written
  {
    TwoViewInfo info;
    info.focal_length_1 = -7.0;
    std::vector<int> inliers = {42};
    CHECK(!EstimateTwoViewInfo(options, a1, a2, pairA, &info, &inliers));  // use_mle == true, the default
    CHECK(info.focal_length_1 == -7.0 && inliers.size() == 1 && inliers[0] == 42);
    for (const RansacType type : {RansacType::PROSAC, RansacType::LMED}) {
      EstimateTwoViewInfoOptions other = count;
      other.ransac_type = type;
      CHECK(!EstimateTwoViewInfo(other, a1, a2, pairA, &info, &inliers));
      CHECK(info.focal_length_1 == -7.0 && inliers.size() == 1 && inliers[0] == 42);
    }
    RelativePose pose;
    pose.position[0] = -3.0;
    RansacSummary rs;
    CHECK(!EstimateRelativePose(rp, RansacType::PROSAC, normB, &pose, &rs));
    CHECK(!EstimateRelativePose(rp, RansacType::LMED, normB, &pose, &rs));
    RansacParameters mle = rp;
    mle.use_mle = true;
    CHECK(!EstimateRelativePose(mle, RansacType::RANSAC, normB, &pose, &rs));
    CHECK(pose.position[0] == -3.0 && rs.inliers.empty());
  }
  int ndev = 0;
  {
    // (a call with an empty batch reaches the device check: TMI_BA_ERR_NO_DEVICE without one)
    tmi_ba_two_view_ransac_options c_options;
    tmi_ba_two_view_ransac_options_init(&c_options);
    tmi_ba_two_view_ransac_summary s;
    const int64_t zero = 0;
    ndev = tmi_ba_estimate_calibrated_relative_poses(&c_options, 0, &zero, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                     nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &s) == TMI_BA_OK;
  }
  if (!ndev) {
    CHECK(!need_device);
    TwoViewInfo info;
    info.focal_length_1 = -7.0;
    std::vector<int> inliers;
    CHECK(!EstimateTwoViewInfo(count, a1, a2, pairA, &info, &inliers));
    CHECK(info.focal_length_1 == -7.0 && inliers.empty());
    RelativePose pose;
    pose.position[0] = -3.0;
    CHECK(!EstimateRelativePose(rp, RansacType::RANSAC, normB, &pose, nullptr));
    CHECK(pose.position[0] == -3.0);
    std::printf(g_failed ? "two-view calibrated shim: FAILED\n" : "two-view calibrated shim: OK\n");
    return g_failed ? 1 : 0;
  }
  // on the device
  TwoViewInfo infoA, infoB;
  std::vector<int> inliersA = {5}, inliersB;
  infoA.visibility_score = 99;
  CHECK(EstimateTwoViewInfo(count, a1, a2, pairA, &infoA, &inliersA));
  CHECK(EstimateTwoViewInfo(count, b1, b2, pairB, &infoB, &inliersB));
  CHECK(infoA.visibility_score == 0 && infoB.visibility_score == 0);
  CHECK(infoA.num_verified_matches == static_cast<int>(inliersA.size()) && inliersA.size() >= 100 && inliersA[0] >= 20);
  CHECK(inliersB.size() == 70);
  CHECK(infoA.focal_length_1 == 900.0 && infoA.focal_length_2 == 1250.0);  // the priors (:180-181)
  CHECK(infoB.focal_length_1 == 1100.0 && infoB.focal_length_2 == 820.0);
  const double pn = std::sqrt(1.0 + 0.16 + 0.04);
  CHECK(std::fabs(infoA.position_2[0] - 1.0 / pn) < 1e-6 && std::fabs(infoA.position_2[1] - 0.4 / pn) < 1e-6);
  CHECK(std::fabs(infoB.position_2[0] - 1.0 / pn) < 1e-6 && std::fabs(infoB.position_2[2] + 0.2 / pn) < 1e-6);
  // batched == one-by-one, bit for bit, in a batch that mixes both kinds of pair
  {
    TwoViewInfo uA;
    std::vector<int> uiA;
    CHECK(EstimateTwoViewInfo(count, u1, u2, pairA, &uA, &uiA));  // the same pixels without priors: eight-point
    TwoViewInfo bA, bB, bU;
    std::vector<int> iA, iB, iU;
    TwoViewInfoProblem qA, qB, qU;
    qA.intrinsics1 = &a1;
    qA.intrinsics2 = &a2;
    qB.intrinsics1 = &b1;
    qB.intrinsics2 = &b2;
    qU.intrinsics1 = &u1;
    qU.intrinsics2 = &u2;
    qA.correspondences = qU.correspondences = &pairA;
    qB.correspondences = &pairB;
    qA.twoview_info = &bA;
    qB.twoview_info = &bB;
    qU.twoview_info = &bU;
    qA.inlier_indices = &iA;
    qB.inlier_indices = &iB;
    qU.inlier_indices = &iU;
    const std::vector<bool> ok = EstimateTwoViewInfos(count, {qA, qU, qB});
    CHECK(ok.size() == 3 && ok[0] && ok[1] && ok[2] && iA == inliersA && iB == inliersB && iU == uiA);
    for (int i = 0; i < 3; ++i) {
      CHECK(bA.rotation_2[i] == infoA.rotation_2[i] && bA.position_2[i] == infoA.position_2[i]);
      CHECK(bB.rotation_2[i] == infoB.rotation_2[i] && bB.position_2[i] == infoB.position_2[i]);
      CHECK(bU.rotation_2[i] == uA.rotation_2[i] && bU.position_2[i] == uA.position_2[i]);
    }
    CHECK(bA.focal_length_1 == 900.0 && bB.focal_length_2 == 820.0 && bU.focal_length_1 == uA.focal_length_1);
    CHECK(std::fabs(bU.focal_length_1 - 900.0) < 1e-6);  // estimated, not a prior
  }
  // EstimateRelativePose on normalised correspondences
  {
    RelativePose pose;
    RansacSummary rs;
    CHECK(EstimateRelativePose(rp, RansacType::RANSAC, normB, &pose, &rs));
    CHECK(rs.inliers.size() == 70 && rs.num_input_data_points == 70 && rs.num_iterations >= 10);
    for (int i = 0; i < 3; ++i) CHECK(pose.position[i] == infoB.position_2[i]);
    const Eigen::Matrix3d& R = pose.rotation;
    const double det = R(0, 0) * (R(1, 1) * R(2, 2) - R(1, 2) * R(2, 1)) - R(0, 1) * (R(1, 0) * R(2, 2) - R(1, 2) * R(2, 0)) +
                       R(0, 2) * (R(1, 0) * R(2, 1) - R(1, 1) * R(2, 0));
    CHECK(std::fabs(det - 1.0) < 1e-12);
    double ss = 0.0, worst = 0.0;
    for (int i = 0; i < 9; ++i) ss += pose.essential_matrix.data()[i] * pose.essential_matrix.data()[i];
    CHECK(std::fabs(ss - 1.0) < 1e-12);
    for (const auto& c : normB) {  // x2^T E x1 = 0
      const Eigen::Matrix3d& E = pose.essential_matrix;
      const double x1[3] = {c.feature1.x(), c.feature1.y(), 1.0}, x2[3] = {c.feature2.x(), c.feature2.y(), 1.0};
      double r = 0.0;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r += x2[i] * E(i, j) * x1[j];
      worst = std::fmax(worst, std::fabs(r));
    }
    CHECK(worst < 1e-9);
  }
  std::printf(g_failed ? "two-view calibrated shim: FAILED\n" : "two-view calibrated shim: OK (device)\n");
  return g_failed ? 1 : 0;
}
