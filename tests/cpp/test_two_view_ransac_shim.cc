// The two-view RANSAC shim (theiasfm_amd/host/two_view_ransac_ops.cc): the signatures and defaults against the
// reference's, the calibrated-branch and non-RANSAC refusals, without a device false with the outputs untouched, and
// with one (--need-device) the estimate on a noise-free pair, visibility_score == 0 and batched == one-by-one.
// Stand-alone: its own main.
#include <cmath>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "theia/sfm/estimate_twoview_info.h"
#include "theia/sfm/estimators/estimate_uncalibrated_relative_pose.h"
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

// the reference's signatures
static_assert(std::is_same<decltype(&EstimateUncalibratedRelativePose),
                           bool (*)(const RansacParameters&, const RansacType&, const std::vector<FeatureCorrespondence>&,
                                    UncalibratedRelativePose*, RansacSummary*)>::value, "signature");
static_assert(std::is_same<decltype(&EstimateTwoViewInfo),
                           bool (*)(const EstimateTwoViewInfoOptions&, const CameraIntrinsicsPrior&,
                                    const CameraIntrinsicsPrior&, const std::vector<FeatureCorrespondence>&, TwoViewInfo*,
                                    std::vector<int>*)>::value, "signature");

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

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::string(argv[1]) == "--need-device";
  // defaults: estimate_twoview_info.h:55-72, create_and_initialize_ransac_variant.h:51-56
  EstimateTwoViewInfoOptions options;
  CHECK(options.ransac_type == RansacType::RANSAC && options.max_sampson_error_pixels == 6.0);
  CHECK(options.expected_ransac_confidence == 0.9999 && options.min_ransac_iterations == 10);
  CHECK(options.max_ransac_iterations == 1000 && options.use_mle == true && options.rng == nullptr);
  CHECK(static_cast<int>(RansacType::PROSAC) == 1 && static_cast<int>(RansacType::LMED) == 2 &&
        static_cast<int>(RansacType::EXHAUSTIVE) == 3);
  tmi_ba_two_view_ransac_options c_options;
  tmi_ba_two_view_ransac_options_init(&c_options);
  CHECK(c_options.min_iterations == 10 && c_options.max_iterations == 1000 && c_options.failure_probability == 0.01);

  CameraIntrinsicsPrior prior1, prior2;
  prior1.image_width = prior2.image_width = 1024;
  prior1.image_height = prior2.image_height = 768;
  const std::vector<FeatureCorrespondence> pairA = MakePair(120, 900.0, 1250.0, 0.25, 20);
  const std::vector<FeatureCorrespondence> pairB = MakePair(70, 1100.0, 820.0, -0.3, 0);

  // the refusals: nothing is written
  {
    TwoViewInfo info;
    info.focal_length_1 = -7.0;
    std::vector<int> inliers = {42};
    CameraIntrinsicsPrior k1 = prior1, k2 = prior2;
    k1.focal_length.is_set = k2.focal_length.is_set = true;
    k1.focal_length.value[0] = 900.0;
    k2.focal_length.value[0] = 1250.0;
    CHECK(!EstimateTwoViewInfo(options, k1, k2, pairA, &info, &inliers));  // the calibrated branch
    CHECK(info.focal_length_1 == -7.0 && inliers.size() == 1 && inliers[0] == 42);
    EstimateTwoViewInfoOptions prosac = options;
    prosac.ransac_type = RansacType::PROSAC;
    CHECK(!EstimateTwoViewInfo(prosac, prior1, prior2, pairA, &info, &inliers));
    CHECK(info.focal_length_1 == -7.0 && inliers.size() == 1);
    RansacParameters rp;
    rp.error_thresh = 36.0;
    rp.max_iterations = 1000;
    UncalibratedRelativePose pose;
    pose.focal_length1 = -3.0;
    RansacSummary rs;
    CHECK(!EstimateUncalibratedRelativePose(rp, RansacType::LMED, pairA, &pose, &rs));
    rp.use_mle = true;
    CHECK(!EstimateUncalibratedRelativePose(rp, RansacType::RANSAC, pairA, &pose, &rs));
    CHECK(pose.focal_length1 == -3.0 && rs.inliers.empty());
  }
  int ndev = 0;
  {
    // (a call with an empty batch reaches the device check: TMI_BA_ERR_NO_DEVICE without one)
    tmi_ba_two_view_ransac_summary s;
    const int64_t zero = 0;
    ndev = tmi_ba_estimate_uncalibrated_relative_poses(&c_options, 0, &zero, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                       &s) == TMI_BA_OK;
  }
  if (!ndev) {
    CHECK(!need_device);
    TwoViewInfo info;
    std::vector<int> inliers;
    CHECK(!EstimateTwoViewInfo(options, prior1, prior2, pairA, &info, &inliers));
    CHECK(info.focal_length_1 == 0.0 && inliers.empty());
    std::printf(g_failed ? "two-view ransac shim: FAILED\n" : "two-view ransac shim: OK\n");
    return g_failed ? 1 : 0;
  }
  // on the device
  TwoViewInfo infoA, infoB;
  std::vector<int> inliersA = {5}, inliersB;
  infoA.visibility_score = 99;
  CHECK(EstimateTwoViewInfo(options, prior1, prior2, pairA, &infoA, &inliersA));
  CHECK(EstimateTwoViewInfo(options, prior1, prior2, pairB, &infoB, &inliersB));
  CHECK(infoA.visibility_score == 0 && infoB.visibility_score == 0);
  CHECK(infoA.num_verified_matches == static_cast<int>(inliersA.size()) && inliersA.size() >= 100 && inliersA[0] >= 20);
  CHECK(inliersB.size() == 70);
  // fundamental_matrix_util_test.cc:55: 1e-6 on noise-free data
  CHECK(std::fabs(infoA.focal_length_1 - 900.0) < 1e-6 && std::fabs(infoA.focal_length_2 - 1250.0) < 1e-6);
  CHECK(std::fabs(infoB.focal_length_1 - 1100.0) < 1e-6 && std::fabs(infoB.focal_length_2 - 820.0) < 1e-6);
  const double pn = std::sqrt(1.0 + 0.16 + 0.04);
  CHECK(std::fabs(infoA.position_2[0] - 1.0 / pn) < 1e-6 && std::fabs(infoA.position_2[1] - 0.4 / pn) < 1e-6);
  // batched == one-by-one, bit for bit
  {
    TwoViewInfo bA, bB;
    std::vector<int> iA, iB;
    TwoViewInfoProblem qA, qB;
    qA.intrinsics1 = qB.intrinsics1 = &prior1;
    qA.intrinsics2 = qB.intrinsics2 = &prior2;
    qA.correspondences = &pairA;
    qB.correspondences = &pairB;
    qA.twoview_info = &bA;
    qB.twoview_info = &bB;
    qA.inlier_indices = &iA;
    qB.inlier_indices = &iB;
    const std::vector<bool> ok = EstimateTwoViewInfos(options, {qA, qB});
    CHECK(ok.size() == 2 && ok[0] && ok[1] && iA == inliersA && iB == inliersB);
    for (int i = 0; i < 3; ++i) {
      CHECK(bA.rotation_2[i] == infoA.rotation_2[i] && bA.position_2[i] == infoA.position_2[i]);
      CHECK(bB.rotation_2[i] == infoB.rotation_2[i] && bB.position_2[i] == infoB.position_2[i]);
    }
    CHECK(bA.focal_length_1 == infoA.focal_length_1 && bB.focal_length_2 == infoB.focal_length_2);
  }
  // EstimateUncalibratedRelativePose on centred pixels
  {
    std::vector<FeatureCorrespondence> centred = pairB;
    for (auto& c : centred) {
      c.feature1 = Feature(c.feature1.x() - 512, c.feature1.y() - 384);
      c.feature2 = Feature(c.feature2.x() - 512, c.feature2.y() - 384);
    }
    RansacParameters rp;
    rp.error_thresh = 36.0;
    rp.failure_probability = 1.0 - 0.9999;
    rp.min_iterations = 10;
    rp.max_iterations = 1000;
    UncalibratedRelativePose pose;
    RansacSummary rs;
    CHECK(EstimateUncalibratedRelativePose(rp, RansacType::RANSAC, centred, &pose, &rs));
    CHECK(pose.focal_length1 == infoB.focal_length_1 && pose.focal_length2 == infoB.focal_length_2);
    CHECK(rs.inliers.size() == 70 && rs.num_input_data_points == 70 && rs.num_iterations >= 10);
    double det = 0.0;
    const Eigen::Matrix3d& R = pose.rotation;
    det = R(0, 0) * (R(1, 1) * R(2, 2) - R(1, 2) * R(2, 1)) - R(0, 1) * (R(1, 0) * R(2, 2) - R(1, 2) * R(2, 0)) +
          R(0, 2) * (R(1, 0) * R(2, 1) - R(1, 1) * R(2, 0));
    CHECK(std::fabs(det - 1.0) < 1e-12);
  }
  std::printf(g_failed ? "two-view ransac shim: FAILED\n" : "two-view ransac shim: OK (device)\n");
  return g_failed ? 1 : 0;
}
