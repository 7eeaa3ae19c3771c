// The known-orientation shims (theiasfm_amd/host/known_orientation_ops.cc): the signatures against the reference's, the
// refusals with the outputs untouched, without a device false with the outputs untouched, and with one (--need-device)
// the scenes of the reference's estimator tests within the reference's bounds, and the batched forms equal to the
// one-by-one forms.  Stand-alone: its own main.
#include <cmath>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "theia/sfm/estimators/estimate_absolute_pose_with_known_orientation.h"
#include "theia/sfm/estimators/estimate_relative_pose_with_known_orientation.h"
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

// the reference's signatures (estimate_absolute_pose_with_known_orientation.h:56-62,
// estimate_relative_pose_with_known_orientation.h:54-59)
static_assert(std::is_same<decltype(&EstimateAbsolutePoseWithKnownOrientation),
                           bool (*)(const RansacParameters&, const RansacType&, const Eigen::Vector3d&,
                                    const std::vector<FeatureCorrespondence2D3D>&, Eigen::Vector3d*,
                                    RansacSummary*)>::value, "signature");
static_assert(std::is_same<decltype(&EstimateRelativePoseWithKnownOrientation),
                           bool (*)(const RansacParameters&, const RansacType&, const std::vector<FeatureCorrespondence>&,
                                    Eigen::Vector3d*, RansacSummary*)>::value, "signature");

static unsigned long long g_state = 66;
static double Uniform(double lo, double hi) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (static_cast<double>(g_state >> 11) / 9007199254740992.0);
}

static const double kAngle = 12.0 * 3.14159265358979323846 / 180.0;  // about y: R = [c 0 s; 0 1 0; -s 0 c]

// estimate_absolute_pose_with_known_orientation_test.cc:69-100: 100 points in [-2, 2]^2 x [6, 10], the first
// inlier_ratio * 100 projected by R (X - position), the others uniform in [-1, 1]^2, uniform noise of `noise` pixels at
// focal 1000.
static std::vector<FeatureCorrespondence2D3D> AbsoluteScene(const double position[3], double inlier_ratio, double noise) {
  std::vector<FeatureCorrespondence2D3D> out;
  const double c = std::cos(kAngle), s = std::sin(kAngle);
  for (int i = 0; i < 100; ++i) {
    FeatureCorrespondence2D3D fc;
    fc.world_point = Eigen::Vector3d(Uniform(-2, 2), Uniform(-2, 2), Uniform(6, 10));
    const double d[3] = {fc.world_point[0] - position[0], fc.world_point[1] - position[1], fc.world_point[2] - position[2]};
    const double q[3] = {c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]};
    fc.feature = i < inlier_ratio * 100 ? Eigen::Vector2d(q[0] / q[2], q[1] / q[2])
                                        : Eigen::Vector2d(Uniform(-1, 1), Uniform(-1, 1));
    fc.feature.x() += Uniform(-noise, noise) / 1000.0;
    fc.feature.y() += Uniform(-noise, noise) / 1000.0;
    out.push_back(fc);
  }
  return out;
}

// estimate_relative_pose_with_known_orientation_test.cc:69-103: the features of both views in ONE frame (already
// rotated): X and X - position, hnormalized.
static std::vector<FeatureCorrespondence> RelativeScene(const double position[3], double inlier_ratio, double noise) {
  std::vector<FeatureCorrespondence> out;
  for (int i = 0; i < 100; ++i) {
    const double X[3] = {Uniform(-2, 2), Uniform(-2, 2), Uniform(6, 10)};
    const double Y[3] = {X[0] - position[0], X[1] - position[1], X[2] - position[2]};
    FeatureCorrespondence fc(Feature(X[0] / X[2], X[1] / X[2]), Feature(Y[0] / Y[2], Y[1] / Y[2]));
    if (!(i < inlier_ratio * 100)) {
      fc.feature1 = Feature(Uniform(-1, 1), Uniform(-1, 1));
      fc.feature2 = Feature(Uniform(-1, 1), Uniform(-1, 1));
    }
    fc.feature1.x() += Uniform(-noise, noise) / 1000.0;
    fc.feature1.y() += Uniform(-noise, noise) / 1000.0;
    fc.feature2.x() += Uniform(-noise, noise) / 1000.0;
    fc.feature2.y() += Uniform(-noise, noise) / 1000.0;
    out.push_back(fc);
  }
  return out;
}

// test::ArraysEqualUpToScale (test/test_utils.h:76-85)
static bool EqualUpToScale(const double p[3], const Eigen::Vector3d& q, double tolerance) {
  const double dot = p[0] * q[0] + p[1] * q[1] + p[2] * q[2];
  const double np = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]), nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  return std::fabs(dot / (np * nq)) >= 1.0 - tolerance;
}

static bool SameSummary(const RansacSummary& a, const RansacSummary& b) {
  return a.inliers == b.inliers && a.num_iterations == b.num_iterations && a.confidence == b.confidence &&
         a.num_input_data_points == b.num_input_data_points;
}

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::string(argv[1]) == "--need-device";
  const double positions[2][3] = {{-1.3, 0.0, 0.0}, {0.0, 0.0, 0.5}};
  const Eigen::Vector3d orientation(0.0, kAngle, 0.0);
  RansacParameters rp;  // :128-132 of both test files
  rp.use_mle = true;
  rp.error_thresh = 16.0 / (1000.0 * 1000.0);
  rp.failure_probability = 0.001;
  // (inlier ratio, noise, tolerance) of the four tests of each file
  const double variants[4][3] = {{1.0, 0.0, 1e-4}, {1.0, 1.0, 1e-2}, {0.7, 0.0, 1e-2}, {0.7, 1.0, 1e-2}};
  const std::vector<FeatureCorrespondence2D3D> abs0 = AbsoluteScene(positions[0], 1.0, 0.0);
  const std::vector<FeatureCorrespondence> rel0 = RelativeScene(positions[0], 1.0, 0.0);

  // the refusals: nothing is written
  {
    Eigen::Vector3d c(-7.0, -7.0, -7.0);
    RansacSummary rs;
    rs.num_iterations = 42;
    rs.inliers = {3};
    const RansacType refused[3] = {RansacType::PROSAC, RansacType::LMED, RansacType::EXHAUSTIVE};
    for (const RansacType type : refused) {
      CHECK(!EstimateAbsolutePoseWithKnownOrientation(rp, type, orientation, abs0, &c, &rs));
      CHECK(!EstimateRelativePoseWithKnownOrientation(rp, type, rel0, &c, &rs));
    }
    RansacParameters tdd = rp;
    tdd.use_Tdd_test = true;
    CHECK(!EstimateAbsolutePoseWithKnownOrientation(tdd, RansacType::RANSAC, orientation, abs0, &c, &rs));
    CHECK(!EstimateRelativePoseWithKnownOrientation(tdd, RansacType::RANSAC, rel0, &c, &rs));
    CHECK(!EstimateAbsolutePoseWithKnownOrientation(rp, RansacType::RANSAC, orientation, abs0, nullptr, &rs));
    CHECK(!EstimateRelativePoseWithKnownOrientation(rp, RansacType::RANSAC, rel0, nullptr, &rs));
    KnownOrientationAbsoluteProblem qa;
    qa.normalized_correspondences = &abs0;
    qa.camera_position = &c;
    qa.ransac_summary = &rs;
    const std::vector<bool> ok = EstimateAbsolutePosesWithKnownOrientation(rp, RansacType::LMED, {qa, qa});
    CHECK(ok.size() == 2 && !ok[0] && !ok[1]);
    for (int i = 0; i < 3; ++i) CHECK(c[i] == -7.0);
    CHECK(rs.num_iterations == 42 && rs.inliers.size() == 1 && rs.inliers[0] == 3);
  }
  int ndev = 0;
  {
    // (a call with an empty batch reaches the device check: TMI_BA_ERR_NO_DEVICE without one)
    tmi_ba_homography_ransac_options o;
    tmi_ba_homography_ransac_options_init(&o);
    tmi_ba_two_view_ransac_summary s;
    const int64_t zero = 0;
    const int rc = tmi_ba_estimate_positions_known_orientation(
        &o, 0, &zero, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &s);
    CHECK(rc == TMI_BA_OK || rc == TMI_BA_ERR_NO_DEVICE);
    ndev = rc == TMI_BA_OK;
  }
  if (!ndev) {
    CHECK(!need_device);
    Eigen::Vector3d c(-7.0, -7.0, -7.0);
    RansacSummary rs;
    rs.num_iterations = 42;
    CHECK(!EstimateAbsolutePoseWithKnownOrientation(rp, RansacType::RANSAC, orientation, abs0, &c, &rs));
    CHECK(!EstimateRelativePoseWithKnownOrientation(rp, RansacType::RANSAC, rel0, &c, &rs));
    for (int i = 0; i < 3; ++i) CHECK(c[i] == -7.0);
    CHECK(rs.num_iterations == 42 && rs.inliers.empty());
    std::printf(g_failed ? "known orientation shim: FAILED\n" : "known orientation shim: OK\n");
    return g_failed ? 1 : 0;
  }
  // on the device: the reference's scenes within the reference's bounds, one by one and batched
  std::vector<std::vector<FeatureCorrespondence2D3D>> abs_scenes;
  std::vector<std::vector<FeatureCorrespondence>> rel_scenes;
  std::vector<Eigen::Vector3d> abs_single, rel_single;
  std::vector<RansacSummary> abs_summary, rel_summary;
  for (const auto& v : variants)
    for (const auto& pos : positions) {
      abs_scenes.push_back(AbsoluteScene(pos, v[0], v[1]));
      rel_scenes.push_back(RelativeScene(pos, v[0], v[1]));
      Eigen::Vector3d c, t;
      RansacSummary rs, rt;
      CHECK(EstimateAbsolutePoseWithKnownOrientation(rp, RansacType::RANSAC, orientation, abs_scenes.back(), &c, &rs));
      CHECK(rs.inliers.size() > 3 && rs.num_input_data_points == 100 && rs.num_iterations >= 100);
      CHECK(EqualUpToScale(pos, c, v[2]));
      CHECK(EstimateRelativePoseWithKnownOrientation(rp, RansacType::RANSAC, rel_scenes.back(), &t, &rt));
      CHECK(rt.inliers.size() > 3 && rt.num_input_data_points == 100 && rt.num_iterations >= 100);
      CHECK(EqualUpToScale(pos, t, v[2]));
      CHECK(std::fabs(std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) - 1.0) < 1e-15);
      if (v[0] == 1.0 && v[1] == 0.0) CHECK(rs.inliers.size() == 100 && rt.inliers.size() == 100);
      abs_single.push_back(c);
      rel_single.push_back(t);
      abs_summary.push_back(rs);
      rel_summary.push_back(rt);
    }
  {
    const size_t n = abs_scenes.size();
    std::vector<Eigen::Vector3d> c(n), t(n);
    std::vector<RansacSummary> rs(n), rt(n);
    std::vector<KnownOrientationAbsoluteProblem> qa(n + 1);
    std::vector<KnownOrientationRelativeProblem> qr(n + 1);
    Eigen::Vector3d untouched(-7.0, -7.0, -7.0);
    for (size_t k = 0; k < n; ++k) {
      qa[k].camera_orientation = orientation;
      qa[k].normalized_correspondences = &abs_scenes[k];
      qa[k].camera_position = &c[k];
      qa[k].ransac_summary = &rs[k];
      qr[k].correspondences = &rel_scenes[k];
      qr[k].relative_camera2_position = &t[k];
      qr[k].ransac_summary = &rt[k];
    }
    qa[n].camera_position = &untouched;  // no correspondences: left alone
    qr[n].relative_camera2_position = &untouched;
    const std::vector<bool> oka = EstimateAbsolutePosesWithKnownOrientation(rp, RansacType::RANSAC, qa);
    const std::vector<bool> okr = EstimateRelativePosesWithKnownOrientation(rp, RansacType::RANSAC, qr);
    CHECK(oka.size() == n + 1 && okr.size() == n + 1 && !oka[n] && !okr[n] && untouched[0] == -7.0);
    for (size_t k = 0; k < n; ++k) {
      CHECK(oka[k] && okr[k]);
      for (int i = 0; i < 3; ++i) CHECK(c[k][i] == abs_single[k][i] && t[k][i] == rel_single[k][i]);
      CHECK(SameSummary(rs[k], abs_summary[k]) && SameSummary(rt[k], rel_summary[k]));
    }
    // fewer than two correspondences: false, the summary says so
    const std::vector<FeatureCorrespondence> one(rel0.begin(), rel0.begin() + 1);
    Eigen::Vector3d t1(-7.0, -7.0, -7.0);
    RansacSummary r1;
    CHECK(!EstimateRelativePoseWithKnownOrientation(rp, RansacType::RANSAC, one, &t1, &r1));
    CHECK(t1[0] == -7.0 && r1.num_input_data_points == 1 && r1.inliers.empty());
    // the other scoring is taken from the parameters too
    RansacParameters count = rp;
    count.use_mle = false;
    Eigen::Vector3d c2;
    RansacSummary r2;
    CHECK(EstimateAbsolutePoseWithKnownOrientation(count, RansacType::RANSAC, orientation, abs0, &c2, &r2));
    CHECK(r2.inliers.size() == 100 && EqualUpToScale(positions[0], c2, 1e-4));
  }
  std::printf(g_failed ? "known orientation shim: FAILED\n" : "known orientation shim: OK (device)\n");
  return g_failed ? 1 : 0;
}
