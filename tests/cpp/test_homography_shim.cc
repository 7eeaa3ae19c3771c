// The homography shim (theiasfm_amd/host/homography_ops.cc): the signature and defaults against the reference's, the
// refusals with the outputs untouched, without a device false with the outputs untouched, and with one (--need-device)
// EstimateHomography on the reference's lattice scene, CountHomographyInliers against the C ABI's count for the same
// threshold and the batched form writing TwoViewInfo::num_homography_inliers.  Stand-alone: its own main.
#include <cmath>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "theia/sfm/estimators/estimate_homography.h"
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

// the reference's signature (estimators/estimate_homography.h:57-62)
static_assert(std::is_same<decltype(&EstimateHomography),
                           bool (*)(const RansacParameters&, const RansacType&, const std::vector<FeatureCorrespondence>&,
                                    Eigen::Matrix3d*, RansacSummary*)>::value, "signature");

static unsigned long long g_state = 2024;
static double Uniform(double lo, double hi) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (static_cast<double>(g_state >> 11) / 9007199254740992.0);
}

// estimate_homography_test.cc:65-100 without noise and outliers: the 9x9 lattice at depth 5, view 2 turned about y by
// 12 degrees at position (-1.3, 0, 0); normalised coordinates.
static std::vector<FeatureCorrespondence> Lattice() {
  std::vector<FeatureCorrespondence> out;
  const double a = 12.0 * 3.14159265358979323846 / 180.0, c = std::cos(a), s = std::sin(a);
  // translation = (-R position).normalized() for R = [c 0 s; 0 1 0; -s 0 c], position = (-1.3, 0, 0)
  const double t[3] = {c, 0.0, -s};
  for (int i = -4; i <= 4; ++i)
    for (int j = -4; j <= 4; ++j) {
      const double X[3] = {static_cast<double>(i), static_cast<double>(j), 5.0};
      const double Y[3] = {c * X[0] + s * X[2] + t[0], X[1] + t[1], -s * X[0] + c * X[2] + t[2]};
      out.push_back(FeatureCorrespondence(Feature(X[0] / X[2], X[1] / X[2]), Feature(Y[0] / Y[2], Y[1] / Y[2])));
    }
  return out;
}

// A plane seen by two 1024 x 768 cameras of focal 1000 in pixels; the first `outliers` correspondences are uniform.
static std::vector<FeatureCorrespondence> PlanePixels(int n, double angle, int outliers) {
  std::vector<FeatureCorrespondence> out;
  const double c = std::cos(angle), s = std::sin(angle);
  const double pos[3] = {0.4, -0.1, 0.2};
  while (static_cast<int>(out.size()) < n) {
    const double x = Uniform(-1.5, 1.5), y = Uniform(-1.2, 1.2), z = 5.0 + 0.3 * x + 0.2 * y;
    const double d[3] = {x - pos[0], y - pos[1], z - pos[2]};
    const double q[3] = {c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]};
    FeatureCorrespondence fc(Feature(512 + 1000 * x / z + Uniform(-0.5, 0.5), 384 + 1000 * y / z + Uniform(-0.5, 0.5)),
                             Feature(512 + 1000 * q[0] / q[2] + Uniform(-0.5, 0.5),
                                     384 + 1000 * q[1] / q[2] + Uniform(-0.5, 0.5)));
    if (static_cast<int>(out.size()) < outliers) fc.feature2 = Feature(Uniform(0, 1024), Uniform(0, 768));
    out.push_back(fc);
  }
  return out;
}

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::string(argv[1]) == "--need-device";
  // defaults
  tmi_ba_homography_ransac_options c_options;
  c_options.use_mle = 5;
  tmi_ba_homography_ransac_options_init(&c_options);
  CHECK(c_options.min_iterations == 10 && c_options.max_iterations == 1000 && c_options.failure_probability == 0.01);
  CHECK(c_options.use_mle == 0 && c_options.device == -1 && c_options.seed == 0 && c_options.chunk_iterations == 0);
  EstimateTwoViewInfoOptions options;
  CHECK(options.use_mle == true && options.max_sampson_error_pixels == 6.0);  // MLESAC is what the count runs by default

  const std::vector<FeatureCorrespondence> lattice = Lattice();
  const std::vector<FeatureCorrespondence> pairA = PlanePixels(150, 0.15, 40);
  const std::vector<FeatureCorrespondence> pairB = PlanePixels(60, -0.1, 0);
  RansacParameters rp;  // estimate_homography_test.cc:131-136
  rp.use_mle = true;
  rp.error_thresh = 16.0 / (1000.0 * 1000.0);
  rp.failure_probability = 0.001;

  // the refusals: nothing is written
  {
    Eigen::Matrix3d H;
    for (int i = 0; i < 9; ++i) H.data()[i] = -7.0;
    RansacSummary rs;
    rs.num_iterations = 42;
    rs.inliers = {3};
    const RansacType refused[3] = {RansacType::PROSAC, RansacType::LMED, RansacType::EXHAUSTIVE};
    for (const RansacType type : refused) CHECK(!EstimateHomography(rp, type, lattice, &H, &rs));
    RansacParameters tdd = rp;
    tdd.use_Tdd_test = true;
    CHECK(!EstimateHomography(tdd, RansacType::RANSAC, lattice, &H, &rs));
    CHECK(!EstimateHomography(rp, RansacType::RANSAC, lattice, nullptr, &rs));
    for (int i = 0; i < 9; ++i) CHECK(H.data()[i] == -7.0);
    CHECK(rs.num_iterations == 42 && rs.inliers.size() == 1 && rs.inliers[0] == 3);
    EstimateTwoViewInfoOptions prosac = options;
    prosac.ransac_type = RansacType::PROSAC;
    CHECK(CountHomographyInliers(prosac, 1024, 768, 1024, 768, pairA) == -1);
    TwoViewInfo info;
    info.num_homography_inliers = 17;
    HomographyCountProblem q;
    q.correspondences = &pairA;
    q.info = &info;
    const std::vector<bool> ok = CountHomographyInliersBatch(prosac, {q});
    CHECK(ok.size() == 1 && !ok[0] && info.num_homography_inliers == 17);
  }
  int ndev = 0;
  {
    // (a call with an empty batch reaches the device check: TMI_BA_ERR_NO_DEVICE without one)
    tmi_ba_two_view_ransac_summary s;
    const int64_t zero = 0;
    ndev = tmi_ba_estimate_homographies(&c_options, 0, &zero, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, &s) == TMI_BA_OK;
  }
  if (!ndev) {
    CHECK(!need_device);
    Eigen::Matrix3d H;
    for (int i = 0; i < 9; ++i) H.data()[i] = -7.0;
    RansacSummary rs;
    rs.num_iterations = 42;
    CHECK(!EstimateHomography(rp, RansacType::RANSAC, lattice, &H, &rs));
    for (int i = 0; i < 9; ++i) CHECK(H.data()[i] == -7.0);
    CHECK(rs.num_iterations == 42 && rs.inliers.empty());
    TwoViewInfo info;
    info.num_homography_inliers = 17;
    HomographyCountProblem q;
    q.image_width1 = q.image_width2 = 1024;
    q.image_height1 = q.image_height2 = 768;
    q.correspondences = &pairA;
    q.info = &info;
    const std::vector<bool> ok = CountHomographyInliersBatch(options, {q});
    CHECK(!ok[0] && info.num_homography_inliers == 17);
    CHECK(CountHomographyInliers(options, 1024, 768, 1024, 768, pairA) == -1);
    std::printf(g_failed ? "homography shim: FAILED\n" : "homography shim: OK\n");
    return g_failed ? 1 : 0;
  }
  // on the device: the reference's scene (estimate_homography_test.cc:118-128)
  {
    Eigen::Matrix3d H;
    RansacSummary rs;
    CHECK(EstimateHomography(rp, RansacType::RANSAC, lattice, &H, &rs));
    CHECK(rs.inliers.size() > 4 && rs.inliers.size() == 81 && rs.num_input_data_points == 81);
    CHECK(rs.num_iterations >= 100 && rs.confidence == 1.0);
    // H maps feature1 to feature2
    double worst = 0.0;
    for (const FeatureCorrespondence& c : lattice) {
      const double x = c.feature1.x(), y = c.feature1.y();
      const double p0 = H(0, 0) * x + H(0, 1) * y + H(0, 2), p1 = H(1, 0) * x + H(1, 1) * y + H(1, 2),
                   p2 = H(2, 0) * x + H(2, 1) * y + H(2, 2);
      worst = std::fmax(worst, std::hypot(c.feature2.x() - p0 / p2, c.feature2.y() - p1 / p2));
    }
    std::printf("lattice: worst transfer error %.3e\n", worst);
    CHECK(worst < 1e-9);
    RansacParameters count = rp;
    count.use_mle = false;
    RansacSummary rs2;
    CHECK(EstimateHomography(count, RansacType::RANSAC, lattice, &H, &rs2) && rs2.inliers.size() == 81);
  }
  // CountHomographyInliers == the C ABI's count for the same threshold and options
  int countA = -1, countB = -1;
  {
    countA = CountHomographyInliers(options, 1024, 768, 1024, 768, pairA);
    countB = CountHomographyInliers(options, 1024, 768, 1024, 768, pairB);
    std::printf("homography inliers: %d of 150, %d of 60\n", countA, countB);
    CHECK(countA >= 90 && countA <= 150 && countB >= 50 && countB <= 60);  // 110 and 60 lie on the plane
    tmi_ba_homography_ransac_options o;
    tmi_ba_homography_ransac_options_init(&o);
    o.failure_probability = 1.0 - options.expected_ransac_confidence;
    o.min_iterations = options.min_ransac_iterations;
    o.max_iterations = options.max_ransac_iterations;
    o.use_mle = 1;
    std::vector<double> f1, f2;
    for (const FeatureCorrespondence& c : pairA) {
      f1.push_back(c.feature1.x());
      f1.push_back(c.feature1.y());
      f2.push_back(c.feature2.x());
      f2.push_back(c.feature2.y());
    }
    const int64_t offset[2] = {0, 150};
    const double threshold = 36.0;  // 6 px on either side of a 1024-wide image
    const uint32_t stream = 0;
    int32_t inliers = -1;
    int8_t status = -1;
    tmi_ba_two_view_ransac_summary s;
    CHECK(tmi_ba_estimate_homographies(&o, 1, offset, f1.data(), f2.data(), &threshold, nullptr, &stream, nullptr, 0,
                                       &status, nullptr, &inliers, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, &s) == TMI_BA_OK);
    CHECK(status == 0 && inliers == countA);
    // the two scorings are both taken from the options
    EstimateTwoViewInfoOptions plain = options;
    plain.use_mle = false;
    const int plainA = CountHomographyInliers(plain, 1024, 768, 1024, 768, pairA);
    CHECK(plainA >= 90 && plainA <= 150);
  }
  // the batched form writes num_homography_inliers, equal to one by one
  {
    TwoViewInfo infoA, infoB, infoC;
    infoC.num_homography_inliers = 17;
    HomographyCountProblem qA, qB, qC;
    qA.image_width1 = qA.image_width2 = qB.image_width1 = qB.image_width2 = 1024;
    qA.image_height1 = qA.image_height2 = qB.image_height1 = qB.image_height2 = 768;
    qA.correspondences = &pairA;
    qB.correspondences = &pairB;
    qA.info = &infoA;
    qB.info = &infoB;
    qC.info = &infoC;  // no correspondences: left alone
    const std::vector<bool> ok = CountHomographyInliersBatch(options, {qA, qC, qB});
    CHECK(ok.size() == 3 && ok[0] && !ok[1] && ok[2]);
    CHECK(infoA.num_homography_inliers == countA && infoB.num_homography_inliers == countB);
    CHECK(infoC.num_homography_inliers == 17 && infoA.num_verified_matches == 0);
  }
  std::printf(g_failed ? "homography shim: FAILED\n" : "homography shim: OK (device)\n");
  return g_failed ? 1 : 0;
}
