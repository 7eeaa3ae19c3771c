// The host-only builders of the homography shim (theiasfm_amd/host/homography_ops.cc): the squared threshold of
// CountHomographyInliers and the mapping of RansacParameters / EstimateTwoViewInfoOptions onto the C ABI's options.
// Stand-alone (its own main) so that tests/test_homography_cpu.py can run it under the host's sanitizers; no device is
// touched.
#include <cstdio>
#include <limits>

#include "theia/sfm/estimators/estimate_homography.h"

using namespace theia;  // NOLINT

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

int main() {
  EstimateTwoViewInfoOptions options;
  // two_view_match_geometric_verification.cc:334-346: 6 px w.r.t. 1024 on either side, multiplied
  CHECK(HomographyCountThreshold(options, 1024, 768, 1024, 768) == 36.0);
  CHECK(HomographyCountThreshold(options, 2048, 1000, 300, 512) == 12.0 * 3.0);
  CHECK(HomographyCountThreshold(options, 0, 0, 0, 0) == 36.0);  // no image size: the threshold as it is
  CHECK(HomographyCountThreshold(options, 0, 0, 512, 100) == 6.0 * 3.0);
  options.max_sampson_error_pixels = 4.0;
  CHECK(HomographyCountThreshold(options, 768, 1024, 1024, 768) == 16.0);

  // :348-352
  options.expected_ransac_confidence = 0.75;
  options.min_ransac_iterations = 7;
  options.max_ransac_iterations = 333;
  options.seed = 99;
  for (int mle = 0; mle < 2; ++mle) {
    options.use_mle = mle != 0;
    const RansacParameters p = HomographyCountRansacParameters(options, 16.0);
    CHECK(p.error_thresh == 16.0 && p.failure_probability == 0.25 && p.min_iterations == 7 && p.max_iterations == 333);
    CHECK(p.use_mle == (mle != 0) && !p.use_Tdd_test && p.min_inlier_ratio == 0.0 && p.seed == 99);
    tmi_ba_homography_ransac_options o;
    HomographyDeviceOptions(p, 3, &o);
    CHECK(o.failure_probability == 0.25 && o.min_inlier_ratio == 0.0 && o.min_iterations == 7 && o.max_iterations == 333);
    CHECK(o.chunk_iterations == 0 && o.device == 3 && o.seed == 99 && o.use_mle == mle && o.reserved == 0);
  }
  // the reference's default max_iterations is INT_MAX: the C ABI's limit is taken
  {
    RansacParameters p;
    CHECK(p.max_iterations == std::numeric_limits<int>::max() && p.min_iterations == 100 && !p.use_mle);
    tmi_ba_homography_ransac_options o;
    HomographyDeviceOptions(p, -1, &o);
    CHECK(o.max_iterations == (1 << 20) && o.min_iterations == 100 && o.use_mle == 0 && o.device == -1);
    CHECK(o.failure_probability == 0.01);
  }
  std::printf(g_failed ? "homography builders: FAILED\n" : "homography builders: OK\n");
  return g_failed ? 1 : 0;
}
