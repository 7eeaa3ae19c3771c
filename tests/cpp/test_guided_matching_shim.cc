// The guided matching shim (theiasfm_amd/host/guided_match_ops.cc): the defaults against the reference's header, the
// projection and fundamental matrices of two typed cameras (printed for tests/test_host_shim_guided_matching.py, which
// holds them against the model's), without a device false with the vector untouched, and with one (--need-device) the
// single call against the batched call, matches appended and the result against the C ABI's.  Stand-alone: its own main.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "theia/matching/guided_epipolar_matcher.h"
#include "theia_mi355_ba.h"

using theia::Camera;
using theia::GuidedEpipolarMatcher;
using theia::IndexedFeatureMatch;
using theia::KeypointsAndDescriptors;

static int g_failed = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                   \
    }                                                               \
  } while (0)

static const int kNumPoints = 150, kNumGiven = 90, kDim = 16;

static unsigned long long g_state = 12345;
static double Uniform() {  // a 48-bit linear congruential generator: the same numbers on every machine
  g_state = (g_state * 25214903917ull + 11ull) & ((1ull << 48) - 1);
  return (double)g_state / (double)(1ull << 48);
}

static Camera MakeCamera(double px, double py, double pz, double ax, double ay, double az) {
  Camera camera;
  camera.SetFocalLength(800.0);
  camera.SetPrincipalPoint(512.0, 384.0);
  camera.SetPosition(Eigen::Vector3d(px, py, pz));
  camera.SetOrientationFromAngleAxis(Eigen::Vector3d(ax, ay, az));
  return camera;
}

// The features of the scene's points in `camera`, point i as feature order[i]; descriptors: the point's own plus noise.
static KeypointsAndDescriptors Features(const Camera& camera, const std::vector<double>& points,
                                        const std::vector<float>& base, int shift) {
  double P[12];
  theia::GuidedMatchProjectionMatrix(camera, P);
  KeypointsAndDescriptors f;
  f.keypoints.resize(kNumPoints);
  f.descriptors.resize(kNumPoints);
  for (int i = 0; i < kNumPoints; ++i) {
    const double* X = &points[3 * i];
    double x[3];
    for (int r = 0; r < 3; ++r) x[r] = P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2] + P[4 * r + 3];
    const int j = (i + shift) % kNumPoints;
    f.keypoints[j] = theia::Keypoint(x[0] / x[2] + 0.4 * (Uniform() - 0.5), x[1] / x[2] + 0.4 * (Uniform() - 0.5),
                                     theia::Keypoint::SIFT);
    Eigen::VectorXf d(kDim);
    for (int k = 0; k < kDim; ++k) d(k) = base[kDim * i + k] + (float)(0.02 * (Uniform() - 0.5));
    f.descriptors[j] = d;
  }
  return f;
}

static bool Same(const std::vector<IndexedFeatureMatch>& a, const std::vector<IndexedFeatureMatch>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].feature1_ind != b[i].feature1_ind || a[i].feature2_ind != b[i].feature2_ind ||
        std::memcmp(&a[i].distance, &b[i].distance, sizeof(float)) != 0)
      return false;
  return true;
}

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  // the defaults of guided_epipolar_matcher.h:56-70 and of the C ABI
  GuidedEpipolarMatcher::Options options;
  CHECK(options.guided_matching_max_distance_pixels == 2.0 && options.lowes_ratio == 0.8);
  CHECK(options.seed == 0 && options.device == -1);
  tmi_ba_guided_match_options c;
  tmi_ba_guided_match_options_init(&c);
  CHECK(c.guided_matching_max_distance_pixels == 2.0 && c.lowes_ratio == 0.8 && c.min_num_candidates == 50);
  CHECK(c.device == -1 && c.seed == 0);

  // three cameras; their matrices go to the Python side
  const Camera cameras[3] = {MakeCamera(0, 0, 0, 0, 0, 0), MakeCamera(1.0, 0.1, 0.2, 0.01, -0.02, 0.015),
                             MakeCamera(-0.7, 0.2, -0.1, -0.02, 0.03, 0.01)};
  for (int m = 0; m < 3; ++m) {
    double P[12];
    theia::GuidedMatchProjectionMatrix(cameras[m], P);
    std::printf("P%d:", m);
    for (double v : P) std::printf(" %.17g", v);
    std::printf("\n");
  }
  for (int m = 1; m < 3; ++m) {
    double F[9];
    theia::GuidedMatchFundamentalMatrix(cameras[0], cameras[m], F);
    std::printf("F0%d:", m);
    for (double v : F) std::printf(" %.17g", v);
    std::printf("\n");
  }

  std::vector<double> points(3 * kNumPoints);
  std::vector<float> base(kDim * kNumPoints);
  for (int i = 0; i < kNumPoints; ++i) {
    points[3 * i] = 4.0 * Uniform() - 2.0;
    points[3 * i + 1] = 2.8 * Uniform() - 1.4;
    points[3 * i + 2] = 6.0 + 4.0 * Uniform();
    double n = 0;
    for (int k = 0; k < kDim; ++k) {
      base[kDim * i + k] = (float)(Uniform() - 0.5);
      n += (double)base[kDim * i + k] * base[kDim * i + k];
    }
    for (int k = 0; k < kDim; ++k) base[kDim * i + k] /= (float)std::sqrt(n);
  }
  const int shifts[3] = {0, 17, 53};
  std::vector<KeypointsAndDescriptors> features;
  for (int m = 0; m < 3; ++m) features.push_back(Features(cameras[m], points, base, shifts[m]));
  auto given = [&](int a, int b) {  // the true matches of the first kNumGiven points
    std::vector<IndexedFeatureMatch> matches;
    for (int i = 0; i < kNumGiven; ++i)
      matches.emplace_back((i + shifts[a]) % kNumPoints, (i + shifts[b]) % kNumPoints, 0.25f);
    return matches;
  };
  const std::vector<std::pair<int, int>> pairs = {{0, 1}, {0, 2}, {2, 1}, {1, 0}};
  const std::vector<const KeypointsAndDescriptors*> images = {&features[0], &features[1], &features[2]};
  const std::vector<const Camera*> camera_of = {&cameras[0], &cameras[1], &cameras[2]};

  // single calls
  std::vector<std::vector<IndexedFeatureMatch>> single;
  std::vector<bool> single_ok;
  for (const auto& p : pairs) {
    single.push_back(given(p.first, p.second));
    GuidedEpipolarMatcher matcher(options, cameras[p.first], cameras[p.second], features[p.first], features[p.second]);
    single_ok.push_back(matcher.GetMatches(&single.back()));
  }
  // the batched call
  std::vector<std::vector<IndexedFeatureMatch>> batched;
  for (const auto& p : pairs) batched.push_back(given(p.first, p.second));
  const bool batched_ok = theia::GuidedEpipolarMatches(options, images, pairs, camera_of, &batched);

  // empty descriptors, sizes that do not agree: false and untouched, with or without a device
  {
    KeypointsAndDescriptors empty;
    std::vector<IndexedFeatureMatch> matches = given(0, 1);
    GuidedEpipolarMatcher matcher(options, cameras[0], cameras[1], features[0], empty);
    CHECK(!matcher.GetMatches(&matches) && Same(matches, given(0, 1)));
    std::vector<std::vector<IndexedFeatureMatch>> too_few(1);
    CHECK(!theia::GuidedEpipolarMatches(options, images, pairs, camera_of, &too_few) && too_few.size() == 1 && too_few[0].empty());
    std::vector<std::vector<IndexedFeatureMatch>> four(4, given(0, 1));
    CHECK(!theia::GuidedEpipolarMatches(options, images, {{0, 1}, {0, 3}, {0, 1}, {0, 1}}, camera_of, &four));
    for (const auto& m : four) CHECK(Same(m, given(0, 1)));
  }

  if (!need_device) {
    if (tmi_ba_device_count() <= 0) {  // false, and the vectors are as they were
      for (size_t p = 0; p < pairs.size(); ++p) {
        CHECK(!single_ok[p]);
        CHECK(Same(single[p], given(pairs[p].first, pairs[p].second)));
        CHECK(Same(batched[p], given(pairs[p].first, pairs[p].second)));
      }
      CHECK(!batched_ok);
    }
    std::printf(g_failed ? "guided matching shim: %d FAILED\n" : "guided matching shim: OK\n", g_failed);
    return g_failed ? 1 : 0;
  }

  CHECK(batched_ok);
  size_t added = 0;
  for (size_t p = 0; p < pairs.size(); ++p) {
    CHECK(single_ok[p]);
    CHECK(Same(single[p], batched[p]));  // single call == batched call
    const std::vector<IndexedFeatureMatch> before = given(pairs[p].first, pairs[p].second);
    CHECK(single[p].size() > before.size() + 20);  // appended, not replaced: the input matches come first, unchanged
    CHECK(Same(std::vector<IndexedFeatureMatch>(single[p].begin(), single[p].begin() + before.size()), before));
    added += single[p].size() - before.size();
  }
  // the C ABI on the same arrays: pair 0 alone, stream 0
  {
    const int n = kNumPoints;
    std::vector<float> desc(2 * (size_t)n * kDim);
    std::vector<double> keys(4 * (size_t)n);
    for (int m = 0; m < 2; ++m)
      for (int i = 0; i < n; ++i) {
        for (int k = 0; k < kDim; ++k) desc[((size_t)m * n + i) * kDim + k] = features[m].descriptors[i](k);
        keys[2 * ((size_t)m * n + i)] = features[m].keypoints[i].x();
        keys[2 * ((size_t)m * n + i) + 1] = features[m].keypoints[i].y();
      }
    const int64_t image_begin[3] = {0, n, 2 * n};
    const int32_t i1 = 0, i2 = 1;
    double F[9];
    theia::GuidedMatchFundamentalMatrix(cameras[0], cameras[1], F);
    const std::vector<IndexedFeatureMatch> in = given(0, 1);
    std::vector<int32_t> m1, m2;
    for (const auto& m : in) {
      m1.push_back(m.feature1_ind);
      m2.push_back(m.feature2_ind);
    }
    const int64_t match_begin[2] = {0, (int64_t)in.size()};
    int8_t status = 9;
    int32_t groups = 0;
    int64_t begin[2] = {0, 0};
    std::vector<int32_t> f1(n), f2(n);
    std::vector<float> dist(n);
    tmi_ba_guided_match_summary summary;
    const int rc = tmi_ba_guided_epipolar_match(&c, 2, image_begin, desc.data(), kDim, keys.data(), 1, &i1, &i2, F, match_begin,
                                                m1.data(), m2.data(), nullptr, nullptr, n, &status, &groups, begin, f1.data(),
                                                f2.data(), dist.data(), nullptr, nullptr, nullptr, &summary);
    CHECK(rc == TMI_BA_OK && status == 0 && groups > 0);
    std::vector<IndexedFeatureMatch> abi = in;
    for (int64_t i = begin[0]; i < begin[1]; ++i) abi.emplace_back(f1[i], f2[i], dist[i]);
    CHECK(Same(abi, single[0]));
  }
  std::printf("guided matching shim: added %zu matches over %zu pairs\n", added, pairs.size());
  std::printf(g_failed ? "guided matching shim: %d FAILED\n" : "guided matching shim: OK (device)\n", g_failed);
  return g_failed ? 1 : 0;
}
