// The matching shim (theiasfm_amd/host/match_ops.cc): the defaults against the reference's, without a device false and
// empty outputs, and with one (--need-device) the reference's three tests (brute_force_feature_matcher_test.cc) through
// the shim, batch == single calls, and the correspondence helper.  Stand-alone: its own main.
#include <cstdio>
#include <cstring>
#include <vector>

#include "theia/matching/brute_force_feature_matcher.h"
#include "theia_mi355_ba.h"

using theia::BruteForceFeatureMatcher;
using theia::FeatureMatcherOptions;
using theia::IndexedFeatureMatch;
using theia::KeypointsAndDescriptors;
using Eigen::VectorXf;

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

static const int kNumDescriptors = 10;
static const int kNumDescriptorDimensions = 10;

static FeatureMatcherOptions TestOptions(bool symmetric, bool ratio) {
  FeatureMatcherOptions options;
  options.min_num_feature_matches = 0;
  options.keep_only_symmetric_matches = symmetric;
  options.use_lowes_ratio = ratio;
  options.perform_geometric_verification = false;
  return options;
}

static void NoOptionsFeatures(KeypointsAndDescriptors* f1, KeypointsAndDescriptors* f2) {
  for (int i = 0; i < kNumDescriptors; i++) {
    f1->descriptors.push_back(VectorXf::Constant(kNumDescriptorDimensions, 1).normalized());
    f2->descriptors.push_back(VectorXf::Constant(kNumDescriptorDimensions, 1).normalized());
  }
}
static void RatioFeatures(KeypointsAndDescriptors* f1, KeypointsAndDescriptors* f2) {
  f1->descriptors.push_back(VectorXf::Constant(kNumDescriptorDimensions, 1).normalized());
  VectorXf a = VectorXf::Constant(kNumDescriptorDimensions, 1), b = a;
  a(0) = 0.9f;
  b(0) = 0.89f;
  f2->descriptors.push_back(a.normalized());
  f2->descriptors.push_back(b.normalized());
}
static void SymmetricFeatures(KeypointsAndDescriptors* f1, KeypointsAndDescriptors* f2) {
  f1->descriptors.push_back(VectorXf::Constant(kNumDescriptorDimensions, 1).normalized());
  VectorXf e = VectorXf::Constant(kNumDescriptorDimensions, 0);
  e(0) = 1.0f;
  f1->descriptors.push_back(e);
  VectorXf a = VectorXf::Constant(kNumDescriptorDimensions, 1), b = a;
  a(0) = 0;
  b(1) = 0;
  b(2) = 0;
  f2->descriptors.push_back(a.normalized());
  f2->descriptors.push_back(b.normalized());
}
static void AddKeypoints(KeypointsAndDescriptors* f, double offset) {
  for (size_t i = 0; i < f->descriptors.size(); ++i)
    f->keypoints.emplace_back(offset + 10.0 * i, offset + 1.0 + 10.0 * i, theia::Keypoint::SIFT);
}

static bool SameMatches(const std::vector<IndexedFeatureMatch>& a, const std::vector<IndexedFeatureMatch>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].feature1_ind != b[i].feature1_ind || a[i].feature2_ind != b[i].feature2_ind ||
        std::memcmp(&a[i].distance, &b[i].distance, sizeof(float)) != 0)
      return false;
  return true;
}

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  // the defaults of feature_matcher_options.h:45-71 and indexed_feature_match.h
  {
    const FeatureMatcherOptions o;
    CHECK(o.num_threads == 1 && o.keep_only_symmetric_matches && o.use_lowes_ratio && o.lowes_ratio == 0.8f);
    CHECK(o.perform_geometric_verification && o.min_num_feature_matches == 30);
    tmi_ba_match_options c;
    tmi_ba_match_options_init(&c);
    CHECK(c.use_lowes_ratio == 1 && c.lowes_ratio == 0.8f && c.keep_only_symmetric_matches == 1 &&
          c.min_num_feature_matches == 30 && c.device == -1 && c.pairs_per_chunk == 0);
    CHECK(theia::CompareFeaturesByDistance(IndexedFeatureMatch(0, 0, 1.f), IndexedFeatureMatch(0, 0, 2.f)));
    const theia::Keypoint k;
    CHECK(k.keypoint_type() == theia::Keypoint::INVALID && !k.has_scale() && !k.has_strength() && !k.has_orientation());
    VectorXf v = VectorXf::Constant(4, 2.f);
    CHECK(v.size() == 4 && v.squaredNorm() == 16.f && v.normalized()(3) == 0.5f);
  }
  KeypointsAndDescriptors n1, n2, r1, r2, s1, s2;
  NoOptionsFeatures(&n1, &n2);
  RatioFeatures(&r1, &r2);
  SymmetricFeatures(&s1, &s2);
  AddKeypoints(&s1, 100.0);
  AddKeypoints(&s2, 200.0);
  const bool have_device = tmi_ba_device_count() > 0;
  if (!have_device) {
    if (need_device) {
      std::printf("matching shim: no device\n");
      return 2;
    }
    BruteForceFeatureMatcher matcher(TestOptions(false, false));
    std::vector<IndexedFeatureMatch> matches(3);
    CHECK(!matcher.MatchImagePair(n1, n2, &matches) && matches.empty());
    std::vector<std::vector<IndexedFeatureMatch>> per_pair;
    std::vector<bool> ok;
    matcher.MatchImagePairs({&n1, &n2}, {{0, 1}, {1, 0}}, &per_pair, &ok);
    CHECK(per_pair.size() == 2 && per_pair[0].empty() && per_pair[1].empty() && ok.size() == 2 && !ok[0] && !ok[1]);
    std::vector<theia::FeatureCorrespondence> none(2);
    theia::MatchesToFeatureCorrespondences(s1, s2, matches, &none);
    CHECK(none.empty());
    std::printf(g_failed ? "matching shim: FAILED\n" : "matching shim: OK\n");
    return g_failed != 0;
  }
  std::vector<IndexedFeatureMatch> m;
  {  // NoOptions: every row keeps its best; all distances are 0 and the lower column wins
    BruteForceFeatureMatcher matcher(TestOptions(false, false));
    CHECK(matcher.MatchImagePair(n1, n2, &m) && m.size() == 10u);
    for (size_t i = 0; i < m.size(); ++i)
      CHECK(m[i].feature1_ind == static_cast<int>(i) && m[i].feature2_ind == 0 && m[i].distance == 0.f);
  }
  {  // RatioTest: the pair is reported (min 0) and the nearly equidistant candidates leave no match
    BruteForceFeatureMatcher matcher(TestOptions(false, true));
    CHECK(matcher.MatchImagePair(r1, r2, &m) && m.empty());
    FeatureMatcherOptions strict = TestOptions(false, true);
    strict.min_num_feature_matches = 1;
    BruteForceFeatureMatcher matcher1(strict);
    CHECK(!matcher1.MatchImagePair(r1, r2, &m) && m.empty());
  }
  {  // SymmetricMatches: one match, (0, 0); batch == single calls; the correspondences
    BruteForceFeatureMatcher matcher(TestOptions(true, false));
    CHECK(matcher.MatchImagePair(s1, s2, &m) && m.size() == 1u && m[0].feature1_ind == 0 && m[0].feature2_ind == 0);
    std::vector<theia::FeatureCorrespondence> c;
    theia::MatchesToFeatureCorrespondences(s1, s2, m, &c);
    CHECK(c.size() == 1u && c[0].feature1.x() == 100.0 && c[0].feature1.y() == 101.0 && c[0].feature2.x() == 200.0 &&
          c[0].feature2.y() == 201.0);
    const std::vector<const KeypointsAndDescriptors*> images = {&s1, &s2, &n1, &n2, &r1, &r2};
    const std::vector<std::pair<int, int>> pairs = {{0, 1}, {1, 0}, {2, 3}, {4, 5}, {5, 4}, {0, 0}, {2, 0}};
    std::vector<std::vector<IndexedFeatureMatch>> per_pair;
    std::vector<bool> ok;
    matcher.MatchImagePairs(images, pairs, &per_pair, &ok);
    CHECK(per_pair.size() == pairs.size() && ok.size() == pairs.size());
    for (size_t p = 0; p < pairs.size() && p < per_pair.size(); ++p) {
      std::vector<IndexedFeatureMatch> single;
      const bool ok1 = matcher.MatchImagePair(*images[pairs[p].first], *images[pairs[p].second], &single);
      CHECK(ok1 == ok[p] && SameMatches(single, per_pair[p]));
    }
    CHECK(per_pair[0].size() == 1u && per_pair[5].size() == 2u);
  }
  std::printf(g_failed ? "matching shim: FAILED\n" : "matching shim: OK (device)\n");
  return g_failed != 0;
}
