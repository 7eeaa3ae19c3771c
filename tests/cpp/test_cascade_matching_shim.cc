// The cascade hashing shim (theiasfm_amd/host/cascade_match_ops.cc): the defaults against the reference's, without a
// device false and empty outputs, and with one (--need-device) the reference's tests
// (cascade_hashing_feature_matcher_test.cc: NoOptions and RatioTest; it has no third) through the shim, batch ==
// single calls, two matchers of one seed, and the correspondence helper.  Stand-alone: its own main.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "theia/matching/brute_force_feature_matcher.h"
#include "theia/matching/cascade_hashing_feature_matcher.h"
#include "theia_mi355_ba.h"

using theia::CascadeHashingFeatureMatcher;
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

// NoOptions: ten copies of one descriptor in both images.  Every row of an image has the same hash, so every row
// meets all ten columns in all six groups (60 candidate incidences > 10): the reference's own size serves.
static void NoOptionsFeatures(KeypointsAndDescriptors* f1, KeypointsAndDescriptors* f2) {
  for (int i = 0; i < kNumDescriptors; i++) {
    f1->descriptors.push_back(VectorXf::Constant(kNumDescriptorDimensions, 1).normalized());
    f2->descriptors.push_back(VectorXf::Constant(kNumDescriptorDimensions, 1).normalized());
  }
}
// RatioTest at the reference's size: one row against two.  At most 12 candidate incidences exist and the lone row's
// centred descriptor is exactly zero (all bits 0) while the two columns' are opposite, so the buckets are too thin
// for any row to be matched: the reference's assertion (the pair is reported, min 0) holds with no match at all and
// says nothing about the ratio test.
static void RatioFeatures(KeypointsAndDescriptors* f1, KeypointsAndDescriptors* f2) {
  f1->descriptors.push_back(VectorXf::Constant(kNumDescriptorDimensions, 1).normalized());
  VectorXf a = VectorXf::Constant(kNumDescriptorDimensions, 1), b = a;
  a(0) = 0.9f;
  b(0) = 0.89f;
  f2->descriptors.push_back(a.normalized());
  f2->descriptors.push_back(b.normalized());
}
// Two scene descriptors u and v, twelve copies of each per image (u first in image 1, v first in image 2).  The
// centred descriptors are +-(u - v) / 2, so the copies of u share every bucket with each other and none with v's
// (unless a projection is exactly 0): 72 incidences per row, twelve columns at Hamming distance 0, eleven of them
// shortlisted, all at distance 0 -- the lowest column wins.  Found with tests/cascade_matching_model.py, not on the
// device.
static void TwoSceneFeatures(KeypointsAndDescriptors* f1, KeypointsAndDescriptors* f2) {
  VectorXf u = VectorXf::Constant(kNumDescriptorDimensions, 1), v = u;
  u(0) = 0.f;
  v(1) = 0.f;
  v(2) = 0.f;
  u.normalize();
  v.normalize();
  for (int i = 0; i < 12; ++i) f1->descriptors.push_back(u);
  for (int i = 0; i < 12; ++i) f1->descriptors.push_back(v);
  for (int i = 0; i < 12; ++i) f2->descriptors.push_back(v);
  for (int i = 0; i < 12; ++i) f2->descriptors.push_back(u);
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
  {  // the defaults of feature_matcher_options.h:45-71, and the ABI's
    const FeatureMatcherOptions o;
    CHECK(o.keep_only_symmetric_matches && o.use_lowes_ratio && o.lowes_ratio == 0.8f && o.min_num_feature_matches == 30);
    tmi_ba_cascade_match_options c;
    tmi_ba_cascade_match_options_init(&c);
    CHECK(c.use_lowes_ratio == 1 && c.lowes_ratio == 0.8f && c.keep_only_symmetric_matches == 1 &&
          c.min_num_feature_matches == 30 && c.device == -1 && c.pairs_per_chunk == 0);
    CascadeHashingFeatureMatcher matcher(TestOptions(true, true));
    CHECK(matcher.seed() == CascadeHashingFeatureMatcher::kDefaultSeed && matcher.projections().empty() &&
          matcher.descriptor_dimension() == 0);
  }
  KeypointsAndDescriptors n1, n2, r1, r2, s1, s2, empty, other;
  NoOptionsFeatures(&n1, &n2);
  RatioFeatures(&r1, &r2);
  TwoSceneFeatures(&s1, &s2);
  AddKeypoints(&s1, 100.0);
  AddKeypoints(&s2, 200.0);
  other.descriptors.push_back(VectorXf::Constant(kNumDescriptorDimensions + 1, 1).normalized());
  {  // the projections: drawn at the first non-empty image, in the order and from the generator the header states
    CascadeHashingFeatureMatcher matcher(TestOptions(false, false), 5u);
    std::vector<IndexedFeatureMatch> m(2);
    CHECK(!matcher.MatchImagePair(empty, empty, &m) && m.empty() && matcher.projections().empty());
    matcher.MatchImagePair(empty, n1, &m);
    CHECK(matcher.descriptor_dimension() == kNumDescriptorDimensions &&
          matcher.projections().size() == 188u * kNumDescriptorDimensions);
    std::mt19937 generator(5u);
    bool same = matcher.projections().size() == 188u * kNumDescriptorDimensions;
    for (size_t i = 0; same && i < matcher.projections().size(); ++i) {
      std::normal_distribution<double> distribution(0.0, 1.0);
      same = matcher.projections()[i] == static_cast<float>(distribution(generator));
    }
    CHECK(same);
    const std::vector<float> before = matcher.projections();
    CHECK(!matcher.MatchImagePair(other, other, &m) && m.empty());  // another dimension later on: false
    CHECK(matcher.projections() == before);
    CascadeHashingFeatureMatcher by_default(TestOptions(false, false));
    by_default.MatchImagePair(n1, n2, &m);
    std::mt19937 g2(CascadeHashingFeatureMatcher::kDefaultSeed);
    std::normal_distribution<double> first(0.0, 1.0);
    CHECK(!by_default.projections().empty() && by_default.projections()[0] == static_cast<float>(first(g2)));
  }
  const bool have_device = tmi_ba_device_count() > 0;
  if (!have_device) {
    if (need_device) {
      std::printf("cascade matching shim: no device\n");
      return 2;
    }
    CascadeHashingFeatureMatcher matcher(TestOptions(false, false));
    std::vector<IndexedFeatureMatch> matches(3);
    CHECK(!matcher.MatchImagePair(n1, n2, &matches) && matches.empty());
    std::vector<std::vector<IndexedFeatureMatch>> per_pair;
    std::vector<bool> ok;
    matcher.MatchImagePairs({&n1, &n2}, {{0, 1}, {1, 0}}, &per_pair, &ok);
    CHECK(per_pair.size() == 2 && per_pair[0].empty() && per_pair[1].empty() && ok.size() == 2 && !ok[0] && !ok[1]);
    FeatureMatcherOptions negative = TestOptions(false, false);
    negative.min_num_feature_matches = -1;
    CascadeHashingFeatureMatcher refuses(negative);
    CHECK(!refuses.MatchImagePair(n1, n2, &matches) && matches.empty());
    std::printf(g_failed ? "cascade matching shim: FAILED\n" : "cascade matching shim: OK\n");
    return g_failed != 0;
  }
  std::vector<IndexedFeatureMatch> m;
  {  // NoOptions: EXPECT_GT(NumMatches, 0); here all ten rows, at distance 0, to the lowest column
    CascadeHashingFeatureMatcher matcher(TestOptions(false, false));
    CHECK(matcher.MatchImagePair(n1, n2, &m) && m.size() == 10u);
    for (size_t i = 0; i < m.size(); ++i)
      CHECK(m[i].feature1_ind == static_cast<int>(i) && m[i].feature2_ind == 0 && m[i].distance == 0.f);
  }
  {  // RatioTest: the pair is reported (min 0) without a match; with a minimum of one it is not
    CascadeHashingFeatureMatcher matcher(TestOptions(false, true));
    CHECK(matcher.MatchImagePair(r1, r2, &m) && m.empty());
    FeatureMatcherOptions strict = TestOptions(false, true);
    strict.min_num_feature_matches = 1;
    CascadeHashingFeatureMatcher matcher1(strict);
    CHECK(!matcher1.MatchImagePair(r1, r2, &m) && m.empty());
  }
  {  // two scenes: every row finds the first copy of its scene descriptor; symmetric keeps rows 0 and 12
    CascadeHashingFeatureMatcher one_way(TestOptions(false, true));
    CHECK(one_way.MatchImagePair(s1, s2, &m) && m.size() == 24u);
    for (size_t i = 0; i < m.size(); ++i)
      CHECK(m[i].feature1_ind == static_cast<int>(i) && m[i].feature2_ind == (i < 12 ? 12 : 0) && m[i].distance == 0.f);
    CascadeHashingFeatureMatcher matcher(TestOptions(true, true));
    CHECK(matcher.MatchImagePair(s1, s2, &m) && m.size() == 2u && m[0].feature1_ind == 0 && m[0].feature2_ind == 12 &&
          m[1].feature1_ind == 12 && m[1].feature2_ind == 0);
    std::vector<theia::FeatureCorrespondence> c;
    theia::MatchesToFeatureCorrespondences(s1, s2, m, &c);
    CHECK(c.size() == 2u && c[0].feature1.x() == 100.0 && c[0].feature1.y() == 101.0 && c[0].feature2.x() == 320.0 &&
          c[0].feature2.y() == 321.0 && c[1].feature1.x() == 220.0 && c[1].feature2.x() == 200.0);
    // batch == single calls, in order
    const std::vector<const KeypointsAndDescriptors*> images = {&s1, &s2, &n1, &n2, &r1, &r2, &empty};
    const std::vector<std::pair<int, int>> pairs = {{0, 1}, {1, 0}, {2, 3}, {4, 5}, {5, 4}, {0, 0}, {2, 0}, {6, 0}, {0, 6}};
    std::vector<std::vector<IndexedFeatureMatch>> per_pair;
    std::vector<bool> ok;
    matcher.MatchImagePairs(images, pairs, &per_pair, &ok);
    CHECK(per_pair.size() == pairs.size() && ok.size() == pairs.size());
    for (size_t p = 0; p < pairs.size() && p < per_pair.size(); ++p) {
      std::vector<IndexedFeatureMatch> single;
      const bool ok1 = matcher.MatchImagePair(*images[pairs[p].first], *images[pairs[p].second], &single);
      CHECK(ok1 == ok[p] && SameMatches(single, per_pair[p]));
    }
    CHECK(per_pair[0].size() == 2u && per_pair[5].size() == 2u && per_pair[7].empty() && per_pair[8].empty());
    // two matchers of one seed give identical matches; the matches are there whatever the seed
    CascadeHashingFeatureMatcher a(TestOptions(true, true), 99u), b(TestOptions(true, true), 99u);
    std::vector<std::vector<IndexedFeatureMatch>> pa, pb;
    a.MatchImagePairs(images, pairs, &pa, &ok);
    b.MatchImagePairs(images, pairs, &pb, &ok);
    CHECK(pa.size() == pb.size() && a.projections() == b.projections() && a.projections() != matcher.projections());
    for (size_t p = 0; p < pa.size() && p < pb.size(); ++p) CHECK(SameMatches(pa[p], pb[p]));
  }
  std::printf(g_failed ? "cascade matching shim: FAILED\n" : "cascade matching shim: OK (device)\n");
  return g_failed != 0;
}
