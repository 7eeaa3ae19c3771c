// Host shim of theia::BruteForceFeatureMatcher (reference brute_force_feature_matcher.cc:49-117) on the C ABI: the
// images' descriptors are packed once into one row-major array, all pairs go through one tmi_ba_match_features call,
// and the compacted matches are handed back pair by pair.
#include <cstdio>

#include "theia/matching/brute_force_feature_matcher.h"
#include "theia_mi355_ba.h"

namespace theia {

BruteForceFeatureMatcher::BruteForceFeatureMatcher(const FeatureMatcherOptions& options) : options_(options) {
  if (options_.perform_geometric_verification)
    std::fprintf(stderr,
                 "[theia::BruteForceFeatureMatcher] perform_geometric_verification is not provided and left alone: "
                 "the matches are returned unverified\n");
}

void BruteForceFeatureMatcher::MatchImagePairs(const std::vector<const KeypointsAndDescriptors*>& features_per_image,
                                               const std::vector<std::pair<int, int>>& pairs,
                                               std::vector<std::vector<IndexedFeatureMatch>>* matches_per_pair,
                                               std::vector<bool>* ok_per_pair) {
  if (matches_per_pair != nullptr) matches_per_pair->assign(pairs.size(), std::vector<IndexedFeatureMatch>());
  if (ok_per_pair != nullptr) ok_per_pair->assign(pairs.size(), false);
  if (pairs.empty() || options_.min_num_feature_matches < 0) return;
  // one descriptor length for the whole batch: that of the first descriptor met
  int dim = 0;
  std::vector<int64_t> image_begin(features_per_image.size() + 1, 0);
  for (size_t m = 0; m < features_per_image.size(); ++m) {
    const KeypointsAndDescriptors* f = features_per_image[m];
    const size_t n = f != nullptr ? f->descriptors.size() : 0;
    image_begin[m + 1] = image_begin[m] + static_cast<int64_t>(n);
    for (size_t i = 0; i < n; ++i) {
      if (dim == 0) dim = f->descriptors[i].size();
      if (f->descriptors[i].size() != dim || dim < 1) {
        std::fprintf(stderr, "[theia::BruteForceFeatureMatcher] descriptors of differing or zero length\n");
        return;
      }
    }
  }
  if (dim == 0) dim = 1;  // no descriptor at all: every pair is empty
  std::vector<float> descriptors(static_cast<size_t>(image_begin.back()) * static_cast<size_t>(dim));
  for (size_t m = 0; m < features_per_image.size(); ++m) {
    if (features_per_image[m] == nullptr) continue;
    float* out = descriptors.data() + static_cast<size_t>(image_begin[m]) * static_cast<size_t>(dim);
    for (const Eigen::VectorXf& d : features_per_image[m]->descriptors) {
      for (int k = 0; k < dim; ++k) out[k] = d[k];
      out += dim;
    }
  }
  std::vector<int32_t> image1(pairs.size()), image2(pairs.size());
  int64_t capacity = 0;
  const int num_images = static_cast<int>(features_per_image.size());
  for (size_t p = 0; p < pairs.size(); ++p) {
    image1[p] = pairs[p].first;
    image2[p] = pairs[p].second;
    if (image1[p] >= 0 && image1[p] < num_images) capacity += image_begin[image1[p] + 1] - image_begin[image1[p]];
  }
  tmi_ba_match_options O;
  tmi_ba_match_options_init(&O);
  O.use_lowes_ratio = options_.use_lowes_ratio ? 1 : 0;
  O.lowes_ratio = options_.lowes_ratio;
  O.keep_only_symmetric_matches = options_.keep_only_symmetric_matches ? 1 : 0;
  O.min_num_feature_matches = options_.min_num_feature_matches;
  O.device = options_.device;
  std::vector<int8_t> status(pairs.size(), 1);
  std::vector<int32_t> num_forward(pairs.size(), 0), feature1(static_cast<size_t>(capacity)),
      feature2(static_cast<size_t>(capacity));
  std::vector<int64_t> begin(pairs.size() + 1, 0);
  std::vector<float> distance(static_cast<size_t>(capacity));
  tmi_ba_match_summary summary;
  const int rc = tmi_ba_match_features(&O, num_images, image_begin.data(), descriptors.data(), dim,
                                       static_cast<int32_t>(pairs.size()), image1.data(), image2.data(), capacity,
                                       status.data(), num_forward.data(), begin.data(), feature1.data(),
                                       feature2.data(), distance.data(), &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::BruteForceFeatureMatcher] device call failed: %s\n", tmi_ba_last_error());
    return;
  }
  for (size_t p = 0; p < pairs.size(); ++p) {
    if (ok_per_pair != nullptr) (*ok_per_pair)[p] = status[p] == 0;
    if (matches_per_pair == nullptr) continue;
    std::vector<IndexedFeatureMatch>& out = (*matches_per_pair)[p];
    out.reserve(static_cast<size_t>(begin[p + 1] - begin[p]));
    for (int64_t i = begin[p]; i < begin[p + 1]; ++i) out.emplace_back(feature1[i], feature2[i], distance[i]);
  }
}

bool BruteForceFeatureMatcher::MatchImagePair(const KeypointsAndDescriptors& features1,
                                              const KeypointsAndDescriptors& features2,
                                              std::vector<IndexedFeatureMatch>* matches) {
  std::vector<std::vector<IndexedFeatureMatch>> per_pair;
  std::vector<bool> ok;
  MatchImagePairs({&features1, &features2}, {{0, 1}}, &per_pair, &ok);
  if (matches != nullptr) {
    matches->clear();
    if (!per_pair.empty()) matches->swap(per_pair[0]);
  }
  return !ok.empty() && ok[0];
}

void MatchesToFeatureCorrespondences(const KeypointsAndDescriptors& features1, const KeypointsAndDescriptors& features2,
                                     const std::vector<IndexedFeatureMatch>& matches,
                                     std::vector<FeatureCorrespondence>* correspondences) {
  if (correspondences == nullptr) return;
  correspondences->clear();
  correspondences->reserve(matches.size());
  for (const IndexedFeatureMatch& m : matches) {
    if (m.feature1_ind < 0 || m.feature2_ind < 0 || static_cast<size_t>(m.feature1_ind) >= features1.keypoints.size() ||
        static_cast<size_t>(m.feature2_ind) >= features2.keypoints.size())
      continue;
    const Keypoint& k1 = features1.keypoints[m.feature1_ind];
    const Keypoint& k2 = features2.keypoints[m.feature2_ind];
    correspondences->emplace_back(Feature(k1.x(), k1.y()), Feature(k2.x(), k2.y()));
  }
}

}  // namespace theia
