// Host shim of theia::CascadeHashingFeatureMatcher (reference cascade_hashing_feature_matcher.cc:130-166) on the C
// ABI: the hash projections are drawn once from the matcher's seed, the images' descriptors are packed once into one
// row-major array, all pairs go through one tmi_ba_match_features_cascade call, and the compacted matches are handed
// back pair by pair.
#include <cstdio>
#include <random>

#include "theia/matching/cascade_hashing_feature_matcher.h"
#include "theia_mi355_ba.h"

namespace theia {

constexpr unsigned CascadeHashingFeatureMatcher::kDefaultSeed;

CascadeHashingFeatureMatcher::CascadeHashingFeatureMatcher(const FeatureMatcherOptions& options)
    : CascadeHashingFeatureMatcher(options, kDefaultSeed) {}

CascadeHashingFeatureMatcher::CascadeHashingFeatureMatcher(const FeatureMatcherOptions& options, unsigned seed)
    : options_(options), seed_(seed) {
  if (options_.perform_geometric_verification)
    std::fprintf(stderr,
                 "[theia::CascadeHashingFeatureMatcher] perform_geometric_verification is not provided and left "
                 "alone: the matches are returned unverified\n");
}

void CascadeHashingFeatureMatcher::MatchImagePairs(
    const std::vector<const KeypointsAndDescriptors*>& features_per_image, const std::vector<std::pair<int, int>>& pairs,
    std::vector<std::vector<IndexedFeatureMatch>>* matches_per_pair, std::vector<bool>* ok_per_pair) {
  if (matches_per_pair != nullptr) matches_per_pair->assign(pairs.size(), std::vector<IndexedFeatureMatch>());
  if (ok_per_pair != nullptr) ok_per_pair->assign(pairs.size(), false);
  if (pairs.empty() || options_.min_num_feature_matches < 0) return;
  // one descriptor length for the matcher's life: that of the first descriptor it met
  int dim = dimension_;
  std::vector<int64_t> image_begin(features_per_image.size() + 1, 0);
  for (size_t m = 0; m < features_per_image.size(); ++m) {
    const KeypointsAndDescriptors* f = features_per_image[m];
    const size_t n = f != nullptr ? f->descriptors.size() : 0;
    image_begin[m + 1] = image_begin[m] + static_cast<int64_t>(n);
    for (size_t i = 0; i < n; ++i) {
      if (dim == 0) dim = f->descriptors[i].size();
      if (f->descriptors[i].size() != dim || dim < 1) {
        std::fprintf(stderr, "[theia::CascadeHashingFeatureMatcher] descriptors of differing or zero length\n");
        return;
      }
    }
  }
  if (dim == 0) return;  // no descriptor at all: every pair is empty, and no projection is drawn yet
  if (dimension_ == 0) {
    // CascadeHasher::Initialize (cascade_hasher.cc:66-89): the primary projection's 128 rows, then the ten rows of
    // each of the six bucket groups, every row in ascending dimension; RandGaussian (random.cc:87-91) builds a fresh
    // distribution per draw
    dimension_ = dim;
    std::mt19937 generator(seed_);
    projections_.resize(static_cast<size_t>(188) * static_cast<size_t>(dim));
    for (float& p : projections_) {
      std::normal_distribution<double> distribution(0.0, 1.0);
      p = static_cast<float>(distribution(generator));
    }
  }
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
  tmi_ba_cascade_match_options O;
  tmi_ba_cascade_match_options_init(&O);
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
  tmi_ba_cascade_match_summary summary;
  const int rc = tmi_ba_match_features_cascade(
      &O, num_images, image_begin.data(), descriptors.data(), dim, projections_.data(),
      static_cast<int32_t>(pairs.size()), image1.data(), image2.data(), capacity, status.data(), num_forward.data(),
      begin.data(), feature1.data(), feature2.data(), distance.data(), nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::CascadeHashingFeatureMatcher] device call failed: %s\n", tmi_ba_last_error());
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

bool CascadeHashingFeatureMatcher::MatchImagePair(const KeypointsAndDescriptors& features1,
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

}  // namespace theia
