// reference: src/theia/matching/cascade_hashing_feature_matcher.h and .cc:130-166 with CascadeHasher
// (cascade_hasher.cc:55-277) -- the matcher the reference's applications run by default
// (--matching_strategy=CASCADE_HASHING): hashed shortlists, exact squared-L2 distances on eleven columns per row,
// Lowe's ratio test and the symmetric intersection, on the C ABI (tmi_ba_match_features_cascade, where the semantics
// and the stated deviations are listed).
//
// Provided: MatchImagePair (private in the reference, reached there through FeatureMatcher::MatchImages) and a batched
// MatchImagePairs that equals the single calls in order.  The hash projections are drawn at the first non-empty image,
// for its descriptor length: std::mt19937(seed), a fresh std::normal_distribution<double>(0, 1) per draw cast to float,
// in the order of CascadeHasher::Initialize (cascade_hasher.cc:66-89, random.cc:87-91).  DEVIATION: the reference
// seeds its generator from the clock; here the seed is the constructor's, kDefaultSeed by default, so that two
// matchers give the same matches.  Not rebuilt: AddImage(s) / MatchImages, the LRU cache of hashed images (a call
// hashes each image once), the features and matches databases, threading, and geometric verification -- with
// options.perform_geometric_verification the constructor says so once on stderr and the matches come back
// unverified, as theia/matching/brute_force_feature_matcher.h reports it; MatchesToFeatureCorrespondences is declared
// there.
#ifndef THEIA_MI355_MATCHING_CASCADE_HASHING_FEATURE_MATCHER_H_
#define THEIA_MI355_MATCHING_CASCADE_HASHING_FEATURE_MATCHER_H_
#include <utility>
#include <vector>

#include "theia/matching/feature_matcher_options.h"
#include "theia/matching/indexed_feature_match.h"
#include "theia/matching/keypoints_and_descriptors.h"

namespace theia {
class CascadeHashingFeatureMatcher {
 public:
  static constexpr unsigned kDefaultSeed = 20140623u;
  explicit CascadeHashingFeatureMatcher(const FeatureMatcherOptions& options);
  CascadeHashingFeatureMatcher(const FeatureMatcherOptions& options, unsigned seed);
  // True where the reference returns true: at least min_num_feature_matches matches after the forward pass and again
  // after the intersection.  *matches holds the surviving matches in ascending feature1_ind, and is EMPTY on false.
  // False and empty without a device, for descriptors of differing lengths or of another length than the one the
  // projections were drawn for, and for a negative min_num_feature_matches.
  bool MatchImagePair(const KeypointsAndDescriptors& features1, const KeypointsAndDescriptors& features2,
                      std::vector<IndexedFeatureMatch>* matches);
  // Extension of the MI355X path: all pairs (indices into features_per_image) in one C ABI call; every image is
  // hashed once.  One entry per pair, in order, equal to the single calls.
  void MatchImagePairs(const std::vector<const KeypointsAndDescriptors*>& features_per_image,
                       const std::vector<std::pair<int, int>>& pairs,
                       std::vector<std::vector<IndexedFeatureMatch>>* matches_per_pair, std::vector<bool>* ok_per_pair);
  const FeatureMatcherOptions& options() const { return options_; }
  unsigned seed() const { return seed_; }
  // [188 x dimension, row-major]; empty until the first non-empty image has been seen.
  const std::vector<float>& projections() const { return projections_; }
  int descriptor_dimension() const { return dimension_; }

 private:
  FeatureMatcherOptions options_;
  unsigned seed_;
  int dimension_ = 0;
  std::vector<float> projections_;
};
}  // namespace theia
#endif
