// reference: src/theia/matching/brute_force_feature_matcher.h:51-66 and .cc:49-117 -- exact nearest-neighbour
// descriptor matching under squared L2 with Lowe's ratio test and the symmetric intersection, on the C ABI
// (tmi_ba_match_features, where the semantics and the two stated deviations are listed).
//
// Provided: MatchImagePair (private in the reference, reached there through FeatureMatcher::MatchImages), a batched
// MatchImagePairs that equals the single calls in order, and the step of FeatureMatcher::MatchImages that turns the
// matches into pixel correspondences (feature_matcher.cc:170-180).  Not rebuilt: AddImage / MatchImages, the features
// and matches databases, threading, and geometric verification (cascade hashing is
// theia/matching/cascade_hashing_feature_matcher.h) -- with
// options.perform_geometric_verification the constructor says so once on stderr and the matches come back
// unverified; BundleAdjustRelativePose (theia/sfm/two_view_match_geometric_verification.h) takes the correspondences.
#ifndef THEIA_MI355_MATCHING_BRUTE_FORCE_FEATURE_MATCHER_H_
#define THEIA_MI355_MATCHING_BRUTE_FORCE_FEATURE_MATCHER_H_
#include <utility>
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/matching/feature_matcher_options.h"
#include "theia/matching/image_pair_match.h"
#include "theia/matching/indexed_feature_match.h"
#include "theia/matching/keypoints_and_descriptors.h"

namespace theia {
class BruteForceFeatureMatcher {
 public:
  explicit BruteForceFeatureMatcher(const FeatureMatcherOptions& options);
  // True where the reference returns true: at least min_num_feature_matches matches after the forward pass and again
  // after the intersection.  *matches holds the surviving matches in ascending feature1_ind, and is EMPTY on false
  // (the reference leaves the rejected forward matches in it).  False and empty without a device, for descriptors of
  // differing lengths, and for a negative min_num_feature_matches (the reference's size_t comparison fails every pair).
  bool MatchImagePair(const KeypointsAndDescriptors& features1, const KeypointsAndDescriptors& features2,
                      std::vector<IndexedFeatureMatch>* matches);
  // Extension of the MI355X path: all pairs (indices into features_per_image) in one C ABI call; every image's
  // descriptors go to the device once.  One entry per pair, in order, equal to the single calls.
  void MatchImagePairs(const std::vector<const KeypointsAndDescriptors*>& features_per_image,
                       const std::vector<std::pair<int, int>>& pairs,
                       std::vector<std::vector<IndexedFeatureMatch>>* matches_per_pair, std::vector<bool>* ok_per_pair);
  const FeatureMatcherOptions& options() const { return options_; }

 private:
  FeatureMatcherOptions options_;
};

// feature_matcher.cc:170-180: the matches as pixel correspondences, Feature(keypoint1.x, keypoint1.y) and
// Feature(keypoint2.x, keypoint2.y), in the matches' order.  A match whose index has no keypoint is skipped.
void MatchesToFeatureCorrespondences(const KeypointsAndDescriptors& features1, const KeypointsAndDescriptors& features2,
                                     const std::vector<IndexedFeatureMatch>& matches,
                                     std::vector<FeatureCorrespondence>* correspondences);
}  // namespace theia
#endif
