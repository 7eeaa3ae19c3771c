// reference: src/theia/matching/guided_epipolar_matcher.h:55-86 and .cc:93-318 -- more matches along the epipolar lines
// of a known two-view geometry, on the C ABI (tmi_ba_guided_epipolar_match, where the semantics and the stated
// deviations are listed: exact search instead of FLANN, seeded fill, endpoints outside uint16 skipped).
//
// Provided: the constructor and GetMatches with the reference's signatures, and a batched GuidedEpipolarMatches that
// equals the single calls in order.  Options is the reference's with `rng` replaced by `seed` and `device`.  The
// fundamental matrix comes from the two cameras as FundamentalMatrixFromProjectionMatrices(P2, P1) forms it
// (guided_epipolar_matcher.cc:201-207, fundamental_matrix_util.cc:222-241), restated on the host in fp64.
#ifndef THEIA_MI355_MATCHING_GUIDED_EPIPOLAR_MATCHER_H_
#define THEIA_MI355_MATCHING_GUIDED_EPIPOLAR_MATCHER_H_
#include <cstdint>
#include <utility>
#include <vector>

#include "theia/matching/indexed_feature_match.h"
#include "theia/matching/keypoints_and_descriptors.h"
#include "theia/sfm/camera/camera.h"

namespace theia {
class GuidedEpipolarMatcher {
 public:
  struct Options {
    // The fill of a group with too few candidates draws from the splitmix64 stream of this seed (the reference
    // takes a RandomNumberGenerator).
    uint64_t seed = 0;
    int device = -1;  // -1 = the current device
    // Features closer than this to the epipolar line are considered for matching.
    double guided_matching_max_distance_pixels = 2.0;
    // A match is kept when its distance is below lowes_ratio^2 times the second-best distance.
    double lowes_ratio = 0.8;
  };

  GuidedEpipolarMatcher(const Options& options, const Camera& camera1, const Camera& camera2,
                        const KeypointsAndDescriptors& features1, const KeypointsAndDescriptors& features2)
      : options_(options), camera1_(camera1), camera2_(camera2), features1_(features1), features2_(features2) {}

  // The guided matches are APPENDED to *matches; only features that are in no match of *matches take part.  False,
  // with *matches untouched and a line on stderr: no device, empty descriptors (or keypoints that do not pair with
  // them), a failed call.
  bool GetMatches(std::vector<IndexedFeatureMatch>* matches);

 private:
  const Options options_;
  const Camera& camera1_;
  const Camera& camera2_;
  const KeypointsAndDescriptors& features1_;
  const KeypointsAndDescriptors& features2_;
};

// Extension of the MI355X path: all pairs (indices into features_per_image and cameras) in one C ABI call; every
// image goes to the device once.  (*matches_per_pair)[p] holds the input matches of pair p and gets its guided
// matches appended, exactly as the single call on that pair would.  False with *matches_per_pair untouched under the
// conditions of GetMatches, for an index out of range and for sizes that do not agree.
bool GuidedEpipolarMatches(const GuidedEpipolarMatcher::Options& options,
                           const std::vector<const KeypointsAndDescriptors*>& features_per_image,
                           const std::vector<std::pair<int, int>>& pairs, const std::vector<const Camera*>& cameras,
                           std::vector<std::vector<IndexedFeatureMatch>>* matches_per_pair);

// Camera::GetProjectionMatrix (camera.cc:191-198, projection_matrix_utils.cc:121-135): K [R | -R c], row-major [12].
void GuidedMatchProjectionMatrix(const Camera& camera, double pmatrix[12]);
// The matcher's F, row-major [9]: it maps a point of image 1 to its line in image 2.
void GuidedMatchFundamentalMatrix(const Camera& camera1, const Camera& camera2, double fmatrix[9]);
}  // namespace theia
#endif
