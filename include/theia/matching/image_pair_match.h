// reference: src/theia/matching/image_pair_match.h:51-72 -- the matches of an image pair as pixel correspondences,
// with the pair's two-view geometry once verified.  Serialisation is not provided.
#ifndef THEIA_MI355_MATCHING_IMAGE_PAIR_MATCH_H_
#define THEIA_MI355_MATCHING_IMAGE_PAIR_MATCH_H_
#include <string>
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/twoview_info.h"
namespace theia {
struct ImagePairMatch {
  std::string image1;
  std::string image2;
  TwoViewInfo twoview_info;
  std::vector<FeatureCorrespondence> correspondences;
};
}  // namespace theia
#endif
