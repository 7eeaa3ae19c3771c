// reference: src/theia/matching/indexed_feature_match.h:40-57 -- a match between feature indices of two images and
// its descriptor distance.
#ifndef THEIA_MI355_MATCHING_INDEXED_FEATURE_MATCH_H_
#define THEIA_MI355_MATCHING_INDEXED_FEATURE_MATCH_H_
namespace theia {
struct IndexedFeatureMatch {
  IndexedFeatureMatch() {}
  IndexedFeatureMatch(int f1_ind, int f2_ind, float dist) : feature1_ind(f1_ind), feature2_ind(f2_ind), distance(dist) {}
  int feature1_ind;
  int feature2_ind;
  float distance;
};
inline bool CompareFeaturesByDistance(const IndexedFeatureMatch& feature1, const IndexedFeatureMatch& feature2) {
  return feature1.distance < feature2.distance;
}
}  // namespace theia
#endif
