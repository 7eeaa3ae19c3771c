// reference: src/theia/matching/feature_matcher_options.h:45-71 -- the options of matching an image collection, with
// the reference's names and defaults.  num_threads is not used (a batch is one device call);
// perform_geometric_verification = true is reported and left alone (theia/matching/brute_force_feature_matcher.h), and
// geometric_verification_options holds the fields this shim's verification step reads.
#ifndef THEIA_MI355_MATCHING_FEATURE_MATCHER_OPTIONS_H_
#define THEIA_MI355_MATCHING_FEATURE_MATCHER_OPTIONS_H_
#include "theia/sfm/two_view_match_geometric_verification.h"
namespace theia {
struct FeatureMatcherOptions {
  int num_threads = 1;
  bool keep_only_symmetric_matches = true;
  bool use_lowes_ratio = true;
  float lowes_ratio = 0.8;
  bool perform_geometric_verification = true;
  TwoViewMatchGeometricVerificationOptions geometric_verification_options;
  int min_num_feature_matches = 30;
  // extension of the MI355X path
  int device = -1;  // -1 = the current device
};
}  // namespace theia
#endif
