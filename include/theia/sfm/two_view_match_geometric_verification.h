// reference: src/theia/sfm/two_view_match_geometric_verification.h:59-92 (options) and
// two_view_match_geometric_verification.cc:185-324 (TriangulatePoints, BundleAdjustRelativePose) with the two tests
// VerifyMatches puts around the latter (:171-176, :181): the verification bundle adjustment of a view pair --
// triangulate every match, adjust camera 2, the (optionally free) focal lengths and the points, filter by
// reprojection error, update the TwoViewInfo.  Implemented on the C ABI (tmi_ba_verify_two_views, where the steps are
// listed line by line); the batched form runs many pairs in ONE call, one wavefront per pair.
//
// The RANSAC of EstimateTwoViewInfo (:128-134) that runs before this step exists for both branches
// (theia/sfm/estimate_twoview_info.h on tmi_ba_estimate_uncalibrated_relative_poses and, with inlier-count scoring,
// tmi_ba_estimate_calibrated_relative_poses; DESIGN.md sections 8.10 and 8.11), and so does the homography inlier count
// VerifyMatches takes first (:124, :326-363: theia/sfm/estimators/estimate_homography.h, CountHomographyInliers on
// tmi_ba_estimate_homographies).  Out of scope: guided matching
// (:157-168).  The caller hands over what VerifyMatches has once those ran: the two cameras (SetupCameras :56-68) and
// the pair's correspondences.
#ifndef THEIA_MI355_TWO_VIEW_MATCH_GEOMETRIC_VERIFICATION_H_
#define THEIA_MI355_TWO_VIEW_MATCH_GEOMETRIC_VERIFICATION_H_
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/camera/camera.h"
#include "theia/sfm/twoview_info.h"

namespace theia {
// The fields of TwoViewMatchGeometricVerification::Options this step reads, with the reference's names and defaults.
struct TwoViewMatchGeometricVerificationOptions {
  int min_num_inlier_matches = 30;
  bool bundle_adjustment = true;  // false: triangulate and gate only (an extension, not a path of the reference)
  double triangulation_max_reprojection_error = 15.0;
  double min_triangulation_angle_degrees = 4.0;
  double final_max_reprojection_error = 5.0;
  // extensions of the MI355X path
  int point_dof = 4;  // 4 = the reference (homogeneous points, no parameterization)
  int device = -1;    // -1 = the current device
};

// One entry per view pair; every pointer must stay valid for the call.
struct TwoViewVerificationProblem {
  const std::vector<FeatureCorrespondence>* correspondences = nullptr;  // pixels
  Camera* camera1 = nullptr;  // held constant but for a free focal length
  Camera* camera2 = nullptr;  // adjusted in place when the call returns true
  bool constant_camera1_intrinsics = true;  // intrinsics1_.focal_length.is_set (:276-279)
  bool constant_camera2_intrinsics = true;
  TwoViewInfo* info = nullptr;                 // out: rotation_2, position_2 (unit norm), the focal lengths (:316-321)
  std::vector<int>* inlier_indices = nullptr;  // out (optional): the matches still kept, in order
};

// TwoViewMatchGeometricVerification::BundleAdjustRelativePose.  True where the reference returns true: the pair had
// more than min_num_inlier_matches matches, at least that many triangulated and the adjustment succeeded.  Then the
// cameras, *info and *inlier_indices are updated; whether MORE than min_num_inlier_matches are left (:181) is for the
// caller to test on inlier_indices->size(), as VerifyMatches does.  Otherwise nothing is written.
bool BundleAdjustRelativePose(const TwoViewMatchGeometricVerificationOptions& options,
                              const TwoViewVerificationProblem& problem);

// Extension of the MI355X path: all pairs in one C ABI call.  One result per problem, in order.
std::vector<bool> BundleAdjustRelativePoseBatch(const TwoViewMatchGeometricVerificationOptions& options,
                                                std::vector<TwoViewVerificationProblem>* problems);
}  // namespace theia
#endif
