// reference: src/theia/sfm/bundle_adjustment/optimize_relative_position_with_known_rotation.h:52-56
// (declaration) and .cc:53-197 (semantics): the unit direction of camera 2's position in camera 1's
// frame from correspondences in normalised image coordinates and the two known world-to-camera
// rotations (angle-axis), by iteratively reweighted least squares on the epipolar constraint.
// Implemented on the C ABI (tmi_ba_optimize_relative_positions); the batched forms solve many view
// pairs in ONE device launch, one wavefront per pair, where the reference runs one call per view-graph
// edge on a CPU thread pool (reconstruction_estimator_utils.cc:244-269).
#ifndef THEIA_MI355_OPTIMIZE_RELATIVE_POSITION_WITH_KNOWN_ROTATION_H_
#define THEIA_MI355_OPTIMIZE_RELATIVE_POSITION_WITH_KNOWN_ROTATION_H_
#include <unordered_map>
#include <utility>
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/reconstruction.h"
#include "theia/sfm/twoview_info.h"
#include "theia/sfm/types.h"
#include "theia/util/eigen_lite.h"

namespace theia {
// *relative_position is an output only (the reference overwrites it before reading it).  true when a
// position was written -- the reference returns true whether its loop converged or ran out of
// iterations; false for no correspondences, non-finite input or a failed device call.
bool OptimizeRelativePositionWithKnownRotation(const std::vector<FeatureCorrespondence>& correspondences,
                                               const Eigen::Vector3d& rotation1, const Eigen::Vector3d& rotation2,
                                               Eigen::Vector3d* relative_position);

// Extension of the MI355X path: many pairs in one launch.  Every pointer must stay valid for the call.
struct RelativePositionProblem {
  const std::vector<FeatureCorrespondence>* correspondences = nullptr;
  Eigen::Vector3d rotation1 = Eigen::Vector3d::Zero();
  Eigen::Vector3d rotation2 = Eigen::Vector3d::Zero();
  Eigen::Vector3d* relative_position = nullptr;
};
// One flag per problem, in order: what the single call returns for it.  device: -1 = the current one.
std::vector<bool> OptimizeRelativePositionsWithKnownRotationsBatch(std::vector<RelativePositionProblem>* problems,
                                                                   int device = -1);

// reference: reconstruction_estimator_utils.cc:244-269 with the edge list in place of the ViewGraph
// (fill it from view_graph->GetAllEdges() / GetMutableEdge).  For every edge the
// features of the tracks both views see (GetNormalizedFeatureCorrespondences, :65-91, in
// view1.TrackIds() order) go to the device as PIXELS with the views' camera models, which normalises
// them there, and info->position_2 is written.  An edge without common tracks, with a view missing
// from the reconstruction or from `orientations`, or with a null info is left alone.  Returns the
// number of edges written.
int RefineRelativeTranslationsWithKnownRotations(const Reconstruction& reconstruction,
                                                 const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                                 std::vector<std::pair<ViewIdPair, TwoViewInfo*>>* edges,
                                                 int device = -1);
}  // namespace theia
#endif
