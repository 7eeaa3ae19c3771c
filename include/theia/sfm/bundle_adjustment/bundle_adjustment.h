// Source-compatible mirror of
//   /root/reference/src/theia/sfm/bundle_adjustment/bundle_adjustment.h:65-155
// (OptimizeIntrinsicsType, BundleAdjustmentOptions, BundleAdjustmentSummary, the
// four free functions).  Same names, same defaults, same meaning; the work is
// done by the MI355X engine behind include/theia_mi355_ba.h instead of Ceres.
#ifndef THEIA_MI355_BUNDLE_ADJUSTMENT_H_
#define THEIA_MI355_BUNDLE_ADJUSTMENT_H_
#include <unordered_map>
#include <unordered_set>
#include "ceres/types.h"
#include "theia/sfm/bundle_adjustment/create_loss_function.h"
#include "theia/sfm/types.h"

namespace theia {
class Reconstruction;

// bundle_adjustment.h:65-76
enum class OptimizeIntrinsicsType {
  NONE = 0x00,
  FOCAL_LENGTH = 0x01,
  ASPECT_RATIO = 0x02,
  SKEW = 0x04,
  PRINCIPAL_POINTS = 0x08,
  RADIAL_DISTORTION = 0x10,
  TANGENTIAL_DISTORTION = 0x20,
  ALL = FOCAL_LENGTH | ASPECT_RATIO | SKEW | PRINCIPAL_POINTS | RADIAL_DISTORTION |
        TANGENTIAL_DISTORTION,
};
inline OptimizeIntrinsicsType operator|(OptimizeIntrinsicsType a, OptimizeIntrinsicsType b) {
  return static_cast<OptimizeIntrinsicsType>(static_cast<int>(a) | static_cast<int>(b));
}
inline OptimizeIntrinsicsType operator&(OptimizeIntrinsicsType a, OptimizeIntrinsicsType b) {
  return static_cast<OptimizeIntrinsicsType>(static_cast<int>(a) & static_cast<int>(b));
}
inline OptimizeIntrinsicsType& operator|=(OptimizeIntrinsicsType& a, OptimizeIntrinsicsType b) {
  a = a | b;
  return a;
}

// bundle_adjustment.h:78-122 (defaults identical)
struct BundleAdjustmentOptions {
  LossFunctionType loss_function_type = LossFunctionType::TRIVIAL;
  double robust_loss_width = 2.0;
  ceres::LinearSolverType linear_solver_type = ceres::SPARSE_SCHUR;
  ceres::PreconditionerType preconditioner_type = ceres::SCHUR_JACOBI;
  ceres::VisibilityClusteringType visibility_clustering_type = ceres::CANONICAL_VIEWS;
  bool verbose = false;
  bool constant_camera_orientation = false;
  bool constant_camera_position = false;
  OptimizeIntrinsicsType intrinsics_to_optimize =
      OptimizeIntrinsicsType::FOCAL_LENGTH | OptimizeIntrinsicsType::RADIAL_DISTORTION;
  int num_threads = 1;
  int max_num_iterations = 100;
  double max_solver_time_in_seconds = 3600.0;
  bool use_inner_iterations = true;  // one coordinate-descent sweep after every LM step
  double function_tolerance = 1e-6;
  double gradient_tolerance = 1e-10;
  double parameter_tolerance = 1e-8;
  double max_trust_region_radius = 1e12;

  // Extensions of the MI355X path (not in the reference):
  //   4 = optimise the homogeneous point as the reference does, 3 = hold w fixed.
  int point_dof = 4;
  int device = -1;  // HIP device ordinal, -1 = current
  //   ceres::SCHUR_JACOBI builds its block diagonal per PARAMETER block: a 6 x 6 extrinsics block and a separate
  //   intrinsics block per view (ceres/schur_jacobi_preconditioner.cc).  That is what preconditioner_type = SCHUR_JACOBI
  //   means here too (false).  true = ONE merged [extrinsics | private intrinsics] block per view: a strictly stronger
  //   preconditioner at the same cost per application (several times fewer PCG iterations, the same reduced system
  //   and stopping rule) -- the device path's fast mode, and an explicit opt-in because it is not Ceres' trajectory.
  bool merged_view_blocks_in_preconditioner = false;
  //   true: BundleAdjustReconstruction keeps the flattened problem and the device-resident solver of its last call; the
  //   next call on the same Reconstruction with an unchanged residual set re-uses them (only parameter values travel:
  //   0.05 s instead of 0.31 s wall at Venice size).  An extension, hence OFF by default: the reference builds and frees
  //   everything inside the call, and so does false.  Validity of a kept session = the data-model mutation stamp
  //   (types.h; needs the one-line hooks in the mutators) AND a structural fingerprint of the
  //   reconstruction (counts of views / tracks / estimated ones / their features) recomputed at every re-use.
  bool keep_problem_resident = false;
};

// bundle_adjustment.h:125-133
struct BundleAdjustmentSummary {
  bool success = false;
  double initial_cost = 0.0;
  double final_cost = 0.0;
  double setup_time_in_seconds = 0.0;
  double solve_time_in_seconds = 0.0;
  // Extensions (behind the reference's five fields, bundle_adjustment.h:124-133).  The preconditioner PCG ran with,
  // as a ceres::PreconditionerType, and whether it differs from what BundleAdjustmentOptions asked for:
  // ceres::CLUSTER_TRIDIAGONAL is not implemented on the device path and is served by CLUSTER_JACOBI; CLUSTER_JACOBI
  // on a handle without clusters (several ranks, clusters that do not fit) keeps the SCHUR_JACOBI blocks;
  // ceres::JACOBI runs as SCHUR_JACOBI.  (Exact linear solvers: IDENTITY, not substituted.)
  ceres::PreconditionerType effective_preconditioner_type = ceres::IDENTITY;
  bool preconditioner_substituted = false;
};

// Extensions: the resident session BundleAdjustReconstruction keeps (one per process; it holds the problem's HBM).
void ReleaseBundleAdjustmentSession();
bool BundleAdjustmentSessionIsResident(const Reconstruction* reconstruction);

// bundle_adjustment.h:136-155
BundleAdjustmentSummary BundleAdjustReconstruction(const BundleAdjustmentOptions& options,
                                                   Reconstruction* reconstruction);
BundleAdjustmentSummary BundleAdjustPartialReconstruction(
    const BundleAdjustmentOptions& options, const std::unordered_set<ViewId>& views_to_optimize,
    const std::unordered_set<TrackId>& tracks_to_optimize, Reconstruction* reconstruction);
BundleAdjustmentSummary BundleAdjustView(const BundleAdjustmentOptions& options, const ViewId view_id,
                                         Reconstruction* reconstruction);
BundleAdjustmentSummary BundleAdjustTrack(const BundleAdjustmentOptions& options,
                                          const TrackId track_id, Reconstruction* reconstruction);

// Extension of the MI355X path: BundleAdjustTrack for many tracks in ONE device launch
// (one independent trust-region problem per GPU thread) instead of one call per track per
// CPU thread (estimate_track.cc:166-204,238-246).  Same per-track semantics and summary as
// BundleAdjustTrack; tracks that are not estimated are skipped (absent from the result).
std::unordered_map<TrackId, BundleAdjustmentSummary> BundleAdjustTracks(
    const BundleAdjustmentOptions& options, const std::unordered_set<TrackId>& track_ids,
    Reconstruction* reconstruction);

// Extension of the MI355X path: BundleAdjustView for many views in ONE device launch
// (theiasfm_amd/host/view_ops.cc; tmi_ba_adjust_views).  The result equals calling BundleAdjustView once per view
// in ascending ViewId order, each call starting from the parameters the previous ones left (views sharing
// intrinsics with free entries run in sequence on the device).  Views that are not estimated are skipped
// (absent from the result).
std::unordered_map<ViewId, BundleAdjustmentSummary> BundleAdjustViews(const BundleAdjustmentOptions& options,
                                                                      const std::unordered_set<ViewId>& view_ids,
                                                                      Reconstruction* reconstruction);
}  // namespace theia
#endif
