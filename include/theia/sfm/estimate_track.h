// reference: src/theia/sfm/estimate_track.h:55-117 (same Options, Summary and public methods)
// EstimateTracks hands every requested unestimated track to ONE tmi_ba_estimate_tracks call (batched
// triangulation, track BA and acceptance on the device; theiasfm_amd/host/track_estimate_ops.cc) instead of a
// thread pool calling EstimateTrack per track.  Options::num_threads and multithreaded_step_size are accepted and
// unused.  Ids that are not in the reconstruction are skipped (the reference would dereference a null track).
#ifndef THEIA_MI355_SFM_ESTIMATE_TRACK_H_
#define THEIA_MI355_SFM_ESTIMATE_TRACK_H_
#include <unordered_set>
#include <vector>

#include "theia/sfm/bundle_adjustment/bundle_adjustment.h"
#include "theia/sfm/types.h"

namespace theia {
class Reconstruction;

class TrackEstimator {
 public:
  struct Options {
    // Number of threads for multithreading (unused: the device runs every track at once).
    int num_threads = 1;
    // Maximum reprojection error for successful triangulation.
    double max_acceptable_reprojection_error_pixels = 5.0;
    // Minimum triangulation angle between two views required for triangulation.
    double min_triangulation_angle_degrees = 3.0;
    // Perform bundle adjustment on the track as soon as a position is estimated.
    bool bundle_adjustment = true;
    BundleAdjustmentOptions ba_options;
    // Tracks per thread-pool worker in the reference (unused).
    int multithreaded_step_size = 100;
  };

  struct Summary {
    // Number of estimated tracks that were input.
    int input_num_estimated_tracks = 0;
    // Number of triangulation attempts made.
    int num_triangulation_attempts = 0;
    // TrackId of the newly estimated tracks (not including tracks that were input as estimated).
    std::unordered_set<TrackId> estimated_tracks;
  };

  TrackEstimator(const Options& options, Reconstruction* reconstruction)
      : options_(options), reconstruction_(reconstruction) {}

  // Attempts to estimate all unestimated tracks seen by an estimated view.
  Summary EstimateAllTracks();

  // Estimate only the tracks supplied by the user.
  Summary EstimateTracks(const std::unordered_set<TrackId>& track_ids);

 private:
  const Options options_;
  Reconstruction* reconstruction_;
};

}  // namespace theia

#endif  // THEIA_MI355_SFM_ESTIMATE_TRACK_H_
