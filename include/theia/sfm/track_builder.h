// reference: src/theia/sfm/track_builder.h:58-78 and track_builder.cc:53-151 on ConnectedComponents
// (math/graph/connected_components.h:87-162) -- the tracks of a Reconstruction from the feature correspondences of
// all view pairs, by union-find on the device (tmi_ba_build_tracks, where the semantics and the stated deviations are
// listed: the cap by replay, the lowest node id kept per view, tracks in ascending label).
//
// The builder keeps one Feature-to-local-index map per view (a feature's index is the order of its first use in that
// view; equality is Eigen::Vector2d's ==, so -0.0 equals 0.0) and sends (view, index) endpoints through the C ABI;
// coordinates never reach the device.  BuildTracks then calls Reconstruction::AddTrack in track order, so TrackIds
// are deterministic.  DEVIATIONS: BuildTracks returns bool (void in the reference) and returns false, writing NOTHING
// to the reconstruction, where the reference CHECK-aborts -- a correspondence inside one view was added
// (track_builder.cc:66), a view named by a correspondence is not in the reconstruction (:121) -- and when there is no
// device or the device call fails.  Extension: AddFeatureCorrespondences adds a view pair's correspondences at once.
#ifndef THEIA_MI355_SFM_TRACK_BUILDER_H_
#define THEIA_MI355_SFM_TRACK_BUILDER_H_
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "theia/matching/feature_correspondence.h"
#include "theia/sfm/feature.h"
#include "theia/sfm/types.h"

namespace theia {
class Reconstruction;

class TrackBuilder {
 public:
  TrackBuilder(const int min_track_length, const int max_track_length);
  // Adds a feature correspondence between two views.
  void AddFeatureCorrespondence(const ViewId view_id1, const Feature& feature1, const ViewId view_id2,
                                const Feature& feature2);
  // Extension: the same as one AddFeatureCorrespondence(view_id1, c.feature1, view_id2, c.feature2) per element, in
  // order.
  void AddFeatureCorrespondences(const ViewId view_id1, const ViewId view_id2,
                                 const std::vector<FeatureCorrespondence>& correspondences);
  // Generates all tracks and adds them to the reconstruction; false (nothing written) as described above.
  bool BuildTracks(Reconstruction* reconstruction);

  int min_track_length() const { return min_track_length_; }
  int max_track_length() const { return max_track_length_; }
  // -1 = the current device
  void set_device(int device) { device_ = device; }
  std::size_t NumCorrespondences() const { return endpoint_view_.size() / 2; }
  // of the last BuildTracks that reached the device
  int num_small_tracks() const { return num_small_tracks_; }
  int num_inconsistent_features() const { return num_inconsistent_features_; }

 private:
  struct FeatureHash {
    std::size_t operator()(const Feature& f) const;
  };
  struct FeatureEqual {
    bool operator()(const Feature& a, const Feature& b) const { return a.x() == b.x() && a.y() == b.y(); }
  };
  typedef std::unordered_map<Feature, std::uint32_t, FeatureHash, FeatureEqual> FeatureIndex;
  std::uint32_t LocalIndex(const ViewId view_id, const Feature& feature);

  const int min_track_length_;
  const int max_track_length_;
  int device_ = -1;
  bool same_view_added_ = false;
  int num_small_tracks_ = 0;
  int num_inconsistent_features_ = 0;
  std::unordered_map<ViewId, FeatureIndex> index_of_view_;
  std::unordered_map<ViewId, std::vector<Feature> > features_of_view_;  // by local index
  std::vector<std::uint32_t> endpoint_view_, endpoint_feature_;
};
}  // namespace theia
#endif
