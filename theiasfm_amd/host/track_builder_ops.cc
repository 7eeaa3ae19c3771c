// Host shim of theia::TrackBuilder (reference track_builder.cc:53-151) on the C ABI: every view keeps a
// Feature-to-local-index map, the (view, index) endpoints of all correspondences go through one tmi_ba_build_tracks
// call, and the tracks come back as a CSR that is handed to Reconstruction::AddTrack in track order.
#include <cstdio>
#include <cstring>
#include <utility>

#include "theia/sfm/reconstruction.h"
#include "theia/sfm/track_builder.h"
#include "theia_mi355_ba.h"

namespace theia {

std::size_t TrackBuilder::FeatureHash::operator()(const Feature& f) const {
  // x + 0.0 turns -0.0 into 0.0, so features that compare equal hash alike
  const double v[2] = {f.x() + 0.0, f.y() + 0.0};
  std::uint64_t bits[2];
  std::memcpy(bits, v, sizeof(bits));
  return std::hash<std::uint64_t>()(bits[0] * 0x9e3779b97f4a7c15ull ^ (bits[1] + (bits[0] >> 29)));
}

TrackBuilder::TrackBuilder(const int min_track_length, const int max_track_length)
    : min_track_length_(min_track_length), max_track_length_(max_track_length) {}

std::uint32_t TrackBuilder::LocalIndex(const ViewId view_id, const Feature& feature) {
  FeatureIndex& index = index_of_view_[view_id];
  std::vector<Feature>& features = features_of_view_[view_id];
  const auto inserted = index.emplace(feature, static_cast<std::uint32_t>(features.size()));
  if (inserted.second) features.push_back(feature);
  return inserted.first->second;
}

void TrackBuilder::AddFeatureCorrespondence(const ViewId view_id1, const Feature& feature1, const ViewId view_id2,
                                            const Feature& feature2) {
  if (view_id1 == view_id2) {  // the reference's CHECK_NE (track_builder.cc:66): BuildTracks will return false
    same_view_added_ = true;
    return;
  }
  const std::uint32_t index1 = LocalIndex(view_id1, feature1), index2 = LocalIndex(view_id2, feature2);
  endpoint_view_.push_back(view_id1);
  endpoint_feature_.push_back(index1);
  endpoint_view_.push_back(view_id2);
  endpoint_feature_.push_back(index2);
}

void TrackBuilder::AddFeatureCorrespondences(const ViewId view_id1, const ViewId view_id2,
                                             const std::vector<FeatureCorrespondence>& correspondences) {
  endpoint_view_.reserve(endpoint_view_.size() + 2 * correspondences.size());
  endpoint_feature_.reserve(endpoint_feature_.size() + 2 * correspondences.size());
  for (const FeatureCorrespondence& c : correspondences) AddFeatureCorrespondence(view_id1, c.feature1, view_id2, c.feature2);
}

bool TrackBuilder::BuildTracks(Reconstruction* reconstruction) {
  if (reconstruction == nullptr) return false;
  if (same_view_added_) {
    std::fprintf(stderr, "[theia::TrackBuilder] a correspondence between two features of the same view was added\n");
    return false;
  }
  for (const auto& view : features_of_view_)
    if (reconstruction->View(view.first) == nullptr) {
      std::fprintf(stderr, "[theia::TrackBuilder] view %u of a correspondence is not in the reconstruction\n",
                   static_cast<unsigned>(view.first));
      return false;
    }
  tmi_ba_track_build_options options;
  tmi_ba_track_build_options_init(&options);
  options.min_track_length = min_track_length_;
  options.max_track_length = max_track_length_;
  options.device = device_;
  // a track has at least two observations and an observation is a node: the most there can be
  const int64_t num_edges = static_cast<int64_t>(endpoint_view_.size() / 2);
  std::vector<int64_t> track_begin(static_cast<size_t>(num_edges) + 1, 0);
  std::vector<std::uint32_t> obs_view(static_cast<size_t>(2 * num_edges)), obs_feature(static_cast<size_t>(2 * num_edges));
  tmi_ba_track_build_summary summary;
  const int rc = tmi_ba_build_tracks(&options, num_edges, endpoint_view_.data(), endpoint_feature_.data(), num_edges,
                                     2 * num_edges, track_begin.data(), obs_view.data(), obs_feature.data(), nullptr,
                                     nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::TrackBuilder] device call failed: %s\n", tmi_ba_last_error());
    return false;
  }
  num_small_tracks_ = static_cast<int>(summary.num_small_tracks);
  num_inconsistent_features_ = static_cast<int>(summary.num_inconsistent_features);
  std::vector<std::pair<ViewId, Feature> > track;
  for (int64_t t = 0; t < summary.num_tracks; ++t) {
    track.clear();
    for (int64_t i = track_begin[t]; i < track_begin[t + 1]; ++i)
      track.emplace_back(obs_view[i], features_of_view_.at(obs_view[i])[obs_feature[i]]);
    // every view is known and a track names a view once, so this cannot fail (the reference's CHECK_NE, :121)
    if (reconstruction->AddTrack(track) == kInvalidTrackId) {
      std::fprintf(stderr, "[theia::TrackBuilder] Reconstruction::AddTrack refused track %lld\n", static_cast<long long>(t));
      return false;
    }
  }
  return true;
}

}  // namespace theia
