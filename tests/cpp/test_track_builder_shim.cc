// The track builder shim (theiasfm_amd/host/track_builder_ops.cc): the defaults against the reference's, without a
// device BuildTracks returning false with the reconstruction untouched, and with one (--need-device) the reference's
// five tests (track_builder_test.cc:64-199) with its VerifyTracks, bulk add == single adds, deterministic TrackIds,
// -0.0 == 0.0, and the cases where the reference aborts and the shim returns false with nothing written.
// Stand-alone: its own main.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "theia/sfm/reconstruction.h"
#include "theia/sfm/track_builder.h"
#include "theia_mi355_ba.h"

using theia::Feature;
using theia::FeatureCorrespondence;
using theia::Reconstruction;
using theia::TrackBuilder;
using theia::TrackId;
using theia::ViewId;

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

static const int kMinTrackLength = 2;

static void AddViews(Reconstruction* reconstruction, int n) {
  for (int i = 0; i < n; ++i) reconstruction->AddView(std::to_string(i));
}

// Ensure that each track has been added to every view (track_builder_test.cc:52-61).
static void VerifyTracks(const Reconstruction& reconstruction) {
  for (const TrackId track_id : reconstruction.TrackIds()) {
    const theia::Track* track = reconstruction.Track(track_id);
    CHECK(track != nullptr);
    if (track == nullptr) continue;
    CHECK(track->NumViews() >= 2);
    for (const ViewId view_id : track->ViewIds()) {
      const theia::View* view = reconstruction.View(view_id);
      CHECK(view != nullptr && view->GetFeature(track_id) != nullptr);
    }
  }
}

// The tracks as (view, x, y) lists in TrackId order, for comparing two reconstructions.
static std::vector<std::vector<double>> Flatten(const Reconstruction& reconstruction) {
  std::vector<std::vector<double>> out;
  for (TrackId t = 0; t < static_cast<TrackId>(reconstruction.NumTracks()); ++t) {
    std::vector<double> row;
    const theia::Track* track = reconstruction.Track(t);
    if (track == nullptr) continue;
    for (ViewId v = 0; v < static_cast<ViewId>(reconstruction.NumViews()); ++v) {
      const Feature* f = reconstruction.View(v)->GetFeature(t);
      if (f != nullptr) {
        row.push_back(v);
        row.push_back(f->x());
        row.push_back(f->y());
      }
    }
    out.push_back(row);
  }
  return out;
}

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  {  // the defaults (reconstruction_builder.h:81-85)
    tmi_ba_track_build_options o;
    tmi_ba_track_build_options_init(&o);
    CHECK(o.min_track_length == 2 && o.max_track_length == 50 && o.device == -1);
    TrackBuilder builder(o.min_track_length, o.max_track_length);
    CHECK(builder.min_track_length() == 2 && builder.max_track_length() == 50 && builder.NumCorrespondences() == 0u);
  }
  const ViewId pairs[4][2] = {{0, 1}, {0, 1}, {1, 2}, {1, 2}};
  const bool have_device = tmi_ba_device_count() > 0;
  if (!have_device) {
    if (need_device) {
      std::printf("track builder shim: no device\n");
      return 2;
    }
    TrackBuilder builder(kMinTrackLength, 10);
    for (int i = 0; i < 4; i++) builder.AddFeatureCorrespondence(pairs[i][0], Feature(i, i), pairs[i][1], Feature(i, i));
    CHECK(builder.NumCorrespondences() == 4u);
    Reconstruction reconstruction;
    AddViews(&reconstruction, 3);
    const std::vector<std::pair<ViewId, Feature>> existing = {{0, Feature(7, 7)}, {1, Feature(8, 8)}};
    CHECK(reconstruction.AddTrack(existing) == 0u);
    CHECK(!builder.BuildTracks(&reconstruction));
    CHECK(reconstruction.NumTracks() == 1 && reconstruction.View(2)->TrackIds().empty());
    CHECK(!builder.BuildTracks(nullptr));
    // invalid arguments are reported before the device is looked for
    tmi_ba_track_build_options o;
    tmi_ba_track_build_options_init(&o);
    tmi_ba_track_build_summary summary;
    const uint32_t view[2] = {4, 4}, feature[2] = {0, 1};
    int64_t begin[2] = {-1, -1};
    CHECK(tmi_ba_build_tracks(&o, 1, view, feature, 1, 0, begin, nullptr, nullptr, nullptr, nullptr, &summary) ==
          TMI_BA_ERR_INVALID_ARGUMENT);
    const uint32_t view2[2] = {4, 5};
    CHECK(tmi_ba_build_tracks(&o, 1, view2, feature, 1, 0, begin, nullptr, nullptr, nullptr, nullptr, &summary) ==
          TMI_BA_ERR_NO_DEVICE);
    CHECK(begin[0] == -1 && begin[1] == -1);
    std::printf(g_failed ? "track builder shim: FAILED\n" : "track builder shim: OK\n");
    return g_failed != 0;
  }
  {  // ConsistentTracks: perfect tracks
    TrackBuilder builder(kMinTrackLength, 10);
    for (int i = 0; i < 4; i++) builder.AddFeatureCorrespondence(pairs[i][0], Feature(i, i), pairs[i][1], Feature(i, i));
    Reconstruction reconstruction;
    AddViews(&reconstruction, 3);
    CHECK(builder.BuildTracks(&reconstruction));
    VerifyTracks(reconstruction);
    CHECK(reconstruction.NumTracks() == 4);
    // deterministic TrackIds: track i is the i-th correspondence
    for (int i = 0; i < 4; i++) {
      const Feature* f = reconstruction.View(pairs[i][0])->GetFeature(i);
      CHECK(f != nullptr && f->x() == i && f->y() == i);
    }
  }
  {  // SingletonTracks: a small max track length forces a singleton
    TrackBuilder builder(kMinTrackLength, 2);
    builder.AddFeatureCorrespondence(0, Feature(0, 0), 1, Feature(0, 0));
    builder.AddFeatureCorrespondence(1, Feature(0, 0), 2, Feature(0, 0));
    Reconstruction reconstruction;
    AddViews(&reconstruction, 3);
    CHECK(builder.BuildTracks(&reconstruction));
    VerifyTracks(reconstruction);
    CHECK(reconstruction.NumTracks() == 1 && builder.num_small_tracks() == 1);
  }
  {  // InconsistentTracks
    TrackBuilder builder(kMinTrackLength, 10);
    for (int i = 0; i < 4; i++)
      builder.AddFeatureCorrespondence(pairs[i][0], Feature(0, 0), pairs[i][1], Feature(i + 1, i + 1));
    Reconstruction reconstruction;
    AddViews(&reconstruction, 3);
    CHECK(builder.BuildTracks(&reconstruction));
    VerifyTracks(reconstruction);
    CHECK(reconstruction.NumTracks() == 2 && builder.num_inconsistent_features() == 2);
  }
  {  // MaxTrackLength: tracks limited by size
    TrackBuilder builder(kMinTrackLength, 2);
    for (int i = 0; i < 5; i++) builder.AddFeatureCorrespondence(i, Feature(0, 0), i + 1, Feature(0, 0));
    Reconstruction reconstruction;
    AddViews(&reconstruction, 6);
    CHECK(builder.BuildTracks(&reconstruction));
    VerifyTracks(reconstruction);
    CHECK(reconstruction.NumTracks() == 3);
  }
  {  // MinTrackLength
    TrackBuilder builder(3, 10);
    for (int i = 0; i < 5; i++) builder.AddFeatureCorrespondence(i, Feature(0, 0), i + 1, Feature(0, 0));
    builder.AddFeatureCorrespondence(0, Feature(1, 1), 1, Feature(1, 1));
    Reconstruction reconstruction;
    AddViews(&reconstruction, 6);
    CHECK(builder.BuildTracks(&reconstruction));
    VerifyTracks(reconstruction);
    CHECK(reconstruction.NumTracks() == 1 && reconstruction.Track(0)->NumViews() == 6);
  }
  {  // bulk add == single adds; -0.0 names the feature 0.0 names
    TrackBuilder single(kMinTrackLength, 4), bulk(kMinTrackLength, 4);
    unsigned state = 12345u;
    auto next = [&state](unsigned n) {
      state = state * 1664525u + 1013904223u;
      return (state >> 8) % n;
    };
    for (ViewId a = 0; a < 6; ++a)
      for (ViewId b = a + 1; b < 6; ++b) {
        std::vector<FeatureCorrespondence> c;
        for (int i = 0; i < 12; ++i) {
          const double f = next(10);
          c.emplace_back(Feature(f == 0 && i % 2 ? -0.0 : f, 2 * f), Feature(next(5) ? f : f + 1, next(5) ? 2 * f : 2 * f + 2));
        }
        bulk.AddFeatureCorrespondences(a, b, c);
        for (const FeatureCorrespondence& k : c) single.AddFeatureCorrespondence(a, k.feature1, b, k.feature2);
      }
    Reconstruction r1, r2;
    AddViews(&r1, 6);
    AddViews(&r2, 6);
    CHECK(single.BuildTracks(&r1) && bulk.BuildTracks(&r2));
    VerifyTracks(r1);
    CHECK(r1.NumTracks() > 4 && r1.NumTracks() == r2.NumTracks() && Flatten(r1) == Flatten(r2));
    CHECK(single.num_small_tracks() == bulk.num_small_tracks() &&
          single.num_inconsistent_features() == bulk.num_inconsistent_features());
    TrackBuilder zero(kMinTrackLength, 10);
    zero.AddFeatureCorrespondence(0, Feature(0.0, 0.0), 1, Feature(3, 3));
    zero.AddFeatureCorrespondence(0, Feature(-0.0, -0.0), 2, Feature(4, 4));
    Reconstruction r3;
    AddViews(&r3, 3);
    CHECK(zero.BuildTracks(&r3) && r3.NumTracks() == 1 && r3.Track(0)->NumViews() == 3);
  }
  {  // an unknown view, and a correspondence inside one view: false, nothing written
    TrackBuilder builder(kMinTrackLength, 10);
    builder.AddFeatureCorrespondence(0, Feature(0, 0), 1, Feature(0, 0));
    builder.AddFeatureCorrespondence(1, Feature(1, 1), 3, Feature(1, 1));
    Reconstruction reconstruction;
    AddViews(&reconstruction, 3);
    CHECK(!builder.BuildTracks(&reconstruction));
    CHECK(reconstruction.NumTracks() == 0 && reconstruction.View(0)->TrackIds().empty());
    reconstruction.AddView("3");
    CHECK(builder.BuildTracks(&reconstruction) && reconstruction.NumTracks() == 2);
    TrackBuilder same(kMinTrackLength, 10);
    same.AddFeatureCorrespondence(0, Feature(0, 0), 1, Feature(0, 0));
    same.AddFeatureCorrespondence(2, Feature(0, 0), 2, Feature(1, 1));
    Reconstruction other;
    AddViews(&other, 3);
    CHECK(!same.BuildTracks(&other) && other.NumTracks() == 0);
  }
  std::printf(g_failed ? "track builder shim: FAILED\n" : "track builder shim: OK (device)\n");
  return g_failed != 0;
}
