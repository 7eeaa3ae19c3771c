// Host shim of theia::OptimizeRelativePositionWithKnownRotation (reference
// optimize_relative_position_with_known_rotation.cc:53-197) and of its caller
// RefineRelativeTranslationsWithKnownRotations (reconstruction_estimator_utils.cc:244-269) on the C
// ABI: the pairs are flattened into one tmi_ba_relative_position_batch -- a rotation per view, an
// edge list, the correspondences of every edge -- and solved in one device launch.
#include <cstdio>
#include <vector>

#include "theia/sfm/bundle_adjustment/optimize_relative_position_with_known_rotation.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
// The flattened batch and the call.  status[p] as tmi_ba_optimize_relative_positions writes it, -1 where the call failed.
struct FlatBatch {
  std::vector<double> rotation, intrinsics, f1, f2, position;
  std::vector<int32_t> model, view1, view2;
  std::vector<int64_t> ptr = {0};
  int AddView(const Eigen::Vector3d& r) {
    for (int a = 0; a < 3; ++a) rotation.push_back(r[a]);
    return static_cast<int>(rotation.size() / 3) - 1;
  }
  void AddCorrespondence(const Feature& a, const Feature& b) {
    f1.push_back(a.x());
    f1.push_back(a.y());
    f2.push_back(b.x());
    f2.push_back(b.y());
  }
  void ClosePair(int v1, int v2) {
    view1.push_back(v1);
    view2.push_back(v2);
    ptr.push_back(static_cast<int64_t>(f1.size() / 2));
  }
  std::vector<int8_t> Run(int device) {
    const size_t P = view1.size();
    std::vector<int8_t> status(P, -1);
    if (P == 0) return status;
    position.assign(3 * P, 0.0);
    tmi_ba_relative_position_batch B;
    B.num_views = static_cast<int32_t>(rotation.size() / 3);
    B.view_rotation = rotation.data();
    B.view_model = model.empty() ? nullptr : model.data();
    B.view_intrinsics = model.empty() ? nullptr : intrinsics.data();
    B.num_pairs = static_cast<int32_t>(P);
    B.pair_view1 = view1.data();
    B.pair_view2 = view2.data();
    B.correspondence_ptr = ptr.data();
    B.features1 = f1.data();
    B.features2 = f2.data();
    B.position2 = position.data();
    tmi_ba_track_batch_summary bs;
    const int rc = tmi_ba_optimize_relative_positions(&B, device, status.data(), nullptr, nullptr, nullptr, &bs);
    if (rc != TMI_BA_OK) {
      std::fprintf(stderr, "[theia::OptimizeRelativePositionWithKnownRotation] device batch failed: %s\n",
                   tmi_ba_last_error());
      status.assign(P, -1);
    }
    return status;
  }
};
}  // namespace

std::vector<bool> OptimizeRelativePositionsWithKnownRotationsBatch(std::vector<RelativePositionProblem>* problems,
                                                                   int device) {
  std::vector<bool> ok;
  if (problems == nullptr || problems->empty()) return ok;
  const size_t P = problems->size();
  ok.assign(P, false);
  FlatBatch flat;
  for (const RelativePositionProblem& q : *problems) {
    const int v1 = flat.AddView(q.rotation1), v2 = flat.AddView(q.rotation2);
    // the reference CHECK-fails on a null argument; the shim reports failure (an empty pair)
    if (q.correspondences != nullptr && q.relative_position != nullptr)
      for (const FeatureCorrespondence& m : *q.correspondences) flat.AddCorrespondence(m.feature1, m.feature2);
    flat.ClosePair(v1, v2);
  }
  const std::vector<int8_t> status = flat.Run(device);
  for (size_t p = 0; p < P; ++p) {
    if (status[p] != 0 && status[p] != 1) continue;  // the reference returns true for both
    ok[p] = true;
    for (int a = 0; a < 3; ++a) (*(*problems)[p].relative_position)[a] = flat.position[3 * p + a];
  }
  return ok;
}

bool OptimizeRelativePositionWithKnownRotation(const std::vector<FeatureCorrespondence>& correspondences,
                                               const Eigen::Vector3d& rotation1, const Eigen::Vector3d& rotation2,
                                               Eigen::Vector3d* relative_position) {
  std::vector<RelativePositionProblem> one(1);
  one[0].correspondences = &correspondences;
  one[0].rotation1 = rotation1;
  one[0].rotation2 = rotation2;
  one[0].relative_position = relative_position;
  const std::vector<bool> r = OptimizeRelativePositionsWithKnownRotationsBatch(&one);
  return !r.empty() && r[0];
}

int RefineRelativeTranslationsWithKnownRotations(const Reconstruction& reconstruction,
                                                 const std::unordered_map<ViewId, Eigen::Vector3d>& orientations,
                                                 std::vector<std::pair<ViewIdPair, TwoViewInfo*>>* edges, int device) {
  if (edges == nullptr || edges->empty()) return 0;
  FlatBatch flat;
  std::unordered_map<ViewId, int> index;  // ViewId -> row of the view tables
  auto view_row = [&](const ViewId id) -> int {
    const auto found = index.find(id);
    if (found != index.end()) return found->second;
    const View* view = reconstruction.View(id);
    const auto orientation = orientations.find(id);
    if (view == nullptr || orientation == orientations.end()) return index[id] = -1;
    const Camera& camera = view->Camera();
    flat.model.push_back(static_cast<int32_t>(camera.GetCameraIntrinsicsModelType()));
    const int n = camera.CameraIntrinsics()->NumParameters();
    for (int a = 0; a < TMI_BA_MAX_INTRINSICS; ++a) flat.intrinsics.push_back(a < n ? camera.intrinsics()[a] : 0.0);
    return index[id] = flat.AddView(orientation->second);
  };
  std::vector<size_t> edge_of_pair;
  for (size_t e = 0; e < edges->size(); ++e) {
    const ViewIdPair& ids = (*edges)[e].first;
    if ((*edges)[e].second == nullptr) continue;
    const int v1 = view_row(ids.first), v2 = view_row(ids.second);
    if (v1 < 0 || v2 < 0) continue;
    const View* view1 = reconstruction.View(ids.first);
    const View* view2 = reconstruction.View(ids.second);
    // GetNormalizedFeatureCorrespondences (:65-91) without the normalisation: the device does it
    for (const TrackId track_id : view1->TrackIds()) {
      const Feature* feature2 = view2->GetFeature(track_id);
      if (feature2 == nullptr) continue;
      flat.AddCorrespondence(*view1->GetFeature(track_id), *feature2);
    }
    flat.ClosePair(v1, v2);
    edge_of_pair.push_back(e);
  }
  const std::vector<int8_t> status = flat.Run(device);
  int written = 0;
  for (size_t p = 0; p < edge_of_pair.size(); ++p) {
    if (status[p] != 0 && status[p] != 1) continue;
    TwoViewInfo* info = (*edges)[edge_of_pair[p]].second;
    for (int a = 0; a < 3; ++a) info->position_2[a] = flat.position[3 * p + a];
    ++written;
  }
  return written;
}

}  // namespace theia
