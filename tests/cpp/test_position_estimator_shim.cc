// tests/test_host_shim_position_estimator.py: the position estimator shim (theiasfm_amd/host/position_ops.cc).
//   without a device: EstimatePositions returns false and leaves the position map as it is.
//   with a device:    the shim equals the C ABI called on the pairs between oriented views, in ascending ViewIdPair
//                     order, with the views numbered in ascending ViewId order and the smallest id fixed, bit for bit;
//                     pairs with a view without an orientation are dropped; a failed call leaves the map unchanged.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "theia/sfm/global_pose_estimation/least_unsquared_deviation_position_estimator.h"
#include "theia_mi355_ba.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      return 1;                                                            \
    }                                                                      \
  } while (0)

using theia::TwoViewInfo;
using theia::ViewId;
using theia::ViewIdPair;
using Vectors = std::unordered_map<ViewId, Eigen::Vector3d>;

namespace {
struct Lcg {
  unsigned long long s;
  double next() {  // uniform in [-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(s >> 11) / 4503599627370496.0 - 1.0;
  }
};

bool SameBits(const Vectors& a, const Vectors& b) {
  if (a.size() != b.size()) return false;
  for (const auto& e : a) {
    const auto it = b.find(e.first);
    if (it == b.end()) return false;
    for (int k = 0; k < 3; ++k)
      if (std::memcmp(&e.second[k], &it->second[k], sizeof(double)) != 0) return false;
  }
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  const bool have_device = tmi_ba_device_count() > 0;
  CHECK(have_device || !need_device);

  // views on scattered ids (NOT ascending) with small orientations and positions in a box; unit directions from the
  // positions with a little noise, in an order unrelated to the ids; view 4242 has pairs but no orientation
  const std::vector<ViewId> ids = {50, 7, 300, 12, 9, 1000, 3, 77};
  Lcg rng{9876};
  Vectors orientations, truth;
  for (const ViewId id : ids)
    for (int a = 0; a < 3; ++a) {
      orientations[id][a] = 0.1 * rng.next();
      truth[id][a] = 10.0 * rng.next();
    }
  truth[4242] = Eigen::Vector3d::Zero();
  const ViewId pairs[][2] = {{50, 7},  {300, 7},  {300, 12}, {9, 12},   {9, 1000}, {3, 1000}, {3, 77},
                             {50, 77}, {50, 9},   {1000, 7}, {12, 77},  {300, 3},  {7, 4242}, {4242, 1000}};
  const int n = static_cast<int>(sizeof(pairs) / sizeof(pairs[0]));
  std::unordered_map<ViewIdPair, TwoViewInfo> view_pairs;
  for (int e = 0; e < n; ++e) {
    TwoViewInfo info;
    double norm = 0.0;
    for (int a = 0; a < 3; ++a) {
      info.position_2[a] = truth[pairs[e][1]][a] - truth[pairs[e][0]][a] + 0.05 * rng.next();
      norm += info.position_2[a] * info.position_2[a];
    }
    for (int a = 0; a < 3; ++a) info.position_2[a] /= std::sqrt(norm);
    view_pairs[ViewIdPair(pairs[e][0], pairs[e][1])] = info;
  }
  CHECK(static_cast<int>(view_pairs.size()) == n);
  theia::LeastUnsquaredDeviationPositionEstimator::Options options;
  CHECK(options.max_num_iterations == 400 && options.max_num_reweighted_iterations == 10);
  CHECK(options.convergence_criterion == 1e-4 && options.device == -1);
  Vectors start;
  start[ViewId(1)] = Eigen::Vector3d::Zero();
  start[ViewId(1)][1] = 5.0;  // what a failed call must leave in place, and a successful one must clear

  if (!have_device) {
    Vectors p = start;
    theia::LeastUnsquaredDeviationPositionEstimator estimator(options);
    theia::PositionEstimator* base = &estimator;  // the interface class
    CHECK(!base->EstimatePositions(view_pairs, orientations, &p));
    CHECK(SameBits(p, start));
    std::printf("position estimator shim without a device: OK\n");
    return 0;
  }

  // ---- the C ABI on ascending ids, built independently of the shim ---------------------------------------------------
  std::vector<ViewId> sorted = ids;
  std::sort(sorted.begin(), sorted.end());
  auto index = [&](ViewId id) {
    return static_cast<int32_t>(std::lower_bound(sorted.begin(), sorted.end(), id) - sorted.begin());
  };
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> ordered;  // ascending (view1, view2), oriented views only
  for (const auto& vp : view_pairs)
    if (vp.first.first != 4242 && vp.first.second != 4242) ordered.emplace_back(vp.first, vp.second.position_2);
  std::sort(ordered.begin(), ordered.end(),
            [](const std::pair<ViewIdPair, Eigen::Vector3d>& a, const std::pair<ViewIdPair, Eigen::Vector3d>& b) {
              return a.first < b.first;
            });
  CHECK(static_cast<int>(ordered.size()) == n - 2);
  std::vector<int32_t> view1, view2;
  std::vector<double> position2, rotation;
  for (const auto& c : ordered) {
    view1.push_back(index(c.first.first));
    view2.push_back(index(c.first.second));
    for (int a = 0; a < 3; ++a) position2.push_back(c.second[a]);
  }
  for (const ViewId id : sorted)
    for (int a = 0; a < 3; ++a) rotation.push_back(orientations.at(id)[a]);
  CHECK(index(50) == 4 && index(3) == 0);  // ids {3, 7, 9, 12, 50, 77, 300, 1000}
  tmi_ba_view_pair_batch B;
  B.num_views = static_cast<int32_t>(sorted.size());
  B.view_rotation = rotation.data();
  B.num_pairs = n - 2;
  B.pair_view1 = view1.data();
  B.pair_view2 = view2.data();
  B.pair_rotation2 = nullptr;
  B.pair_position2 = position2.data();
  tmi_ba_lud_position_options o;
  tmi_ba_lud_position_options_init(&o);
  tmi_ba_lud_position_summary summary;
  std::vector<double> position(3 * sorted.size(), 7.0);
  CHECK(tmi_ba_estimate_global_positions_lud(&B, &o, 0, -1, position.data(), nullptr, nullptr, nullptr, nullptr,
                                             &summary) == TMI_BA_OK);
  CHECK(summary.num_views == 8 && summary.num_pairs == n - 2 && summary.num_admm_iterations >= 1);
  Vectors want;
  for (size_t i = 0; i < sorted.size(); ++i)
    for (int a = 0; a < 3; ++a) want[sorted[i]][a] = position[3 * i + a];
  for (int a = 0; a < 3; ++a) CHECK(want[3][a] == 0.0);  // the smallest id is the fixed view
  CHECK(want[50][0] != 0.0 && want[50][0] != 7.0);

  // ---- the shim ---------------------------------------------------------------------------------------------------------
  {
    Vectors got = start;
    theia::LeastUnsquaredDeviationPositionEstimator estimator(options);
    CHECK(estimator.EstimatePositions(view_pairs, orientations, &got));
    CHECK(got.size() == 8 && got.count(ViewId(1)) == 0 && got.count(ViewId(4242)) == 0);  // cleared, then filled
    CHECK(SameBits(got, want));
    // the estimator's own options are only checked: other positive values change nothing
    theia::LeastUnsquaredDeviationPositionEstimator::Options other = options;
    other.max_num_iterations = 3;
    other.convergence_criterion = 0.5;
    Vectors again;
    theia::LeastUnsquaredDeviationPositionEstimator second(other);
    CHECK(second.EstimatePositions(view_pairs, orientations, &again) && SameBits(again, want));
  }
  // fewer orientations: fewer views; errors: false, the map unchanged
  {
    Vectors p = start;
    Vectors fewer = orientations;  // without 3, 77 and 50 the cycle 7 - 300 - 12 - 9 - 1000 - 7 remains
    fewer.erase(ViewId(3));
    fewer.erase(ViewId(77));
    fewer.erase(ViewId(50));
    theia::LeastUnsquaredDeviationPositionEstimator estimator(options);
    CHECK(estimator.EstimatePositions(view_pairs, fewer, &p) && p.size() == 5);
    p = start;
    Vectors split = orientations;  // without 50, 12 and 1000 view 9 has no pair left and 7 - 300 - 3 - 77 remains
    split.erase(ViewId(50));
    split.erase(ViewId(12));
    split.erase(ViewId(1000));
    CHECK(estimator.EstimatePositions(view_pairs, split, &p) && p.size() == 4 && p.count(ViewId(9)) == 0);
    p = start;
    std::unordered_map<ViewIdPair, TwoViewInfo> two_parts;  // two components
    two_parts[ViewIdPair(50, 7)] = view_pairs[ViewIdPair(50, 7)];
    two_parts[ViewIdPair(300, 12)] = view_pairs[ViewIdPair(300, 12)];
    CHECK(!estimator.EstimatePositions(two_parts, orientations, &p) && SameBits(p, start));
    CHECK(!estimator.EstimatePositions({}, orientations, &p) && SameBits(p, start));
    CHECK(!estimator.EstimatePositions(view_pairs, {}, &p) && SameBits(p, start));
    theia::LeastUnsquaredDeviationPositionEstimator::Options bad = options;
    bad.max_num_reweighted_iterations = 0;  // the reference CHECK_GTs it
    theia::LeastUnsquaredDeviationPositionEstimator refused(bad);
    CHECK(!refused.EstimatePositions(view_pairs, orientations, &p) && SameBits(p, start));
  }
  std::printf("position estimator shim: OK\n");
  return 0;
}
