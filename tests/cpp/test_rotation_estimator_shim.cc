// tests/test_host_shim_rotation_estimator.py: the rotation estimator shim (theiasfm_amd/host/rotation_ops.cc).
//   without a device: both interfaces return false and leave the orientation map as it is.
//   with a device:    the shim equals the C ABI called on the same constraints with the views numbered in ascending
//                     ViewId order and the smallest id fixed, bit for bit; the map form equals the one-by-one form on
//                     the pairs in ascending order; a constraint on a view without an orientation is an error.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "theia/sfm/global_pose_estimation/robust_rotation_estimator.h"
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
using Orientations = std::unordered_map<ViewId, Eigen::Vector3d>;

namespace {
struct Lcg {
  unsigned long long s;
  double next() {  // uniform in [-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(s >> 11) / 4503599627370496.0 - 1.0;
  }
};

bool SameBits(const Orientations& a, const Orientations& b) {
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

  // views on scattered ids (NOT ascending) with small orientations; small relative rotations (consistent or not: the
  // arithmetic is what is compared), in an order unrelated to the ids
  const std::vector<ViewId> ids = {50, 7, 300, 12, 9, 1000, 3, 77};
  Lcg rng{4321};
  Orientations start;
  for (const ViewId id : ids)
    for (int a = 0; a < 3; ++a) start[id][a] = 0.1 * rng.next();
  const int pairs[][2] = {{0, 1}, {2, 1}, {2, 3}, {4, 3}, {4, 5}, {6, 5}, {6, 7}, {0, 7}, {0, 4}, {5, 1}, {3, 7}, {2, 6}};
  const int n = static_cast<int>(sizeof(pairs) / sizeof(pairs[0]));
  std::unordered_map<ViewIdPair, TwoViewInfo> view_pairs;
  for (int e = 0; e < n; ++e) {
    TwoViewInfo info;
    for (int a = 0; a < 3; ++a) info.rotation_2[a] = 0.05 * rng.next();
    view_pairs[ViewIdPair(ids[pairs[e][0]], ids[pairs[e][1]])] = info;
  }
  CHECK(static_cast<int>(view_pairs.size()) == n);
  theia::RobustRotationEstimator::Options options;
  CHECK(options.max_num_l1_iterations == 5 && options.max_num_irls_iterations == 100);
  CHECK(options.l1_step_convergence_threshold == 0.001 && options.irls_step_convergence_threshold == 0.001);
  CHECK(std::fabs(options.irls_loss_parameter_sigma - 5.0 * M_PI / 180.0) < 1e-16);

  if (!have_device) {
    Orientations o = start;
    theia::RobustRotationEstimator by_map(options);
    CHECK(!by_map.EstimateRotations(view_pairs, &o));
    CHECK(SameBits(o, start));
    theia::RobustRotationEstimator one_by_one(options);
    for (const auto& vp : view_pairs) one_by_one.AddRelativeRotationConstraint(vp.first, vp.second.rotation_2);
    theia::RotationEstimator* base = &one_by_one;  // the interface class
    CHECK(!one_by_one.EstimateRotations(&o) && !base->EstimateRotations({}, &o));
    CHECK(SameBits(o, start));
    std::printf("rotation estimator shim without a device: OK\n");
    return 0;
  }

  // ---- the C ABI on ascending ids, built independently of the shim ---------------------------------------------------
  std::vector<ViewId> sorted = ids;
  std::sort(sorted.begin(), sorted.end());
  auto index = [&](ViewId id) {
    return static_cast<int32_t>(std::lower_bound(sorted.begin(), sorted.end(), id) - sorted.begin());
  };
  std::vector<std::pair<ViewIdPair, Eigen::Vector3d>> ordered;  // ascending (view1, view2): the map form's order
  for (const auto& vp : view_pairs) ordered.emplace_back(vp.first, vp.second.rotation_2);
  std::sort(ordered.begin(), ordered.end(),
            [](const std::pair<ViewIdPair, Eigen::Vector3d>& a, const std::pair<ViewIdPair, Eigen::Vector3d>& b) {
              return a.first < b.first;
            });
  std::vector<int32_t> view1, view2;
  std::vector<double> relative, rotation;
  for (const auto& c : ordered) {
    view1.push_back(index(c.first.first));
    view2.push_back(index(c.first.second));
    for (int a = 0; a < 3; ++a) relative.push_back(c.second[a]);
  }
  for (const ViewId id : sorted)
    for (int a = 0; a < 3; ++a) rotation.push_back(start.at(id)[a]);
  CHECK(index(50) == 4 && index(3) == 0);  // ids {3, 7, 9, 12, 50, 77, 300, 1000}
  tmi_ba_relative_rotation_batch B;
  B.num_views = static_cast<int32_t>(sorted.size());
  B.num_pairs = n;
  B.pair_view1 = view1.data();
  B.pair_view2 = view2.data();
  B.pair_rotation = relative.data();
  tmi_ba_robust_rotation_options o;
  tmi_ba_robust_rotation_options_init(&o);
  tmi_ba_robust_rotation_summary summary;
  CHECK(tmi_ba_estimate_global_rotations_robust(&B, &o, 0, -1, rotation.data(), nullptr, nullptr, nullptr, nullptr,
                                                nullptr, &summary) == TMI_BA_OK);
  CHECK(summary.num_views == 8 && summary.num_pairs == n && summary.num_irls_iterations >= 1);
  Orientations want;
  for (size_t i = 0; i < sorted.size(); ++i)
    for (int a = 0; a < 3; ++a) want[sorted[i]][a] = rotation[3 * i + a];
  CHECK(!SameBits(want, start));
  for (int a = 0; a < 3; ++a) CHECK(want[3][a] == start[3][a]);  // the smallest id is the fixed view

  // ---- both interfaces ------------------------------------------------------------------------------------------------
  {
    Orientations got = start;
    theia::RobustRotationEstimator by_map(options);
    CHECK(by_map.EstimateRotations(view_pairs, &got));
    CHECK(SameBits(got, want));
    Orientations again = start;
    theia::RobustRotationEstimator one_by_one(options);
    for (const auto& c : ordered) one_by_one.AddRelativeRotationConstraint(c.first, c.second);
    CHECK(one_by_one.EstimateRotations(&again));
    CHECK(SameBits(again, want));
  }
  // a pair twice and in either direction is accepted (robust_rotation_estimator.h:93-103)
  {
    Orientations got = start;
    theia::RobustRotationEstimator twice(options);
    for (const auto& c : ordered) twice.AddRelativeRotationConstraint(c.first, c.second);
    Eigen::Vector3d back;
    for (int a = 0; a < 3; ++a) back[a] = -ordered[0].second[a];
    twice.AddRelativeRotationConstraint(ViewIdPair(ordered[0].first.second, ordered[0].first.first), back);
    twice.AddRelativeRotationConstraint(ordered[1].first, ordered[1].second);
    CHECK(twice.EstimateRotations(&got));
    CHECK(!SameBits(got, start));
  }
  // errors: false, the map unchanged
  {
    Orientations fewer = start;
    fewer.erase(ViewId(300));  // a constraint on a view without an orientation
    const Orientations before = fewer;
    theia::RobustRotationEstimator missing(options);
    CHECK(!missing.EstimateRotations(view_pairs, &fewer));
    CHECK(SameBits(fewer, before));
    Orientations more = start;
    more[ViewId(5000)] = Eigen::Vector3d::Zero();  // a view that no constraint reaches
    const Orientations before_more = more;
    theia::RobustRotationEstimator lonely(options);
    CHECK(!lonely.EstimateRotations(view_pairs, &more));
    CHECK(SameBits(more, before_more));
    Orientations none = start;
    theia::RobustRotationEstimator empty(options);
    CHECK(!empty.EstimateRotations(&none) && SameBits(none, start));
  }
  std::printf("rotation estimator shim: OK\n");
  return 0;
}
