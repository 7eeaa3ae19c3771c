// tests/test_host_shim_nonlinear_rotation.py: the nonlinear rotation estimator shim
// (theiasfm_amd/host/nonlinear_rotation_ops.cc).
//   always:           the default loss width is the reference's (0.1); an empty map and empty pairs return false and
//                     leave the map as it is.
//   without a device: EstimateRotations returns false and leaves the map as it is.
//   with a device:    a 12-view noisy graph in which one view is absent from the map: it stays absent, the others
//                     change, and the result equals the C ABI called on the same flattened input -- views in ascending
//                     ViewId order, the absent one unmarked, pairs in ascending ViewIdPair order, no view held -- bit for
//                     bit.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "theia/sfm/global_pose_estimation/nonlinear_rotation_estimator.h"
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
using Pairs = std::unordered_map<ViewIdPair, TwoViewInfo>;

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

  // ---- the defaults: the reference's constructor and nonlinear_rotation_estimator.cc:94 --------------------------------
  tmi_ba_nonlinear_rotation_options abi_options;
  tmi_ba_nonlinear_rotation_options_init(&abi_options);
  CHECK(abi_options.robust_loss_width == 0.1 && abi_options.max_num_iterations == 200 && abi_options.fixed_view == -1);
  theia::NonlinearRotationEstimator estimator;
  theia::NonlinearRotationEstimator wide(0.25);
  CHECK(estimator.device == -1 && wide.device == -1);
  theia::RotationEstimator* base = &estimator;  // the interface class

  // ---- 12 views on scattered ids, a ring with chords; small rotations, so that rotation_2 = x2 - x1 plus noise is a
  //      relative rotation with an error of a few hundredths of a radian.  View 77 has pairs and no orientation. ---------
  const std::vector<ViewId> ids = {5, 9, 14, 20, 33, 41, 58, 77, 90, 101, 250, 999};
  Lcg rng{97531};
  Vectors truth, start;
  for (const ViewId id : ids)
    for (int a = 0; a < 3; ++a) {
      truth[id][a] = 0.1 * rng.next();
      if (id != 77) start[id][a] = truth[id][a] + 0.05 * rng.next();
    }
  Pairs view_pairs;
  for (size_t i = 0; i < ids.size(); ++i)
    for (const size_t step : {size_t(1), size_t(3)}) {
      const ViewId a = ids[i], b = ids[(i + step) % ids.size()];
      TwoViewInfo info;
      for (int k = 0; k < 3; ++k) info.rotation_2[k] = truth[std::max(a, b)][k] - truth[std::min(a, b)][k] + 0.01 * rng.next();
      view_pairs[ViewIdPair(std::min(a, b), std::max(a, b))] = info;
    }
  CHECK(view_pairs.size() == 24 && start.size() == 11);

  // ---- the two refusals: false, nothing written, with or without a device ---------------------------------------------------
  {
    Vectors o = start, none;
    CHECK(!base->EstimateRotations(view_pairs, &none) && none.empty());  // :53-57
    CHECK(!base->EstimateRotations({}, &o) && SameBits(o, start));       // :58-62
    CHECK(!base->EstimateRotations(view_pairs, nullptr));
  }
  if (!have_device) {
    Vectors o = start;
    CHECK(!base->EstimateRotations(view_pairs, &o));
    CHECK(SameBits(o, start));
    std::printf("nonlinear rotation estimator shim without a device: OK\n");
    return 0;
  }

  // ---- the C ABI on the flattened input, built independently of the shim -----------------------------------------------------
  std::vector<std::pair<ViewIdPair, TwoViewInfo>> sorted(view_pairs.begin(), view_pairs.end());
  std::sort(sorted.begin(), sorted.end(),
            [](const std::pair<ViewIdPair, TwoViewInfo>& a, const std::pair<ViewIdPair, TwoViewInfo>& b) {
              return a.first < b.first;
            });
  auto index = [&](ViewId id) { return static_cast<int32_t>(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); };
  std::vector<int32_t> view1, view2;
  std::vector<double> relative, rotation(36, 0.0);
  std::vector<uint8_t> given(12, 1);
  for (const auto& edge : sorted) {
    view1.push_back(index(edge.first.first));
    view2.push_back(index(edge.first.second));
    for (int a = 0; a < 3; ++a) relative.push_back(edge.second.rotation_2[a]);
  }
  given[index(77)] = 0;
  for (size_t i = 0; i < ids.size(); ++i)
    if (given[i])
      for (int a = 0; a < 3; ++a) rotation[3 * i + a] = start.at(ids[i])[a];
  tmi_ba_view_pair_batch B;
  B.num_views = 12;
  B.view_rotation = nullptr;
  B.num_pairs = 24;
  B.pair_view1 = view1.data();
  B.pair_view2 = view2.data();
  B.pair_rotation2 = relative.data();
  B.pair_position2 = nullptr;
  tmi_ba_nonlinear_rotation_summary summary;
  CHECK(tmi_ba_estimate_global_rotations_nonlinear(&B, &abi_options, given.data(), -1, rotation.data(), nullptr, nullptr,
                                                   nullptr, nullptr, &summary) == TMI_BA_OK);
  CHECK(summary.num_views == 11 && summary.num_pairs == 20 && summary.usable && summary.num_iterations >= 1);
  CHECK(summary.final_cost < summary.initial_cost);
  Vectors want;
  for (size_t i = 0; i < ids.size(); ++i)
    if (given[i])
      for (int a = 0; a < 3; ++a) want[ids[i]][a] = rotation[3 * i + a];

  // ---- the shim ------------------------------------------------------------------------------------------------------------
  Vectors got = start;
  CHECK(base->EstimateRotations(view_pairs, &got));
  CHECK(got.size() == 11 && got.count(ViewId(77)) == 0);  // the view without an initialisation stays absent
  for (const auto& e : start) CHECK(std::memcmp(&e.second[0], &got.at(e.first)[0], 3 * sizeof(double)) != 0);  // all change
  CHECK(SameBits(got, want));
  Vectors other = start;  // another width is another problem
  CHECK(wide.EstimateRotations(view_pairs, &other) && other.size() == 11 && !SameBits(other, want));
  std::printf("nonlinear rotation estimator shim: OK\n");
  return 0;
}
