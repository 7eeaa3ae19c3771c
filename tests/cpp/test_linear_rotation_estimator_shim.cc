// tests/test_host_shim_linear_rotation.py: the linear rotation estimator shim
// (theiasfm_amd/host/linear_rotation_ops.cc).
//   always:           the defaults are Spectra's (1000 iterations, 1e-10); no constraints, a pair added twice and
//                     constraints that are not connected return false and leave the map as it is.
//   without a device: EstimateRotations returns false and leaves the map as it is.
//   with a device:    a 12-view noisy graph: the result equals the C ABI called on the same flattened input -- views in
//                     ascending ViewId order, pairs in ascending ViewIdPair order -- bit for bit; a key present
//                     beforehand keeps its value; AddRelativeRotationConstraint + EstimateRotations(&map) equals the
//                     one-call form.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "theia/sfm/global_pose_estimation/linear_rotation_estimator.h"
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

  // ---- the defaults: Spectra's, which linear_rotation_estimator.cc:173-177 leaves alone -------------------------------------
  tmi_ba_linear_rotation_options abi_options;
  tmi_ba_linear_rotation_options_init(&abi_options);
  CHECK(abi_options.max_iterations == 1000 && abi_options.tolerance == 1e-10 && abi_options.seed == 0);
  CHECK(abi_options.relative_shift > 0.0 && abi_options.relative_shift < 1e-6);
  theia::LinearRotationEstimator estimator;
  CHECK(estimator.device == -1);
  theia::RotationEstimator* base = &estimator;  // the interface class

  // ---- 12 views on scattered ids, a ring with chords; small rotations, so that rotation_2 = x2 - x1 plus noise is a
  //      relative rotation with an error of a few hundredths of a radian ----------------------------------------------------
  const std::vector<ViewId> ids = {5, 9, 14, 20, 33, 41, 58, 77, 90, 101, 250, 999};
  Lcg rng{97531};
  Vectors truth;
  for (const ViewId id : ids)
    for (int a = 0; a < 3; ++a) truth[id][a] = 0.1 * rng.next();
  Pairs view_pairs;
  for (size_t i = 0; i < ids.size(); ++i)
    for (const size_t step : {size_t(1), size_t(3)}) {
      const ViewId a = ids[i], b = ids[(i + step) % ids.size()];
      TwoViewInfo info;
      for (int k = 0; k < 3; ++k) info.rotation_2[k] = truth[std::max(a, b)][k] - truth[std::min(a, b)][k] + 0.01 * rng.next();
      view_pairs[ViewIdPair(std::min(a, b), std::max(a, b))] = info;
    }
  CHECK(view_pairs.size() == 24);
  const Eigen::Vector3d kept(0.25, -0.5, 0.75);
  Vectors before;
  before[ViewId(33)] = kept;
  before[ViewId(4242)] = kept;  // a key the constraints do not name

  // ---- the refusals: false, nothing written, with or without a device -----------------------------------------------------
  {
    Vectors o = before;
    theia::LinearRotationEstimator none;
    CHECK(!none.EstimateRotations(&o) && SameBits(o, before));  // no constraints
    CHECK(!none.EstimateRotations(Pairs(), &o) && SameBits(o, before));
    CHECK(!none.EstimateRotations(nullptr));
    theia::LinearRotationEstimator twice;
    twice.AddRelativeRotationConstraint(ViewIdPair(1, 2), truth[5]);
    twice.AddRelativeRotationConstraint(ViewIdPair(2, 3), truth[9]);
    twice.AddRelativeRotationConstraint(ViewIdPair(1, 2), truth[5]);
    CHECK(!twice.EstimateRotations(&o) && SameBits(o, before));  // a pair added twice
    theia::LinearRotationEstimator apart;
    apart.AddRelativeRotationConstraint(ViewIdPair(1, 2), truth[5]);
    apart.AddRelativeRotationConstraint(ViewIdPair(3, 4), truth[9]);
    CHECK(!apart.EstimateRotations(&o) && SameBits(o, before));  // two components
  }
  if (!have_device) {
    Vectors o = before;
    CHECK(!base->EstimateRotations(view_pairs, &o));
    CHECK(SameBits(o, before));
    std::printf("linear rotation estimator shim without a device: OK\n");
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
  for (const auto& edge : sorted) {
    view1.push_back(index(edge.first.first));
    view2.push_back(index(edge.first.second));
    for (int a = 0; a < 3; ++a) relative.push_back(edge.second.rotation_2[a]);
  }
  tmi_ba_view_pair_batch B;
  B.num_views = 12;
  B.view_rotation = nullptr;
  B.num_pairs = 24;
  B.pair_view1 = view1.data();
  B.pair_view2 = view2.data();
  B.pair_rotation2 = relative.data();
  B.pair_position2 = nullptr;
  tmi_ba_linear_rotation_summary summary;
  CHECK(tmi_ba_estimate_global_rotations_linear(&B, &abi_options, -1, rotation.data(), &summary) == TMI_BA_OK);
  CHECK(summary.num_views == 12 && summary.num_pairs == 24 && summary.order == 36 && summary.usable && summary.converged);
  CHECK(summary.num_iterations >= 1 && (summary.num_reflected == 0 || summary.num_reflected == 12));
  CHECK(summary.eigenvalue[2] < 0.1 * summary.eigenvalue[3]);  // the gap
  Vectors want;
  for (size_t i = 0; i < ids.size(); ++i)
    for (int a = 0; a < 3; ++a) want[ids[i]][a] = rotation[3 * i + a];

  // ---- the shim ------------------------------------------------------------------------------------------------------------
  Vectors got;
  CHECK(base->EstimateRotations(view_pairs, &got));
  CHECK(got.size() == 12 && SameBits(got, want));
  // a key present beforehand keeps its value; the others are emplaced
  Vectors mixed = before;
  theia::LinearRotationEstimator again;
  CHECK(again.EstimateRotations(view_pairs, &mixed));
  CHECK(mixed.size() == 13);
  CHECK(std::memcmp(&mixed.at(ViewId(33))[0], &kept[0], 3 * sizeof(double)) == 0);
  CHECK(std::memcmp(&mixed.at(ViewId(4242))[0], &kept[0], 3 * sizeof(double)) == 0);
  for (const auto& e : want)
    if (e.first != ViewId(33)) CHECK(std::memcmp(&mixed.at(e.first)[0], &e.second[0], 3 * sizeof(double)) == 0);
  // constraint by constraint, in the map's own (unspecified) order
  theia::LinearRotationEstimator one_by_one;
  for (const auto& view_pair : view_pairs) one_by_one.AddRelativeRotationConstraint(view_pair.first, view_pair.second.rotation_2);
  Vectors stepwise;
  CHECK(one_by_one.EstimateRotations(&stepwise) && SameBits(stepwise, want));
  // the estimator keeps its constraints, as the reference's does: the same pairs again are pairs added twice
  Vectors repeat;
  CHECK(!base->EstimateRotations(view_pairs, &repeat) && repeat.empty());
  std::printf("linear rotation estimator shim: OK\n");
  return 0;
}
