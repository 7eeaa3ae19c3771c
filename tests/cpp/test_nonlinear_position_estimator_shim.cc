// tests/test_host_shim_nonlinear_position_estimator.py: the nonlinear position estimator shim
// (theiasfm_amd/host/nonlinear_position_ops.cc).
//   always:           the options' defaults are the reference's (nonlinear_position_estimator.h:70-81); every refusal
//                     returns false and leaves the position map as it is.
//   without a device: EstimatePositions returns false and leaves the position map as it is.
//   with a device:    the reference's 4-view / 6-pair scene within its bound after alignment; the shim equals the C ABI
//                     called on the pairs between oriented views, in ascending ViewIdPair order, with the views numbered
//                     in ascending ViewId order and the smallest id fixed, bit for bit; views without a kept pair are
//                     absent from the result.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "theia/sfm/global_pose_estimation/nonlinear_position_estimator.h"
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

// position_2 of a pair as the reference's test makes it without noise: R(orientation1) (c2 - c1) / |c2 - c1|, with
// Rodrigues' formula for the rotation
Eigen::Vector3d Direction(const Eigen::Vector3d& aa, const Eigen::Vector3d& c1, const Eigen::Vector3d& c2) {
  double d[3], norm = 0.0, theta = 0.0;
  for (int a = 0; a < 3; ++a) {
    d[a] = c2[a] - c1[a];
    norm += d[a] * d[a];
    theta += aa[a] * aa[a];
  }
  norm = std::sqrt(norm);
  theta = std::sqrt(theta);
  for (int a = 0; a < 3; ++a) d[a] /= norm;
  Eigen::Vector3d out;
  if (theta == 0.0) {
    for (int a = 0; a < 3; ++a) out[a] = d[a];
    return out;
  }
  const double w[3] = {aa[0] / theta, aa[1] / theta, aa[2] / theta};
  const double c = std::cos(theta), s = std::sin(theta);
  const double wd = w[0] * d[0] + w[1] * d[1] + w[2] * d[2];
  const double cross[3] = {w[1] * d[2] - w[2] * d[1], w[2] * d[0] - w[0] * d[2], w[0] * d[1] - w[1] * d[0]};
  for (int a = 0; a < 3; ++a) out[a] = d[a] * c + cross[a] * s + w[a] * wd * (1.0 - c);
  return out;
}

// The largest squared distance between gt and s est + t for the least-squares scale s and translation t.  The
// reference's test aligns by a similarity (AlignPointCloudsUmeyama); with the orientations given the estimate can only
// differ from the truth by scale and translation, and leaving the rotation out can only make the error larger.
double LargestSquaredErrorAfterAlignment(const std::vector<ViewId>& ids, const Vectors& gt, const Vectors& est) {
  double mean_g[3] = {0.0, 0.0, 0.0}, mean_e[3] = {0.0, 0.0, 0.0}, ge = 0.0, ee = 0.0;
  for (const ViewId id : ids)
    for (int k = 0; k < 3; ++k) {
      mean_g[k] += gt.at(id)[k] / static_cast<double>(ids.size());
      mean_e[k] += est.at(id)[k] / static_cast<double>(ids.size());
    }
  for (const ViewId id : ids)
    for (int k = 0; k < 3; ++k) {
      ge += (gt.at(id)[k] - mean_g[k]) * (est.at(id)[k] - mean_e[k]);
      ee += (est.at(id)[k] - mean_e[k]) * (est.at(id)[k] - mean_e[k]);
    }
  const double s = ge / ee;
  double worst = 0.0;
  for (const ViewId id : ids) {
    double sq = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double d = gt.at(id)[k] - (s * (est.at(id)[k] - mean_e[k]) + mean_g[k]);
      sq += d * d;
    }
    worst = std::max(worst, sq);
  }
  return worst;
}
}  // namespace

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  const bool have_device = tmi_ba_device_count() > 0;
  CHECK(have_device || !need_device);

  // ---- the options' defaults: nonlinear_position_estimator.h:70-81 ------------------------------------------------------
  theia::NonlinearPositionEstimator::Options options;
  CHECK(options.num_threads == 1 && options.max_num_iterations == 400 && options.robust_loss_width == 0.1);
  CHECK(options.min_num_points_per_view == 0 && options.point_to_camera_weight == 0.5);
  CHECK(options.seed == 0 && options.device == -1 && options.initial_positions == nullptr);
  tmi_ba_nonlinear_position_options abi_options;
  tmi_ba_nonlinear_position_options_init(&abi_options);
  CHECK(abi_options.max_num_iterations == 400 && abi_options.robust_loss_width == 0.1);

  // ---- the reference's scene: 4 views on scattered ids, all 6 pairs, no noise; view 4242 has pairs, no orientation ------
  const std::vector<ViewId> ids = {50, 7, 300, 12};
  Lcg rng{2468};
  Vectors orientations, truth;
  for (const ViewId id : ids)
    for (int a = 0; a < 3; ++a) {
      orientations[id][a] = 0.2 * rng.next();
      truth[id][a] = 10.0 * rng.next();
    }
  for (int a = 0; a < 3; ++a) truth[4242][a] = 10.0 * rng.next();
  Pairs view_pairs;
  const ViewId pairs[][2] = {{7, 12}, {7, 50}, {7, 300}, {12, 50}, {12, 300}, {50, 300}, {7, 4242}, {300, 4242}};
  for (const auto& p : pairs) {
    TwoViewInfo info;
    info.position_2 = Direction(orientations.at(p[0]), truth.at(p[0]), truth.at(p[1]));
    view_pairs[ViewIdPair(p[0], p[1])] = info;
  }
  CHECK(view_pairs.size() == 8);
  theia::Reconstruction reconstruction;
  Vectors start;
  start[ViewId(1)] = Eigen::Vector3d::Zero();
  start[ViewId(1)][1] = 5.0;  // what a failed call must leave in place, and a successful one must clear

  // ---- the refusals: false, nothing written, with or without a device -----------------------------------------------------
  {
    Vectors p = start;
    theia::NonlinearPositionEstimator estimator(options, reconstruction);
    theia::PositionEstimator* base = &estimator;  // the interface class
    CHECK(!base->EstimatePositions({}, orientations, &p) && SameBits(p, start));  // :107-111
    CHECK(!base->EstimatePositions(view_pairs, {}, &p) && SameBits(p, start));
    CHECK(!base->EstimatePositions(view_pairs, orientations, nullptr));
    theia::NonlinearPositionEstimator::Options bad = options;
    bad.min_num_points_per_view = 3;  // the point-to-camera constraints are not provided
    theia::NonlinearPositionEstimator with_points(bad, reconstruction);
    CHECK(!with_points.EstimatePositions(view_pairs, orientations, &p) && SameBits(p, start));
    bad = options;
    bad.robust_loss_width = 0.0;  // the reference CHECK_GTs it (:93)
    theia::NonlinearPositionEstimator no_width(bad, reconstruction);
    CHECK(!no_width.EstimatePositions(view_pairs, orientations, &p) && SameBits(p, start));
    bad = options;
    bad.num_threads = 0;  // (:90)
    theia::NonlinearPositionEstimator no_threads(bad, reconstruction);
    CHECK(!no_threads.EstimatePositions(view_pairs, orientations, &p) && SameBits(p, start));
    Pairs two_parts;  // pairs that do not connect
    two_parts[ViewIdPair(7, 12)] = view_pairs[ViewIdPair(7, 12)];
    two_parts[ViewIdPair(50, 300)] = view_pairs[ViewIdPair(50, 300)];
    CHECK(!base->EstimatePositions(two_parts, orientations, &p) && SameBits(p, start));
    Vectors only_one;  // no pair between oriented views
    only_one[ViewId(7)] = orientations[ViewId(7)];
    CHECK(!base->EstimatePositions(view_pairs, only_one, &p) && SameBits(p, start));
    Vectors incomplete;  // a start that lacks a view
    incomplete[ViewId(7)] = truth[ViewId(7)];
    bad = options;
    bad.initial_positions = &incomplete;
    theia::NonlinearPositionEstimator lacking(bad, reconstruction);
    CHECK(!lacking.EstimatePositions(view_pairs, orientations, &p) && SameBits(p, start));
  }

  if (!have_device) {
    Vectors p = start;
    theia::NonlinearPositionEstimator estimator(options, reconstruction);
    CHECK(!estimator.EstimatePositions(view_pairs, orientations, &p));
    CHECK(SameBits(p, start));
    std::printf("nonlinear position estimator shim without a device: OK\n");
    return 0;
  }

  // ---- the C ABI on ascending ids, built independently of the shim --------------------------------------------------------
  std::vector<ViewId> sorted = ids;
  std::sort(sorted.begin(), sorted.end());  // {7, 12, 50, 300}
  auto index = [&](ViewId id) {
    return static_cast<int32_t>(std::lower_bound(sorted.begin(), sorted.end(), id) - sorted.begin());
  };
  std::vector<int32_t> view1, view2;
  std::vector<double> position2, rotation;
  for (int e = 0; e < 6; ++e) {  // (the six pairs above are in ascending ViewIdPair order)
    view1.push_back(index(pairs[e][0]));
    view2.push_back(index(pairs[e][1]));
    for (int a = 0; a < 3; ++a) position2.push_back(view_pairs[ViewIdPair(pairs[e][0], pairs[e][1])].position_2[a]);
  }
  for (const ViewId id : sorted)
    for (int a = 0; a < 3; ++a) rotation.push_back(orientations.at(id)[a]);
  tmi_ba_view_pair_batch B;
  B.num_views = 4;
  B.view_rotation = rotation.data();
  B.num_pairs = 6;
  B.pair_view1 = view1.data();
  B.pair_view2 = view2.data();
  B.pair_rotation2 = nullptr;
  B.pair_position2 = position2.data();
  tmi_ba_nonlinear_position_summary summary;
  std::vector<double> position(12, 7.0);
  CHECK(tmi_ba_estimate_global_positions_nonlinear(&B, &abi_options, 0, -1, position.data(), nullptr, nullptr, nullptr,
                                                   nullptr, nullptr, &summary) == TMI_BA_OK);
  CHECK(summary.num_views == 4 && summary.num_pairs == 6 && summary.usable && summary.num_iterations >= 1);
  Vectors want;
  for (size_t i = 0; i < sorted.size(); ++i)
    for (int a = 0; a < 3; ++a) want[sorted[i]][a] = position[3 * i + a];

  // ---- the shim -----------------------------------------------------------------------------------------------------------
  {
    Vectors got = start;
    theia::NonlinearPositionEstimator estimator(options, reconstruction);
    CHECK(estimator.EstimatePositions(view_pairs, orientations, &got));
    CHECK(got.size() == 4 && got.count(ViewId(1)) == 0);  // cleared, then filled
    CHECK(got.count(ViewId(4242)) == 0);                  // a view without a kept pair is absent
    CHECK(SameBits(got, want));
    for (int a = 0; a < 3; ++a) CHECK(got[ViewId(7)][a] == 0.0);  // the smallest id is at the origin
    // the reference's bound (nonlinear_position_estimator_test.cc:259-269): squared error below 1e-4 after alignment
    const double worst = LargestSquaredErrorAfterAlignment(sorted, truth, got);
    std::printf("largest squared error after alignment: %.3e\n", worst);
    CHECK(worst < 1e-4);
    // the seed changes the start, not the solution of a noise-free scene; num_threads changes nothing at all
    theia::NonlinearPositionEstimator::Options other = options;
    other.num_threads = 8;
    Vectors again;
    theia::NonlinearPositionEstimator threaded(other, reconstruction);
    CHECK(threaded.EstimatePositions(view_pairs, orientations, &again) && SameBits(again, want));
    // a start near the truth, shifted so that view 7 is at the origin: the same solution
    Vectors near_truth;
    for (const ViewId id : ids)
      for (int a = 0; a < 3; ++a) near_truth[id][a] = truth[id][a] - truth[ViewId(7)][a] + 0.01 * rng.next();
    other = options;
    other.initial_positions = &near_truth;
    Vectors from_start;
    theia::NonlinearPositionEstimator started(other, reconstruction);
    CHECK(started.EstimatePositions(view_pairs, orientations, &from_start) && from_start.size() == 4);
    CHECK(LargestSquaredErrorAfterAlignment(sorted, truth, from_start) < 1e-4);
    // fewer orientations: fewer views
    Vectors fewer = orientations;
    fewer.erase(ViewId(50));
    Vectors p = start;
    CHECK(estimator.EstimatePositions(view_pairs, fewer, &p) && p.size() == 3 && p.count(ViewId(50)) == 0);
  }
  std::printf("nonlinear position estimator shim: OK\n");
  return 0;
}
