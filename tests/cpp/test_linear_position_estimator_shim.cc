// tests/test_host_shim_linear_position.py: the linear position estimator shim (theiasfm_amd/host/linear_position_ops.cc).
//   always:           the options' defaults are the reference's (linear_position_estimator.h:61-70); every refusal returns
//                     false, leaves the position map as it is and says why on stderr (the wrapper reads the messages).
//   without a device: EstimatePositions returns false and leaves the position map as it is.
//   with a device:    the reference's two tests (linear_position_estimator_test.cc: 4 views, 50 tracks, 6 pairs; within
//                     1e-4 without noise and 0.25 at 1 degree of pose noise after alignment) through
//                     theia::LinearPositionEstimator on a theia::Reconstruction with scattered view ids; the key set of
//                     the map is exactly the estimated views: a view without an orientation, a view that hangs on one
//                     pair and a key present beforehand are all absent; a graph without a triangle returns false.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "theia/sfm/global_pose_estimation/linear_position_estimator.h"
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
constexpr double kF = 800.0, kPP = 500.0;

struct Lcg {
  unsigned long long s;
  double next() {  // uniform in [-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(s >> 11) / 4503599627370496.0 - 1.0;
  }
};

struct Mat {
  double m[3][3];
};

// Rodrigues' formula, R[r][c]
Mat FromAngleAxis(const double aa[3]) {
  const double t = std::sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
  Mat R = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
  if (t == 0.0) return R;
  const double w[3] = {aa[0] / t, aa[1] / t, aa[2] / t}, c = std::cos(t), s = std::sin(t), o = 1.0 - c;
  const double K[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) R.m[r][q] = (r == q ? c : 0.0) + s * K[r][q] + o * w[r] * w[q];
  return R;
}

Mat Mul(const Mat& A, const Mat& B, bool transpose_b) {
  Mat C = {};
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q)
      for (int k = 0; k < 3; ++k) C.m[r][q] += A.m[r][k] * (transpose_b ? B.m[q][k] : B.m[k][q]);
  return C;
}

// (angles well inside (0, pi))
Eigen::Vector3d ToAngleAxis(const Mat& R) {
  const double c = std::min(1.0, std::max(-1.0, 0.5 * (R.m[0][0] + R.m[1][1] + R.m[2][2] - 1.0)));
  const double t = std::acos(c), s = std::sin(t);
  Eigen::Vector3d aa = Eigen::Vector3d::Zero();
  if (s < 1e-12) return aa;
  aa[0] = t * (R.m[2][1] - R.m[1][2]) / (2.0 * s);
  aa[1] = t * (R.m[0][2] - R.m[2][0]) / (2.0 * s);
  aa[2] = t * (R.m[1][0] - R.m[0][1]) / (2.0 * s);
  return aa;
}

Mat Noise(Lcg* rng, double degrees) {
  double axis[3] = {rng->next(), rng->next(), rng->next()};
  const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
  for (double& a : axis) a *= degrees * (M_PI / 180.0) / n;
  return FromAngleAxis(axis);
}

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

// The largest distance between gt and s est + t for the least-squares scale s and translation t.  The reference's test
// aligns by a similarity; with the orientations given the estimate differs from the truth by scale and translation, and
// leaving the rotation out can only make the error larger.
double LargestErrorAfterAlignment(const std::vector<ViewId>& ids, const Vectors& gt, const Vectors& est) {
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
    worst = std::max(worst, std::sqrt(sq));
  }
  return s > 0.0 ? worst : 1e300;  // (a negative scale: the sign vote went wrong)
}

// The reference's scene on the ids given (in the order given): cameras at 10 x rand, rotations 0.2 x rand, focal 800,
// 50 points at rand + (0, 0, 20) seen by every view, the pairs with `noise` degrees on rotation and direction.
struct Scene {
  theia::Reconstruction reconstruction;
  Vectors orientations, truth;
  Pairs view_pairs;
  std::unordered_map<ViewId, ViewId> id_of;  // the caller's label -> the reconstruction's ViewId
};

void Build(const std::vector<int>& labels, const std::vector<std::pair<int, int>>& pairs, double noise, unsigned long long seed,
           Scene* scene) {
  Lcg rng{seed};
  std::unordered_map<int, ViewId> id;
  // AddView hands out ascending ids: scatter them by adding unused views in between
  for (const int label : labels) {
    for (int k = 0; k < 1 + label % 3; ++k) scene->reconstruction.AddView("unused" + std::to_string(label) + "_" + std::to_string(k));
    id[label] = scene->reconstruction.AddView("view" + std::to_string(label));
    theia::Camera* camera = scene->reconstruction.MutableView(id[label])->MutableCamera();
    Eigen::Vector3d position, aa;
    for (int a = 0; a < 3; ++a) {
      position[a] = 10.0 * rng.next();
      aa[a] = 0.2 * rng.next();
    }
    camera->SetPosition(position);
    camera->SetOrientationFromAngleAxis(aa);
    camera->SetFocalLength(kF);
    camera->SetPrincipalPoint(kPP, kPP);
    scene->orientations[id[label]] = aa;
    scene->truth[id[label]] = position;
    scene->id_of[static_cast<ViewId>(label)] = id[label];
  }
  for (int t = 0; t < 50; ++t) {
    const theia::TrackId track = scene->reconstruction.AddTrack();
    const double X[3] = {rng.next(), rng.next(), rng.next() + 20.0};
    for (const int label : labels) {
      const Eigen::Vector3d& c = scene->truth[id[label]];
      const Mat R = FromAngleAxis(scene->orientations[id[label]].data());
      double q[3];
      for (int r = 0; r < 3; ++r) q[r] = R.m[r][0] * (X[0] - c[0]) + R.m[r][1] * (X[1] - c[1]) + R.m[r][2] * (X[2] - c[2]);
      scene->reconstruction.AddObservation(id[label], track, theia::Feature(kF * q[0] / q[2] + kPP, kF * q[1] / q[2] + kPP));
    }
  }
  for (const auto& p : pairs) {
    const ViewId a = id[p.first], b = id[p.second];  // (labels ascend with ids)
    const Mat Ra = FromAngleAxis(scene->orientations[a].data()), Rb = FromAngleAxis(scene->orientations[b].data());
    const double level[2] = {noise * rng.next(), noise * rng.next()};
    TwoViewInfo info;
    info.rotation_2 = ToAngleAxis(Mul(Noise(&rng, level[0]), Mul(Rb, Ra, true), false));
    double d[3], n = 0.0;
    for (int k = 0; k < 3; ++k) {
      d[k] = scene->truth[b][k] - scene->truth[a][k];
      n += d[k] * d[k];
    }
    const Mat N = Mul(Noise(&rng, level[1]), Ra, false);
    for (int r = 0; r < 3; ++r) info.position_2[r] = (N.m[r][0] * d[0] + N.m[r][1] * d[1] + N.m[r][2] * d[2]) / std::sqrt(n);
    scene->view_pairs[ViewIdPair(a, b)] = info;
  }
}
}  // namespace

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  const bool have_device = tmi_ba_device_count() > 0;
  CHECK(have_device || !need_device);

  // ---- the options' defaults: linear_position_estimator.h:61-70 -------------------------------------------------------------
  theia::LinearPositionEstimator::Options options;
  CHECK(options.num_threads == 1 && options.max_power_iterations == 1000 && options.eigensolver_threshold == 1e-8);
  CHECK(options.device == -1);

  // views 0 .. 3 with all six pairs; view 4 hangs on one pair (no triangle); view 5 has pairs and no orientation
  const std::vector<int> labels = {0, 1, 2, 3, 4, 5};
  const std::vector<std::pair<int, int>> pairs = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}, {3, 4}, {0, 5}, {1, 5}};
  Vectors start;
  start[ViewId(100000)] = Eigen::Vector3d::Zero();
  start[ViewId(100000)][1] = 5.0;  // what a failed call must leave in place, and a successful one must clear

  // ---- the refusals: false, nothing written, with or without a device -----------------------------------------------------
  {
    Scene scene;
    Build(labels, pairs, 0.0, 97531, &scene);
    scene.orientations.erase(scene.id_of[5]);
    Vectors p = start;
    theia::LinearPositionEstimator estimator(options, scene.reconstruction);
    theia::PositionEstimator* base = &estimator;  // the interface class
    CHECK(!base->EstimatePositions({}, scene.orientations, &p) && SameBits(p, start));
    CHECK(!base->EstimatePositions(scene.view_pairs, {}, &p) && SameBits(p, start));
    CHECK(!base->EstimatePositions(scene.view_pairs, scene.orientations, nullptr));
    theia::LinearPositionEstimator::Options bad = options;
    bad.num_threads = 0;  // the reference CHECK_GTs it (:160)
    theia::LinearPositionEstimator no_threads(bad, scene.reconstruction);
    CHECK(!no_threads.EstimatePositions(scene.view_pairs, scene.orientations, &p) && SameBits(p, start));
    bad = options;
    bad.max_power_iterations = 0;
    theia::LinearPositionEstimator no_iterations(bad, scene.reconstruction);
    CHECK(!no_iterations.EstimatePositions(scene.view_pairs, scene.orientations, &p) && SameBits(p, start));
    Pairs unordered = scene.view_pairs;  // a key whose first id is not below its second
    unordered[ViewIdPair(scene.id_of[2], scene.id_of[1])] = TwoViewInfo();
    CHECK(!base->EstimatePositions(unordered, scene.orientations, &p) && SameBits(p, start));
    Vectors only_one;  // no pair between oriented views
    only_one[scene.id_of[0]] = scene.orientations[scene.id_of[0]];
    CHECK(!base->EstimatePositions(scene.view_pairs, only_one, &p) && SameBits(p, start));
    Pairs foreign;  // a pair of views that are not in the reconstruction
    foreign[ViewIdPair(200000, 200001)] = TwoViewInfo();
    Vectors foreign_orientations;
    foreign_orientations[ViewId(200000)] = Eigen::Vector3d::Zero();
    foreign_orientations[ViewId(200001)] = Eigen::Vector3d::Zero();
    CHECK(!base->EstimatePositions(foreign, foreign_orientations, &p) && SameBits(p, start));
    if (!have_device) {
      CHECK(!base->EstimatePositions(scene.view_pairs, scene.orientations, &p) && SameBits(p, start));
      std::printf("linear position estimator shim without a device: OK\n");
      return 0;
    }
    // a path has no triangle: nothing to solve from
    Pairs path;
    for (const auto& e : {std::make_pair(0, 1), std::make_pair(1, 2), std::make_pair(2, 3)})
      path[ViewIdPair(scene.id_of[e.first], scene.id_of[e.second])] =
          scene.view_pairs[ViewIdPair(scene.id_of[e.first], scene.id_of[e.second])];
    CHECK(!base->EstimatePositions(path, scene.orientations, &p) && SameBits(p, start));
  }

  // ---- the reference's two tests ---------------------------------------------------------------------------------------------
  const double noises[2] = {0.0, 1.0}, bounds[2] = {1e-4, 0.25};
  for (int k = 0; k < 2; ++k) {
    Scene scene;
    Build(labels, pairs, noises[k], 97531 + k, &scene);
    scene.orientations.erase(scene.id_of[5]);
    Vectors got = start;
    theia::LinearPositionEstimator::Options threaded = options;
    threaded.num_threads = 8;  // accepted, ignored
    theia::LinearPositionEstimator estimator(threaded, scene.reconstruction);
    CHECK(estimator.EstimatePositions(scene.view_pairs, scene.orientations, &got));
    // the key set: exactly the four views of the triplets
    std::vector<ViewId> four = {scene.id_of[0], scene.id_of[1], scene.id_of[2], scene.id_of[3]};
    CHECK(got.size() == 4);
    for (const ViewId id : four) CHECK(got.count(id) == 1);
    CHECK(got.count(ViewId(100000)) == 0);      // cleared, then filled
    CHECK(got.count(scene.id_of[4]) == 0);      // in a pair, in no triplet
    CHECK(got.count(scene.id_of[5]) == 0);      // no orientation
    const double worst = LargestErrorAfterAlignment(four, scene.truth, got);
    std::printf("noise %.1f: largest error after alignment %.3e (bound %.3e)\n", noises[k], worst, bounds[k]);
    CHECK(worst < bounds[k]);
    Vectors again;  // the same bits from call to call
    CHECK(estimator.EstimatePositions(scene.view_pairs, scene.orientations, &again) && SameBits(again, got));
  }
  std::printf("linear position estimator shim: OK\n");
  return 0;
}
