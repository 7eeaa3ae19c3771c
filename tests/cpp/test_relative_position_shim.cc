// -m gpu (tests/test_host_shim_relative_position.py): the relative-position shim
// (theiasfm_amd/host/relative_position_ops.cc).
//   1. OptimizeRelativePositionWithKnownRotation (single) == OptimizeRelativePositionsWithKnownRotationsBatch ==
//      tmi_ba_optimize_relative_positions on the same data, bit for bit.
//   2. RefineRelativeTranslationsWithKnownRotations on a small Reconstruction (PINHOLE with k1 != 0, three views,
//      three edges, one of them without common tracks): position_2 equals -- within max(1e-12 rad, 100 x the spread
//      between two orders of the restatement) -- an in-test restatement of the reference that normalises the pixels on
//      the host; the empty edge's position_2 is left alone.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "theia/sfm/bundle_adjustment/optimize_relative_position_with_known_rotation.h"
#include "theia_mi355_ba.h"

using namespace theia;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

struct V3 {
  double v[3];
};
struct M3 {
  double m[3][3];
};

// ceres::AngleAxisToRotationMatrix with its first-order branch
static M3 Rot(const double aa[3]) {
  M3 R;
  const double t2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (t2 > 2.220446049250313e-16) {
    const double t = std::sqrt(t2), x = aa[0] / t, y = aa[1] / t, z = aa[2] / t, c = std::cos(t), s = std::sin(t), o = 1 - c;
    const double r[3][3] = {{c + x * x * o, x * y * o - z * s, y * s + x * z * o},
                            {z * s + x * y * o, c + y * y * o, -x * s + y * z * o},
                            {-y * s + x * z * o, x * s + y * z * o, c + z * z * o}};
    std::memcpy(R.m, r, sizeof(r));
  } else {
    const double r[3][3] = {{1, -aa[2], aa[1]}, {aa[2], 1, -aa[0]}, {-aa[1], aa[0], 1}};
    std::memcpy(R.m, r, sizeof(r));
  }
  return R;
}
static V3 Mul(const M3& R, const V3& a, bool transpose) {
  V3 o;
  for (int i = 0; i < 3; ++i) {
    o.v[i] = 0;
    for (int j = 0; j < 3; ++j) o.v[i] += (transpose ? R.m[j][i] : R.m[i][j]) * a.v[j];
  }
  return o;
}
static double Angle(const double a[3], const double b[3]) {
  const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  return std::atan2(std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}

// Smallest eigenvector of a symmetric 3 x 3 by cyclic Jacobi (the restatement's own; plain textbook form).
static void SmallestEigenvector(double A[3][3], double t[3]) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 60; ++sweep) {
    if (std::fabs(A[0][1]) + std::fabs(A[0][2]) + std::fabs(A[1][2]) == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int m = 0;
  for (int i = 1; i < 3; ++i)
    if (A[i][i] < A[m][m]) m = i;
  for (int k = 0; k < 3; ++k) t[k] = V[k][m];
}

// optimize_relative_position_with_known_rotation.cc:53-197 on normalised correspondences, in the given order
static void Restatement(const std::vector<FeatureCorrespondence>& corr, const double r1[3], const double r2[3],
                        double t[3]) {
  const M3 R1 = Rot(r1), R2 = Rot(r2);
  const size_t n = corr.size();
  std::vector<V3> c(n);
  for (size_t i = 0; i < n; ++i) {
    const V3 h1 = {{corr[i].feature1.x(), corr[i].feature1.y(), 1.0}}, h2 = {{corr[i].feature2.x(), corr[i].feature2.y(), 1.0}};
    const V3 a = Mul(R1, h1, true), b = Mul(R2, h2, true);
    const V3 x = {{b.v[1] * a.v[2] - b.v[2] * a.v[1], b.v[2] * a.v[0] - b.v[0] * a.v[2], b.v[0] * a.v[1] - b.v[1] * a.v[0]}};
    c[i] = Mul(R1, x, false);
  }
  std::vector<double> w(n, 1.0);
  double cost = 0.0;
  int inner = 0;
  for (int it = 0; it < 100 && inner < 10; ++it) {
    double M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (size_t i = 0; i < n; ++i) {
      const double wi = std::max(w[i], 1e-7);
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) M[a][b] += c[i].v[a] * c[i].v[b] / wi;
    }
    SmallestEigenvector(M, t);
    double new_cost = 0.0;
    for (size_t i = 0; i < n; ++i) {
      w[i] = std::fabs(t[0] * c[i].v[0] + t[1] * c[i].v[1] + t[2] * c[i].v[2]);
      new_cost += w[i];
    }
    const double delta = std::max(std::fabs(cost - new_cost), 1.0 - (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]));
    inner = delta <= 1e-5 ? inner + 1 : 0;
    cost = new_cost;
  }
  // the sign: more than n / 2 in front of both cameras (triangulation.cc:216-232 with R = R2 R1^T)
  size_t front = 0;
  for (size_t i = 0; i < n; ++i) {
    const V3 d1 = {{corr[i].feature1.x(), corr[i].feature1.y(), 1.0}}, h2 = {{corr[i].feature2.x(), corr[i].feature2.y(), 1.0}};
    const V3 d2 = Mul(R1, Mul(R2, h2, true), false);
    double s1 = 0, s2 = 0, s12 = 0, t1 = 0, t2 = 0;
    for (int k = 0; k < 3; ++k) {
      s1 += d1.v[k] * d1.v[k];
      s2 += d2.v[k] * d2.v[k];
      s12 += d1.v[k] * d2.v[k];
      t1 += d1.v[k] * t[k];
      t2 += d2.v[k] * t[k];
    }
    if (s2 * t1 - s12 * t2 > 0 && s12 * t1 - s1 * t2 > 0) ++front;
  }
  if (!(front > n / 2))
    for (int k = 0; k < 3; ++k) t[k] = -t[k];
}

// PINHOLE PixelToCameraCoordinates (pinhole_camera_model.h:259-296): fixed-point undistortion, then z = 1
static void Normalise(const double* K, const Feature& px, double out[2]) {
  const double fy = K[0] * K[1];
  const double dy = (px.y() - K[4]) / fy, dx = (px.x() - K[3] - dy * K[2]) / K[0];
  double u[2] = {dx, dy};
  for (int it = 0; it < 100; ++it) {
    const double p0 = u[0], p1 = u[1], r = u[0] * u[0] + u[1] * u[1], d = 1.0 + r * (K[5] + K[6] * r);
    u[0] = dx / d;
    u[1] = dy / d;
    if (std::fabs(u[0] - p0) < 1e-10 && std::fabs(u[1] - p1) < 1e-10) break;
  }
  out[0] = u[0];
  out[1] = u[1];
}

int main() {
  std::mt19937 gen(11);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  // ---- 1. single == batch == ABI ----
  const int P = 9;
  const int sizes[P] = {5, 40, 64, 65, 130, 300, 513, 900, 33};
  std::vector<std::vector<FeatureCorrespondence>> corr(P);
  std::vector<Eigen::Vector3d> r1(P), r2(P);
  for (int p = 0; p < P; ++p) {
    double a1[3], a2[3];
    for (int k = 0; k < 3; ++k) {
      a1[k] = 0.2 * U(gen);
      a2[k] = 0.2 * U(gen);
    }
    r1[p] = Eigen::Vector3d(a1[0], a1[1], a1[2]);
    r2[p] = Eigen::Vector3d(a2[0], a2[1], a2[2]);
    const M3 R1 = Rot(a1), R2 = Rot(a2);
    const V3 C1 = {{U(gen), U(gen), U(gen)}}, C2 = {{U(gen), U(gen), U(gen)}};
    for (int i = 0; i < sizes[p]; ++i) {
      const V3 X = {{2 * U(gen), 2 * U(gen), 9 + U(gen)}};
      const V3 q1 = Mul(R1, V3{{X.v[0] - C1.v[0], X.v[1] - C1.v[1], X.v[2] - C1.v[2]}}, false);
      const V3 q2 = Mul(R2, V3{{X.v[0] - C2.v[0], X.v[1] - C2.v[1], X.v[2] - C2.v[2]}}, false);
      corr[p].emplace_back(Feature(q1.v[0] / q1.v[2] + 1e-3 * U(gen), q1.v[1] / q1.v[2] + 1e-3 * U(gen)),
                           Feature(q2.v[0] / q2.v[2] + 1e-3 * U(gen), q2.v[1] / q2.v[2] + 1e-3 * U(gen)));
    }
  }
  std::vector<Eigen::Vector3d> single(P, Eigen::Vector3d(9, 9, 9)), batch(P, Eigen::Vector3d(9, 9, 9));
  for (int p = 0; p < P; ++p) CHECK(OptimizeRelativePositionWithKnownRotation(corr[p], r1[p], r2[p], &single[p]));
  std::vector<RelativePositionProblem> problems(P);
  for (int p = 0; p < P; ++p) {
    problems[p].correspondences = &corr[p];
    problems[p].rotation1 = r1[p];
    problems[p].rotation2 = r2[p];
    problems[p].relative_position = &batch[p];
  }
  const std::vector<bool> ok = OptimizeRelativePositionsWithKnownRotationsBatch(&problems);
  CHECK(ok.size() == (size_t)P);
  // the ABI on the same data
  std::vector<double> rot, f1, f2, pos(3 * P, 9.0);
  std::vector<int32_t> v1, v2;
  std::vector<int64_t> ptr(1, 0);
  for (int p = 0; p < P; ++p) {
    for (int k = 0; k < 3; ++k) rot.push_back(r1[p][k]);
    for (int k = 0; k < 3; ++k) rot.push_back(r2[p][k]);
    v1.push_back(2 * p);
    v2.push_back(2 * p + 1);
    for (const FeatureCorrespondence& m : corr[p]) {
      f1.push_back(m.feature1.x());
      f1.push_back(m.feature1.y());
      f2.push_back(m.feature2.x());
      f2.push_back(m.feature2.y());
    }
    ptr.push_back((int64_t)f1.size() / 2);
  }
  tmi_ba_relative_position_batch B;
  B.num_views = 2 * P;
  B.view_rotation = rot.data();
  B.view_model = nullptr;
  B.view_intrinsics = nullptr;
  B.num_pairs = P;
  B.pair_view1 = v1.data();
  B.pair_view2 = v2.data();
  B.correspondence_ptr = ptr.data();
  B.features1 = f1.data();
  B.features2 = f2.data();
  B.position2 = pos.data();
  std::vector<int8_t> status(P);
  tmi_ba_track_batch_summary bs;
  CHECK(tmi_ba_optimize_relative_positions(&B, -1, status.data(), nullptr, nullptr, nullptr, &bs) == TMI_BA_OK);
  for (int p = 0; p < P; ++p) {
    CHECK(ok[p] && (status[p] == 0 || status[p] == 1));
    double s[3], b[3];
    for (int k = 0; k < 3; ++k) s[k] = single[p][k], b[k] = batch[p][k];
    CHECK(std::memcmp(s, b, sizeof(s)) == 0);
    CHECK(std::memcmp(s, &pos[3 * p], sizeof(s)) == 0);
    double t[3];
    Restatement(corr[p], r1[p].data(), r2[p].data(), t);
    const double a = Angle(s, t);
    std::printf("pair %d (%d correspondences): single == batch == ABI, angle to the restatement %.3e rad\n", p, sizes[p], a);
    CHECK(a < 1e-7);
  }
  // no correspondences: false, the position left alone
  std::vector<FeatureCorrespondence> none;
  Eigen::Vector3d untouched(1, 2, 3);
  CHECK(!OptimizeRelativePositionWithKnownRotation(none, r1[0], r2[0], &untouched));
  CHECK(untouched[0] == 1 && untouched[1] == 2 && untouched[2] == 3);

  // ---- 2. RefineRelativeTranslationsWithKnownRotations ----
  Reconstruction rec;
  const double aa[3][3] = {{0.02, -0.05, 0.01}, {-0.03, 0.12, 0.02}, {0.04, 0.3, -0.02}};
  const double C[3][3] = {{0, 0, 0}, {1.5, 0.1, 0.2}, {3.1, -0.2, 0.5}};
  ViewId ids[3];
  std::unordered_map<ViewId, Eigen::Vector3d> orientations;
  for (int v = 0; v < 3; ++v) {
    ids[v] = rec.AddView("view" + std::to_string(v));
    Camera* cam = rec.MutableView(ids[v])->MutableCamera();
    cam->SetPosition(Eigen::Vector3d(C[v][0], C[v][1], C[v][2]));
    cam->SetOrientationFromAngleAxis(Eigen::Vector3d(aa[v][0], aa[v][1], aa[v][2]));
    double* K = cam->mutable_intrinsics();  // PINHOLE [f, ar, skew, px, py, k1, k2]
    K[0] = 700 + 40 * v, K[1] = 1.0, K[2] = 0.0, K[3] = 500, K[4] = 400, K[5] = -0.06, K[6] = 0.01;
    orientations[ids[v]] = Eigen::Vector3d(aa[v][0], aa[v][1], aa[v][2]);
  }
  auto project = [&](int v, const V3& X) {
    const M3 R = Rot(aa[v]);
    const V3 q = Mul(R, V3{{X.v[0] - C[v][0], X.v[1] - C[v][1], X.v[2] - C[v][2]}}, false);
    const double* K = rec.View(ids[v])->Camera().intrinsics();
    const double x = q.v[0] / q.v[2], y = q.v[1] / q.v[2], r = x * x + y * y, d = 1 + r * (K[5] + K[6] * r);
    return Feature(K[0] * x * d + K[2] * y * d + K[3] + 0.3 * U(gen), K[0] * K[1] * y * d + K[4] + 0.3 * U(gen));
  };
  // tracks seen by views 0 and 1, and tracks seen by views 1 and 2; none by 0 and 2
  for (int i = 0; i < 150; ++i) {
    const V3 X = {{1.5 * U(gen) + 1.5, 1.5 * U(gen), 9 + U(gen)}};
    const int a = i < 80 ? 0 : 1;
    rec.AddTrack({{ids[a], project(a, X)}, {ids[a + 1], project(a + 1, X)}});
  }
  TwoViewInfo info01, info12, info02;
  info02.position_2 = Eigen::Vector3d(0.25, 0.5, 0.75);
  std::vector<std::pair<ViewIdPair, TwoViewInfo*>> edges = {{ViewIdPair(ids[0], ids[1]), &info01},
                                                            {ViewIdPair(ids[0], ids[2]), &info02},
                                                            {ViewIdPair(ids[1], ids[2]), &info12}};
  CHECK(RefineRelativeTranslationsWithKnownRotations(rec, orientations, &edges) == 2);
  CHECK(info02.position_2[0] == 0.25 && info02.position_2[1] == 0.5 && info02.position_2[2] == 0.75);
  const int pairs[2][2] = {{0, 1}, {1, 2}};
  TwoViewInfo* infos[2] = {&info01, &info12};
  for (int e = 0; e < 2; ++e) {
    const View* va = rec.View(ids[pairs[e][0]]);
    const View* vb = rec.View(ids[pairs[e][1]]);
    std::vector<FeatureCorrespondence> m;
    for (const TrackId id : va->TrackIds()) {
      const Feature* fb = vb->GetFeature(id);
      if (!fb) continue;
      double n1[2], n2[2];
      Normalise(va->Camera().intrinsics(), *va->GetFeature(id), n1);
      Normalise(vb->Camera().intrinsics(), *fb, n2);
      m.emplace_back(Feature(n1[0], n1[1]), Feature(n2[0], n2[1]));
    }
    double t[3], tr[3];
    Restatement(m, aa[pairs[e][0]], aa[pairs[e][1]], t);
    std::vector<FeatureCorrespondence> reversed(m.rbegin(), m.rend());
    Restatement(reversed, aa[pairs[e][0]], aa[pairs[e][1]], tr);
    const double spread = Angle(t, tr), tol = std::max(1e-12, 100.0 * spread);
    const double got[3] = {infos[e]->position_2[0], infos[e]->position_2[1], infos[e]->position_2[2]};
    const double a = Angle(got, t);
    // the truth, for scale: R1 (C2 - C1) normalised
    const V3 d = Mul(Rot(aa[pairs[e][0]]), V3{{C[pairs[e][1]][0] - C[pairs[e][0]][0], C[pairs[e][1]][1] - C[pairs[e][0]][1],
                                               C[pairs[e][1]][2] - C[pairs[e][0]][2]}}, false);
    std::printf("edge (%d, %d): %zu correspondences, shim to restatement %.3e rad (restatement spread %.3e, tolerance "
                "%.3e), to the truth %.3e rad\n", pairs[e][0], pairs[e][1], m.size(), a, spread, tol, Angle(got, d.v));
    CHECK(m.size() > 60);
    CHECK(a <= tol);
    CHECK(Angle(got, d.v) < 0.05);
  }
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("relative-position shim: all checks passed\n");
  return 0;
}
