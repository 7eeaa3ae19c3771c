// theia::TrackEstimator (theiasfm_amd/host/track_estimate_ops.cc) against an in-test restatement of
// EstimateTrack (estimate_track.cc:205-264) on a second copy of the same reconstruction: midpoint triangulation
// of the pixel rays (PINHOLE without distortion), the shim's per-call BundleAdjustTrack, the acceptance test.
// Compared: the estimated set, IsEstimated, the points and the Summary fields.
//   ./test_track_estimator_shim        (needs a GPU)
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <string>
#include <unordered_set>
#include <vector>

#include "theia/sfm/bundle_adjustment/bundle_adjustment.h"
#include "theia/sfm/estimate_track.h"
#include "theia/sfm/reconstruction.h"

using namespace theia;

static int g_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static const double kF = 800.0, kPP = 500.0;

static double urand(unsigned* s) {
  *s = *s * 1664525u + 1013904223u;
  return ((*s >> 8) & 0xffffff) / double(0x1000000);
}

// ceres::AngleAxisRotatePoint
static void Rodrigues(const double* w, const double* a, double* q) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double wxa[3] = {w[1] * a[2] - w[2] * a[1], w[2] * a[0] - w[0] * a[2], w[0] * a[1] - w[1] * a[0]};
  if (t2 < 2.220446049250313e-16) {
    for (int i = 0; i < 3; ++i) q[i] = a[i] + wxa[i];
    return;
  }
  const double t = std::sqrt(t2), c = std::cos(t), s = std::sin(t);
  const double wa = (w[0] * a[0] + w[1] * a[1] + w[2] * a[2]) * (1 - c) / t2;
  for (int i = 0; i < 3; ++i) q[i] = a[i] * c + wxa[i] * s / t + w[i] * wa;
}

// ceres::AngleAxisToRotationMatrix, R[r][c]
static void RotationMatrix(const double* aa, double R[3][3]) {
  const double t2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (t2 > 2.220446049250313e-16) {
    const double t = std::sqrt(t2), wx = aa[0] / t, wy = aa[1] / t, wz = aa[2] / t;
    const double c = std::cos(t), s = std::sin(t), o = 1.0 - c;
    R[0][0] = c + wx * wx * o;      R[0][1] = wx * wy * o - wz * s;  R[0][2] = wy * s + wx * wz * o;
    R[1][0] = wz * s + wx * wy * o; R[1][1] = c + wy * wy * o;       R[1][2] = -wx * s + wy * wz * o;
    R[2][0] = -wy * s + wx * wz * o; R[2][1] = wx * s + wy * wz * o; R[2][2] = c + wz * wz * o;
  } else {
    R[0][0] = 1;      R[0][1] = -aa[2]; R[0][2] = aa[1];
    R[1][0] = aa[2];  R[1][1] = 1;      R[1][2] = -aa[0];
    R[2][0] = -aa[1]; R[2][1] = aa[0];  R[2][2] = 1;
  }
}

// Camera::ProjectPoint of a PINHOLE camera without distortion; returns the depth
static double Project(const Camera& cam, const double* X, double* px) {
  const double* e = cam.extrinsics();
  const double a[3] = {X[0] - X[3] * e[0], X[1] - X[3] * e[1], X[2] - X[3] * e[2]};
  double q[3];
  Rodrigues(e + 3, a, q);
  px[0] = kF * q[0] / q[2] + kPP;
  px[1] = kF * q[1] / q[2] + kPP;
  return q[2] / X[3];
}

// EstimateTrack restated; true if the track is estimated
static bool EstimateTrack(const TrackEstimator::Options& opt, TrackId t, Reconstruction* rec) {
  Track* track = rec->MutableTrack(t);
  std::vector<ViewId> views;
  for (const ViewId v : track->ViewIds())
    if (rec->View(v)->IsEstimated()) views.push_back(v);
  std::sort(views.begin(), views.end());
  std::vector<std::array<double, 3> > rays, origins;
  for (const ViewId v : views) {
    const Camera& cam = rec->View(v)->Camera();
    const Feature& f = *rec->View(v)->GetFeature(t);
    const double u[3] = {(f[0] - kPP) / kF, (f[1] - kPP) / kF, 1.0};
    double R[3][3];
    RotationMatrix(cam.extrinsics() + 3, R);
    std::array<double, 3> r;
    for (int i = 0; i < 3; ++i) r[i] = R[0][i] * u[0] + R[1][i] * u[1] + R[2][i] * u[2];
    const double n = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (int i = 0; i < 3; ++i) r[i] /= n;
    rays.push_back(r);
    origins.push_back({cam.extrinsics()[0], cam.extrinsics()[1], cam.extrinsics()[2]});
  }
  if (rays.size() < 2) return false;
  const double cos_min = std::cos(opt.min_triangulation_angle_degrees * M_PI / 180.0);
  bool sufficient = false;
  for (size_t i = 0; i < rays.size() && !sufficient; ++i)
    for (size_t j = i + 1; j < rays.size(); ++j)
      if (rays[i][0] * rays[j][0] + rays[i][1] * rays[j][1] + rays[i][2] * rays[j][2] < cos_min) sufficient = true;
  if (!sufficient) return false;
  // TriangulateMidpoint: the 3 x 3 block, w = n / (sqrt n sqrt n)
  double A[3][3] = {}, b[3] = {};
  for (size_t k = 0; k < rays.size(); ++k)
    for (int r = 0; r < 3; ++r) {
      double br = 0.0;
      for (int c = 0; c < 3; ++c) {
        const double T = (r == c ? 1.0 : 0.0) - rays[k][r] * rays[k][c];
        A[r][c] += T;
        br += T * origins[k][c];
      }
      b[r] += br;
    }
  double L[3][3] = {};
  for (int k = 0; k < 3; ++k) {
    double x = A[k][k];
    for (int m = 0; m < k; ++m) x -= L[k][m] * L[k][m];
    if (x <= 0.0) return false;
    L[k][k] = std::sqrt(x);
    for (int r = k + 1; r < 3; ++r) {
      double v = A[r][k];
      for (int m = 0; m < k; ++m) v -= L[r][m] * L[k][m];
      L[r][k] = v / L[k][k];
    }
  }
  double y[3], X[4];
  for (int i = 0; i < 3; ++i) {
    double v = b[i];
    for (int m = 0; m < i; ++m) v -= L[i][m] * y[m];
    y[i] = v / L[i][i];
  }
  for (int i = 2; i >= 0; --i) {
    double v = y[i];
    for (int m = i + 1; m < 3; ++m) v -= L[m][i] * X[m];
    X[i] = v / L[i][i];
  }
  const double n = static_cast<double>(rays.size()), sn = std::sqrt(n);
  X[3] = (n / sn) / sn;
  for (int i = 0; i < 4; ++i) (*track->MutablePoint())[i] = X[i];
  if (opt.bundle_adjustment) {
    track->SetEstimated(true);
    const BundleAdjustmentSummary s = BundleAdjustTrack(opt.ba_options, t, rec);
    track->SetEstimated(false);
    if (!s.success) return false;
  }
  const double max_sq = opt.max_acceptable_reprojection_error_pixels * opt.max_acceptable_reprojection_error_pixels;
  double sum = 0.0;
  for (const ViewId v : views) {
    double px[2];
    if (Project(rec->View(v)->Camera(), track->Point().data(), px) < 0) return false;
    const Feature& f = *rec->View(v)->GetFeature(t);
    sum += (f[0] - px[0]) * (f[0] - px[0]) + (f[1] - px[1]) * (f[1] - px[1]);
  }
  if (!(sum / static_cast<double>(views.size()) < max_sq)) return false;
  track->SetEstimated(true);
  return true;
}

// 12 estimated views on a line looking down +z, one view that is not estimated; tracks with noisy or grossly
// wrong features, far-away tracks (insufficient angle), tracks seen once, a track seen only by the view that is
// not estimated, and a few tracks that are already estimated.
static void BuildScene(Reconstruction* rec, unsigned seed) {
  unsigned s = seed;
  std::vector<ViewId> vids;
  for (int i = 0; i < 13; ++i) {
    const ViewId id = rec->AddView("view" + std::to_string(i));
    vids.push_back(id);
    Camera* cam = rec->MutableView(id)->MutableCamera();
    cam->SetPosition(Eigen::Vector3d(2.0 * i - 12.0 + 0.3 * urand(&s), 0.5 * (urand(&s) - 0.5), -30.0));
    cam->SetOrientationFromAngleAxis(Eigen::Vector3d(0.05 * (urand(&s) - 0.5), 0.05 * (urand(&s) - 0.5),
                                                     0.05 * (urand(&s) - 0.5)));
    cam->SetFocalLength(kF);
    cam->SetPrincipalPoint(kPP, kPP);
    rec->MutableView(id)->SetEstimated(i < 12);
  }
  for (int t = 0; t < 160; ++t) {
    const TrackId tid = rec->AddTrack();
    double X[4] = {8 * (urand(&s) - 0.5), 8 * (urand(&s) - 0.5), 8 * (urand(&s) - 0.5), 1.0};
    if (t % 10 == 3) X[2] = 3e4;  // far away: tiny angles
    const int kind = t % 10;
    for (int v = 0; v < 13; ++v) {
      if (kind == 5 && v != 12) continue;  // seen by the view that is not estimated only
      if (kind == 6 && v != 4) continue;   // seen once
      if (urand(&s) < 0.3) continue;
      double px[2];
      Project(rec->View(vids[v])->Camera(), X, px);
      px[0] += 0.6 * (urand(&s) - 0.5) + (kind == 7 ? 40.0 * (urand(&s) - 0.5) : 0.0);
      px[1] += 0.6 * (urand(&s) - 0.5);
      rec->AddObservation(vids[v], tid, Feature(px[0], px[1]));
    }
    Track* tr = rec->MutableTrack(tid);
    for (int i = 0; i < 4; ++i) (*tr->MutablePoint())[i] = (kind == 9) ? X[i] : 1.0 + 0.01 * i;
    tr->SetEstimated(kind == 9);
  }
}

static void Compare(bool ba, bool all, unsigned seed) {
  Reconstruction a, b;
  BuildScene(&a, seed);
  BuildScene(&b, seed);
  TrackEstimator::Options opt;
  opt.bundle_adjustment = ba;
  opt.max_acceptable_reprojection_error_pixels = 2.0;
  opt.num_threads = 8;  // accepted, unused
  TrackEstimator estimator(opt, &a);
  std::unordered_set<TrackId> ids;
  for (const TrackId t : a.TrackIds()) ids.insert(t);
  ids.insert(100000);  // absent: skipped
  const TrackEstimator::Summary got = all ? estimator.EstimateAllTracks() : estimator.EstimateTracks(ids);
  // the restatement, over the tracks EstimateAllTracks / EstimateTracks pick
  std::vector<TrackId> order = b.TrackIds();
  std::sort(order.begin(), order.end());
  int input_estimated = 0, attempts = 0;
  std::unordered_set<TrackId> estimated;
  for (const TrackId t : order) {
    const Track* tr = b.Track(t);
    if (all) {
      bool seen = false;
      for (const ViewId v : tr->ViewIds()) seen = seen || b.View(v)->IsEstimated();
      if (!seen) continue;
    }
    if (tr->IsEstimated()) {
      ++input_estimated;
      continue;
    }
    ++attempts;
    if (EstimateTrack(opt, t, &b)) estimated.insert(t);
  }
  std::printf("ba %d all %d: attempts %d/%d input estimated %d/%d estimated %zu/%zu\n", ba, all,
              got.num_triangulation_attempts, attempts, got.input_num_estimated_tracks, input_estimated,
              got.estimated_tracks.size(), estimated.size());
  EXPECT(got.num_triangulation_attempts == attempts);
  EXPECT(got.input_num_estimated_tracks == input_estimated);
  EXPECT(got.estimated_tracks == estimated);
  EXPECT(!estimated.empty());
  EXPECT(estimated.size() < static_cast<size_t>(attempts));
  for (const TrackId t : order) {
    const Track* ta = a.Track(t);
    const Track* tb = b.Track(t);
    EXPECT(ta->IsEstimated() == tb->IsEstimated());
    const double scale = std::max(1.0, std::sqrt(tb->Point()[0] * tb->Point()[0] + tb->Point()[1] * tb->Point()[1] +
                                                 tb->Point()[2] * tb->Point()[2]));
    for (int i = 0; i < 4; ++i)
      if (!(std::fabs(ta->Point()[i] - tb->Point()[i]) <= 1e-8 * scale)) {
        std::printf("track %u [%d]: %.17g vs %.17g\n", (unsigned)t, i, ta->Point()[i], tb->Point()[i]);
        ++g_fail;
      }
  }
}

int main() {
  Compare(true, false, 3u);
  Compare(false, false, 5u);
  Compare(true, true, 7u);
  std::printf(g_fail ? "FAILED (%d)\n" : "OK\n", g_fail);
  return g_fail ? 1 : 0;
}
