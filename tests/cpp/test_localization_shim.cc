// theia::LocalizeViewToReconstruction / LocalizeViewsToReconstruction (theiasfm_amd/host/localize_ops.cc).
//   ./test_localization_shim                 whatever the machine has: the defaults, the unsupported paths and -- without
//                                            a device -- false for every view and an untouched reconstruction
//   ./test_localization_shim --need-device   also: the write-back rules per status, the poses, batch == sequential
#include <cmath>
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "theia/sfm/localize_view_to_reconstruction.h"
#include "theia_mi355_ba.h"

using namespace theia;

static int g_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static double urand(unsigned* s) {
  *s = *s * 1664525u + 1013904223u;
  return ((*s >> 8) & 0xffffff) / double(0x1000000);
}

static void Rodrigues(const double* w, const double* a, double* q) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double wxa[3] = {w[1] * a[2] - w[2] * a[1], w[2] * a[0] - w[0] * a[2], w[0] * a[1] - w[1] * a[0]};
  if (t2 < 1e-30) {
    for (int i = 0; i < 3; ++i) q[i] = a[i] + wxa[i];
    return;
  }
  const double t = std::sqrt(t2), c = std::cos(t), s = std::sin(t);
  const double wa = (w[0] * a[0] + w[1] * a[1] + w[2] * a[2]) * (1 - c) / t2;
  for (int i = 0; i < 3; ++i) q[i] = a[i] * c + wxa[i] * s / t + w[i] * wa;
}

// The candidates and their true poses.  Views 0..4: 120 matches, 30 % of them uniform over the image; view 5: 10
// matches (too few); view 6: every match an outlier (too few inliers); view 7: as 0..4 but without a focal length prior
// (unknown intrinsics); view 8: matches of an unestimated track only.  Pinhole f = 800, 1024 x 768, exact projections.
struct Scene {
  Reconstruction rec;
  std::vector<ViewId> ids;
  std::vector<std::vector<double> > truth;
};

static void BuildScene(Scene* S, unsigned seed) {
  unsigned s = seed;
  Reconstruction* rec = &S->rec;
  std::vector<TrackId> tracks;
  std::vector<std::vector<double> > X;
  for (int t = 0; t < 121; ++t) {
    const TrackId tid = rec->AddTrack();
    Track* tr = rec->MutableTrack(tid);
    X.push_back({4 * (urand(&s) - 0.5), 4 * (urand(&s) - 0.5), 4 * (urand(&s) - 0.5)});
    for (int i = 0; i < 3; ++i) (*tr->MutablePoint())[i] = X.back()[i];
    (*tr->MutablePoint())[3] = 1.0;
    tr->SetEstimated(t < 120);  // the last track is not estimated
    tracks.push_back(tid);
  }
  for (int v = 0; v < 9; ++v) {
    const ViewId id = rec->AddView("view" + std::to_string(v));
    S->ids.push_back(id);
    View* view = rec->MutableView(id);
    Camera* cam = view->MutableCamera();
    const double pose[6] = {2 * (urand(&s) - 0.5), 2 * (urand(&s) - 0.5), -9 + urand(&s),
                            0.2 * (urand(&s) - 0.5), 0.2 * (urand(&s) - 0.5), 0.2 * (urand(&s) - 0.5)};
    S->truth.push_back(std::vector<double>(pose, pose + 6));
    cam->SetFocalLength(800.0);
    cam->SetPrincipalPoint(512.0, 384.0);
    cam->SetImageSize(1024, 768);
    if (v != 7) view->MutableCameraIntrinsicsPrior()->focal_length.is_set = true;
    const int first = v == 8 ? 120 : 0, last = v == 5 ? 10 : (v == 8 ? 121 : 120);
    for (int t = first; t < last; ++t) {
      const double a[3] = {X[t][0] - pose[0], X[t][1] - pose[1], X[t][2] - pose[2]};
      double q[3];
      Rodrigues(pose + 3, a, q);
      double u = 800.0 * q[0] / q[2] + 512.0, w = 800.0 * q[1] / q[2] + 384.0;
      const bool outlier = v == 6 || (v < 5 && t % 10 < 3) || (v == 7 && t % 10 < 3);
      if (outlier) {
        u = 1024.0 * urand(&s);
        w = 768.0 * urand(&s);
      }
      rec->AddObservation(id, tracks[t], Feature(u, w));
    }
  }
}

static bool SameCamera(const Reconstruction& a, const Reconstruction& b, ViewId v) {
  return std::memcmp(a.View(v)->Camera().extrinsics(), b.View(v)->Camera().extrinsics(), 6 * sizeof(double)) == 0 &&
         a.View(v)->IsEstimated() == b.View(v)->IsEstimated();
}

static void TestDefaults() {
  // sample_consensus_estimator.h:57-65, localize_view_to_reconstruction.h:48-72
  RansacParameters rp;
  EXPECT(rp.error_thresh == -1 && rp.failure_probability == 0.01 && rp.min_inlier_ratio == 0);
  EXPECT(rp.min_iterations == 100 && rp.max_iterations == INT_MAX && !rp.use_mle && !rp.use_Tdd_test && !rp.rng);
  LocalizeViewToReconstructionOptions o;
  EXPECT(o.reprojection_error_threshold_pixels == 4.0 && !o.assume_known_orientation && o.bundle_adjust_view);
  EXPECT(o.min_num_inliers == 30);
  EXPECT(ComputeResolutionScaledThreshold(4.0, 0, 0) == 4.0);
  EXPECT(ComputeResolutionScaledThreshold(4.0, 2048, 1000) == 8.0);
  EXPECT(ComputeResolutionScaledThreshold(4.0, 300, 512) == 2.0);
}

static void TestUnsupported() {
  Scene S, ref;
  BuildScene(&S, 3u);
  BuildScene(&ref, 3u);
  RansacSummary sum;
  for (int mode = 0; mode < 3; ++mode) {
    LocalizeViewToReconstructionOptions o;
    if (mode == 0) o.assume_known_orientation = true;
    if (mode == 1) o.ransac_params.use_mle = true;
    if (mode == 2) o.ransac_params.use_Tdd_test = true;
    EXPECT(!LocalizeViewToReconstruction(S.ids[0], o, &S.rec, &sum));
    EXPECT(SameCamera(S.rec, ref.rec, S.ids[0]));
  }
  LocalizeViewToReconstructionOptions o;
  EXPECT(!LocalizeViewToReconstruction(S.ids[7], o, &S.rec, &sum));  // unknown intrinsics
  EXPECT(!LocalizeViewToReconstruction(1000, o, &S.rec, &sum));      // no such view
  for (const ViewId v : S.ids) EXPECT(SameCamera(S.rec, ref.rec, v));
}

static void TestWithoutDevice() {
  Scene S, ref;
  BuildScene(&S, 3u);
  BuildScene(&ref, 3u);
  std::vector<RansacSummary> sums;
  const std::vector<bool> ok = LocalizeViewsToReconstruction(S.ids, LocalizeViewToReconstructionOptions(), &S.rec, &sums);
  EXPECT(ok.size() == S.ids.size() && sums.size() == S.ids.size());
  for (size_t k = 0; k < ok.size(); ++k) EXPECT(!ok[k]);
  for (const ViewId v : S.ids) EXPECT(SameCamera(S.rec, ref.rec, v));
}

static void TestOnDevice(bool bundle_adjust_view) {
  Scene S, seq, ref;
  BuildScene(&S, 3u);
  BuildScene(&seq, 3u);
  BuildScene(&ref, 3u);
  LocalizeViewToReconstructionOptions o;
  o.bundle_adjust_view = bundle_adjust_view;
  o.ransac_params.max_iterations = 500;
  o.ransac_params.seed = 17;
  std::vector<RansacSummary> sums;
  const std::vector<bool> ok = LocalizeViewsToReconstruction(S.ids, o, &S.rec, &sums);
  for (int v = 0; v < 9; ++v) {
    const ViewId id = S.ids[v];
    EXPECT(ok[v] == (v < 5));
    if (v < 5) {  // status 0: pose written, estimated; the RANSAC pose of exact projections is near the truth (the
                  // reference tests' 1e-4).  The adjustment fits ALL matches, outliers included, as the reference's does.
      EXPECT(S.rec.View(id)->IsEstimated());
      if (!bundle_adjust_view)
        for (int i = 0; i < 6; ++i) EXPECT(std::fabs(S.rec.View(id)->Camera().extrinsics()[i] - S.truth[v][i]) < 1e-4);
      EXPECT(sums[v].num_input_data_points == 120 && (int)sums[v].inliers.size() == 84);
      for (const int j : sums[v].inliers) EXPECT(j % 10 >= 3);  // ascending TrackId == generation order
      EXPECT(sums[v].num_iterations >= 100 && sums[v].confidence > 0.99);
    } else {      // statuses 1, 3 and the unsupported ones: left alone
      EXPECT(SameCamera(S.rec, ref.rec, id));
      EXPECT(!S.rec.View(id)->IsEstimated());
    }
  }
  EXPECT(sums[5].num_input_data_points == 10 && sums[5].num_iterations == 0);
  EXPECT(sums[6].num_input_data_points == 120 && (int)sums[6].inliers.size() < 30 && sums[6].num_iterations == 500);
  // the batch equals the single-view form called in the same order
  for (int v = 0; v < 9; ++v) {
    RansacSummary one;
    const bool r = LocalizeViewToReconstruction(seq.ids[v], o, &seq.rec, &one);
    EXPECT(r == ok[v]);
    EXPECT(SameCamera(S.rec, seq.rec, seq.ids[v]));
    EXPECT(one.inliers == sums[v].inliers && one.num_iterations == sums[v].num_iterations &&
           one.confidence == sums[v].confidence && one.num_input_data_points == sums[v].num_input_data_points);
  }
}

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  const bool device = tmi_ba_device_count() > 0;
  if (need_device && !device) {
    std::printf("FAILED: no device\n");
    return 1;
  }
  TestDefaults();
  TestUnsupported();
  if (!device) TestWithoutDevice();
  if (device) {
    TestOnDevice(false);
    TestOnDevice(true);
  }
  if (g_fail)
    std::printf("localization shim: FAILED (%d)\n", g_fail);
  else
    std::printf("localization shim: OK%s\n", device ? " (device)" : "");
  return g_fail ? 1 : 0;
}
