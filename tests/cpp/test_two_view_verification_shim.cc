// The two-view verification shim (theiasfm_amd/host/two_view_verify_ops.cc) against the C ABI on the device: the
// single call equals the batch call equals tmi_ba_verify_two_views bit for bit; position_2 has unit norm;
// inlier_indices are the status-0 indices in order; pairs the reference returns false for are left untouched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "theia/sfm/two_view_match_geometric_verification.h"
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

// a PINHOLE camera without distortion
static void Project(const double* e, double f, const double* X, double* px) {
  const double a[3] = {X[0] - e[0], X[1] - e[1], X[2] - e[2]};
  double q[3];
  Rodrigues(e + 3, a, q);
  px[0] = f * q[0] / q[2] + kPP;
  px[1] = f * q[1] / q[2] + kPP;
}

struct Pair {
  Camera camera1, camera2;
  std::vector<FeatureCorrespondence> matches;
  bool free_focal = false;
  TwoViewInfo info;
  std::vector<int> inliers;
};

static void SetPinhole(Camera* cam, const double* ext, double f) {
  for (int a = 0; a < 6; ++a) cam->mutable_extrinsics()[a] = ext[a];
  cam->SetFocalLength(f);
  cam->mutable_intrinsics()[1] = 1.0;
  cam->SetPrincipalPoint(kPP, kPP);
}

// n matches of a true pose with half a pixel of noise, every fifth one a far point (no triangulation angle) and every
// seventh one 14 pixels off in image 2; camera 2 starts a little off the truth
static void MakePair(unsigned seed, int n, bool free_focal, Pair* out) {
  unsigned s = seed;
  const double e1[6] = {0, 0, 0, 0, 0, 0};
  const double e2[6] = {1.0 + 0.2 * urand(&s), 0.1 * urand(&s), -0.05, 0.03, -0.08 * urand(&s), 0.02};
  for (int i = 0; i < n; ++i) {
    const double z = (i % 5 == 4) ? 300.0 + 100.0 * urand(&s) : 4.0 + 3.0 * urand(&s);
    const double X[3] = {z * (0.4 * urand(&s) - 0.2) + 0.5, z * (0.4 * urand(&s) - 0.2), z};
    double p1[2], p2[2];
    Project(e1, kF, X, p1);
    Project(e2, kF, X, p2);
    FeatureCorrespondence m;
    m.feature1 = Feature(p1[0] + urand(&s) - 0.5, p1[1] + urand(&s) - 0.5);
    m.feature2 = Feature(p2[0] + urand(&s) - 0.5, p2[1] + urand(&s) - 0.5 + (i % 7 == 6 ? 14.0 : 0.0));
    out->matches.push_back(m);
  }
  double e2_start[6];
  for (int a = 0; a < 6; ++a) e2_start[a] = e2[a] + (a < 3 ? 0.01 : 0.002) * (urand(&s) - 0.5);
  out->camera1 = Camera(CameraIntrinsicsModelType::PINHOLE);
  out->camera2 = Camera(CameraIntrinsicsModelType::PINHOLE);
  SetPinhole(&out->camera1, e1, free_focal ? kF * 1.004 : kF);
  SetPinhole(&out->camera2, e2_start, free_focal ? kF * 0.996 : kF);
  out->free_focal = free_focal;
  out->info.focal_length_1 = -1.0;
}

static TwoViewVerificationProblem Problem(Pair* p) {
  TwoViewVerificationProblem q;
  q.correspondences = &p->matches;
  q.camera1 = &p->camera1;
  q.camera2 = &p->camera2;
  q.constant_camera1_intrinsics = q.constant_camera2_intrinsics = !p->free_focal;
  q.info = &p->info;
  q.inlier_indices = &p->inliers;
  return q;
}

static bool SameBits(const double* a, const double* b, int n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

int main() {
  const int sizes[] = {200, 30, 90, 64, 45, 12, 333};  // 30 and 12: at / under the input gate; 45: 36 near points
  const int P = sizeof(sizes) / sizeof(sizes[0]);
  std::vector<Pair> batch(P), single(P), raw(P);
  for (int p = 0; p < P; ++p) {
    MakePair(100 + p, sizes[p], p % 2 == 1, &batch[p]);
    MakePair(100 + p, sizes[p], p % 2 == 1, &single[p]);
    MakePair(100 + p, sizes[p], p % 2 == 1, &raw[p]);
  }
  TwoViewMatchGeometricVerificationOptions opt;

  // the batch call
  std::vector<TwoViewVerificationProblem> problems;
  for (int p = 0; p < P; ++p) problems.push_back(Problem(&batch[p]));
  const std::vector<bool> ok = BundleAdjustRelativePoseBatch(opt, &problems);
  EXPECT((int)ok.size() == P);

  // the C ABI on the same pairs
  std::vector<double> e1(6 * P), e2(6 * P), k1(10 * P, 0.0), k2(10 * P, 0.0), f1, f2;
  std::vector<int32_t> m1(P, 0), m2(P, 0);
  std::vector<uint8_t> c1(P), c2(P);
  std::vector<int64_t> ptr(P + 1, 0);
  for (int p = 0; p < P; ++p) {
    for (int a = 0; a < 6; ++a) {
      e1[6 * p + a] = raw[p].camera1.extrinsics()[a];
      e2[6 * p + a] = raw[p].camera2.extrinsics()[a];
    }
    for (int a = 0; a < 7; ++a) {
      k1[10 * p + a] = raw[p].camera1.intrinsics()[a];
      k2[10 * p + a] = raw[p].camera2.intrinsics()[a];
    }
    c1[p] = c2[p] = raw[p].free_focal ? 0 : 1;
    for (const FeatureCorrespondence& m : raw[p].matches) {
      f1.push_back(m.feature1.x());
      f1.push_back(m.feature1.y());
      f2.push_back(m.feature2.x());
      f2.push_back(m.feature2.y());
    }
    ptr[p + 1] = ptr[p] + (int64_t)raw[p].matches.size();
  }
  std::vector<double> pts(4 * ptr[P], 0.0);
  tmi_ba_two_view_batch B;
  B.num_pairs = P;
  B.extrinsics1 = e1.data();
  B.extrinsics2 = e2.data();
  B.model1 = m1.data();
  B.model2 = m2.data();
  B.intrinsics1 = k1.data();
  B.intrinsics2 = k2.data();
  B.constant_intrinsics1 = c1.data();
  B.constant_intrinsics2 = c2.data();
  B.correspondence_ptr = ptr.data();
  B.features1 = f1.data();
  B.features2 = f2.data();
  B.points = pts.data();
  tmi_ba_two_view_verification_options vo;
  tmi_ba_two_view_verification_options_init(&vo);
  std::vector<int8_t> cst(ptr[P], -1), pst(P, -1);
  std::vector<int32_t> cnt(P, 0);
  tmi_ba_two_view_verification_summary vs;
  const int rc = tmi_ba_verify_two_views(&B, &vo, 4, 200, -1, cst.data(), pst.data(), cnt.data(), nullptr, nullptr,
                                         nullptr, nullptr, &vs);
  EXPECT(rc == TMI_BA_OK);
  if (rc != TMI_BA_OK) {
    std::printf("ABI call failed: %s\n", tmi_ba_last_error());
    return 1;
  }

  int n_true = 0, n_false = 0;
  for (int p = 0; p < P; ++p) {
    // the single call
    const bool one = BundleAdjustRelativePose(opt, Problem(&single[p]));
    const bool want = pst[p] == 0 || pst[p] == 4;
    std::printf("pair %d: n %d status %d verified %d  batch %d single %d\n", p, sizes[p], (int)pst[p], cnt[p],
                (int)ok[p], (int)one);
    EXPECT(ok[p] == want);
    EXPECT(one == want);
    want ? ++n_true : ++n_false;
    for (Pair* q : {&batch[p], &single[p]}) {
      if (!want) {  // nothing is written
        EXPECT(SameBits(q->camera2.extrinsics(), raw[p].camera2.extrinsics(), 6));
        EXPECT(q->camera1.FocalLength() == raw[p].camera1.FocalLength());
        EXPECT(q->info.focal_length_1 == -1.0 && q->inliers.empty());
        continue;
      }
      EXPECT(SameBits(q->camera2.extrinsics(), &e2[6 * p], 6));
      EXPECT(q->camera1.FocalLength() == k1[10 * p] && q->camera2.FocalLength() == k2[10 * p]);
      EXPECT(SameBits(q->camera1.extrinsics(), raw[p].camera1.extrinsics(), 6));
      EXPECT(q->info.focal_length_1 == k1[10 * p] && q->info.focal_length_2 == k2[10 * p]);
      for (int a = 0; a < 3; ++a) EXPECT(q->info.rotation_2[a] == e2[6 * p + 3 + a]);
      const double n2 = q->info.position_2[0] * q->info.position_2[0] + q->info.position_2[1] * q->info.position_2[1] +
                        q->info.position_2[2] * q->info.position_2[2];
      EXPECT(std::fabs(n2 - 1.0) < 1e-15);
      const double n = std::sqrt(e2[6 * p] * e2[6 * p] + e2[6 * p + 1] * e2[6 * p + 1] + e2[6 * p + 2] * e2[6 * p + 2]);
      for (int a = 0; a < 3; ++a) EXPECT(q->info.position_2[a] == e2[6 * p + a] / n);
      std::vector<int> expect;
      for (int64_t i = ptr[p]; i < ptr[p + 1]; ++i)
        if (cst[i] == 0) expect.push_back((int)(i - ptr[p]));
      EXPECT(q->inliers == expect);
      EXPECT((int)expect.size() == cnt[p]);
    }
    if (want) {
      EXPECT(!SameBits(&e2[6 * p], raw[p].camera2.extrinsics(), 6));  // the adjustment moved camera 2
      if (raw[p].free_focal) EXPECT(k1[10 * p] != raw[p].camera1.FocalLength());
      else EXPECT(k1[10 * p] == raw[p].camera1.FocalLength());
    }
  }
  EXPECT(n_true >= 4 && n_false >= 2);
  EXPECT(pst[1] == 1 && pst[5] == 1);
  // null arguments: false, not a crash
  TwoViewVerificationProblem none;
  EXPECT(!BundleAdjustRelativePose(opt, none));
  std::vector<TwoViewVerificationProblem> empty;
  EXPECT(BundleAdjustRelativePoseBatch(opt, &empty).empty());
  std::printf(g_fail ? "%d FAILED\n" : "all passed\n", g_fail);
  return g_fail ? 1 : 0;
}
