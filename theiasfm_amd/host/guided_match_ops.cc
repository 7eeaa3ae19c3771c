// Host shim of theia::GuidedEpipolarMatcher (reference guided_epipolar_matcher.cc) on the C ABI: the images'
// descriptors and keypoints are packed once, F of every pair is formed from its two cameras, all pairs go through one
// tmi_ba_guided_epipolar_match call, and the added matches are appended pair by pair.
#include <cmath>
#include <cstdio>

#include "theia/matching/guided_epipolar_matcher.h"
#include "theia_mi355_ba.h"

namespace theia {
namespace {
bool HasSkew(const CameraIntrinsicsModelType type) {
  return type == CameraIntrinsicsModelType::PINHOLE || type == CameraIntrinsicsModelType::PINHOLE_RADIAL_TANGENTIAL ||
         type == CameraIntrinsicsModelType::FISHEYE;
}

double Det4(const double* r0, const double* r1, const double* r2, const double* r3) {
  // the 2 x 2 minors of the upper and of the lower two rows, paired by complementary columns
  const double s0 = r0[0] * r1[1] - r0[1] * r1[0], s1 = r0[0] * r1[2] - r0[2] * r1[0];
  const double s2 = r0[0] * r1[3] - r0[3] * r1[0], s3 = r0[1] * r1[2] - r0[2] * r1[1];
  const double s4 = r0[1] * r1[3] - r0[3] * r1[1], s5 = r0[2] * r1[3] - r0[3] * r1[2];
  const double c5 = r2[2] * r3[3] - r2[3] * r3[2], c4 = r2[1] * r3[3] - r2[3] * r3[1];
  const double c3 = r2[1] * r3[2] - r2[2] * r3[1], c2 = r2[0] * r3[3] - r2[3] * r3[0];
  const double c1 = r2[0] * r3[2] - r2[2] * r3[0], c0 = r2[0] * r3[1] - r2[1] * r3[0];
  return s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
}
}  // namespace

void GuidedMatchProjectionMatrix(const Camera& camera, double P[12]) {
  const double* in = camera.intrinsics();
  const bool skew = HasSkew(camera.GetCameraIntrinsicsModelType());
  const int pp = skew ? 3 : 2;
  const double K[9] = {in[0], skew ? in[2] : 0.0, in[pp], 0.0, in[0] * in[1], in[pp + 1], 0.0, 0.0, 1.0};
  const Eigen::Vector3d aa = camera.GetOrientationAsAngleAxis(), c = camera.GetPosition();
  const double angle = std::sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (angle != 0.0) {  // Rodrigues: cos I + (1 - cos) a a^T + sin [a]x
    const double a[3] = {aa[0] / angle, aa[1] / angle, aa[2] / angle};
    const double co = std::cos(angle), si = std::sin(angle), t = 1.0 - co;
    R[0] = co + t * a[0] * a[0];
    R[1] = t * a[0] * a[1] - si * a[2];
    R[2] = t * a[0] * a[2] + si * a[1];
    R[3] = t * a[1] * a[0] + si * a[2];
    R[4] = co + t * a[1] * a[1];
    R[5] = t * a[1] * a[2] - si * a[0];
    R[6] = t * a[2] * a[0] - si * a[1];
    R[7] = t * a[2] * a[1] + si * a[0];
    R[8] = co + t * a[2] * a[2];
  }
  double Rt[12];
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) Rt[4 * r + k] = R[3 * r + k];
    Rt[4 * r + 3] = -(R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]);
  }
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) P[4 * r + k] = K[3 * r] * Rt[k] + K[3 * r + 1] * Rt[4 + k] + K[3 * r + 2] * Rt[8 + k];
}

void GuidedMatchFundamentalMatrix(const Camera& camera1, const Camera& camera2, double F[9]) {
  // FundamentalMatrixFromProjectionMatrices(pmatrix1 = P of camera 2, pmatrix2 = P of camera 1)
  double P1[12], P2[12];
  GuidedMatchProjectionMatrix(camera2, P1);
  GuidedMatchProjectionMatrix(camera1, P2);
  const int index1[3] = {1, 2, 0}, index2[3] = {2, 0, 1};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      F[3 * r + c] = Det4(P2 + 4 * index1[c], P2 + 4 * index2[c], P1 + 4 * index1[r], P1 + 4 * index2[r]);
}

bool GuidedEpipolarMatches(const GuidedEpipolarMatcher::Options& options,
                           const std::vector<const KeypointsAndDescriptors*>& features_per_image,
                           const std::vector<std::pair<int, int>>& pairs, const std::vector<const Camera*>& cameras,
                           std::vector<std::vector<IndexedFeatureMatch>>* matches_per_pair) {
  auto fail = [](const char* why) {
    std::fprintf(stderr, "[theia::GuidedEpipolarMatcher] %s\n", why);
    return false;
  };
  if (matches_per_pair == nullptr || matches_per_pair->size() != pairs.size()) return fail("one match vector per pair is needed");
  if (cameras.size() != features_per_image.size()) return fail("one camera per image is needed");
  const int num_images = static_cast<int>(features_per_image.size());
  int dim = 0;
  std::vector<int64_t> image_begin(features_per_image.size() + 1, 0);
  for (size_t m = 0; m < features_per_image.size(); ++m) {
    const KeypointsAndDescriptors* f = features_per_image[m];
    const size_t n = f != nullptr ? f->descriptors.size() : 0;
    if (f != nullptr && f->keypoints.size() != n) return fail("keypoints and descriptors differ in number");
    image_begin[m + 1] = image_begin[m] + static_cast<int64_t>(n);
    for (size_t i = 0; i < n; ++i) {
      if (dim == 0) dim = f->descriptors[i].size();
      if (f->descriptors[i].size() != dim || dim < 1) return fail("descriptors of differing or zero length");
    }
  }
  for (const std::pair<int, int>& p : pairs) {
    for (const int m : {p.first, p.second}) {
      if (m < 0 || m >= num_images || features_per_image[m] == nullptr || cameras[m] == nullptr)
        return fail("image index out of range");
      if (features_per_image[m]->descriptors.empty()) return fail("empty descriptors");
    }
  }
  if (pairs.empty()) return true;
  std::vector<float> descriptors(static_cast<size_t>(image_begin.back()) * static_cast<size_t>(dim));
  std::vector<double> keypoints(2 * static_cast<size_t>(image_begin.back()));
  for (size_t m = 0; m < features_per_image.size(); ++m) {
    if (features_per_image[m] == nullptr) continue;
    float* out = descriptors.data() + static_cast<size_t>(image_begin[m]) * static_cast<size_t>(dim);
    double* key = keypoints.data() + 2 * static_cast<size_t>(image_begin[m]);
    for (const Eigen::VectorXf& d : features_per_image[m]->descriptors) {
      for (int k = 0; k < dim; ++k) out[k] = d[k];
      out += dim;
    }
    for (const Keypoint& k : features_per_image[m]->keypoints) {
      *key++ = k.x();
      *key++ = k.y();
    }
  }
  const size_t P = pairs.size();
  std::vector<int32_t> image1(P), image2(P), match1, match2;
  std::vector<int64_t> match_begin(P + 1, 0);
  std::vector<double> F(9 * P);
  std::vector<uint32_t> stream(P, 0u);  // every pair draws as the single call does: stream 0
  int64_t capacity = 0;
  for (size_t p = 0; p < P; ++p) {
    image1[p] = pairs[p].first;
    image2[p] = pairs[p].second;
    GuidedMatchFundamentalMatrix(*cameras[image1[p]], *cameras[image2[p]], F.data() + 9 * p);
    for (const IndexedFeatureMatch& m : (*matches_per_pair)[p]) {
      match1.push_back(m.feature1_ind);
      match2.push_back(m.feature2_ind);
    }
    match_begin[p + 1] = static_cast<int64_t>(match1.size());
    capacity += image_begin[image1[p] + 1] - image_begin[image1[p]];
  }
  tmi_ba_guided_match_options O;
  tmi_ba_guided_match_options_init(&O);
  O.guided_matching_max_distance_pixels = options.guided_matching_max_distance_pixels;
  O.lowes_ratio = options.lowes_ratio;
  O.seed = options.seed;
  O.device = options.device;
  std::vector<int8_t> status(P, 1);
  std::vector<int32_t> num_groups(P, 0), feature1(static_cast<size_t>(capacity)), feature2(static_cast<size_t>(capacity));
  std::vector<int64_t> begin(P + 1, 0);
  std::vector<float> distance(static_cast<size_t>(capacity));
  tmi_ba_guided_match_summary summary;
  const int rc = tmi_ba_guided_epipolar_match(
      &O, num_images, image_begin.data(), descriptors.data(), dim, keypoints.data(), static_cast<int32_t>(P),
      image1.data(), image2.data(), F.data(), match_begin.data(), match1.data(), match2.data(), nullptr, stream.data(),
      capacity, status.data(), num_groups.data(), begin.data(), feature1.data(), feature2.data(), distance.data(),
      nullptr, nullptr, nullptr, &summary);
  if (rc != TMI_BA_OK) {
    std::fprintf(stderr, "[theia::GuidedEpipolarMatcher] device call failed: %s\n", tmi_ba_last_error());
    return false;
  }
  for (size_t p = 0; p < P; ++p) {
    std::vector<IndexedFeatureMatch>& out = (*matches_per_pair)[p];
    out.reserve(out.size() + static_cast<size_t>(begin[p + 1] - begin[p]));
    for (int64_t i = begin[p]; i < begin[p + 1]; ++i) out.emplace_back(feature1[i], feature2[i], distance[i]);
  }
  return true;
}

bool GuidedEpipolarMatcher::GetMatches(std::vector<IndexedFeatureMatch>* matches) {
  if (matches == nullptr) return false;
  std::vector<std::vector<IndexedFeatureMatch>> per_pair(1, *matches);
  if (!GuidedEpipolarMatches(options_, {&features1_, &features2_}, {{0, 1}}, {&camera1_, &camera2_}, &per_pair))
    return false;
  matches->swap(per_pair[0]);
  return true;
}

}  // namespace theia
