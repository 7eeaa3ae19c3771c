// tests/test_host_shim_view_pair_filter.py: the view-pair filter shim (theiasfm_amd/host/view_pair_filter_ops.cc).
//   without a device: both calls leave the edge vector as it is and return 0.
//   with a device:    the shim equals the C ABI called on the same edges with the views numbered in ascending ViewId
//                     order; removed edges are erased and the others keep their order; the orientation filter removes
//                     an edge with a view that has no orientation without sending it to the device.
// `--need-device` makes the absence of a device a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <unordered_map>
#include <vector>

#include "theia/sfm/filter_view_pairs_from_orientation.h"
#include "theia/sfm/filter_view_pairs_from_relative_translation.h"
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
using EdgeList = std::vector<std::pair<ViewIdPair, TwoViewInfo*>>;

namespace {
// a small deterministic generator for the scene
struct Lcg {
  unsigned long long s;
  double next() {  // uniform in [-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(s >> 11) / 4503599627370496.0 - 1.0;
  }
};

struct Scene {
  std::vector<ViewId> ids;  // NOT ascending
  std::unordered_map<ViewId, Eigen::Vector3d> orientations;
  std::vector<TwoViewInfo> infos;
  EdgeList edges;
};

// Views on scattered ids with small rotations; edges between them in an order unrelated to the ids.  Translations in
// the frame of view 1 are random (the filter's arithmetic is what is compared, not its verdict), rotation_2 is small
// for even edges and large for odd ones.
Scene MakeScene() {
  Scene sc;
  sc.ids = {50, 7, 300, 12, 9, 1000, 3, 77};
  Lcg rng{12345};
  for (const ViewId id : sc.ids) {
    Eigen::Vector3d r;
    for (int a = 0; a < 3; ++a) r[a] = 0.05 * rng.next();
    sc.orientations[id] = r;
  }
  const int pairs[][2] = {{0, 1}, {2, 1}, {2, 3}, {4, 3}, {4, 5}, {6, 5}, {6, 7}, {0, 7}, {0, 4}, {5, 1}, {3, 7}, {2, 6}};
  const int n = static_cast<int>(sizeof(pairs) / sizeof(pairs[0]));
  sc.infos.resize(n);
  for (int e = 0; e < n; ++e) {
    TwoViewInfo& info = sc.infos[e];
    double norm = 0.0;
    for (int a = 0; a < 3; ++a) {
      info.position_2[a] = rng.next();
      norm += info.position_2[a] * info.position_2[a];
      info.rotation_2[a] = (e % 2 ? 0.8 : 0.01) * rng.next();
    }
    for (int a = 0; a < 3; ++a) info.position_2[a] /= std::sqrt(norm);
    sc.edges.emplace_back(ViewIdPair(sc.ids[pairs[e][0]], sc.ids[pairs[e][1]]), &sc.infos[e]);
  }
  return sc;
}

// The dense batch of `edges` with the views in ascending ViewId order, built independently of the shim.
struct Dense {
  std::vector<double> rotation, rotation2, position2;
  std::vector<int32_t> view1, view2;
  tmi_ba_view_pair_batch B;
};
void MakeDense(const Scene& sc, const EdgeList& edges, Dense* d) {
  std::vector<ViewId> sorted;
  for (const auto& e : edges) {
    sorted.push_back(e.first.first);
    sorted.push_back(e.first.second);
  }
  std::sort(sorted.begin(), sorted.end());
  sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
  for (const ViewId id : sorted)
    for (int a = 0; a < 3; ++a) d->rotation.push_back(sc.orientations.at(id)[a]);
  auto index = [&](ViewId id) {
    return static_cast<int32_t>(std::lower_bound(sorted.begin(), sorted.end(), id) - sorted.begin());
  };
  for (const auto& e : edges) {
    d->view1.push_back(index(e.first.first));
    d->view2.push_back(index(e.first.second));
    for (int a = 0; a < 3; ++a) {
      d->rotation2.push_back(e.second->rotation_2[a]);
      d->position2.push_back(e.second->position_2[a]);
    }
  }
  d->B.num_views = static_cast<int32_t>(sorted.size());
  d->B.view_rotation = d->rotation.data();
  d->B.num_pairs = static_cast<int32_t>(edges.size());
  d->B.pair_view1 = d->view1.data();
  d->B.pair_view2 = d->view2.data();
  d->B.pair_rotation2 = d->rotation2.data();
  d->B.pair_position2 = d->position2.data();
}

EdgeList Survivors(const EdgeList& edges, const std::vector<uint8_t>& flag) {
  EdgeList out;
  for (size_t e = 0; e < edges.size(); ++e)
    if (!flag[e]) out.push_back(edges[e]);
  return out;
}
}  // namespace

int main(int argc, char** argv) {
  const bool need_device = argc > 1 && std::strcmp(argv[1], "--need-device") == 0;
  const bool have_device = tmi_ba_device_count() > 0;
  CHECK(have_device || !need_device);
  Scene sc = MakeScene();
  const EdgeList all = sc.edges;
  theia::FilterViewPairsFromRelativeTranslationOptions options;
  options.num_iterations = 7;
  options.translation_projection_tolerance = 0.02;
  options.num_threads = 4;  // accepted and unused
  Lcg rng{99};
  for (int i = 0; i < options.num_iterations; ++i) {
    Eigen::Vector3d a;
    double norm = 0.0;
    for (int k = 0; k < 3; ++k) {
      a[k] = rng.next();
      norm += a[k] * a[k];
    }
    for (int k = 0; k < 3; ++k) a[k] /= std::sqrt(norm);
    options.axes.push_back(a);
  }

  if (!have_device) {
    EdgeList edges = all;
    CHECK(theia::FilterViewPairsFromRelativeTranslation(options, sc.orientations, &edges) == 0);
    CHECK(edges == all);
    CHECK(theia::FilterViewPairsFromOrientation(sc.orientations, 5.0, &edges) == 0);
    CHECK(edges == all);
    sc.orientations.erase(ViewId(300));  // even the host-side rule waits for the device call to succeed
    CHECK(theia::FilterViewPairsFromOrientation(sc.orientations, 5.0, &edges) == 0);
    CHECK(edges == all);
    std::printf("view-pair filter shim without a device: OK\n");
    return 0;
  }

  // ---- the translation filter: the shim equals the C ABI on ascending ids --------------------------------------------
  {
    Dense d;
    MakeDense(sc, all, &d);
    CHECK(d.view1[0] == 4 && d.view2[0] == 1);  // ids 50 and 7 among {3, 7, 9, 12, 50, 77, 300, 1000}
    tmi_ba_translation_filter_options o;
    tmi_ba_translation_filter_options_init(&o);
    o.num_iterations = options.num_iterations;
    o.translation_projection_tolerance = options.translation_projection_tolerance;
    std::vector<double> axes;
    for (const auto& a : options.axes)
      for (int k = 0; k < 3; ++k) axes.push_back(a[k]);
    std::vector<uint8_t> flag(all.size());
    tmi_ba_view_pair_filter_summary fs;
    CHECK(tmi_ba_filter_view_pairs_from_relative_translation(&d.B, &o, axes.data(), 1, -1, flag.data(), nullptr, nullptr,
                                                             nullptr, &fs) == TMI_BA_OK);
    const EdgeList want = Survivors(all, flag);
    CHECK(fs.num_pairs_removed > 0 && want.size() + fs.num_pairs_removed == all.size() && !want.empty());
    EdgeList edges = all;
    CHECK(theia::FilterViewPairsFromRelativeTranslation(options, sc.orientations, &edges) == fs.num_pairs_removed);
    CHECK(edges == want);
    // drawn axes: deterministic in the seed
    theia::FilterViewPairsFromRelativeTranslationOptions drawn;
    drawn.seed = 5;
    EdgeList a = all, b = all;
    const int ra = theia::FilterViewPairsFromRelativeTranslation(drawn, sc.orientations, &a);
    CHECK(theia::FilterViewPairsFromRelativeTranslation(drawn, sc.orientations, &b) == ra && a == b);
    CHECK(a.size() + ra == all.size());
    // a view without an orientation: the reference dies; here nothing is filtered
    auto fewer = sc.orientations;
    fewer.erase(ViewId(300));
    edges = all;
    CHECK(theia::FilterViewPairsFromRelativeTranslation(options, fewer, &edges) == 0 && edges == all);
  }

  // ---- the orientation filter ----------------------------------------------------------------------------------------
  {
    Dense d;
    MakeDense(sc, all, &d);
    std::vector<uint8_t> flag(all.size());
    tmi_ba_view_pair_filter_summary fs;
    CHECK(tmi_ba_filter_view_pairs_from_orientation(&d.B, 5.0, -1, flag.data(), nullptr, &fs) == TMI_BA_OK);
    const EdgeList want = Survivors(all, flag);
    CHECK(fs.num_pairs_removed > 0 && !want.empty());
    EdgeList edges = all;
    CHECK(theia::FilterViewPairsFromOrientation(sc.orientations, 5.0, &edges) == fs.num_pairs_removed);
    CHECK(edges == want);
    // the missing-orientation rule (:94-103): every edge of view 300 goes, the rest is filtered as before
    auto fewer = sc.orientations;
    fewer.erase(ViewId(300));
    EdgeList rest, expect;
    for (const auto& e : all)
      if (e.first.first != 300 && e.first.second != 300) rest.push_back(e);
    CHECK(rest.size() + 3 == all.size());
    Dense dr;
    MakeDense(sc, rest, &dr);
    CHECK(dr.B.num_views == 7);
    std::vector<uint8_t> flag_rest(rest.size());
    CHECK(tmi_ba_filter_view_pairs_from_orientation(&dr.B, 5.0, -1, flag_rest.data(), nullptr, &fs) == TMI_BA_OK);
    expect = Survivors(rest, flag_rest);
    edges = all;
    CHECK(theia::FilterViewPairsFromOrientation(fewer, 5.0, &edges) == static_cast<int>(all.size() - expect.size()));
    CHECK(edges == expect);
    // 180 degrees removes nothing; a negative threshold filters nothing
    edges = all;
    CHECK(theia::FilterViewPairsFromOrientation(sc.orientations, 180.0, &edges) == 0 && edges == all);
    CHECK(theia::FilterViewPairsFromOrientation(sc.orientations, -1.0, &edges) == 0 && edges == all);
  }
  std::printf("view-pair filter shim: OK\n");
  return 0;
}
