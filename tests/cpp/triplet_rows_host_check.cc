// tests/test_triplet_rows_host_cpu.py: the three host builders of the linear position estimator
// (theiasfm_amd/csrc/pose_graph_host.h: build_sorted_adjacency, build_view_tracks, build_triplet_rows) with a main of
// their own, compiled for the host under -fsanitize=address,undefined.  Reads commands from stdin, prints the arrays:
//   adjacency V E  a b ...            -> ptr / adj (neighbour edge ...) / owner
//   tracks V N  view track ...        -> ptr / track / obs / repeated
//   triplets V C  a b c ...           -> views / view_column / view_count / column / view_ptr / view_entry / block_ptr /
//                                        block_pq / block_entry
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "pose_graph_host.h"

namespace {
template <class T>
void print(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (const T& x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}
void print(const char* name, const std::vector<int2>& v) {
  std::printf("%s", name);
  for (const int2& x : v) std::printf(" %d %d", x.x, x.y);
  std::printf("\n");
}
}  // namespace

int main() {
  std::string what;
  while (std::cin >> what) {
    int V, n;
    std::cin >> V >> n;
    if (what == "adjacency") {
      std::vector<int32_t> a(n), b(n);
      for (int e = 0; e < n; ++e) std::cin >> a[e] >> b[e];
      const tmi::SortedAdjacency S = tmi::build_sorted_adjacency(V, n, a.data(), b.data());
      print("ptr", S.ptr);
      print("adj", S.adj);
      print("owner", S.owner);
    } else if (what == "tracks") {
      std::vector<int32_t> view(n), track(n);
      for (int i = 0; i < n; ++i) std::cin >> view[i] >> track[i];
      const tmi::ViewTracks T = tmi::build_view_tracks(V, n, view.data(), track.data());
      print("ptr", T.ptr);
      print("track", T.track);
      print("obs", T.obs);
      std::printf("repeated %d\n", (int)T.repeated);
    } else if (what == "triplets") {
      std::vector<int> view(3 * (size_t)n);
      for (int& v : view) std::cin >> v;
      const tmi::TripletRows R = tmi::build_triplet_rows(V, n, view.data());
      print("views", R.views);
      print("view_column", R.view_column);
      print("view_count", R.view_count);
      print("column", R.column);
      print("view_ptr", R.view_ptr);
      print("view_entry", R.view_entry);
      print("block_ptr", R.block_ptr);
      print("block_pq", R.block_pq);
      print("block_entry", R.block_entry);
    } else {
      return 2;
    }
  }
  return 0;
}
