// What tmi_ba_build_tracks is measured against (tools/track_build_probe.py): a single-thread restatement of the
// reference's loop on the host -- a hash map from (view, feature) to a node id in order of first use
// (track_builder.cc:133-151), a hash map from node id to {root id, size} united by size under the cap on every edge in
// order with the root search that flattens on the way back (connected_components.h:87-162), the sets gathered per root
// and one observation kept per view (track_builder.cc:89-119).  That part is timed.  The sets are then put into the
// ABI's order (label = smallest node id, the lowest node id per view kept, tracks and observations ascending; not
// timed, the reference has no such order) and written out so that the probe can compare them with the device's.
//
//   track_build_host_baseline IN OUT     IN:  int64 E, int32 min, int32 max, uint32 view[2E], uint32 feature[2E]
//                                        OUT: int64 num_tracks, int64 num_obs, int64 begin[num_tracks + 1],
//                                             uint32 view[num_obs], uint32 feature[num_obs]
// Prints one JSON line with the times.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace {
struct Root {
  uint64_t id;
  int size;
};
typedef std::unordered_map<uint64_t, Root> DisjointSet;

Root* FindRoot(DisjointSet* set, uint64_t node) {
  Root* entry = &set->find(node)->second;
  if (entry->id == node) return entry;
  Root* root = FindRoot(set, entry->id);
  *entry = *root;
  return root;
}

double Now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int64_t E = 0;
  int32_t min_length = 0, max_length = 0;
  if (std::fread(&E, 8, 1, in) != 1 || std::fread(&min_length, 4, 1, in) != 1 || std::fread(&max_length, 4, 1, in) != 1) return 2;
  std::vector<uint32_t> view(2 * E), feature(2 * E);
  if (std::fread(view.data(), 4, 2 * E, in) != (size_t)(2 * E) || std::fread(feature.data(), 4, 2 * E, in) != (size_t)(2 * E)) return 2;
  std::fclose(in);

  const double t0 = Now();
  std::unordered_map<uint64_t, uint64_t> node_of;  // (view << 32 | feature) -> id
  std::vector<uint64_t> key_of_node;
  DisjointSet set;
  auto node_id = [&](int64_t i) {
    const uint64_t key = ((uint64_t)view[i] << 32) | feature[i];
    const auto inserted = node_of.emplace(key, (uint64_t)key_of_node.size());
    if (inserted.second) key_of_node.push_back(key);
    return inserted.first->second;
  };
  auto root_of = [&](uint64_t node) {
    const auto inserted = set.emplace(node, Root{node, 1});
    return inserted.second ? &inserted.first->second : FindRoot(&set, node);
  };
  for (int64_t e = 0; e < E; ++e) {
    const uint64_t a = node_id(2 * e), b = node_id(2 * e + 1);
    Root* ra = root_of(a);
    Root* rb = root_of(b);
    if (ra->id == rb->id || ra->size + rb->size > max_length) continue;
    if (ra->size < rb->size) {
      rb->size += ra->size;
      *ra = *rb;
    } else {
      ra->size += rb->size;
      *rb = *ra;
    }
  }
  const double t1 = Now();
  std::unordered_map<uint64_t, std::vector<uint64_t>> members;
  for (const auto& node : set) members[FindRoot(&set, node.first)->id].push_back(node.first);
  int64_t num_small = 0, num_inconsistent = 0, num_kept = 0;
  for (const auto& m : members) {
    if ((int)m.second.size() < std::max(min_length, 2)) {
      ++num_small;
      continue;
    }
    std::unordered_set<uint32_t> views;
    for (const uint64_t node : m.second) {
      if (views.insert((uint32_t)(key_of_node[node] >> 32)).second)
        ++num_kept;
      else
        ++num_inconsistent;
    }
  }
  const double t2 = Now();

  // the ABI's order
  std::vector<std::pair<uint64_t, const std::vector<uint64_t>*>> tracks;
  for (auto& m : members) {
    if ((int)m.second.size() < std::max(min_length, 2)) continue;
    std::sort(m.second.begin(), m.second.end());
    tracks.emplace_back(m.second[0], &m.second);
  }
  std::sort(tracks.begin(), tracks.end());
  std::vector<int64_t> begin(1, 0);
  std::vector<uint32_t> obs_view, obs_feature;
  for (const auto& t : tracks) {
    std::unordered_set<uint32_t> views;
    for (const uint64_t node : *t.second) {
      const uint64_t key = key_of_node[node];
      if (!views.insert((uint32_t)(key >> 32)).second) continue;
      obs_view.push_back((uint32_t)(key >> 32));
      obs_feature.push_back((uint32_t)key);
    }
    begin.push_back((int64_t)obs_view.size());
  }
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  const int64_t num_tracks = (int64_t)tracks.size(), num_obs = (int64_t)obs_view.size();
  std::fwrite(&num_tracks, 8, 1, out);
  std::fwrite(&num_obs, 8, 1, out);
  std::fwrite(begin.data(), 8, begin.size(), out);
  std::fwrite(obs_view.data(), 4, obs_view.size(), out);
  std::fwrite(obs_feature.data(), 4, obs_feature.size(), out);
  std::fclose(out);
  std::printf("{\"host_seconds\": %.6f, \"host_union_seconds\": %.6f, \"host_extract_seconds\": %.6f, "
              "\"host_num_nodes\": %lld, \"host_num_tracks\": %lld, \"host_num_observations\": %lld, "
              "\"host_num_small_tracks\": %lld, \"host_num_inconsistent_features\": %lld}\n",
              t2 - t0, t1 - t0, t2 - t1, (long long)key_of_node.size(), (long long)num_tracks, (long long)num_obs,
              (long long)num_small, (long long)num_inconsistent);
  return num_kept == num_obs ? 0 : 1;
}
