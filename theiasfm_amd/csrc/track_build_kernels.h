// TrackBuilder on the device (tmi_ba_build_tracks; the steps are numbered in include/theia_mi355_ba.h): node ids from
// the sorted (view, feature) keys, the components of the unconstrained graph by a concurrent union-find, the replay of
// the components above the cap one thread each, and the tracks as a CSR.  Everything is integers; every count goes
// through integer atomic adds, so no result depends on the order in which threads arrive.
//
// The union-find (tb_union_kernel) always makes the SMALLER root the parent, so node ids strictly decrease along a
// parent chain and a component's root is its smallest node id whatever the interleaving.  Inside that launch parent[]
// is touched only by agent-scope atomic loads, min and compare-and-swap: a plain load may be served from a CU's L1
// that no other CU's store refreshes.  A stale parent that does get read is an OLDER one, which is still in the same
// set and has a smaller id than the reader, so it costs steps and never correctness.  Every loop has a bound (a chain
// has fewer than num_nodes links; a link can fail at most once per link another thread made); a thread that reaches
// one raises counters[kTbError] and leaves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tmi {
enum { kTbComponents = 0, kTbOversize, kTbSets, kTbSmall, kTbInconsistent, kTbError, kTbCounters = 8 };
constexpr unsigned kTbNoLabel = 0xffffffffu;  // node ids are below 2^31

__device__ __forceinline__ unsigned tb_load(unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One add per wavefront of the lanes with `flag`.
__device__ __forceinline__ void tb_count(bool flag, unsigned long long* counter) {
  const unsigned long long m = __ballot(flag);
  if (m && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// table[key] += 1 for every lane with key != kTbNoLabel, one atomic per run of equal keys on consecutive lanes (the
// endpoints of an edge, and the edges of a track, sit next to each other).  Called by every lane of the wavefront.
__device__ __forceinline__ void tb_run_add(unsigned key, unsigned* table) {
  const int lane = (int)__lane_id();
  const unsigned prev = __shfl_up(key, 1);
  const bool head = lane == 0 || prev != key;
  const unsigned long long above = (__ballot(head) >> lane) >> 1;  // the heads on higher lanes
  if (head && key != kTbNoLabel) atomicAdd(&table[key], above ? (unsigned)__ffsll((long long)above) : (unsigned)(64 - lane));
}

// ---- step 1: node ids ---------------------------------------------------------------------------
__global__ void tb_keys_kernel(const unsigned* __restrict__ view, const unsigned* __restrict__ feature, long long n,
                               unsigned long long* __restrict__ key, unsigned* __restrict__ index) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = ((unsigned long long)view[i] << 32) | feature[i];
  index[i] = (unsigned)i;
}

// The sort is stable and the indices went in ascending, so a run's head holds the smallest endpoint index of its key:
// the first appearance.
__global__ void tb_run_heads_kernel(const unsigned long long* __restrict__ key, const unsigned* __restrict__ index,
                                    long long n, unsigned* __restrict__ head, unsigned* __restrict__ first) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool h = i == 0 || key[i] != key[i - 1];
  head[i] = h;
  if (h) first[index[i]] = 1;  // (first[] was cleared)
}

// heads_before / firsts_before: the exclusive sums of head[] and first[].
__global__ void tb_run_nodes_kernel(const unsigned long long* __restrict__ key, const unsigned* __restrict__ index,
                                    const unsigned* __restrict__ head, const unsigned* __restrict__ heads_before,
                                    const unsigned* __restrict__ firsts_before, long long n,
                                    unsigned* __restrict__ run_node, unsigned* __restrict__ node_view,
                                    unsigned* __restrict__ node_feature) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  const unsigned node = firsts_before[index[i]];
  run_node[heads_before[i]] = node;
  node_view[node] = (unsigned)(key[i] >> 32);
  node_feature[node] = (unsigned)key[i];
}

__global__ void tb_endpoint_nodes_kernel(const unsigned* __restrict__ index, const unsigned* __restrict__ head,
                                         const unsigned* __restrict__ heads_before, const unsigned* __restrict__ run_node,
                                         long long n, unsigned* __restrict__ endpoint_node) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  endpoint_node[index[i]] = run_node[heads_before[i] + head[i] - 1];
}

__global__ void tb_iota_kernel(unsigned* __restrict__ a, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = i;
}

// ---- step 2: the components, the hot kernel -----------------------------------------------------
// The root of x, with path halving; kTbNoLabel when the bound is reached.
__device__ __forceinline__ unsigned tb_find(unsigned* parent, unsigned x, unsigned num_nodes) {
  for (unsigned step = 0; step < num_nodes; ++step) {
    const unsigned p = tb_load(&parent[x]);
    if (p == x) return x;
    const unsigned g = tb_load(&parent[p]);
    if (g == p) return p;
    __hip_atomic_fetch_min(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
  return kTbNoLabel;
}

__global__ void tb_union_kernel(const unsigned* __restrict__ endpoint_node, long long num_edges, unsigned num_nodes,
                                unsigned* parent, unsigned long long* counters) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= num_edges) return;
  unsigned a = endpoint_node[2 * e], b = endpoint_node[2 * e + 1];
  // a failed link means another thread linked this root first: at most num_nodes - 1 links are ever made
  for (unsigned attempt = 0; attempt <= num_nodes; ++attempt) {
    a = tb_find(parent, a, num_nodes);
    b = tb_find(parent, b, num_nodes);
    if (a == kTbNoLabel || b == kTbNoLabel) break;
    if (a == b) return;
    if (a < b) {
      const unsigned t = a;
      a = b;
      b = t;
    }
    unsigned expected = a;  // the larger root goes under the smaller; verified: it must still be a root
    if (__hip_atomic_compare_exchange_strong(&parent[a], &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
  }
  atomicAdd(&counters[kTbError], 1ull);
}

// A launch of its own: parent[] is final and read plainly.
__global__ void tb_flatten_kernel(const unsigned* __restrict__ parent, unsigned num_nodes, unsigned* __restrict__ label,
                                  unsigned long long* counters) {
  const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= num_nodes) return;
  unsigned x = n;
  for (unsigned step = 0; step < num_nodes; ++step) {
    const unsigned p = parent[x];
    if (p == x) {
      label[n] = x;
      return;
    }
    x = p;
  }
  label[n] = n;
  atomicAdd(&counters[kTbError], 1ull);
}

// size[label[n]] += 1 (component sizes, and later the sizes of the final sets).
__global__ void tb_sizes_kernel(const unsigned* __restrict__ label, unsigned num_nodes, unsigned* size) {
  const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;  // (the grid is whole wavefronts)
  tb_run_add(n < num_nodes ? label[n] : kTbNoLabel, size);
}

__global__ void tb_component_stats_kernel(const unsigned* __restrict__ label, const unsigned* __restrict__ size,
                                          unsigned num_nodes, unsigned cap, unsigned long long* counters) {
  const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;
  const bool root = n < num_nodes && label[n] == n;
  tb_count(root, &counters[kTbComponents]);
  tb_count(root && size[n] > cap, &counters[kTbOversize]);
}

// ---- step 3: the replay of the components above the cap -----------------------------------------
// flag[e] = the edge's component is oversize; edge_count[component] += 1 for those.
__global__ void tb_replay_edges_kernel(const unsigned* __restrict__ endpoint_node, const unsigned* __restrict__ label,
                                       const unsigned* __restrict__ size, long long num_edges, unsigned cap,
                                       unsigned* __restrict__ flag, unsigned* edge_count) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned key = kTbNoLabel;
  if (e < num_edges) {
    const unsigned c = label[endpoint_node[2 * e]];
    const bool over = size[c] > cap;
    flag[e] = over;
    if (over) key = c;
  }
  tb_run_add(key, edge_count);
}

// The flagged edges in ascending edge index, each with its component as the key of the stable sort that groups them.
__global__ void tb_replay_compact_kernel(const unsigned* __restrict__ endpoint_node, const unsigned* __restrict__ label,
                                         const unsigned* __restrict__ flag, const unsigned* __restrict__ before,
                                         long long num_edges, unsigned* __restrict__ key, unsigned* __restrict__ edge) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= num_edges || !flag[e]) return;
  key[before[e]] = label[endpoint_node[2 * e]];
  edge[before[e]] = (unsigned)e;
}

// Nodes sorted by (component, node id): position[node], and flag[i] at the first node of every oversize component.
__global__ void tb_component_heads_kernel(const unsigned* __restrict__ sorted_label, const unsigned* __restrict__ sorted_node,
                                          const unsigned* __restrict__ size, unsigned num_nodes, unsigned cap,
                                          unsigned* __restrict__ position, unsigned* __restrict__ flag) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_nodes) return;
  position[sorted_node[i]] = i;
  const unsigned c = sorted_label[i];
  flag[i] = (i == 0 || sorted_label[i - 1] != c) && size[c] > cap;
}

// The oversize components in ascending label: where their nodes begin in the sorted order, how many, how many edges.
__global__ void tb_component_list_kernel(const unsigned* __restrict__ sorted_label, const unsigned* __restrict__ flag,
                                         const unsigned* __restrict__ before, const unsigned* __restrict__ size,
                                         const unsigned* __restrict__ edge_count, unsigned num_nodes,
                                         unsigned* __restrict__ list_node_begin, unsigned* __restrict__ list_num_nodes,
                                         unsigned* __restrict__ list_num_edges) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_nodes || !flag[i]) return;
  const unsigned k = before[i], c = sorted_label[i];
  list_node_begin[k] = i;
  list_num_nodes[k] = size[c];
  list_num_edges[k] = edge_count[c];
}

// One thread per oversize component: the reference's capped union-find (connected_components.h:87-108) over the
// component's edges in ascending edge index.  A node's local number is its position among the nodes sorted by
// (component, node id), so a component owns the slots [begin, begin + count) of work_parent / work_size (preset to
// the identity and to 1) and positions ascend with node ids.  The smaller position becomes the parent -- only the
// partition matters, not which root survives -- so a set's root is its smallest node id, its label.  Sequential
// inside a component, which is what the rule demands; parallel across them.
__global__ void tb_replay_kernel(const unsigned* __restrict__ list_node_begin, const unsigned* __restrict__ list_num_nodes,
                                 const unsigned* __restrict__ list_edge_begin, unsigned num_components,
                                 const unsigned* __restrict__ sorted_edge, const unsigned* __restrict__ endpoint_node,
                                 const unsigned* __restrict__ position, const unsigned* __restrict__ sorted_node,
                                 unsigned cap, unsigned* __restrict__ work_parent, unsigned* __restrict__ work_size,
                                 unsigned* __restrict__ final_label, unsigned long long* counters) {
  const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= num_components) return;
  const unsigned begin = list_node_begin[k], count = list_num_nodes[k], end = begin + count;
  auto find = [&](unsigned x) -> unsigned {
    for (unsigned step = 0; step < count; ++step) {
      const unsigned p = work_parent[x];
      if (p == x) return x;
      const unsigned g = work_parent[p];
      work_parent[x] = g;
      x = g;
    }
    return kTbNoLabel;
  };
  bool failed = false;
  for (unsigned j = list_edge_begin[k]; j < list_edge_begin[k + 1] && !failed; ++j) {
    const unsigned e = sorted_edge[j];
    const unsigned a = position[endpoint_node[2ull * e]], b = position[endpoint_node[2ull * e + 1]];
    if (a < begin || a >= end || b < begin || b >= end) {
      failed = true;
      break;
    }
    unsigned ra = find(a), rb = find(b);
    if (ra == kTbNoLabel || rb == kTbNoLabel) {
      failed = true;
      break;
    }
    if (ra == rb) continue;
    const unsigned merged = work_size[ra] + work_size[rb];
    if (merged > cap) continue;  // the refused merge
    if (ra > rb) {
      const unsigned t = ra;
      ra = rb;
      rb = t;
    }
    work_parent[rb] = ra;
    work_size[ra] = merged;
  }
  for (unsigned x = begin; x < end && !failed; ++x) {
    const unsigned r = find(x);
    if (r == kTbNoLabel)
      failed = true;
    else
      final_label[sorted_node[x]] = sorted_node[r];
  }
  if (failed) atomicAdd(&counters[kTbError], 1ull);
}

// ---- steps 4 to 6: small sets, consistency, the CSR ---------------------------------------------
__global__ void tb_view_keys_kernel(const unsigned* __restrict__ final_label, const unsigned* __restrict__ node_view,
                                    unsigned num_nodes, unsigned long long* __restrict__ key) {
  const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < num_nodes) key[n] = ((unsigned long long)final_label[n] << 32) | node_view[n];
}

// Nodes sorted by (label, view, node id): the first of every (label, view) is kept.
__global__ void tb_keep_kernel(const unsigned long long* __restrict__ sorted_key, const unsigned* __restrict__ sorted_node,
                               const unsigned* __restrict__ set_size, unsigned num_nodes, unsigned min_length,
                               unsigned* __restrict__ keep, unsigned long long* counters) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool dropped = false;
  if (i < num_nodes) {
    const bool first = i == 0 || sorted_key[i - 1] != sorted_key[i];
    keep[sorted_node[i]] = first;
    dropped = !first && set_size[(unsigned)(sorted_key[i] >> 32)] >= min_length;  // counted in emitted sets only
  }
  tb_count(dropped, &counters[kTbInconsistent]);
}

// Nodes sorted by (label, node id): the output order.
__global__ void tb_output_flags_kernel(const unsigned* __restrict__ sorted_label, const unsigned* __restrict__ sorted_node,
                                       const unsigned* __restrict__ set_size, const unsigned* __restrict__ keep,
                                       unsigned num_nodes, unsigned min_length, unsigned* __restrict__ obs_flag,
                                       unsigned* __restrict__ track_flag, unsigned long long* counters) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool head = false, emitted = false;
  if (i < num_nodes) {
    const unsigned label = sorted_label[i];
    head = i == 0 || sorted_label[i - 1] != label;
    emitted = set_size[label] >= min_length;
    obs_flag[i] = emitted && keep[sorted_node[i]];
    track_flag[i] = emitted && head;
  }
  tb_count(head, &counters[kTbSets]);
  tb_count(head && !emitted, &counters[kTbSmall]);
}

__global__ void tb_emit_kernel(const unsigned* __restrict__ sorted_node, const unsigned* __restrict__ obs_flag,
                               const unsigned* __restrict__ obs_before, const unsigned* __restrict__ track_flag,
                               const unsigned* __restrict__ track_before, const unsigned* __restrict__ node_view,
                               const unsigned* __restrict__ node_feature, unsigned num_nodes,
                               long long* __restrict__ track_begin, unsigned* __restrict__ obs_view,
                               unsigned* __restrict__ obs_feature) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > num_nodes) return;
  if (i == num_nodes) {  // the sums' last element: the totals
    track_begin[track_before[i]] = obs_before[i];
    return;
  }
  if (track_flag[i]) track_begin[track_before[i]] = obs_before[i];
  if (obs_flag[i]) {
    const unsigned node = sorted_node[i];
    obs_view[obs_before[i]] = node_view[node];
    obs_feature[obs_before[i]] = node_feature[node];
  }
}

__global__ void tb_endpoint_labels_kernel(const unsigned* __restrict__ endpoint_node, const unsigned* __restrict__ final_label,
                                          long long n, unsigned* __restrict__ endpoint_label) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) endpoint_label[i] = final_label[endpoint_node[i]];
}
}  // namespace tmi
