// The two view-graph steps between the edge filters and the global solvers (tmi_ba_largest_connected_component and
// tmi_ba_orientations_from_maximum_spanning_tree; the steps are numbered in include/theia_mi355_ba.h):
//
//   theia::RemoveDisconnectedViewPairs          (view_graph/remove_disconnected_view_pairs.cc:48-95)
//   theia::OrientationsFromMaximumSpanningTree  (view_graph/orientations_from_maximum_spanning_tree.cc:109-180)
//
// on a dense view table and an edge list.  Every graph result is an integer and every count, minimum and maximum goes
// through an integer atomic, so no result depends on the order in which threads arrive.
//
// components      vg_union_kernel: the concurrent union-find of track_build_kernels.h (tb_find; the smaller index
//                 becomes the parent, so a component's root is its smallest view) over the alive edges; then
//                 tb_flatten_kernel and tb_sizes_kernel as they are.  vg_component_stats_kernel reduces the roots with
//                 at least one edge on the key (size << 32 | ~label) by a 64-bit atomic max: most views, then the
//                 smallest label.  vg_keep_kernel / vg_view_flags_kernel read that key in a later launch.
// ranks           the kept edges in the order of the reference's std::sort (minimum_spanning_tree.h:83): ascending
//                 (-num_verified_matches, min(view1, view2), max(view1, view2)), by two stable radix sorts (the pair
//                 key, then the weight key); a repeated pair keeps its edge index order.  Edges outside the largest
//                 component sort behind all others.  rank -> edge is edge_of_rank.
// spanning tree   Boruvka rounds on the ranks.  vg_min_edge_kernel: every component takes its lowest-rank outgoing
//                 edge by atomicMin.  vg_hook_kernel: every root with an edge marks it as a tree edge and hooks onto
//                 the component at the other end; a mutual choice keeps the smaller label as the root.  Ranks are
//                 unique, so the hooks have no other cycle, and tb_flatten_kernel (a launch of its own: hook[] is
//                 final and read plainly) follows them to the new roots.  A chosen edge is the lightest edge leaving
//                 its component, so it belongs to THE minimum spanning tree of the total order: Kruskal's tree.  The
//                 host runs ceil(log2 V) + 1 rounds, a fixed number: the components with an outgoing edge at least
//                 halve per round.
// rooting         vg_tree_degree_kernel / vg_tree_fill_kernel: the tree's CSR (row order as the atomics fall: every
//                 view has one parent whatever the order).  vg_root_kernel: ONE workgroup walks the levels from the
//                 root with __syncthreads() between them: parent, parent pair, depth and ComputeOrientation (:62-84)
//                 when a view is reached.  The level loop is bounded by num_views and the frontier by num_views slots,
//                 so a wrong tree ends the walk (and the host compares the views reached with the component's size).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rotation_kernels.h"
#include "track_build_kernels.h"

namespace tmi {
// counters of one call; kVgError is kTbError: tb_flatten_kernel reports there
enum {
  kVgBest = 0,     // (size << 32) | (0xffffffff - label) of the largest component; 0: no alive edge
  kVgComponents,   // components with at least one edge
  kVgEdgeViews,    // views with at least one alive edge
  kVgKept,         // alive edges inside the largest component
  kVgAlive,        // alive edges
  kVgError = kTbError,
  kVgTreePairs,
  kVgReached,      // views the walk reached
  kVgDepth,        // the deepest level
  kVgRoot,
  kVgBadRoot,      // the root is outside the largest component
  kVgCounters = 12
};
constexpr unsigned kVgNone = 0xffffffffu;
constexpr int kVgRootThreads = 256;

__device__ __forceinline__ unsigned vg_largest_label(const unsigned long long* counters) {
  const unsigned long long best = counters[kVgBest];
  return best ? 0xffffffffu - (unsigned)best : kVgNone;
}

// ---- components ---------------------------------------------------------------------------------
// tb_union_kernel on (pair_view1, pair_view2) under the mask.
__global__ void vg_union_kernel(const int* __restrict__ view1, const int* __restrict__ view2,
                                const unsigned char* __restrict__ mask, int num_pairs, unsigned num_views,
                                unsigned* parent, unsigned long long* counters) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= num_pairs || (mask && !mask[e])) return;
  unsigned a = (unsigned)view1[e], b = (unsigned)view2[e];
  // a failed link means another thread linked this root first: at most num_views - 1 links are ever made
  for (unsigned attempt = 0; attempt <= num_views; ++attempt) {
    a = tb_find(parent, a, num_views);
    b = tb_find(parent, b, num_views);
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
  atomicAdd(&counters[kVgError], 1ull);
}

// A component with an edge has at least two views (no view pairs itself).
__global__ void vg_component_stats_kernel(const unsigned* __restrict__ label, const unsigned* __restrict__ size,
                                          unsigned num_views, unsigned long long* counters) {
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool root = v < num_views && label[v] == v && size[v] >= 2;
  tb_count(root, &counters[kVgComponents]);
  if (root) {
    atomicAdd(&counters[kVgEdgeViews], (unsigned long long)size[v]);
    atomicMax(&counters[kVgBest], ((unsigned long long)size[v] << 32) | (unsigned long long)(0xffffffffu - v));
  }
}

__global__ void vg_keep_kernel(const int* __restrict__ view1, const unsigned char* __restrict__ mask,
                               const unsigned* __restrict__ label, int num_pairs, unsigned char* __restrict__ keep,
                               unsigned long long* counters) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned largest = vg_largest_label(counters);
  bool alive = false, kept = false;
  if (e < num_pairs) {
    alive = !mask || mask[e];
    kept = alive && label[view1[e]] == largest;
    keep[e] = (unsigned char)kept;
  }
  tb_count(alive, &counters[kVgAlive]);
  tb_count(kept, &counters[kVgKept]);
}

__global__ void vg_view_flags_kernel(const unsigned* __restrict__ label, unsigned num_views,
                                     const unsigned long long* __restrict__ counters,
                                     unsigned char* __restrict__ in_largest) {
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < num_views) in_largest[v] = (unsigned char)(label[v] == vg_largest_label(counters));
}

// ---- ranks --------------------------------------------------------------------------------------
__global__ void vg_pair_keys_kernel(const int* __restrict__ view1, const int* __restrict__ view2, int num_pairs,
                                    unsigned long long* __restrict__ key, unsigned* __restrict__ index) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= num_pairs) return;
  const unsigned a = (unsigned)view1[e], b = (unsigned)view2[e];
  key[e] = ((unsigned long long)min(a, b) << 32) | max(a, b);
  index[e] = (unsigned)e;
}

// The weight key of the edge at every position of the pair order: ascending key = descending weight.
__global__ void vg_weight_keys_kernel(const unsigned* __restrict__ index, const int* __restrict__ weight,
                                      const unsigned char* __restrict__ keep, int num_pairs,
                                      unsigned* __restrict__ key) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_pairs) return;
  const unsigned e = index[i];
  key[i] = keep[e] ? 0x7fffffffu - (unsigned)weight[e] : kVgNone;
}

// ---- spanning tree ------------------------------------------------------------------------------
// best[c] = the lowest rank of an edge that leaves component c (best[] was set to kVgNone).
__global__ void vg_min_edge_kernel(const unsigned* __restrict__ edge_of_rank, const unsigned char* __restrict__ keep,
                                   const int* __restrict__ view1, const int* __restrict__ view2,
                                   const unsigned* __restrict__ comp, int num_pairs, unsigned* best) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_pairs) return;
  const unsigned e = edge_of_rank[r];
  if (!keep[e]) return;
  const unsigned ca = comp[view1[e]], cb = comp[view2[e]];
  if (ca == cb) return;
  atomicMin(&best[ca], (unsigned)r);
  atomicMin(&best[cb], (unsigned)r);
}

// hook[v]: the component v goes under (v itself: v stays, or becomes, a root).  comp[] and best[] are read only.
__global__ void vg_hook_kernel(const unsigned* __restrict__ edge_of_rank, const int* __restrict__ view1,
                               const int* __restrict__ view2, const unsigned* __restrict__ comp,
                               const unsigned* __restrict__ best, unsigned num_views, unsigned* __restrict__ hook,
                               unsigned char* __restrict__ in_tree) {
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_views) return;
  const unsigned c = comp[v];
  unsigned h = c;
  if (c == v && best[v] != kVgNone) {
    const unsigned e = edge_of_rank[best[v]];
    const unsigned ca = comp[view1[e]], cb = comp[view2[e]];
    const unsigned other = ca == v ? cb : ca;
    in_tree[e] = 1;  // (both ends of a mutual choice store the same value)
    h = (best[other] == best[v] && v < other) ? v : other;
  }
  hook[v] = h;
}

// ---- rooting and orientations -------------------------------------------------------------------
// degree[v] += 1 per tree edge at v (degree [V + 1] was cleared; its exclusive sum is the CSR's row_ptr).
__global__ void vg_tree_degree_kernel(const unsigned char* __restrict__ in_tree, const int* __restrict__ view1,
                                      const int* __restrict__ view2, int num_pairs, unsigned* degree,
                                      unsigned long long* counters) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const bool tree = e < num_pairs && in_tree[e];
  if (tree) {
    atomicAdd(&degree[view1[e]], 1u);
    atomicAdd(&degree[view2[e]], 1u);
  }
  tb_count(tree, &counters[kVgTreePairs]);
}

// row: (neighbour, edge << 1 | (this view is the edge's view2)); cursor starts as a copy of row_ptr.
__global__ void vg_tree_fill_kernel(const unsigned char* __restrict__ in_tree, const int* __restrict__ view1,
                                    const int* __restrict__ view2, int num_pairs, unsigned* cursor,
                                    int2* __restrict__ row) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= num_pairs || !in_tree[e]) return;
  const int a = view1[e], b = view2[e];
  row[atomicAdd(&cursor[a], 1u)] = make_int2(b, e << 1);
  row[atomicAdd(&cursor[b], 1u)] = make_int2(a, (e << 1) | 1);
}

// ComputeOrientation (orientations_from_maximum_spanning_tree.cc:62-84): R_rel R_parent when the parent is the edge's
// view1, R_rel^T R_parent when it is view2; the sums of a product left to right as Eigen's 3x3 product writes them.
__device__ __forceinline__ void vg_compute_orientation(const double parent[3], const double relative[3],
                                                       bool parent_is_view2, double out[3]) {
#pragma clang fp contract(off)
  double Rp[9], Rr[9], N[9];
  // one copy of the conversion's code run twice: two inlined copies of its sincos need more scalar registers (12
  // spilled into VGPR lanes against 7)
#pragma nounroll
  for (int k = 0; k < 2; ++k) {
    const double in[3] = {k ? relative[0] : parent[0], k ? relative[1] : parent[1], k ? relative[2] : parent[2]};
    double M[9];
    angle_axis_to_rotation_matrix(in, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (k) Rr[i] = M[i];
      else Rp[i] = M[i];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double a0 = parent_is_view2 ? Rr[3 * r] : Rr[r];
      const double a1 = parent_is_view2 ? Rr[3 * r + 1] : Rr[r + 3];
      const double a2 = parent_is_view2 ? Rr[3 * r + 2] : Rr[r + 6];
      N[r + 3 * c] = (a0 * Rp[3 * c] + a1 * Rp[3 * c + 1]) + a2 * Rp[3 * c + 2];
    }
  rot::rotation_matrix_to_angle_axis(N, out);
}

// ONE workgroup.  tree [5 V]: parent, parent_pair and depth (each [V], set to -1) and the two frontiers, one
// allocation behind one pointer; orientation was set to 0.
// root_view < 0: the largest component's label.  Nothing is written without an alive edge or for a root outside the
// largest component (counters[kVgBadRoot]).
__global__ __launch_bounds__(kVgRootThreads) void vg_root_kernel(
    int num_views, int root_view, const unsigned* __restrict__ label, const unsigned* __restrict__ row_ptr,
    const int2* __restrict__ row, const double* __restrict__ relative, double* orientation, int* tree,
    unsigned long long* counters) {
  __shared__ int s_count[2];
  int* parent = tree;
  int* parent_pair = tree + (size_t)num_views;
  int* depth = tree + 2 * (size_t)num_views;
  int* frontier = tree + 3 * (size_t)num_views;
  const int tid = threadIdx.x;
  const unsigned largest = vg_largest_label(counters);
  if (largest == kVgNone) return;  // (uniform)
  const int root = root_view < 0 ? (int)largest : root_view;
  if (root >= num_views || label[root] != largest) {
    if (tid == 0) counters[kVgBadRoot] = 1;
    return;
  }
  if (tid == 0) {
    depth[root] = 0;
    frontier[0] = root;
    s_count[0] = 1;
    s_count[1] = 0;
  }
  __syncthreads();
  int reached = 1, deepest = 0;
  for (int level = 0; level < num_views; ++level) {
    const int* cur = frontier + (size_t)(level & 1) * num_views;
    int* next = frontier + (size_t)((level + 1) & 1) * num_views;
    const int n = min(s_count[level & 1], num_views);
    if (n == 0) break;  // (uniform: s_count is read between two barriers)
    for (int i = tid; i < n; i += kVgRootThreads) {
      const int u = cur[i];
      const double ou[3] = {orientation[3 * (size_t)u], orientation[3 * (size_t)u + 1], orientation[3 * (size_t)u + 2]};
      const unsigned r1 = row_ptr[u + 1];
      for (unsigned r = row_ptr[u]; r < r1; ++r) {
        const int2 ent = row[r];
        const int w = ent.x, e = ent.y >> 1;
        if (depth[w] >= 0) continue;  // the parent (in a tree every other neighbour is a child)
        const int slot = atomicAdd(&s_count[(level + 1) & 1], 1);
        if (slot >= num_views) continue;  // (not a tree: the walk stays inside its arrays and ends)
        next[slot] = w;
        depth[w] = level + 1;
        parent[w] = u;
        parent_pair[w] = e;
        const double rel[3] = {relative[3 * (size_t)e], relative[3 * (size_t)e + 1], relative[3 * (size_t)e + 2]};
        double ow[3];
        vg_compute_orientation(ou, rel, (bool)(ent.y & 1), ow);
        orientation[3 * (size_t)w] = ow[0];
        orientation[3 * (size_t)w + 1] = ow[1];
        orientation[3 * (size_t)w + 2] = ow[2];
      }
    }
    __syncthreads();
    const int made = min(s_count[(level + 1) & 1], num_views);
    if (made) {
      reached += made;
      deepest = level + 1;
    }
    if (tid == 0) s_count[level & 1] = 0;  // the buffer after next
    __syncthreads();
  }
  if (tid == 0) {
    counters[kVgReached] = (unsigned long long)reached;
    counters[kVgDepth] = (unsigned long long)deepest;
    counters[kVgRoot] = (unsigned long long)root;
  }
}
}  // namespace tmi
