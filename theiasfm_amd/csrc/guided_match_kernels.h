// Batched GuidedEpipolarMatcher (reference matching/guided_epipolar_matcher.cc): the unmatched features of image 1 are
// grouped by where their epipolar lines cross the box of the unmatched features of image 2, a group's candidates are
// the features of image 2 in the grid cells along its mean line, and every feature of the group is matched exactly
// against those candidates.  The semantics are stated at tmi_ba_guided_epipolar_match (theia_mi355_ba.h, steps a to
// f); DESIGN 8.23 has the kernel table and the limits.
//
// Index spaces of a call with S selected pairs: ROW1 = the image-1 rows of the selected pairs laid end to end (pair s
// owns base1 .. base1 + n1 - 1), ROW2 the same for image 2, POSITION = the features that have a line, sorted by
// (pair, code, feature): pair s owns vbegin[s] .. vbegin[s + 1] - 1.  Group g of pair s is SLOT vbegin[s] + g (a pair
// has no more groups than positions).  ENTRY 4 row2 + grid of the cell lists, sorted by (pair, grid, cell key): the
// segment of (s, grid) starts at 4 ubegin[s] + grid u2[s], u2 the pair's unmatched image-2 features.
#pragma once

#include "match_kernels.h"
#include "ransac_core.h"

namespace tmi {

constexpr int kGmMaxImageRows = 131072;              // bits of the candidate bitmap of a group: 16 KiB of LDS
constexpr int kGmListCap = 4096;                     // indices of the compacted candidate list in LDS: 16 KiB
constexpr int kGmPassWords = 128;                    // bitmap words compacted at once: 128 * 32 bits <= kGmListCap
constexpr int kGmThreads = 256;
constexpr int kGmMaxCandidatesFill = 64;             // min_num_candidates is at most this: one draw per thread

struct GmPair {
  long long row1, row2;  // first device row of image 1 and of image 2 (descriptors and keypoints)
  int n1, n2;
  int base1, base2;      // the pair's first ROW1 and ROW2
  unsigned stream;       // q of step e
  int pad;
  double F[9];
};

struct GmPairState {  // written by gm_box_kernel
  double box[4];      // top_left.x, top_left.y, bottom_right.x, bottom_right.y
  int status;         // 0, or 1: nothing to match
  int pad;
};

struct GmNn {  // per POSITION
  float* best_d;
  int* best_i;
  float* second_d;
};

// The selected pair of an index in a table of S + 1 ascending begins: the last s < S with begin[s] <= i.
__device__ __forceinline__ int gm_pair_of(const int* __restrict__ begin, int S, int i) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ int gm_pair_of_row1(const GmPair* __restrict__ pairs, int S, int row) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pairs[mid].base1 <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ int gm_pair_of_row2(const GmPair* __restrict__ pairs, int S, int row) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pairs[mid].base2 <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Step a: the ROW1 / ROW2 of every input match are flagged.
__global__ __launch_bounds__(256) void gm_mark_kernel(const int* __restrict__ match_row1,
                                                      const int* __restrict__ match_row2, long long num_matches,
                                                      unsigned char* __restrict__ matched1,
                                                      unsigned char* __restrict__ matched2) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= num_matches) return;
  matched1[match_row1[m]] = 1;
  matched2[match_row2[m]] = 1;
}

// Step a, one workgroup per pair: the box of the unmatched image-2 keypoints, the two unmatched counts, the status.
// Minimum and maximum do not depend on the order of the reduction.
__global__ __launch_bounds__(256) void gm_box_kernel(const GmPair* __restrict__ pairs,
                                                     const double* __restrict__ keypoints,
                                                     const unsigned char* __restrict__ matched1,
                                                     const unsigned char* __restrict__ matched2,
                                                     GmPairState* __restrict__ state, unsigned* __restrict__ u2) {
  __shared__ double red[4][256];
  __shared__ int cnt[2][256];
  const GmPair P = pairs[blockIdx.x];
  const int tid = threadIdx.x;
  double lo_x = __builtin_inf(), lo_y = __builtin_inf(), hi_x = -__builtin_inf(), hi_y = -__builtin_inf();
  int c1 = 0, c2 = 0;
  for (int j = tid; j < P.n2; j += 256) {
    if (matched2[P.base2 + j]) continue;
    const double x = keypoints[2 * (P.row2 + j)], y = keypoints[2 * (P.row2 + j) + 1];
    lo_x = x < lo_x ? x : lo_x;
    hi_x = x > hi_x ? x : hi_x;
    lo_y = y < lo_y ? y : lo_y;
    hi_y = y > hi_y ? y : hi_y;
    ++c2;
  }
  for (int i = tid; i < P.n1; i += 256) c1 += matched1[P.base1 + i] ? 0 : 1;
  red[0][tid] = lo_x;
  red[1][tid] = lo_y;
  red[2][tid] = hi_x;
  red[3][tid] = hi_y;
  cnt[0][tid] = c1;
  cnt[1][tid] = c2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] = red[0][tid + w] < red[0][tid] ? red[0][tid + w] : red[0][tid];
      red[1][tid] = red[1][tid + w] < red[1][tid] ? red[1][tid + w] : red[1][tid];
      red[2][tid] = red[2][tid + w] > red[2][tid] ? red[2][tid + w] : red[2][tid];
      red[3][tid] = red[3][tid + w] > red[3][tid] ? red[3][tid + w] : red[3][tid];
      cnt[0][tid] += cnt[0][tid + w];
      cnt[1][tid] += cnt[1][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    GmPairState st;
    for (int k = 0; k < 4; ++k) st.box[k] = red[k][0];
    st.status = (cnt[0][0] == 0 || cnt[1][0] == 0) ? 1 : 0;
    st.pad = 0;
    state[blockIdx.x] = st;
    u2[blockIdx.x] = st.status ? 0u : (unsigned)cnt[1][0];
  }
}

// Step b, one thread per ROW1: the code of the feature's line, the pair as the second sort key (S: no line) and the
// pair's count of features with a line.
__global__ __launch_bounds__(256) void gm_lines_kernel(const GmPair* __restrict__ pairs, int S, int num_rows1,
                                                       const double* __restrict__ keypoints,
                                                       const unsigned char* __restrict__ matched1,
                                                       const GmPairState* __restrict__ state,
                                                       unsigned long long* __restrict__ code,
                                                       unsigned* __restrict__ pair_key, unsigned* __restrict__ iota,
                                                       unsigned* __restrict__ num_lines) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= num_rows1) return;
  const int s = gm_pair_of_row1(pairs, S, row);
  const GmPair& P = pairs[s];
  const GmPairState& st = state[s];
  iota[row] = (unsigned)row;
  unsigned long long c = 0;
  bool ok = !st.status && !matched1[row];
  if (ok) {
    const long long r = P.row1 + (row - P.base1);
    const double x = keypoints[2 * r], y = keypoints[2 * r + 1];
    double l0 = (P.F[0] * x + P.F[1] * y) + P.F[2];
    double l1 = (P.F[3] * x + P.F[4] * y) + P.F[5];
    double l2 = (P.F[6] * x + P.F[7] * y) + P.F[8];
    const double n = sqrt(l0 * l0 + l1 * l1);
    l0 = l0 / n;
    l1 = l1 / n;
    l2 = l2 / n;
    const double tlx = st.box[0], tly = st.box[1], brx = st.box[2], bry = st.box[3];
    double ex[4], ey[4];
    int ne = 0;
    const double y_left = -(l2 + l0 * tlx) / l1;
    if (y_left >= tly && y_left <= bry) {
      ex[ne] = tlx;
      ey[ne++] = y_left;
    }
    const double x_top = -(l2 + l1 * tly) / l0;
    if (x_top >= tlx && x_top <= brx) {
      ex[ne] = x_top;
      ey[ne++] = tly;
    }
    const double y_right = -(l2 + l0 * brx) / l1;
    if (y_right >= tly && y_right <= bry) {
      ex[ne] = brx;
      ey[ne++] = y_right;
    }
    const double x_bottom = -(l2 + l1 * bry) / l0;
    if (x_bottom >= tlx && x_bottom <= brx) {
      ex[ne] = x_bottom;
      ey[ne++] = bry;
    }
    ok = ne == 2;
    if (ok) {
      const double v[4] = {trunc(ex[0]), trunc(ey[0]), trunc(ex[1]), trunc(ey[1])};
      for (int k = 0; k < 4; ++k) {
        ok = ok && v[k] >= 0.0 && v[k] <= 65535.0;
        c = (c << 16) | (unsigned long long)(ok ? (unsigned)v[k] : 0u);
      }
    }
  }
  code[row] = ok ? c : ~0ull;
  pair_key[row] = ok ? (unsigned)s : (unsigned)S;
  if (ok) atomicAdd(&num_lines[s], 1u);
}

// out[i] = in[index[i]]: the second sort key in the order the first sort left.
__global__ __launch_bounds__(256) void gm_gather_kernel(const unsigned* __restrict__ in,
                                                        const unsigned* __restrict__ index, int n,
                                                        unsigned* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = in[index[i]];
}

// Step c, ONE LANE PER PAIR (the scan is sequential by definition): the group of every position, per group slot its
// first position, size and endpoints, the pair's number of groups.  pos_row: the ROW1 of a position.
__global__ __launch_bounds__(64) void gm_group_kernel(const GmPair* __restrict__ pairs, int S,
                                                      const int* __restrict__ vbegin,
                                                      const unsigned* __restrict__ pos_row,
                                                      const unsigned long long* __restrict__ code, double max_distance,
                                                      int* __restrict__ slot_first, int* __restrict__ slot_size,
                                                      double* __restrict__ slot_endpoints,
                                                      int* __restrict__ row_group, int* __restrict__ num_groups) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const int b = vbegin[s], e = vbegin[s + 1];
  const double sq_max = max_distance * max_distance;
  int g = -1, size = 0;
  double E0x = 0, E0y = 0, E1x = 0, E1y = 0;
  for (int i = b; i < e; ++i) {
    const unsigned row = pos_row[i];
    const unsigned long long c = code[row];
    const double x1 = (double)(unsigned)((c >> 48) & 0xffffu), y1 = (double)(unsigned)((c >> 32) & 0xffffu);
    const double x2 = (double)(unsigned)((c >> 16) & 0xffffu), y2 = (double)(unsigned)(c & 0xffffu);
    bool fresh = i == b;
    if (!fresh) {
      const double dx = E0x - x1, dy = E0y - y1;
      fresh = dx * dx + dy * dy > sq_max;
    }
    if (fresh) {
      if (g >= 0) {
        slot_size[b + g] = size;
        slot_endpoints[4 * (size_t)(b + g)] = E0x;
        slot_endpoints[4 * (size_t)(b + g) + 1] = E0y;
        slot_endpoints[4 * (size_t)(b + g) + 2] = E1x;
        slot_endpoints[4 * (size_t)(b + g) + 3] = E1y;
      }
      ++g;
      size = 0;
      slot_first[b + g] = i;
      E0x = x1;
      E0y = y1;
      E1x = x2;
      E1y = y2;
    }
    ++size;
    row_group[row] = g;
    const double w = 1.0 / (double)size;
    E0x = (1.0 - w) * E0x + w * x1;
    E0y = (1.0 - w) * E0y + w * y1;
    E1x = (1.0 - w) * E1x + w * x2;
    E1y = (1.0 - w) * E1y + w * y2;
  }
  if (g >= 0) {
    slot_size[b + g] = size;
    slot_endpoints[4 * (size_t)(b + g)] = E0x;
    slot_endpoints[4 * (size_t)(b + g) + 1] = E0y;
    slot_endpoints[4 * (size_t)(b + g) + 2] = E1x;
    slot_endpoints[4 * (size_t)(b + g) + 3] = E1y;
  }
  num_groups[s] = g + 1;
}

// Step d: the centre of (x, y) in grid `grid` as one 64-bit key.
__device__ __forceinline__ unsigned long long gm_cell_key(double x, double y, int grid, double c, int* cx_out,
                                                          int* cy_out) {
#pragma clang fp contract(off)
  const double ox = (grid & 1) ? c : 0.0, oy = (grid & 2) ? c : 0.0;
  const int cx = (int)(((floor((x - ox) / (2.0 * c)) * 2.0) * c + c) + ox);
  const int cy = (int)(((floor((y - oy) / (2.0 * c)) * 2.0) * c + c) + oy);
  *cx_out = cx;
  *cy_out = cy;
  return ((unsigned long long)(unsigned)cx << 32) | (unsigned long long)(unsigned)cy;
}

// Step d, one thread per ENTRY (ROW2, grid): the cell key, and (pair, grid) as the second sort key (4 S: matched).
__global__ __launch_bounds__(256) void gm_cells_kernel(const GmPair* __restrict__ pairs, int S, int num_rows2,
                                                       const double* __restrict__ keypoints,
                                                       const unsigned char* __restrict__ matched2,
                                                       const GmPairState* __restrict__ state, double c,
                                                       unsigned long long* __restrict__ cell_key,
                                                       unsigned* __restrict__ segment_key,
                                                       unsigned* __restrict__ iota) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 4 * num_rows2) return;
  const int row = e >> 2, grid = e & 3;
  const int s = gm_pair_of_row2(pairs, S, row);
  const GmPair& P = pairs[s];
  iota[e] = (unsigned)e;
  const bool ok = !state[s].status && !matched2[row];
  unsigned long long key = ~0ull;
  if (ok) {
    const long long r = P.row2 + (row - P.base2);
    int cx, cy;
    key = gm_cell_key(keypoints[2 * r], keypoints[2 * r + 1], grid, c, &cx, &cy);
  }
  cell_key[e] = key;
  segment_key[e] = ok ? (unsigned)(4 * s + grid) : (unsigned)(4 * S);
}

__device__ __forceinline__ float gm_distance(const float* __restrict__ a, const float* __restrict__ b, int dim) {
#pragma clang fp contract(off)
  float acc = 0.f;
  if ((dim & 3) == 0) {
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    for (int k = 0; k < (dim >> 2); ++k) {
      const float4 p = a4[k], q = b4[k];
      float t;
      t = p.x - q.x;
      acc = acc + t * t;
      t = p.y - q.y;
      acc = acc + t * t;
      t = p.z - q.z;
      acc = acc + t * t;
      t = p.w - q.w;
      acc = acc + t * t;
    }
  } else {
    for (int k = 0; k < dim; ++k) {
      const float t = a[k] - b[k];
      acc = acc + t * t;
    }
  }
  return acc;
}

// Exclusive sum of one int per thread over the workgroup's 256 threads (scratch: 256 ints); *total = the sum.
__device__ __forceinline__ int gm_block_scan(int v, int* scratch, int* total) {
  const int tid = threadIdx.x;
  scratch[tid] = v;
  __syncthreads();
  for (int off = 1; off < kGmThreads; off <<= 1) {
    const int add = tid >= off ? scratch[tid - off] : 0;
    __syncthreads();
    scratch[tid] += add;
    __syncthreads();
  }
  const int inclusive = scratch[tid];
  *total = scratch[kGmThreads - 1];
  __syncthreads();
  return inclusive - v;
}

// Steps e and f, ONE WORKGROUP PER GROUP SLOT (a slot past its pair's groups returns at once).  LDS: the candidate
// bitmap over the pair's image-2 rows (bitmap_words words, at most kGmMaxImageRows / 32), then kGmListCap ints that
// hold first the sample points of 256 steps of the walk and later the compacted candidate list.
//   walk     thread 0 advances the sample point (a chain of fp64 additions that has no closed form with the same
//            rounding), 256 steps at a time; then one thread per step picks the closest centre and sets the bits of
//            that cell, found by binary search in the sorted entries of (pair, grid): entry_sorted[e] is the ENTRY at
//            sorted place e, cell_key is indexed by ENTRY.
//   fill     below min_candidates, draw t is taken by thread t.
//   search   the bitmap is compacted 128 words at a time into the ascending list; when the next 128 words may not fit,
//            the list is searched and emptied (the best / second best of a query do not depend on how the candidates
//            are split, the order being total).  A wavefront per query: lanes stride the list, then the 64 (best,
//            index, second) triples are combined by a butterfly under (distance, then lower index), which is
//            commutative and associative, so every lane holds the same triple.  Lane 0 merges it into the query's
//            triple in global memory, which only this wavefront touches, and applies the ratio test after the last
//            search.
__global__ __launch_bounds__(kGmThreads) void gm_search_kernel(
    const GmPair* __restrict__ pairs, int S, const int* __restrict__ vbegin, const int* __restrict__ ubegin,
    const unsigned* __restrict__ u2, const int* __restrict__ num_groups, const int* __restrict__ slot_first,
    const int* __restrict__ slot_size, const double* __restrict__ slot_endpoints, const unsigned* __restrict__ pos_row,
    const unsigned* __restrict__ entry_sorted, const unsigned long long* __restrict__ cell_key,
    const float* __restrict__ desc, int dim, double c,
    double ratio_sq, int min_candidates, unsigned long long seed, int bitmap_words, GmNn nn,
    unsigned* __restrict__ pass, int* __restrict__ slot_num_candidates, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  extern __shared__ double2 gm_lds2[];
  __shared__ int scratch[kGmThreads];
  const int slot = blockIdx.x;
  if (slot >= vbegin[S]) return;
  const int s = gm_pair_of(vbegin, S, slot);
  const int g = slot - vbegin[s];
  if (g >= num_groups[s]) return;
  const GmPair& P = pairs[s];
  const int tid = threadIdx.x;
  unsigned* bitmap = reinterpret_cast<unsigned*>(gm_lds2);
  int* list = reinterpret_cast<int*>(bitmap + bitmap_words);
  double2* points = reinterpret_cast<double2*>(list);  // (bitmap_words is a multiple of 4: 16-byte aligned)
  const int words = (P.n2 + 31) >> 5;                   // <= bitmap_words: the host sized it for the largest image
  for (int w = tid; w < words; w += kGmThreads) bitmap[w] = 0u;

  // ---- step e: the walk
  const double E0x = slot_endpoints[4 * (size_t)slot], E0y = slot_endpoints[4 * (size_t)slot + 1];
  const double E1x = slot_endpoints[4 * (size_t)slot + 2], E1y = slot_endpoints[4 * (size_t)slot + 3];
  const double dx = E1x - E0x, dy = E1y - E0y;
  const int num_steps = (int)(sqrt(dx * dx + dy * dy) / c);
  const double delta_x = (E0x - E1x) / (double)num_steps, delta_y = (E0y - E1y) / (double)num_steps;
  const int useg = (int)u2[s];
  const int seg0 = 4 * ubegin[s];
  double sx = E1x, sy = E1y;  // thread 0's
  for (int base = 0; base < num_steps; base += kGmThreads) {
    const int n = num_steps - base < kGmThreads ? num_steps - base : kGmThreads;
    __syncthreads();  // the previous points have been read (the first time: the bitmap is cleared)
    if (tid == 0)
      for (int j = 0; j < n; ++j) {
        sx = sx + delta_x;
        sy = sy + delta_y;
        points[j] = make_double2(sx, sy);
      }
    __syncthreads();
    if (tid < n) {
      const double2 p = points[tid];
      double min_dist = 1.7976931348623157e308;
      int min_grid = -1;
      unsigned long long min_key = 0;
      for (int grid = 0; grid < 4; ++grid) {
        int cx, cy;
        const unsigned long long key = gm_cell_key(p.x, p.y, grid, c, &cx, &cy);
        const double ux = (double)cx - p.x, uy = (double)cy - p.y;
        const double dist = ux * ux + uy * uy;
        if (dist < min_dist) {
          min_grid = grid;
          min_dist = dist;
          min_key = key;
        }
      }
      if (min_grid >= 0) {
        const int lo0 = seg0 + min_grid * useg;
        int lo = lo0, hi = lo0 + useg;  // the first entry of the segment whose key is >= min_key
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (cell_key[entry_sorted[mid]] < min_key) lo = mid + 1; else hi = mid;
        }
        for (int e = lo; e < lo0 + useg && cell_key[entry_sorted[e]] == min_key; ++e) {
          const int j = (int)(entry_sorted[e] >> 2) - P.base2;  // the entry's ROW2, local to the image
          if (j >= 0 && j < P.n2) atomicOr(&bitmap[j >> 5], 1u << (j & 31));
        }
      }
    }
  }
  __syncthreads();

  // ---- step e: the fill
  int have = 0, total = 0;
  for (int w = tid; w < words; w += kGmThreads) have += __popc(bitmap[w]);
  gm_block_scan(have, scratch, &total);
  if (total < min_candidates) {
    const int t = total + tid;
    if (t < min_candidates) {
      const unsigned long long word = 64ull * (((unsigned long long)P.stream << 32) + (unsigned long long)g) + (unsigned long long)t;
      const double u = ((double)(splitmix64_word(seed, word) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
      int j = (int)(u * (double)P.n2);
      j = j < P.n2 - 1 ? j : P.n2 - 1;
      atomicOr(&bitmap[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
    have = 0;
    for (int w = tid; w < words; w += kGmThreads) have += __popc(bitmap[w]);
    gm_block_scan(have, scratch, &total);
  }
  const int num_candidates = total;
  const int first = slot_first[slot], size = slot_size[slot];
  if (tid == 0) {
    slot_num_candidates[slot] = num_candidates;
    atomicAdd(&counters[0], 1ull);
    atomicAdd(&counters[1], (unsigned long long)num_candidates);
    atomicAdd(&counters[2], (unsigned long long)num_candidates * (unsigned long long)size);
  }

  // ---- step f
  const int wave = tid >> 6, lane = tid & 63;
  bool searched = false;
  int listn = 0;
  auto search = [&]() {
    __syncthreads();  // the list is written
    for (int qi = wave; qi < size; qi += kGmThreads / 64) {
      const int pos = first + qi;
      const float* a = desc + (size_t)(P.row1 + ((int)pos_row[pos] - P.base1)) * dim;
      float b = __builtin_inff(), sd = __builtin_inff();
      int bi = kMatchNoColumn;
      for (int k = lane; k < listn; k += 64) {
        const int j = list[k];
        match_insert(gm_distance(a, desc + (size_t)(P.row2 + j) * dim, dim), j, b, bi, sd);
      }
      for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(b, off), os = __shfl_xor(sd, off);
        const int oi = __shfl_xor(bi, off);
        match_insert(ob, oi, b, bi, sd);
        if (os < sd) sd = os;
      }
      if (lane == 0) {
        if (searched) {
          float gb = nn.best_d[pos], gs = nn.second_d[pos];
          int gi = nn.best_i[pos];
          match_insert(b, bi, gb, gi, gs);
          if (sd < gs) gs = sd;
          b = gb;
          bi = gi;
          sd = gs;
        }
        nn.best_d[pos] = b;
        nn.best_i[pos] = bi;
        nn.second_d[pos] = sd;
      }
    }
    searched = true;
    listn = 0;
    __syncthreads();  // the list is free
  };
  for (int w0 = 0; w0 < words; w0 += kGmPassWords) {
    const int w = w0 + tid;
    const unsigned bits = (tid < kGmPassWords && w < words) ? bitmap[w] : 0u;
    int pass_total;
    const int before = gm_block_scan(__popc(bits), scratch, &pass_total);
    if (listn + pass_total > kGmListCap) search();
    int o = listn + before;
    for (unsigned rest = bits; rest; rest &= rest - 1) list[o++] = (w << 5) + (__ffs(rest) - 1);
    listn += pass_total;
  }
  if (listn > 0) search();
  for (int qi = wave; qi < size; qi += kGmThreads / 64) {
    if (lane != 0) continue;
    const int pos = first + qi;
    bool ok = searched && num_candidates >= 2;
    if (ok) {
      const int bi = nn.best_i[pos];
      ok = bi >= 0 && bi < P.n2 && (double)nn.best_d[pos] < (double)nn.second_d[pos] * ratio_sq;
    }
    pass[pos] = ok ? 1u : 0u;
  }
}

struct GmRecord {  // one added match: the read-back's unit
  int feature1, feature2;
  float distance;
};

// The added matches, compacted in position order.  scan: the exclusive sum of pass.
__global__ __launch_bounds__(256) void gm_compact_kernel(const GmPair* __restrict__ pairs, int S,
                                                         const int* __restrict__ vbegin,
                                                         const unsigned* __restrict__ pos_row, GmNn nn,
                                                         const unsigned* __restrict__ pass,
                                                         const unsigned* __restrict__ scan,
                                                         GmRecord* __restrict__ out) {
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= vbegin[S] || !pass[pos]) return;
  const int s = gm_pair_of(vbegin, S, pos);
  GmRecord m;
  m.feature1 = (int)pos_row[pos] - pairs[s].base1;
  m.feature2 = nn.best_i[pos];
  m.distance = nn.best_d[pos];
  out[scan[pos]] = m;
}

// counts[4 s .. 4 s + 3] = status, groups, first added match, 0 of selected pair s; counts[4 S] = the total.
__global__ __launch_bounds__(256) void gm_pair_kernel(const GmPairState* __restrict__ state,
                                                      const int* __restrict__ vbegin,
                                                      const int* __restrict__ num_groups,
                                                      const unsigned* __restrict__ scan, int S,
                                                      int* __restrict__ counts) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s > S) return;
  if (s == S) {
    counts[4 * s] = (int)scan[vbegin[S]];
    return;
  }
  counts[4 * s] = state[s].status;
  counts[4 * s + 1] = num_groups[s];
  counts[4 * s + 2] = (int)scan[vbegin[s]];
  counts[4 * s + 3] = 0;
}

}  // namespace tmi
