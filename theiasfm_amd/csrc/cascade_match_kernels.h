// Batched CascadeHashingFeatureMatcher (reference cascade_hasher.cc:55-277, cascade_hashing_feature_matcher.cc:130-166):
// every image is hashed once per call (mean, 128-bit code, six 10-bit bucket ids, the buckets as a CSR), then every
// (pair, direction, row) shortlists the columns that share a bucket with it, keeps the eleven with the smallest
// (Hamming distance, first shared group, column) and spends exact distances on those.  The semantics are stated at
// tmi_ba_match_features_cascade (theia_mi355_ba.h); DESIGN 8.12 has the kernels and what the equality with the numpy
// model rests on.  The per-row result is match_kernels.h's neighbour triple, and its finish kernels serve both calls.
#pragma once

#include <hipcub/hipcub.hpp>

#include "match_kernels.h"

namespace tmi {

constexpr int kCascadeCodeBits = 128;    // kHashCodeSize (cascade_hasher.h:52-58)
constexpr int kCascadeGroups = 6;        // kNumBucketGroups
constexpr int kCascadeGroupBits = 10;    // kNumBucketBits
constexpr int kCascadeBuckets = 1 << kCascadeGroupBits;
constexpr int kCascadeProjRows = kCascadeCodeBits + kCascadeGroups * kCascadeGroupBits;  // 188
constexpr int kCascadeTop = 11;          // kNumTopCandidates + 1: the walk stops once it holds more than ten
constexpr int kCascadeMinTotal = 10;     // a row with this many candidate incidences or fewer has no match
constexpr int kCascadeHashRows = 64;     // descriptor rows of a hash block
constexpr int kCascadeHashK = 32;        // descriptor elements staged at once
constexpr int kCascadeHashPass = 16;     // projection rows staged at once: four per wave
constexpr int kCascadeCounterShards = 64;  // the three call counters, sharded by workgroup
constexpr unsigned long long kCascadeNoKey = ~0ull;

struct CascadeRecord {  // one hashed descriptor: one candidate is one 32-byte gather
  unsigned code[4];      // bit j of the code is bit j % 32 of word j / 32
  unsigned short ids[kCascadeGroups];
  unsigned short pad[2];
};
static_assert(sizeof(CascadeRecord) == 32, "a candidate is one 32-byte record");

// mean[m][k] of image m: a thread per (image, dimension) walks the rows in order; consecutive threads read consecutive
// floats of a row.  An image without rows gets zeros, which nothing reads.
__global__ __launch_bounds__(256) void cascade_mean_kernel(const float* __restrict__ desc, int dim,
                                                           const long long* __restrict__ image_begin, int num_images,
                                                           float* __restrict__ mean) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)num_images * dim) return;
  const int m = (int)(t / dim), k = (int)(t - (long long)m * dim);
  const long long b = image_begin[m], e = image_begin[m + 1];
  float s = 0.f;
  const float* p = desc + (size_t)b * dim + k;
  for (long long i = b; i < e; ++i, p += dim) s = s + *p;
  mean[t] = e > b ? s / (float)(e - b) : 0.f;
}

// One workgroup per (image, block of 64 rows): blocks[b] = (image, row block).  Lane l of every wave owns row l of the
// block; wave w owns four of the sixteen projection rows of a pass, so a projection element is one LDS broadcast.  The
// centred descriptors are staged 32 elements at a time (leading dimension 33: the lanes of a wave fall on different
// banks) beside the pass's projection rows.  Padding is exact: 0 * 0 added to a sum leaves its sign test alone.  For
// every accumulator k runs ascending over the whole dimension.
__global__ __launch_bounds__(256) void cascade_hash_kernel(const float* __restrict__ desc, int dim,
                                                           const float* __restrict__ proj,
                                                           const float* __restrict__ mean,
                                                           const long long* __restrict__ image_begin,
                                                           const int2* __restrict__ blocks,
                                                           CascadeRecord* __restrict__ rec) {
#pragma clang fp contract(off)
  constexpr int kLd = kCascadeHashK + 1;
  constexpr int kBitLd = 192;
  __shared__ float tL[kCascadeHashRows * kLd];
  __shared__ float pL[kCascadeHashPass * kCascadeHashK];
  __shared__ unsigned char bitL[kCascadeHashRows * kBitLd];
  const int2 blk = blocks[blockIdx.x];
  const long long b = image_begin[blk.x];
  const int n = (int)(image_begin[blk.x + 1] - b);
  const int row0 = blk.y * kCascadeHashRows;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* x = desc + (size_t)b * dim;
  const float* mu = mean + (size_t)blk.x * dim;
  constexpr int kPasses = (kCascadeProjRows + kCascadeHashPass - 1) / kCascadeHashPass;
  for (int pass = 0; pass < kPasses; ++pass) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < dim; k0 += kCascadeHashK) {
      __syncthreads();  // the previous chunk has been read
      for (int e = tid; e < kCascadeHashRows * kCascadeHashK; e += 256) {
        const int r = e / kCascadeHashK, k = e - r * kCascadeHashK;
        const int gr = row0 + r, gk = k0 + k;
        tL[r * kLd + k] = (gr < n && gk < dim) ? x[(size_t)gr * dim + gk] - mu[gk] : 0.f;
      }
      for (int e = tid; e < kCascadeHashPass * kCascadeHashK; e += 256) {
        const int r = e / kCascadeHashK, k = e - r * kCascadeHashK;
        const int pr = pass * kCascadeHashPass + r, gk = k0 + k;
        pL[e] = (pr < kCascadeProjRows && gk < dim) ? proj[(size_t)pr * dim + gk] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < kCascadeHashK; ++k) {
        const float tv = tL[lane * kLd + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + pL[(w * 4 + j) * kCascadeHashK + k] * tv;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pr = pass * kCascadeHashPass + w * 4 + j;
      if (pr < kCascadeProjRows) bitL[lane * kBitLd + pr] = acc[j] > 0.f;
    }
  }
  __syncthreads();
  if (tid < kCascadeHashRows && row0 + tid < n) {
    const unsigned char* bits = bitL + tid * kBitLd;
    CascadeRecord r;
    for (int word = 0; word < 4; ++word) {
      unsigned v = 0;
      for (int j = 0; j < 32; ++j) v |= (unsigned)bits[word * 32 + j] << j;
      r.code[word] = v;
    }
    for (int g = 0; g < kCascadeGroups; ++g) {
      unsigned v = 0;
      for (int k = 0; k < kCascadeGroupBits; ++k)
        v |= (unsigned)bits[kCascadeCodeBits + g * kCascadeGroupBits + k] << (kCascadeGroupBits - 1 - k);
      r.ids[g] = (unsigned short)v;
    }
    r.pad[0] = r.pad[1] = 0;
    rec[b + row0 + tid] = r;
  }
}

// One workgroup per (image, group): the histogram of the 1024 bucket ids, its exclusive scan (bucket_begin, 1025 entries
// per (image, group), relative to the group's part of bucket_rows) and the scatter of the row indices.  The order inside
// a bucket is whatever the atomics give: the shortlist is selected by key and does not see it.
__global__ __launch_bounds__(256) void cascade_bucket_kernel(const CascadeRecord* __restrict__ rec,
                                                             const long long* __restrict__ image_begin,
                                                             int* __restrict__ bucket_begin,
                                                             int* __restrict__ bucket_rows) {
  using Scan = hipcub::BlockScan<int, 256>;
  __shared__ int hist[kCascadeBuckets];
  __shared__ typename Scan::TempStorage scan_tmp;
  const int m = blockIdx.x / kCascadeGroups, g = blockIdx.x - m * kCascadeGroups;
  const long long b = image_begin[m];
  const int n = (int)(image_begin[m + 1] - b);
  const int tid = threadIdx.x;
  for (int t = tid; t < kCascadeBuckets; t += 256) hist[t] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) atomicAdd(&hist[rec[b + i].ids[g]], 1);
  __syncthreads();
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = hist[tid * 4 + j];
  Scan(scan_tmp).ExclusiveSum(v, v);
  __syncthreads();  // every count has been read
  int* bb = bucket_begin + (size_t)blockIdx.x * (kCascadeBuckets + 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hist[tid * 4 + j] = v[j];  // from here on the bucket's cursor
    bb[tid * 4 + j] = v[j];
  }
  if (tid == 0) bb[kCascadeBuckets] = n;
  __syncthreads();
  int* out = bucket_rows + (size_t)kCascadeGroups * (size_t)b + (size_t)g * (size_t)n;
  for (int i = tid; i < n; i += 256) out[atomicAdd(&hist[rec[b + i].ids[g]], 1)] = i;
}

// Ascending bitonic sort of one key per lane across the wavefront: 21 fixed xor-shuffle steps.
__device__ __forceinline__ unsigned long long cascade_wave_sort(unsigned long long key, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const unsigned long long other = __shfl_xor(key, j);
      const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
      const unsigned long long lo = key < other ? key : other, hi = key < other ? other : key;
      key = keep_min ? lo : hi;
    }
  }
  return key;
}

// A wavefront per row of the chunk (a workgroup: four rows).  Lanes 0..10 hold the running eleven smallest keys
// (Hamming << 40 | first shared group << 32 | column); lanes 11..63 take 53 entries of the six buckets' concatenated CSR
// ranges at a time, and one sort of the 64 keys leaves the new eleven in lanes 0..10.  A column met in group g whose
// record shares an earlier group with the row has been met there and is dropped: no flag array.  Then lane j < 11
// computes the exact distance of shortlisted column j, k ascending, and the best and second best are taken in the order
// of match_insert.  counters: [shard][0] candidate incidences of the rows not skipped, [1] exact distances, [2] rows
// skipped.
__global__ __launch_bounds__(256) void cascade_candidates_kernel(
    const float* __restrict__ desc, int dim, const MatchTask* __restrict__ tasks, const int* __restrict__ task_col_image,
    int num_tasks, int num_rows, const CascadeRecord* __restrict__ rec, const int* __restrict__ bucket_begin,
    const int* __restrict__ bucket_rows, MatchNn out, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= num_rows) return;  // (the whole wave)
  const int ti = match_task_of_row(tasks, num_tasks, row);
  const MatchTask T = tasks[ti];
  const int i = row - T.out_base;
  float bd = __builtin_inff(), sd = __builtin_inff();
  int bi = kMatchNoColumn;
  if (T.n_cols > 0) {
    const uint4* rec4 = reinterpret_cast<const uint4*>(rec);
    const uint4 qc = rec4[2 * (size_t)(T.row_off + i)], qi = rec4[2 * (size_t)(T.row_off + i) + 1];
    const unsigned long long q0 = (unsigned long long)qc.x | (unsigned long long)qc.y << 32;
    const unsigned long long q1 = (unsigned long long)qc.z | (unsigned long long)qc.w << 32;
    const unsigned qid[kCascadeGroups] = {qi.x & 0xffffu, qi.x >> 16, qi.y & 0xffffu, qi.y >> 16, qi.z & 0xffffu, qi.z >> 16};
    const int* bb = bucket_begin + (size_t)task_col_image[ti] * kCascadeGroups * (kCascadeBuckets + 1);
    const int* br = bucket_rows + (size_t)kCascadeGroups * (size_t)T.col_off;
    int beg[kCascadeGroups];
    long long cum[kCascadeGroups + 1];
    cum[0] = 0;
#pragma unroll
    for (int g = 0; g < kCascadeGroups; ++g) {
      const int* p = bb + g * (kCascadeBuckets + 1) + qid[g];
      beg[g] = p[0];
      cum[g + 1] = cum[g] + (p[1] - p[0]);
    }
    const long long total = cum[kCascadeGroups];  // known before any candidate is loaded
    unsigned long long* my = counters + 4 * (blockIdx.x % kCascadeCounterShards);
    if (total <= kCascadeMinTotal) {
      if (lane == 0) atomicAdd(&my[2], 1ull);
    } else {
      unsigned long long key = kCascadeNoKey;
      constexpr int kFresh = 64 - kCascadeTop;
      for (long long base = 0; base < total; base += kFresh) {
        const long long e = base + (lane - kCascadeTop);
        if (lane >= kCascadeTop) {
          key = kCascadeNoKey;
          if (e < total) {
            int g = 0;
            size_t at = 0;
#pragma unroll
            for (int h = 0; h < kCascadeGroups; ++h)
              if (e >= cum[h] && e < cum[h + 1]) {
                g = h;
                at = (size_t)h * (size_t)T.n_cols + (size_t)beg[h] + (size_t)(e - cum[h]);
              }
            const int c = br[at];
            const uint4 cc = rec4[2 * (size_t)(T.col_off + c)], ci = rec4[2 * (size_t)(T.col_off + c) + 1];
            const unsigned cid[kCascadeGroups] = {ci.x & 0xffffu, ci.x >> 16, ci.y & 0xffffu, ci.y >> 16, ci.z & 0xffffu, ci.z >> 16};
            int first = kCascadeGroups;
#pragma unroll
            for (int h = kCascadeGroups - 1; h >= 0; --h)
              if (cid[h] == qid[h]) first = h;
            if (first == g) {
              const unsigned long long c0 = (unsigned long long)cc.x | (unsigned long long)cc.y << 32;
              const unsigned long long c1 = (unsigned long long)cc.z | (unsigned long long)cc.w << 32;
              const unsigned long long ham = (unsigned long long)(__popcll(q0 ^ c0) + __popcll(q1 ^ c1));
              key = ham << 40 | (unsigned long long)g << 32 | (unsigned long long)(unsigned)c;
            }
          }
        }
        key = cascade_wave_sort(key, lane);
      }
      const bool have = lane < kCascadeTop && key != kCascadeNoKey;
      const int num = __popcll(__ballot(have));  // >= 2: a column counts at most six times and total > 10
      const int c = have ? (int)(unsigned)(key & 0xffffffffull) : kMatchNoColumn;
      float d = __builtin_inff();
      if (have) {
        const float* a = desc + (size_t)(T.row_off + i) * dim;
        const float* bcol = desc + (size_t)(T.col_off + c) * dim;
        float acc = 0.f;
#pragma unroll 4
        for (int k = 0; k < dim; ++k) {
          const float t = a[k] - bcol[k];
          acc = acc + t * t;
        }
        d = acc;
      }
      for (int j = 0; j < num; ++j) match_insert(__shfl(d, j), __shfl(c, j), bd, bi, sd);
      if (lane == 0) {
        atomicAdd(&my[0], (unsigned long long)total);
        atomicAdd(&my[1], (unsigned long long)num);
      }
    }
  }
  if (lane == 0) {
    out.best_d[row] = bd;
    out.best_i[row] = bi;
    out.second_d[row] = sd;
  }
}

}  // namespace tmi
