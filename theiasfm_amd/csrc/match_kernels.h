// Batched BruteForceFeatureMatcher (reference brute_force_feature_matcher.cc:49-117): exact squared-L2 nearest and
// second-nearest neighbour, Lowe's ratio test, the intersection with the reverse direction and the compaction of the
// surviving matches in pair order.  The semantics are stated at tmi_ba_match_features (theia_mi355_ba.h); DESIGN 8.9
// has the tiling and what the equality with the numpy model rests on.
//
// A TASK is one (pair, direction): the rows of one image against the columns of the other.  match_nn_kernel gives every
// row of a task its (best distance, best column, second distance) under the total order (distance, then lower column);
// the finish kernels work on the rows of a chunk of pairs, laid out task after task, forward before reverse.
#pragma once

namespace tmi {

constexpr int kMatchTile = 64;         // rows and columns of a tile; 256 threads own a 4 x 4 block each
constexpr int kMatchChunkK = 32;       // descriptor elements of a column tile staged at once
constexpr int kMatchMaxStagedDim = 160;  // above it the row block is streamed through LDS like the columns
constexpr int kMatchNoColumn = 0x7fffffff;

struct MatchTask {
  long long row_off, col_off;  // first descriptor row of the row image and of the column image
  int n_rows, n_cols;
  int out_base;                // the task's first row among the chunk's rows
  int pair;                    // index of the pair inside the chunk
  int forward;                 // 1: rows = image 1
  int mate_base;               // out_base of the other direction of the pair (-1 without one)
};

struct MatchNn {
  float* best_d;
  int* best_i;
  float* second_d;
};

struct MatchRecord {  // one output match: the read-back's unit
  int feature1, feature2;
  float distance;
};

// (d, j) into the running best and second best of a row.  A NaN compares false everywhere and never enters.
__device__ __forceinline__ void match_insert(float d, int j, float& b, int& bi, float& s) {
  if (d < b || (d == b && j < bi)) {
    s = b;
    b = d;
    bi = j;
  } else if (d < s) {
    s = d;
  }
}

// Leading dimension of an LDS tile of `k` floats per descriptor: a multiple of 4 (float4 reads) that is 4 mod 8, so
// that the float4 reads of consecutive descriptors fall on different banks.
__host__ __device__ inline int match_ld(int k) {
  const int r = (k + 3) & ~3;
  return (r & 4) ? r : r + 4;
}
inline size_t match_lds_bytes(int dim) {
  const int kpad = (dim + kMatchChunkK - 1) / kMatchChunkK * kMatchChunkK;
  const int ldr = dim <= kMatchMaxStagedDim ? match_ld(kpad) : match_ld(kMatchChunkK);
  return (size_t)kMatchTile * (size_t)(ldr + match_ld(kMatchChunkK)) * sizeof(float);
}

// One workgroup per (task, block of 64 rows): blocks[b] = (task, row block).  STAGED: the row block's descriptors sit in
// LDS, zero-padded to a whole number of chunks, for the whole walk over the column tiles; otherwise they are streamed
// chunk by chunk beside the columns.  Padding is exact: (0 - 0)^2 added to a non-negative sum leaves its bits alone.
// Thread t owns rows ty + 16 i and columns tx + 16 j of the tile (tx = t % 16, ty = t / 16); for each of its sixteen
// accumulators k runs ascending over the whole dimension.
template <bool STAGED>
__global__ __launch_bounds__(256) void match_nn_kernel(const float* __restrict__ desc, int dim,
                                                       const MatchTask* __restrict__ tasks,
                                                       const int2* __restrict__ blocks, MatchNn out) {
#pragma clang fp contract(off)
  extern __shared__ float4 match_lds4[];
  float* lds = reinterpret_cast<float*>(match_lds4);
  const int2 blk = blocks[blockIdx.x];
  const MatchTask T = tasks[blk.x];
  const int row0 = blk.y * kMatchTile;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int num_chunks = (dim + kMatchChunkK - 1) / kMatchChunkK;
  const int ldc = match_ld(kMatchChunkK);
  const int ldr = STAGED ? match_ld(num_chunks * kMatchChunkK) : ldc;
  float* rowsL = lds;
  float* colsL = lds + kMatchTile * ldr;
  const float* rows = desc + (size_t)T.row_off * dim;
  const float* cols = desc + (size_t)T.col_off * dim;

  if (STAGED) {
    const int kpad = num_chunks * kMatchChunkK;
    for (int e = tid; e < kMatchTile * kpad; e += 256) {
      const int r = e / kpad, k = e - r * kpad;
      const int gr = row0 + r;
      rowsL[r * ldr + k] = (gr < T.n_rows && k < dim) ? rows[(size_t)gr * dim + k] : 0.f;
    }
  }

  float best[4], second[4];
  int besti[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    best[i] = second[i] = __builtin_inff();
    besti[i] = kMatchNoColumn;
  }

  for (int col0 = 0; col0 < T.n_cols; col0 += kMatchTile) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int c = 0; c < num_chunks; ++c) {
      const int k0 = c * kMatchChunkK;
      __syncthreads();  // the previous chunk has been read (and, the first time, the row block is written)
      for (int e = tid; e < kMatchTile * kMatchChunkK; e += 256) {
        const int r = e / kMatchChunkK, k = e - r * kMatchChunkK;
        const int gc = col0 + r, gk = k0 + k;
        colsL[r * ldc + k] = (gc < T.n_cols && gk < dim) ? cols[(size_t)gc * dim + gk] : 0.f;
        if (!STAGED) {
          const int gr = row0 + r;
          rowsL[r * ldr + k] = (gr < T.n_rows && gk < dim) ? rows[(size_t)gr * dim + gk] : 0.f;
        }
      }
      __syncthreads();
      const float* rp = rowsL + (STAGED ? k0 : 0);
#pragma unroll 2
      for (int k = 0; k < kMatchChunkK; k += 4) {
        float4 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const float4*>(rp + (ty + 16 * i) * ldr + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4*>(colsL + (tx + 16 * j) * ldc + k);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float t;
            t = a[i].x - b[j].x;
            acc[i][j] = acc[i][j] + t * t;
            t = a[i].y - b[j].y;
            acc[i][j] = acc[i][j] + t * t;
            t = a[i].z - b[j].z;
            acc[i][j] = acc[i][j] + t * t;
            t = a[i].w - b[j].w;
            acc[i][j] = acc[i][j] + t * t;
          }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gc = col0 + tx + 16 * j;
      if (gc < T.n_cols) {
#pragma unroll
        for (int i = 0; i < 4; ++i) match_insert(acc[i][j], gc, best[i], besti[i], second[i]);
      }
    }
  }

  // the sixteen threads that share a row merge through LDS: one thread per row walks them
  __syncthreads();
  float* mb = lds;                                   // [64][16]
  int* mi = reinterpret_cast<int*>(lds + 1024);      // [64][16]
  float* ms = lds + 2048;                            // [64][16]   (3072 floats <= the 64 * (36 + 36) of the smallest LDS)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty + 16 * i;
    mb[r * 16 + tx] = best[i];
    mi[r * 16 + tx] = besti[i];
    ms[r * 16 + tx] = second[i];
  }
  __syncthreads();
  if (tid < kMatchTile && row0 + tid < T.n_rows) {
    float b = mb[tid * 16], s = ms[tid * 16];
    int bi = mi[tid * 16];
    for (int t = 1; t < 16; ++t) {
      const float b2 = mb[tid * 16 + t], s2 = ms[tid * 16 + t];
      const int i2 = mi[tid * 16 + t];
      match_insert(b2, i2, b, bi, s);  // the other thread's best, then its second (its index cannot win: s2 >= b2)
      if (s2 < s) s = s2;
    }
    const size_t o = (size_t)T.out_base + (size_t)(row0 + tid);
    out.best_d[o] = b;
    out.best_i[o] = bi;
    out.second_d[o] = s;
  }
}

// The task of chunk row `row`: the last task whose out_base is <= row (tasks without rows share a base with their
// successor and are skipped by taking the last).
__device__ __forceinline__ int match_task_of_row(const MatchTask* __restrict__ tasks, int num_tasks, int row) {
  int lo = 0, hi = num_tasks - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tasks[mid].out_base <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Ratio test of every row of the chunk, both directions: pass[row]; the forward rows of a pair are counted.
// Cascade == false: step 3 of tmi_ba_match_features.  Cascade == true: step 6 of tmi_ba_match_features_cascade, the
// expression cascade_hasher.cc:268-271 types (ratio_sq is 1.0 without the ratio test; a row that was not skipped has
// at least two shortlisted columns).
template <bool Cascade>
__global__ __launch_bounds__(256) void match_ratio_kernel(const MatchTask* __restrict__ tasks, int num_tasks,
                                                          int num_rows, MatchNn nn, int use_ratio, double ratio_sq,
                                                          unsigned char* __restrict__ pass,
                                                          int* __restrict__ pair_num_forward) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= num_rows) return;
  const MatchTask T = tasks[match_task_of_row(tasks, num_tasks, row)];
  const int bi = nn.best_i[row];
  // a row that never saw a column that compares (no columns, or every distance NaN) still holds kMatchNoColumn, which
  // fails the upper bound here; match_symmetric_kernel's `back` index relies on pass[row] implying 0 <= bi < n_cols
  bool ok = bi >= 0 && bi < T.n_cols;
  if (Cascade) {
    if (ok) ok = !((double)nn.best_d[row] > (double)nn.second_d[row] * ratio_sq);
  } else {
    if (ok && use_ratio) ok = T.n_cols >= 2 && (double)nn.best_d[row] < ratio_sq * (double)nn.second_d[row];
  }
  pass[row] = ok;
  if (ok && T.forward) atomicAdd(&pair_num_forward[T.pair], 1);
}

// Forward rows only: the match survives the forward count and, with `symmetric`, the reverse look-up
// (IntersectMatches, feature_matcher_utils.cc:48-71); the survivors of a pair are counted.
__global__ __launch_bounds__(256) void match_symmetric_kernel(const MatchTask* __restrict__ tasks, int num_tasks,
                                                              int num_rows, MatchNn nn,
                                                              const unsigned char* __restrict__ pass,
                                                              const int* __restrict__ pair_num_forward, int symmetric,
                                                              int min_matches, unsigned char* __restrict__ keep,
                                                              int* __restrict__ pair_num_kept) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= num_rows) return;
  const MatchTask T = tasks[match_task_of_row(tasks, num_tasks, row)];
  bool ok = false;
  if (T.forward) {
    ok = pass[row] && pair_num_forward[T.pair] >= min_matches;
    if (ok && symmetric) {
      const int back = T.mate_base + nn.best_i[row];  // (best_i < n_cols = the mate's rows: pass[row] checked it)
      ok = T.mate_base >= 0 && pass[back] && nn.best_i[back] == row - T.out_base;
    }
    if (ok) atomicAdd(&pair_num_kept[T.pair], 1);
  }
  keep[row] = ok;
}

// flag[row] = 1 for a match that is output: kept, and its pair has enough of them.
__global__ __launch_bounds__(256) void match_flag_kernel(const MatchTask* __restrict__ tasks, int num_tasks,
                                                         int num_rows, const unsigned char* __restrict__ keep,
                                                         const int* __restrict__ pair_num_kept, int min_matches,
                                                         int* __restrict__ flag) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row > num_rows) return;
  int f = 0;
  if (row < num_rows) {
    const MatchTask T = tasks[match_task_of_row(tasks, num_tasks, row)];
    f = keep[row] && pair_num_kept[T.pair] >= min_matches;
  }
  flag[row] = f;  // (flag[num_rows] = 0: the scan's last entry is the total)
}

// scan: the exclusive sum of flag over num_rows + 1 entries.  The matches, compacted in row order.
__global__ __launch_bounds__(256) void match_compact_kernel(const MatchTask* __restrict__ tasks, int num_tasks,
                                                            int num_rows, MatchNn nn, const int* __restrict__ flag,
                                                            const int* __restrict__ scan,
                                                            MatchRecord* __restrict__ out) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= num_rows || !flag[row]) return;
  const MatchTask T = tasks[match_task_of_row(tasks, num_tasks, row)];
  MatchRecord m;
  m.feature1 = row - T.out_base;
  m.feature2 = nn.best_i[row];
  m.distance = nn.best_d[row];
  out[scan[row]] = m;
}

// Per pair of the chunk: counts[4 p .. 4 p + 3] = status, forward count, first match (chunk-relative), 0;
// counts[4 num_pairs] = the chunk's total.  fwd_task[p]: the pair's forward task.
__global__ __launch_bounds__(256) void match_pair_kernel(const MatchTask* __restrict__ tasks,
                                                         const int* __restrict__ fwd_task, int num_pairs, int num_rows,
                                                         const int* __restrict__ pair_num_forward,
                                                         const int* __restrict__ pair_num_kept, int min_matches,
                                                         const int* __restrict__ scan, int* __restrict__ counts) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > num_pairs) return;
  if (p == num_pairs) {
    counts[4 * p] = scan[num_rows];
    return;
  }
  const int nf = pair_num_forward[p];
  counts[4 * p] = (nf < min_matches || pair_num_kept[p] < min_matches) ? 1 : 0;
  counts[4 * p + 1] = nf;
  counts[4 * p + 2] = scan[tasks[fwd_task[p]].out_base];
  counts[4 * p + 3] = 0;
}

}  // namespace tmi
