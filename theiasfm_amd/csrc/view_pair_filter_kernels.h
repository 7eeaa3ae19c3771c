// The two view-pair filters of the global pipeline's edge stage (global_reconstruction_estimator.cc:360 and :392):
//
//   theia::FilterViewPairsFromOrientation          (filter_view_pairs_from_orientation.cc:55-122)
//   theia::FilterViewPairsFromRelativeTranslation  (filter_view_pairs_from_relative_translation.cc:68-304; the 1DSfM
//                                                   filter of Wilson and Snavely, ECCV 2014)
//
// on a view table and an edge list.
//
// orientation_filter_kernel   one thread per edge: loop = R(rotation_2)^T (R(o2) R(o1)^T), its angle in [0, pi] as
//                             atan2(|skew part| / 2, (trace - 1) / 2), the flag angle^2 > threshold^2.
// rotate_translations_kernel  one thread per edge: t = AngleAxisRotatePoint(-orientation[view1], position_2) (:68-85).
// translation_moments_kernel  ONE workgroup: the mean over the edges and the sum of squared deviations / (E - 1)
//                             (:180-195).  Thread t sums edges t, t + 256, ... in ascending order, then a binary LDS
//                             tree over the 256 partial sums: a fixed shape, the same bits on every run.
// mfas_order_kernel           ONE WORKGROUP PER ITERATION, every iteration in one launch: the projection of every
//                             edge onto the iteration's axis, OrderTranslationsFromProjections (:114-163) and the
//                             iteration's bad-weight contributions (:233-251).
//                               state     per view: in_w, out_w (the remaining incoming / outgoing weight) and cnt,
//                                         the number of remaining incoming nodes (-1: removed or without edges);
//                                         20 B a view, in LDS up to kMfasLdsViews views, else the same body on the
//                                         workgroup's slice of a per-call global buffer.
//                               set-up    one thread per view sums its CSR row in ascending edge index.
//                               a step    every thread scans its strided share of the views for (a source, smallest
//                                         index) and (largest score, smallest index); a wave butterfly and one
//                                         cross-wave stage in LDS pick the winner (min / max with the index as the tie
//                                         break: independent of the tree shape); the threads then walk the winner's
//                                         CSR row.  A neighbour appears once in a row (no unordered pair twice), so
//                                         exactly one thread touches it: no atomics.  Two barriers a step: scan ->
//                                         pick, update -> next scan.
//                               after     the workgroup walks the edges: contrib[it][e] = |p| where the order
//                                         contradicts the projection's sign, else 0.
//                             The projection is three products and two sums, left to right, WITHOUT contraction into
//                             FMA, and is recomputed wherever it is needed (three loads and five operations) instead
//                             of stored: every use sees the same bits, and so does a CPU model.
// bad_weight_sum_kernel       one thread per edge: the contributions added in ascending iteration order from zero, the
//                             flag weight > threshold, and the count of flags (a wave butterfly and one atomic add per
//                             wave, as filter_finish_kernel counts).
#pragma once
#include <hip/hip_runtime.h>

#include "track_estimate_kernels.h"

namespace tmi {

constexpr int kMfasThreads = 256;
constexpr int kMfasLdsViews = 6144;   // 20 B a view: 120 KB of the CU's 160 KB
constexpr int kMfasLdsHeader = 64;    // the cross-wave stage in front of the per-view arrays (a multiple of 16)

// the dynamic LDS of mfas_order_kernel<true> for `views` views
inline size_t mfas_lds_bytes(int views) {
  const size_t vp = ((size_t)views + 1) & ~(size_t)1;  // (keeps the int array behind the doubles 16-byte aligned)
  return (size_t)kMfasLdsHeader + vp * 20;
}

struct ViewPairGraph {
  int num_views;
  int num_pairs;
  const int* pair_view1;      // [E]
  const int* pair_view2;
  const double* translation;  // [3 E] in the global frame
  const int* row_ptr;         // [V + 1] CSR of the undirected graph
  const int2* row;            // [2 E] (neighbour, edge << 1 | (this view is the edge's view2)), ascending edge index
};

namespace vpf {

// t . a as the reference's Eigen dot product of two 3-vectors evaluates it without FMA: ((tx ax + ty ay) + tz az)
__device__ __forceinline__ double project(const double* __restrict__ t, double ax, double ay, double az) {
#pragma clang fp contract(off)
  const double xx = t[0] * ax;
  const double yy = t[1] * ay;
  const double zz = t[2] * az;
  const double s = xx + yy;
  return s + zz;
}

}  // namespace vpf

// filter_view_pairs_from_orientation.cc:55-68.  R(-x) = R(x)^T bit for bit in Ceres' AngleAxisToRotationMatrix.
__global__ __launch_bounds__(256) void orientation_filter_kernel(int num_pairs, const double* __restrict__ view_rot,
                                                                 const int* __restrict__ view1,
                                                                 const int* __restrict__ view2,
                                                                 const double* __restrict__ rotation2, double sq_max,
                                                                 unsigned char* __restrict__ removed,
                                                                 double* __restrict__ angle_out,
                                                                 int* __restrict__ counter) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  int flag = 0;
  if (e < num_pairs) {
    double R1[9], R2[9], Rr[9], C[9];
    const int a = view1[e], b = view2[e];
    const double o1[3] = {view_rot[3 * a], view_rot[3 * a + 1], view_rot[3 * a + 2]};
    const double o2[3] = {view_rot[3 * b], view_rot[3 * b + 1], view_rot[3 * b + 2]};
    const double rr[3] = {rotation2[3 * (size_t)e], rotation2[3 * (size_t)e + 1], rotation2[3 * (size_t)e + 2]};
    angle_axis_to_rotation_matrix(o1, R1);
    angle_axis_to_rotation_matrix(o2, R2);
    angle_axis_to_rotation_matrix(rr, Rr);
    // column-major: M(r, c) = M[r + 3 c].  C = R2 R1^T, L = Rr^T C
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) C[r + 3 * c] = R2[r] * R1[c] + R2[r + 3] * R1[c + 3] + R2[r + 6] * R1[c + 6];
    double L[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) L[r + 3 * c] = Rr[3 * r] * C[3 * c] + Rr[3 * r + 1] * C[3 * c + 1] + Rr[3 * r + 2] * C[3 * c + 2];
    const double sx = L[2 + 3 * 1] - L[1 + 3 * 2], sy = L[0 + 3 * 2] - L[2 + 3 * 0], sz = L[1 + 3 * 0] - L[0 + 3 * 1];
    const double sin_a = 0.5 * sqrt(sx * sx + sy * sy + sz * sz);
    const double cos_a = 0.5 * (L[0] + L[4] + L[8] - 1.0);
    const double angle = atan2(sin_a, cos_a);
    flag = angle * angle > sq_max;
    if (removed) removed[e] = (unsigned char)flag;
    if (angle_out) angle_out[e] = angle;
  }
  int n = flag;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, n);
}

// filter_view_pairs_from_relative_translation.cc:68-85
__global__ __launch_bounds__(256) void rotate_translations_kernel(int num_pairs, const double* __restrict__ view_rot,
                                                                  const int* __restrict__ view1,
                                                                  const double* __restrict__ position2,
                                                                  double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= num_pairs) return;
  const int a = view1[e];
  const double w[3] = {-view_rot[3 * a], -view_rot[3 * a + 1], -view_rot[3 * a + 2]};
  const double p[3] = {position2[3 * (size_t)e], position2[3 * (size_t)e + 1], position2[3 * (size_t)e + 2]};
  double q[3];
  rotate_point<false, double>(w, p, q, nullptr, nullptr);
  out[3 * (size_t)e] = q[0];
  out[3 * (size_t)e + 1] = q[1];
  out[3 * (size_t)e + 2] = q[2];
}

// :180-195.  out[0..3) the mean, out[3..6) the sum of squared deviations / (E - 1).  One workgroup of 256 threads.
__global__ __launch_bounds__(256) void translation_moments_kernel(int num_pairs, const double* __restrict__ t,
                                                                  double* __restrict__ out) {
  __shared__ double part[3][256];
  const int tid = threadIdx.x;
  double mean[3];
  for (int pass = 0; pass < 2; ++pass) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (int e = tid; e < num_pairs; e += 256)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double x = t[3 * (size_t)e + k];
        acc[k] += pass == 0 ? x : (x - mean[k]) * (x - mean[k]);
      }
#pragma unroll
    for (int k = 0; k < 3; ++k) part[k][tid] = acc[k];
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
      if (tid < half)
#pragma unroll
        for (int k = 0; k < 3; ++k) part[k][tid] += part[k][tid + half];
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double total = part[k][0];
      if (pass == 0) {
        mean[k] = total / (double)num_pairs;
        if (tid == 0) out[k] = mean[k];
      } else if (tid == 0) {
        out[3 + k] = total / (double)(num_pairs - 1);
      }
    }
    __syncthreads();  // (part is rewritten by the next pass)
  }
}

// One workgroup per iteration: blockIdx.x = the iteration.  axes [3 iterations]; order [iterations V] (-1 = a view
// without edges); contrib [iterations E]; ordered_views = the views with at least one edge (the number of steps).
// LDS: the state in dynamic LDS (mfas_lds_bytes(V)); else state = [iterations][20 B * V rounded up to even V] in
// global memory.
template <bool LDS>
__global__ __launch_bounds__(kMfasThreads) void mfas_order_kernel(ViewPairGraph G, const double* __restrict__ axes,
                                                                  int ordered_views, unsigned char* __restrict__ state,
                                                                  int* __restrict__ order_all,
                                                                  double* __restrict__ contrib_all) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mfas_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int it = blockIdx.x;
  const int V = G.num_views, E = G.num_pairs;
  const size_t vp = ((size_t)V + 1) & ~(size_t)1;
  // the cross-wave stage: per wave (source index, best index, best score)
  int* red_src = reinterpret_cast<int*>(mfas_smem);            // [4]
  int* red_idx = red_src + 4;                                  // [4]
  double* red_score = reinterpret_cast<double*>(mfas_smem + 32);  // [4]
  unsigned char* base = LDS ? mfas_smem + kMfasLdsHeader : state + (size_t)it * vp * 20;
  double* in_w = reinterpret_cast<double*>(base);
  double* out_w = in_w + vp;
  int* cnt = reinterpret_cast<int*>(out_w + vp);
  const double ax = axes[3 * it], ay = axes[3 * it + 1], az = axes[3 * it + 2];
  int* order = order_all + (size_t)it * V;
  const int kNone = 0x7fffffff;

  // set-up: the sums of every view's row in ascending edge index (:119-134)
  for (int v = tid; v < V; v += kMfasThreads) {
    double wi = 0.0, wo = 0.0;
    int ci = 0;
    const int r0 = G.row_ptr[v], r1 = G.row_ptr[v + 1];
    for (int r = r0; r < r1; ++r) {
      const int2 ent = G.row[r];
      const double p = vpf::project(G.translation + 3 * (size_t)(ent.y >> 1), ax, ay, az);
      // p > 0: view1 -> view2, else view2 -> view1 (a zero projection is an incoming node of weight 0 at view1)
      const bool outgoing = (p > 0.0) != (bool)(ent.y & 1);
      if (outgoing) {
        wo += fabs(p);
      } else {
        wi += fabs(p);
        ++ci;
      }
    }
    in_w[v] = wi;
    out_w[v] = wo;
    cnt[v] = r1 > r0 ? ci : -1;
    order[v] = -1;
  }
  __syncthreads();

  for (int step = 0; step < ordered_views; ++step) {
    // FindNextViewInOrder (:90-110) with the smallest index where the reference takes its hash map's first
    int src = kNone, best = kNone;
    double score = -HUGE_VAL;  // (the reference starts at 0 and takes score > best; scores are positive)
    for (int v = tid; v < V; v += kMfasThreads) {
      const int c = cnt[v];
      if (c < 0) continue;
      if (c == 0) {
        src = min(src, v);
      } else {
        const double sc = (out_w[v] + 1.0) / (in_w[v] + 1.0);
        if (sc > score) {  // (v ascends: a tie keeps the smaller index)
          score = sc;
          best = v;
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      src = min(src, __shfl_xor(src, o, 64));
      const double s2 = __shfl_xor(score, o, 64);
      const int b2 = __shfl_xor(best, o, 64);
      if (s2 > score || (s2 == score && b2 < best)) {
        score = s2;
        best = b2;
      }
    }
    if (lane == 0) {
      red_src[wave] = src;
      red_idx[wave] = best;
      red_score[wave] = score;
    }
    __syncthreads();
    src = red_src[0];
    best = red_idx[0];
    score = red_score[0];
#pragma unroll
    for (int w = 1; w < kMfasThreads / 64; ++w) {
      src = min(src, red_src[w]);
      const double s2 = red_score[w];
      const int b2 = red_idx[w];
      if (s2 > score || (s2 == score && b2 < best)) {
        score = s2;
        best = b2;
      }
    }
    const int win = src != kNone ? src : best;
    if (win == kNone) break;  // (no remaining view compares: non-finite weights; uniform over the workgroup)
    // :142-159: the winner leaves; every remaining neighbour loses the edge
    if (tid == 0) {
      order[win] = step;
      cnt[win] = -1;
    }
    const int r0 = G.row_ptr[win], r1 = G.row_ptr[win + 1];
    for (int r = r0 + tid; r < r1; r += kMfasThreads) {
      const int2 ent = G.row[r];
      const int n = ent.x;
      if (cnt[n] < 0) continue;
      const double p = vpf::project(G.translation + 3 * (size_t)(ent.y >> 1), ax, ay, az);
      const bool outgoing = (p > 0.0) != (bool)(ent.y & 1);  // win -> n
      if (outgoing) {
        in_w[n] -= fabs(p);
        cnt[n] -= 1;
      } else {
        out_w[n] -= fabs(p);
      }
    }
    __syncthreads();
  }

  // :233-251 (the order array was written by this workgroup: visible after the barrier above)
  __syncthreads();
  double* contrib = contrib_all + (size_t)it * E;
  for (int e = tid; e < E; e += kMfasThreads) {
    const double p = vpf::project(G.translation + 3 * (size_t)e, ax, ay, az);
    const int d = order[G.pair_view2[e]] - order[G.pair_view1[e]];
    contrib[e] = ((d < 0 && p > 0.0) || (d > 0 && p < 0.0)) ? fabs(p) : 0.0;
  }
}

// :262-304.  counter[0] += the number of flags.
__global__ __launch_bounds__(256) void bad_weight_sum_kernel(int num_pairs, int iterations,
                                                             const double* __restrict__ contrib, double threshold,
                                                             unsigned char* __restrict__ removed,
                                                             double* __restrict__ weight, int* __restrict__ counter) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  int flag = 0;
  if (e < num_pairs) {
    double w = 0.0;
    for (int it = 0; it < iterations; ++it) w += contrib[(size_t)it * num_pairs + e];
    flag = w > threshold;
    if (removed) removed[e] = (unsigned char)flag;
    if (weight) weight[e] = w;
  }
  int n = flag;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, n);
}

}  // namespace tmi
