// theia::LinearPositionEstimator (linear_position_estimator.cc:163-470; Jiang, Cui and Tan, ICCV 2013) on the view table
// and edge list of the other position estimators, joined to the tracks of a tmi_ba_problem: global positions as the
// eigenvector of the smallest eigenvalue of A^T A, A three 3-row constraints per view triplet.  The steps are numbered in
// include/theia_mi355_ba.h; the host loop is in pose_graph_calls.h, the rows it uploads come from pose_graph_host.h.
//
// lpos_triplet_kernel<FILL>  one wavefront per slot r of the sorted adjacency rows, the edge (a, b) = (row owner,
//                            neighbour) with a < b: the lanes stride over the later slots of a's row (the neighbours
//                            c > b) and each looks c up in b's row by bisection.  FILL = false counts; after
//                            lpos_scan_kernel FILL = true writes the triangle (a, b, c), its three batch pairs and the
//                            length of the shortest of the three track lists behind the slot's offset, in ascending c:
//                            the triplets come out in lexicographic order.  A hub's row is spread over the lanes.
// lpos_scan_kernel           one workgroup: the exclusive sums of n counts ([n + 1], the total last)
// lpos_feature_kernel        one thread per observation: pixel_to_camera, hnormalized(), homogeneous().normalized()
// lpos_baseline_kernel       one workgroup per triplet: the threads stride over the first view's track list and look
//                            each track up in the other two by bisection; a common track runs the three two-view
//                            triangulations (the angle test and the midpoint solve of track_estimate_kernels.h) and puts
//                            its two depth ratios into LDS (kSelectCap per ratio) or, where the shortest of the three
//                            lists is longer than kSelectCap, into the triplet's scratch in global memory.  The slot
//                            comes from an integer LDS counter: the ORDER of the ratios varies from run to run, the set
//                            does not, and the order statistic lpos_select reads is a function of the set.
// lpos_first_kernel / lpos_link_kernel / lpos_component_stats_kernel
//                            the components of the surviving triplets: first[pair] = the smallest surviving triplet at
//                            the pair (integer atomicMin), every triplet linked to the first of each of its pairs, then
//                            tb_union_kernel, tb_flatten_kernel and tb_sizes_kernel as they are; the largest by the key
//                            (size << 32 | ~label), a 64-bit atomic max (most triplets, then the smallest number)
// lpos_record_kernel         one thread per chosen triplet: the three translation directions, the three rotations
//                            between them (Eigen's FromTwoVectors), the scale ratios and the nine 3 x 3 blocks
// lpos_assemble_kernel       one thread per entry of a 3 x 3 block (p, q) of A^T A: the sum over the block's triplets in
//                            ascending triplet number -- one writer, a fixed order
// lpos_rowsum_kernel / lpos_scalars_kernel / lpos_shift_kernel
//                            |M|_inf and the largest diagonal entry, then M + mu I
// lpos_apply_rows_kernel / lpos_apply_cols_kernel
//                            Z = A^T (A Y) from the records: U = A Y one thread per (triplet, column), then one thread per
//                            (free view, column) over the view's triplets in ascending number
// lpos_vote_kernel           the sign vote over the batch edges (integer counters)
//
// The iteration itself runs on rotation_linear_kernels.h's kernels (start, Gram-Schmidt, Gram, Ritz, rotate).  Every
// kernel is a plain grid launch.  No floating-point atomics, every floating-point sum of fixed shape, no FMA contraction
// in what is written here: the same bytes from call to call.
#pragma once
#include <hip/hip_runtime.h>

#include "pose_graph.h"
#include "rotation_linear_kernels.h"
#include "track_build_kernels.h"
#include "track_estimate_kernels.h"

namespace tmi {
namespace lpos {

constexpr int kSelectCap = 1024;  // ratios per kind that one workgroup keeps in LDS (2 x 8 KB)
constexpr int kRecord = 81;       // doubles of a triplet's record: block C[k][i](r, c) at 27 k + 9 i + 3 r + c
enum { kBest = 0, kComponents, kDroppedRatios, kVotesFor, kVotesAgainst, kError = kTbError, kCounters = 8 };

// the position of `key` in the ascending list[lo, hi), -1: not there
__device__ __forceinline__ int find_sorted(const int* __restrict__ list, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int x = list[mid];
    if (x == key) return mid;
    if (x < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return -1;
}

// GetTriangulatedPointDepths (compute_triplet_baseline_ratios.cc:55-86): origins {0, position_2}, directions
// {f1, R2^T f2}; false where the angle test or the midpoint's LLT fails.
__device__ __forceinline__ bool point_depths(const double* __restrict__ rotation2, const double* __restrict__ position2,
                                             const double f1[3], const double f2[3], double cos_min, double* depth1,
                                             double* depth2) {
#pragma clang fp contract(off)
  const double aa[3] = {rotation2[0], rotation2[1], rotation2[2]};
  const double o2[3] = {position2[0], position2[1], position2[2]};
  double R[9], d2[3];
  angle_axis_to_rotation_matrix(aa, R);
#pragma unroll
  for (int c = 0; c < 3; ++c) d2[c] = R[3 * c] * f2[0] + R[3 * c + 1] * f2[1] + R[3 * c + 2] * f2[2];  // R^T f2
  if (!(f1[0] * d2[0] + f1[1] * d2[1] + f1[2] * d2[2] < cos_min)) return false;
  double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, X[4];
  const double o1[3] = {0.0, 0.0, 0.0};
  midpoint_accumulate(f1, o1, A, b);
  midpoint_accumulate(d2, o2, A, b);
  if (!midpoint_solve(A, b, 2.0, X)) return false;
  const double p[3] = {X[0] / X[3], X[1] / X[3], X[2] / X[3]};
  *depth1 = sqrt(pg::sq3(p[0], p[1], p[2]));
  *depth2 = sqrt(pg::sq3(p[0] - o2[0], p[1] - o2[1], p[2] - o2[2]));
  return true;
}

// the element of rank k (0-based, ascending) of x[0, n): the value nth_element leaves at index k.  Every thread of the
// workgroup counts for its elements; the threads that hold the answer all write the same value.
__device__ __forceinline__ void select_rank(const double* x, int n, int k, double* result) {
  for (int i = threadIdx.x; i < n; i += 256) {
    const double xi = x[i];
    int less = 0, not_greater = 0;
    for (int j = 0; j < n; ++j) {
      const double xj = x[j];
      less += xj < xi;
      not_greater += xj <= xi;
    }
    if (less <= k && k < not_greater) *result = xi;
  }
}

// Eigen's Quaterniond::FromTwoVectors(a, b).toRotationMatrix(), R(r, c) = R[3 r + c].  DEVIATION: where the vectors are
// nearly antiparallel (c < -1 + 1e-12) Eigen takes an axis from an SVD; here the rotation is by pi about
// normalized(v0 x e_k), e_k the coordinate axis of v0's smallest |component| (the first of equals).
__device__ __forceinline__ void from_two_vectors(const double a[3], const double b[3], double R[9]) {
#pragma clang fp contract(off)
  double v0[3], v1[3];
  const double na2 = pg::sq3(a[0], a[1], a[2]), nb2 = pg::sq3(b[0], b[1], b[2]);
  const double na = na2 > 0.0 ? sqrt(na2) : 1.0, nb = nb2 > 0.0 ? sqrt(nb2) : 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v0[k] = a[k] / na;
    v1[k] = b[k] / nb;
  }
  const double c = (v1[0] * v0[0] + v1[1] * v0[1]) + v1[2] * v0[2];
  double x, y, z, w;
  if (c < -1.0 + 1e-12) {
    int k = 0;
    if (fabs(v0[1]) < fabs(v0[k])) k = 1;
    if (fabs(v0[2]) < fabs(v0[k])) k = 2;
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    const double ax = v0[1] * e[2] - v0[2] * e[1], ay = v0[2] * e[0] - v0[0] * e[2], az = v0[0] * e[1] - v0[1] * e[0];
    const double n = sqrt(pg::sq3(ax, ay, az));
    x = ax / n;
    y = ay / n;
    z = az / n;
    w = 0.0;
  } else {
    const double s = sqrt((1.0 + c) * 2.0), invs = 1.0 / s;
    x = (v0[1] * v1[2] - v0[2] * v1[1]) * invs;
    y = (v0[2] * v1[0] - v0[0] * v1[2]) * invs;
    z = (v0[0] * v1[1] - v0[1] * v1[0]) * invs;
    w = s * 0.5;
  }
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
               tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz);
  R[1] = txy - twz;
  R[2] = txz + twy;
  R[3] = txy + twz;
  R[4] = 1.0 - (txx + tzz);
  R[5] = tyz - twx;
  R[6] = txz - twy;
  R[7] = tyz + twx;
  R[8] = 1.0 - (txx + tyy);
}

// -R(orientation)^T position_2: the translation direction of a pair in the global frame
__device__ __forceinline__ void global_direction(const double* __restrict__ orientation,
                                                 const double* __restrict__ position2, double t[3]) {
#pragma clang fp contract(off)
  const double aa[3] = {orientation[0], orientation[1], orientation[2]};
  double R[9];
  angle_axis_to_rotation_matrix(aa, R);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    t[c] = -((R[3 * c] * position2[0] + R[3 * c + 1] * position2[1]) + R[3 * c + 2] * position2[2]);
}

}  // namespace lpos

// adj_ptr [V + 1], adj [2 E] (neighbour, pair) ascending neighbour, adj_view [2 E] the row's owner.  FILL = false:
// count [2 E].  FILL = true: offset [2 E] from the scan; view / pair [3 T], shortest [T].
template <bool FILL>
__global__ __launch_bounds__(256) void lpos_triplet_kernel(int num_slots, const int* __restrict__ adj_ptr,
                                                           const int2* __restrict__ adj, const int* __restrict__ adj_view,
                                                           const int* __restrict__ track_ptr, int* __restrict__ count,
                                                           const int* __restrict__ offset, int* __restrict__ view,
                                                           int* __restrict__ pair, int* __restrict__ shortest) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);  // (uniform over the wavefront)
  const int lane = threadIdx.x & 63;
  if (r >= num_slots) return;
  const int a = adj_view[r];
  const int2 ab = adj[r];
  const int b = ab.x;
  if (b < a) {
    if (!FILL && lane == 0) count[r] = 0;
    return;
  }
  const int a1 = adj_ptr[a + 1], b0 = adj_ptr[b], b1 = adj_ptr[b + 1];
  int found_before = 0;
  for (int s0 = r + 1; s0 < a1; s0 += 64) {  // the later slots of a's row: the neighbours c > b
    const int s = s0 + lane;
    int at = -1;
    int2 ac = make_int2(0, 0);
    if (s < a1) {
      ac = adj[s];
      // bisection on the neighbours of b's row
      int lo = b0, hi = b1;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int x = adj[mid].x;
        if (x == ac.x) {
          at = mid;
          break;
        }
        if (x < ac.x)
          lo = mid + 1;
        else
          hi = mid;
      }
    }
    const unsigned long long mask = __ballot(at >= 0);
    if (FILL && at >= 0) {
      const int t = offset[r] + found_before + __popcll(mask & ((1ull << lane) - 1ull));
      const int c = ac.x;
      view[3 * (size_t)t] = a;
      view[3 * (size_t)t + 1] = b;
      view[3 * (size_t)t + 2] = c;
      pair[3 * (size_t)t] = ab.y;
      pair[3 * (size_t)t + 1] = ac.y;
      pair[3 * (size_t)t + 2] = adj[at].y;
      const int la = track_ptr[a + 1] - track_ptr[a], lb = track_ptr[b + 1] - track_ptr[b],
                lc = track_ptr[c + 1] - track_ptr[c];
      shortest[t] = min(la, min(lb, lc));
    }
    found_before += __popcll(mask);
  }
  if (!FILL && lane == 0) count[r] = found_before;
}

// out [n + 1]: out[i] = the sum of f(in[0 .. i)), f(x) = x (cap < 0) or (x > cap ? 2 x : 0) -- the scratch doubles of a
// triplet on the global selection path.  total: the sum as 64 bits (the caller refuses one above 2^30).
__global__ __launch_bounds__(256) void lpos_scan_kernel(const int* __restrict__ in, int n, int cap, int* __restrict__ out,
                                                        unsigned long long* __restrict__ total) {
  __shared__ unsigned long long part[256];
  const int chunk = (n + 255) / 256;
  const int i0 = min(n, (int)threadIdx.x * chunk), i1 = min(n, i0 + chunk);
  unsigned long long s = 0;
  for (int i = i0; i < i1; ++i) {
    const int x = in[i];
    s += (cap < 0 ? (unsigned long long)x : (x > cap ? 2ull * (unsigned long long)x : 0ull));
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int k = 0; k < 256; ++k) {
      const unsigned long long v = part[k];
      part[k] = run;
      run += v;
    }
    *total = run;
    out[n] = (int)min(run, 0x7fffffffull);
  }
  __syncthreads();
  unsigned long long run = part[threadIdx.x];
  for (int i = i0; i < i1; ++i) {
    out[i] = (int)min(run, 0x7fffffffull);
    const int x = in[i];
    run += (cap < 0 ? (unsigned long long)x : (x > cap ? 2ull * (unsigned long long)x : 0ull));
  }
}

// One thread per slot of the view-major observation order: slot_cam / slot_xy from the host's sort; cam (model, offset,
// count, .) as view_cam_record writes it.  feature [3 x slot].
__global__ __launch_bounds__(256) void lpos_feature_kernel(int num_slots, const int* __restrict__ slot_cam,
                                                           const double* __restrict__ slot_xy,
                                                           const int4* __restrict__ cam, const double* __restrict__ intr,
                                                           double* __restrict__ feature) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= num_slots) return;
  const int4 rec = cam[slot_cam[i]];
  const double* Kp = intr + rec.y;
  double Kv[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) Kv[k] = (k < rec.z) ? Kp[k] : 0.0;
  const double px[2] = {slot_xy[2 * (size_t)i], slot_xy[2 * (size_t)i + 1]};
  double pt[3];
  pixel_to_camera(rec.x, Kv, px, pt);
  // hnormalized(): a ray with negative z flips here, as in the reference; then homogeneous().normalized()
  const double hx = pt[0] / pt[2], hy = pt[1] / pt[2];
  const double n = sqrt(pg::sq3(hx, hy, 1.0));
  feature[3 * (size_t)i] = hx / n;
  feature[3 * (size_t)i + 1] = hy / n;
  feature[3 * (size_t)i + 2] = 1.0 / n;
}

// blockIdx.x = the triplet.  track_ptr [V + 1], track [slots] ascending inside a view.  scratch_at [T + 1] doubles.
// baseline [3 T], num_common / num_used [T].
__global__ __launch_bounds__(256) void lpos_baseline_kernel(
    const int* __restrict__ view, const int* __restrict__ pair, const int* __restrict__ track_ptr,
    const int* __restrict__ track, const double* __restrict__ feature, const double* __restrict__ rotation2,
    const double* __restrict__ position2, double cos_min, const int* __restrict__ shortest,
    const int* __restrict__ scratch_at, double* __restrict__ scratch, double* __restrict__ baseline,
    int* __restrict__ num_common, int* __restrict__ num_used, unsigned long long* counters) {
#pragma clang fp contract(off)
  __shared__ double lds2[lpos::kSelectCap], lds3[lpos::kSelectCap];
  __shared__ int common, used, dropped;
  __shared__ double median[2];
  const int t = blockIdx.x;
  const int va = view[3 * (size_t)t], vb = view[3 * (size_t)t + 1], vc = view[3 * (size_t)t + 2];
  const int e12 = pair[3 * (size_t)t], e13 = pair[3 * (size_t)t + 1], e23 = pair[3 * (size_t)t + 2];
  const int cap = shortest[t];  // no triplet has more common tracks
  double *r2 = lds2, *r3 = lds3;
  if (cap > lpos::kSelectCap) {
    r2 = scratch + scratch_at[t];
    r3 = r2 + cap;
  }
  if (threadIdx.x == 0) {
    common = 0;
    used = 0;
    dropped = 0;
    median[0] = 0.0;
    median[1] = 0.0;
  }
  __syncthreads();
  const int a0 = track_ptr[va], a1 = track_ptr[va + 1];
  for (int i = a0 + threadIdx.x; i < a1; i += 256) {
    const int id = track[i];
    const int j = lpos::find_sorted(track, track_ptr[vb], track_ptr[vb + 1], id);
    if (j < 0) continue;
    const int k = lpos::find_sorted(track, track_ptr[vc], track_ptr[vc + 1], id);
    if (k < 0) continue;
    atomicAdd(&common, 1);
    const double f1[3] = {feature[3 * (size_t)i], feature[3 * (size_t)i + 1], feature[3 * (size_t)i + 2]};
    const double f2[3] = {feature[3 * (size_t)j], feature[3 * (size_t)j + 1], feature[3 * (size_t)j + 2]};
    const double f3[3] = {feature[3 * (size_t)k], feature[3 * (size_t)k + 1], feature[3 * (size_t)k + 2]};
    double d1_12, d2_12, d1_13, d3_13, d2_23, d3_23;
    if (!lpos::point_depths(rotation2 + 3 * (size_t)e12, position2 + 3 * (size_t)e12, f1, f2, cos_min, &d1_12, &d2_12))
      continue;
    if (!lpos::point_depths(rotation2 + 3 * (size_t)e13, position2 + 3 * (size_t)e13, f1, f3, cos_min, &d1_13, &d3_13))
      continue;
    if (!lpos::point_depths(rotation2 + 3 * (size_t)e23, position2 + 3 * (size_t)e23, f2, f3, cos_min, &d2_23, &d3_23))
      continue;
    const double q2 = d1_12 / d1_13, q3 = d2_12 / d2_23;
    // DEVIATION: a ratio that is not finite and positive is dropped (with its partner) and counted
    if (!(q2 > 0.0) || !(q3 > 0.0) || isinf(q2) || isinf(q3)) {
      atomicAdd(&dropped, 1);
      continue;
    }
    const int slot = atomicAdd(&used, 1);
    if (slot < cap) {  // (always: used <= common <= cap)
      r2[slot] = q2;
      r3[slot] = q3;
    }
  }
  __syncthreads();
  const int n = min(used, cap);
  if (n > 0) {
    lpos::select_rank(r2, n, n / 2, &median[0]);
    lpos::select_rank(r3, n, n / 2, &median[1]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    num_common[t] = common;
    num_used[t] = n;
    baseline[3 * (size_t)t] = n > 0 ? 1.0 : 0.0;
    baseline[3 * (size_t)t + 1] = median[0];
    baseline[3 * (size_t)t + 2] = median[1];
    if (dropped) atomicAdd(&counters[lpos::kDroppedRatios], (unsigned long long)dropped);
  }
}

// first [E] was filled with kTbNoLabel
__global__ __launch_bounds__(256) void lpos_first_kernel(int num_triplets, const int* __restrict__ pair,
                                                         const int* __restrict__ num_used, unsigned* first) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= num_triplets || num_used[t] <= 0) return;
#pragma unroll
  for (int s = 0; s < 3; ++s) atomicMin(&first[pair[3 * (size_t)t + s]], (unsigned)t);
}

// link [2 x 3 T]: the endpoints tb_union_kernel reads; a triplet that did not survive links to itself
__global__ __launch_bounds__(256) void lpos_link_kernel(int num_triplets, const int* __restrict__ pair,
                                                        const int* __restrict__ num_used,
                                                        const unsigned* __restrict__ first, unsigned* __restrict__ link) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= num_triplets) return;
  const bool alive = num_used[t] > 0;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    link[2 * (3 * (size_t)t + s)] = (unsigned)t;
    link[2 * (3 * (size_t)t + s) + 1] = alive ? first[pair[3 * (size_t)t + s]] : (unsigned)t;
  }
}

// The surviving roots: their number, and the key (size << 32 | ~label) of the largest.  size [T] counts every triplet of
// a label; a triplet that did not survive is alone under its own.
__global__ __launch_bounds__(256) void lpos_component_stats_kernel(int num_triplets, const int* __restrict__ num_used,
                                                                   const unsigned* __restrict__ label,
                                                                   const unsigned* __restrict__ size,
                                                                   unsigned long long* counters) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool root = t < num_triplets && num_used[t] > 0 && label[t] == (unsigned)t;
  tb_count(root, &counters[lpos::kComponents]);
  if (root)
    atomicMax(&counters[lpos::kBest], ((unsigned long long)size[t] << 32) | (unsigned long long)(0xffffffffu - (unsigned)t));
}

// One thread per chosen triplet c: views / pairs [3 C] (the caller's indices), baseline [3 C], view_count [V] the chosen
// triplets of a view.  record [81 C].
__global__ __launch_bounds__(256) void lpos_record_kernel(int num_chosen, const int* __restrict__ view,
                                                          const int* __restrict__ pair,
                                                          const double* __restrict__ baseline,
                                                          const int* __restrict__ view_count,
                                                          const double* __restrict__ orientation,
                                                          const double* __restrict__ position2,
                                                          double* __restrict__ record) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= num_chosen) return;
  const int v0 = view[3 * (size_t)c], v1 = view[3 * (size_t)c + 1], v2 = view[3 * (size_t)c + 2];
  const int fewest = min(view_count[v0], min(view_count[v1], view_count[v2]));
  const double w = 1.0 / sqrt((double)fewest);
  double t01[3], t02[3], t12[3], m01[3], m02[3], m12[3];
  lpos::global_direction(orientation + 3 * (size_t)v0, position2 + 3 * (size_t)pair[3 * (size_t)c], t01);
  lpos::global_direction(orientation + 3 * (size_t)v0, position2 + 3 * (size_t)pair[3 * (size_t)c + 1], t02);
  lpos::global_direction(orientation + 3 * (size_t)v1, position2 + 3 * (size_t)pair[3 * (size_t)c + 2], t12);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m01[k] = -t01[k];
    m02[k] = -t02[k];
    m12[k] = -t12[k];
  }
  double r012[9], r201[9], r120[9];
  lpos::from_two_vectors(t12, m01, r012);
  lpos::from_two_vectors(t01, t02, r201);
  lpos::from_two_vectors(m02, m12, r120);
  const double b0 = baseline[3 * (size_t)c], b1 = baseline[3 * (size_t)c + 1], b2 = baseline[3 * (size_t)c + 2];
  const double s012 = b0 / b2, s201 = b1 / b0, s120 = b2 / b1;
  double* C = record + (size_t)lpos::kRecord * c;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double I = r == q ? 1.0 : 0.0, two = (-2.0 * w) * I;
      const int at = 3 * r + q, tr = 3 * q + r;  // (r, q) and its transpose
      // t01 taken as exact, solved for c2 (:395-402)
      C[0 + at] = ((-s201 * r201[at] + r012[tr] / s012) + I) * w;
      C[9 + at] = ((s201 * r201[at] - r012[tr] / s012) + I) * w;
      C[18 + at] = two;
      // t02 taken as exact, solved for c1 (:405-411)
      C[27 + at] = ((-r201[tr] / s201 + s120 * r120[at]) + I) * w;
      C[36 + at] = two;
      C[45 + at] = ((r201[tr] / s201 - s120 * r120[at]) + I) * w;
      // t12 taken as exact, solved for c0 (:414-420)
      C[54 + at] = two;
      C[63 + at] = ((-s012 * r012[at] + r120[tr] / s120) + I) * w;
      C[72 + at] = ((s012 * r012[at] - r120[tr] / s120) + I) * w;
    }
}

// One thread per (block, entry): block_ptr [B + 1], block_pq [B] the block's (row, column) view columns, block_entry
// (chosen triplet, 3 i + j: the row's and the column's slot in it) ascending triplet.  A [n][n] was cleared.
__global__ __launch_bounds__(256) void lpos_assemble_kernel(int num_blocks, const int* __restrict__ block_ptr,
                                                            const int2* __restrict__ block_pq,
                                                            const int2* __restrict__ block_entry,
                                                            const double* __restrict__ record, int n,
                                                            double* __restrict__ A) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * num_blocks) return;
  const int blk = i / 9, a = (i - 9 * blk) / 3, b = i - 9 * blk - 3 * a;
  const int2 pq = block_pq[blk];
  double acc = 0.0;
  for (int r = block_ptr[blk]; r < block_ptr[blk + 1]; ++r) {
    const int2 ent = block_entry[r];
    const int si = ent.y / 3, sj = ent.y - 3 * si;
    const double* C = record + (size_t)lpos::kRecord * ent.x;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int row = 0; row < 3; ++row) s += C[27 * k + 9 * si + 3 * row + a] * C[27 * k + 9 * sj + 3 * row + b];
    acc += s;
  }
  A[(size_t)(3 * pq.x + a) * n + (3 * pq.y + b)] = acc;
}

// blockIdx.x = the row: rowsum[i] = sum |A[i][.]|, diagonal[i] = A[i][i]
__global__ __launch_bounds__(256) void lpos_rowsum_kernel(int n, const double* __restrict__ A, double* __restrict__ rowsum,
                                                          double* __restrict__ diagonal) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int i = blockIdx.x;
  double acc = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) acc += fabs(A[(size_t)i * n + j]);
  const double total = pg::block_sum(acc, part);
  if (threadIdx.x == 0) {
    rowsum[i] = total;
    diagonal[i] = A[(size_t)i * n + i];
  }
}

// one workgroup: scalars[0] = the largest diagonal entry, scalars[1] = |M|_inf (a maximum is the same in any order)
__global__ __launch_bounds__(256) void lpos_scalars_kernel(int n, const double* __restrict__ rowsum,
                                                           const double* __restrict__ diagonal,
                                                           double* __restrict__ scalars) {
  __shared__ double big[2][256];
  double d = 0.0, s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    d = fmax(d, diagonal[i]);
    s = fmax(s, rowsum[i]);
  }
  big[0][threadIdx.x] = d;
  big[1][threadIdx.x] = s;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (threadIdx.x < half) {
      big[0][threadIdx.x] = fmax(big[0][threadIdx.x], big[0][threadIdx.x + half]);
      big[1][threadIdx.x] = fmax(big[1][threadIdx.x], big[1][threadIdx.x + half]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    scalars[0] = big[0][0];
    scalars[1] = big[1][0];
  }
}

__global__ __launch_bounds__(256) void lpos_shift_kernel(int n, double relative_shift, const double* __restrict__ scalars,
                                                         double* __restrict__ A) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double mu = relative_shift * scalars[0];
  A[(size_t)i * n + i] += mu;
}

// One thread per (chosen triplet, column): U [9 C][6] = A Y; column [3 C] the slots' view columns (-1: the held view).
__global__ __launch_bounds__(256) void lpos_apply_rows_kernel(int num_chosen, const int* __restrict__ column,
                                                              const double* __restrict__ record,
                                                              const double* __restrict__ Y, double* __restrict__ U) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= num_chosen * lin::kBlock) return;
  const int c = i / lin::kBlock, j = i - c * lin::kBlock;
  const double* C = record + (size_t)lpos::kRecord * c;
  double y[3][3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int col = column[3 * (size_t)c + s];
#pragma unroll
    for (int k = 0; k < 3; ++k) y[s][k] = col >= 0 ? Y[(size_t)(3 * col + k) * lin::kBlock + j] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double u = 0.0;
#pragma unroll
      for (int s = 0; s < 3; ++s)
        u += (C[27 * k + 9 * s + 3 * r] * y[s][0] + C[27 * k + 9 * s + 3 * r + 1] * y[s][1]) +
             C[27 * k + 9 * s + 3 * r + 2] * y[s][2];
      U[(size_t)(9 * c + 3 * k + r) * lin::kBlock + j] = u;
    }
}

// One thread per (free view column p, column j): Z = A^T U over view_ptr / view_entry (chosen triplet, slot), ascending
// triplet.
__global__ __launch_bounds__(256) void lpos_apply_cols_kernel(int num_columns, const int* __restrict__ view_ptr,
                                                              const int2* __restrict__ view_entry,
                                                              const double* __restrict__ record,
                                                              const double* __restrict__ U, double* __restrict__ Z) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= num_columns * lin::kBlock) return;
  const int p = i / lin::kBlock, j = i - p * lin::kBlock;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int r = view_ptr[p]; r < view_ptr[p + 1]; ++r) {
    const int2 ent = view_entry[r];
    const double* C = record + (size_t)lpos::kRecord * ent.x + 9 * ent.y;
    const double* u = U + (size_t)9 * ent.x * lin::kBlock + j;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int row = 0; row < 3; ++row) s += C[27 * k + 3 * row + a] * u[(size_t)(3 * k + row) * lin::kBlock];
      acc[a] += s;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) Z[(size_t)(3 * p + a) * lin::kBlock + j] = acc[a];
}

// view_column [V]: >= 0 a free view's column, -1 the held view, -2 a view that is not estimated.  Q [n][6]: column 0
// is the solution.  position [3 V] (estimated views only); the votes into the counters.
__global__ __launch_bounds__(256) void lpos_position_kernel(int num_views, const int* __restrict__ view_column,
                                                            const double* __restrict__ Q, double* __restrict__ position) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= num_views) return;
  const int col = view_column[v];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    position[3 * (size_t)v + k] = col >= 0 ? Q[(size_t)(3 * col + k) * lin::kBlock] : 0.0;
}

__global__ __launch_bounds__(256) void lpos_vote_kernel(int num_pairs, const int* __restrict__ view1,
                                                        const int* __restrict__ view2, const int* __restrict__ view_column,
                                                        const double* __restrict__ position,
                                                        const double* __restrict__ orientation,
                                                        const double* __restrict__ position2,
                                                        unsigned long long* counters) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  bool counted = false, same = false;
  if (e < num_pairs) {
    const int a = view1[e], b = view2[e];
    if (view_column[a] > -2 && view_column[b] > -2) {
      counted = true;
      double d[3] = {position[3 * (size_t)b] - position[3 * (size_t)a],
                     position[3 * (size_t)b + 1] - position[3 * (size_t)a + 1],
                     position[3 * (size_t)b + 2] - position[3 * (size_t)a + 2]};
      const double n2 = pg::sq3(d[0], d[1], d[2]);
      if (n2 > 0.0) {
        const double n = sqrt(n2);
        d[0] /= n;
        d[1] /= n;
        d[2] /= n;
      }
      const double w[3] = {orientation[3 * (size_t)a], orientation[3 * (size_t)a + 1], orientation[3 * (size_t)a + 2]};
      double q[3];
      rotate_point<false, double>(w, d, q, nullptr, nullptr);
      same = (q[0] * position2[3 * (size_t)e] + q[1] * position2[3 * (size_t)e + 1]) +
                 q[2] * position2[3 * (size_t)e + 2] >
             0.0;
    }
  }
  tb_count(counted && same, &counters[lpos::kVotesFor]);
  tb_count(counted && !same, &counters[lpos::kVotesAgainst]);
}

}  // namespace tmi
