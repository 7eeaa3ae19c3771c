// SampleConsensusEstimator::Estimate (sample_consensus_estimator.h:276-341) for many items at once, as a chunked
// evaluate-then-replay loop (the loop itself is the host's, side_calls.h): the scaffold the batched RANSAC calls share.
// An item is a view (localize_kernels.h) or a view pair (two_view_ransac_kernels.h, two_view_calibrated_kernels.h).  Per
// chunk of iterations three launches, each a template over the problem P:
//
//   ransac_hypothesis_kernel<P>  one thread per (active item, iteration of the chunk): the sample, its correspondences,
//                                P::models: up to P::kSlots models and a flag per slot
//   ransac_score_kernel<P>       one wavefront per (active item, iteration, group of P::kScoreSlots slots): the lanes
//                                stride over the item's correspondences, every correspondence is loaded once and scored
//                                against the group's models, the integer costs come out of a wave reduction of fixed shape
//   ransac_replay_kernel<P>      one thread per active item: Estimate's loop over the chunk's costs in ascending
//                                (iteration, slot) order with a strict < -- best model, max_iterations, the done flag
//
// and ransac_final_inliers<P>, the head of a call's final kernel: the best model's inlier mask and count (:332-341).
//
// A problem P gives: kSample (correspondences per sample), kSlots (models per sample), kModel (doubles per model, at
// most kTwoViewModel), kScoreSlots (slots one wavefront scores per pass over the correspondences; divides kSlots), kPlanes
// (doubles per correspondence), kThreads (hypotheses per workgroup), kSlab (doubles of LDS per hypothesis, element e of
// thread t at lds[e * kThreads + t]; 0: none), and
//   models(pts, slab, models, has)   pts[plane][k] the sampled correspondences; writes models [kSlots kModel] and sets
//                                    has[slot] = 1 for every slot it filled (they arrive cleared)
//   outlier(model, x, thresh)        1 where the correspondence x[plane] is no inlier of the model, else 0
//
// An item's outcome depends only on the ORDER in which its integer costs are replayed, never on the chunk length:
// iterations at or beyond the item's current max_iterations are not evaluated, those evaluated beyond the point where
// the replay stops are discarded.  ComputeMaxIterations is a host-made table over the inlier count (log and pow of the
// host's libm, so that a CPU model gets the same integers).
//
// MLESAC scoring (MLEQualityMeasurement::ComputeCost, solvers/mle_quality_measurement.h:58-71) is a second pair of
// kernels beside the integer ones, for a problem P that also gives residual(model, x), the real residual `outlier` is
// written on:
//
//   ransac_score_mle_kernel<P>   the wavefront of ransac_score_kernel: lane l adds min(r, thresh) of its correspondences
//                                l, l + 64, .. in ascending order from +0.0 and counts those with r < thresh; the 64
//                                partial sums are combined by the xor butterfly with offsets 32, 16, 8, 4, 2, 1 (every
//                                lane ends with the same double: one fixed shape, the same bytes on every run)
//   ransac_replay_mle_kernel<P>  the replay with a double cost (strict <, initially DBL_MAX); the bound is updated from
//                                the INLIER COUNT of the same pass, which under MLE is not the cost
//
// ransac_hypothesis_kernel and ransac_final_inliers serve both scorings.  What the MLE kernels need beyond RansacBatch is
// a struct of its own (RansacMle), passed beside it, so that RansacBatch, RansacState and the integer kernels are what
// they were before MLE existed.
#pragma once
#include <hip/hip_runtime.h>

namespace tmi {

constexpr int kRansacMaxIterations = 1 << 20;
constexpr int kTwoViewModel = 24;  // doubles per two-view model: F row-major, R row-major, position, f1, f2, pad

// Per selected item: what the replay carries from chunk to chunk.
struct RansacState {
  int best_cost;        // INT_MAX: no model yet
  int best_iteration;   // -1
  int best_solution;    // -1; the slot of the best model
  int max_iterations;   // the loop bound, only ever lowered
  int num_iterations;   // iterations replayed
  int done;
  int pad[2];
  double model[kTwoViewModel];  // the best model, P::kModel doubles of it
};

struct RansacBatch {
  int num_selected;
  int max_iterations;             // the options' value: the stride of samples and hypothesis_cost
  int chunk;
  int chunk_start;
  unsigned long long seed;
  // static per call
  const int* sel_item;            // [num_selected] the caller's index of the item (the row of its sample table)
  const unsigned* sel_stream;     // [num_selected] the item's sample stream
  const long long* sel_ptr;       // [num_selected + 1] the item's correspondences in the planes below
  const double* threshold;        // [num_selected]
  const int* samples;             // caller's table [kSample max_iterations num_items], or null
  const int* bound_table;         // ComputeMaxIterations per inlier count: item s, count k at sel_ptr[s] + s + k
  double* plane[5];               // [kPlanes][M] the correspondences, structure of arrays
  // per chunk
  const int* active;              // [num_active] slots still running
  int num_active;
  double* models;                 // [num_active chunk kSlots kModel]
  int* has_model;                 // [num_active chunk kSlots] 0 or 1
  int* cost;                      // [num_active chunk kSlots]
  RansacState* state;             // [num_selected]
  int* hypothesis_cost;           // [num_selected max_iterations kSlots] or null
};

// What the MLE kernels carry beside a RansacBatch.  RansacState::best_cost holds n - inliers of the best model.
struct RansacMle {
  double* cost;                   // [num_active chunk kSlots] per chunk: the MLE cost
  int* inliers;                   // [num_active chunk kSlots] per chunk: the correspondences with r < thresh
  double* best_cost;              // [num_selected] carried from chunk to chunk; DBL_MAX: no model yet
  double* hypothesis_cost;        // [num_selected max_iterations kSlots] or null; preset to NaN by the host
};

// Word c of the splitmix64 stream from state `seed`: the output mix of seed + (c + 1) gamma.
__host__ __device__ __forceinline__ unsigned long long splitmix64_word(unsigned long long seed, unsigned long long c) {
  unsigned long long z = seed + (c + 1ull) * 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// The sample of iteration i of stream p among n >= N correspondences: N swaps of a partial Fisher-Yates on the
// identity, swap k with word N (p 2^32 + i) + k of the stream.  cur[] holds positions 0..N-1, (epos, eval) what the
// swaps put at positions >= N; every index is static.
template <int N>
__host__ __device__ __forceinline__ void ransac_sample(unsigned long long seed, unsigned p, int i, int n, int s[N]) {
#pragma clang fp contract(off)
  int cur[N], epos[N], eval[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    cur[k] = k;
    epos[k] = -1;
    eval[k] = 0;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned long long c = (unsigned long long)N * (((unsigned long long)p << 32) + (unsigned long long)i) + k;
    const double u = ((double)(splitmix64_word(seed, c) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    int j = k + (int)(u * (double)(n - k));
    j = j < n - 1 ? j : n - 1;  // (u < 1, so the product is below n - k; the clamp costs nothing)
    int v = j;
#pragma unroll
    for (int q = 0; q < N; ++q) v = j == q ? cur[q] : v;
#pragma unroll
    for (int m = 0; m < N; ++m)
      if (m < k) v = epos[m] == j ? eval[m] : v;
    const int old = cur[k];
#pragma unroll
    for (int q = 0; q < N; ++q) cur[q] = j == q ? old : cur[q];
    epos[k] = j >= N ? j : -1;
    eval[k] = old;
    cur[k] = v;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = cur[k];
}

#ifdef __HIPCC__
// (register-heavy fp64: a launch of its own, like the ray code of the two-view verification)
template <class P>
__global__ __launch_bounds__(P::kThreads) void ransac_hypothesis_kernel(RansacBatch B) {
  double* slab = nullptr;
  if constexpr (P::kSlab > 0) {
    __shared__ double lds[P::kSlab * P::kThreads];
    slab = lds + threadIdx.x;
  }
  const long long id = (long long)blockIdx.x * P::kThreads + threadIdx.x;
  if (id >= (long long)B.num_active * B.chunk) return;
  const int a = (int)(id / B.chunk), j = (int)(id % B.chunk);
  const int s = B.active[a];
  const int i = B.chunk_start + j;
  int* has = B.has_model + P::kSlots * id;
#pragma unroll
  for (int k = 0; k < P::kSlots; ++k) has[k] = 0;
  if (i >= B.state[s].max_iterations) return;
  const long long o0 = B.sel_ptr[s];
  const int n = (int)(B.sel_ptr[s + 1] - o0);
  int smp[P::kSample];
  if (B.samples) {
    const int* t = B.samples + P::kSample * ((long long)B.max_iterations * B.sel_item[s] + i);
#pragma unroll
    for (int k = 0; k < P::kSample; ++k) smp[k] = t[k];
  } else {
    ransac_sample<P::kSample>(B.seed, B.sel_stream[s], i, n, smp);
  }
  double pts[P::kPlanes][P::kSample];
#pragma unroll
  for (int k = 0; k < P::kSample; ++k) {
    const long long o = o0 + smp[k];
#pragma unroll
    for (int q = 0; q < P::kPlanes; ++q) pts[q][k] = B.plane[q][o];
  }
  P::models(pts, slab, B.models + (long long)P::kSlots * P::kModel * id, has);
}

__device__ __forceinline__ int ransac_wave_sum(int c) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  return c;
}

template <class P>
__global__ __launch_bounds__(256) void ransac_score_kernel(RansacBatch B) {
  constexpr int G = P::kScoreSlots, kGroups = P::kSlots / G;
  static_assert(P::kSlots % G == 0, "kScoreSlots divides kSlots");
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long long id = (long long)blockIdx.x * 4 + wave;  // (active, iteration, group of slots)
  if (id >= (long long)B.num_active * B.chunk * kGroups) return;
  int any = 0;
#pragma unroll
  for (int k = 0; k < G; ++k) any |= B.has_model[G * id + k];
  if (any == 0) return;
  const int s = B.active[(int)(id / ((long long)B.chunk * kGroups))];
  const long long o0 = B.sel_ptr[s];
  const int n = (int)(B.sel_ptr[s + 1] - o0);
  const double thresh = B.threshold[s];
  const double* __restrict__ m = B.models + (long long)P::kModel * G * id;
  int c[G];
#pragma unroll
  for (int k = 0; k < G; ++k) c[k] = 0;
  for (int q = lane; q < n; q += 64) {
    const long long o = o0 + q;
    double x[P::kPlanes];
#pragma unroll
    for (int r = 0; r < P::kPlanes; ++r) x[r] = B.plane[r][o];
#pragma unroll
    for (int k = 0; k < G; ++k) c[k] += P::outlier(m + P::kModel * k, x, thresh);
  }
#pragma unroll
  for (int k = 0; k < G; ++k) c[k] = ransac_wave_sum(c[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < G; ++k) B.cost[G * id + k] = c[k];
  }
}

template <class P>
__global__ __launch_bounds__(64) void ransac_replay_kernel(RansacBatch B) {
  const int a = blockIdx.x * 64 + threadIdx.x;
  if (a >= B.num_active) return;
  const int s = B.active[a];
  RansacState* sp = B.state + s;
  int best_cost = sp->best_cost, best_iteration = sp->best_iteration, best_solution = sp->best_solution;
  int max_iterations = sp->max_iterations, num_iterations = sp->num_iterations;
  const long long o0 = B.sel_ptr[s];
  const int n = (int)(B.sel_ptr[s + 1] - o0);
  const int* __restrict__ bound = B.bound_table + o0 + s;
  long long best_id = -1;
  for (int j = 0; j < B.chunk; ++j) {
    const int i = B.chunk_start + j;
    if (i >= max_iterations) break;
    // the iteration's flags and costs in one round trip each (a slot without a model has an unwritten cost: unused)
    const long long id0 = ((long long)a * B.chunk + j) * P::kSlots;
    int has[P::kSlots], cost[P::kSlots];
#pragma unroll
    for (int k = 0; k < P::kSlots; ++k) has[k] = B.has_model[id0 + k];
#pragma unroll
    for (int k = 0; k < P::kSlots; ++k) cost[k] = B.cost[id0 + k];
#pragma unroll
    for (int k = 0; k < P::kSlots; ++k) {
      const int c = has[k] != 0 ? cost[k] : -1;
      if (has[k] != 0 && c < best_cost) {
        best_cost = c;
        best_iteration = i;
        best_solution = k;
        best_id = id0 + k;
        const int inliers = n - c;
        if (inliers >= P::kSample) {  // (inlier_ratio < kSample / n skips the update of the bound)
          const int m = bound[inliers];
          if (m < max_iterations) max_iterations = m;
        }
      }
      if (B.hypothesis_cost) B.hypothesis_cost[((long long)s * B.max_iterations + i) * P::kSlots + k] = c;
    }
    num_iterations = i + 1;
  }
  sp->best_cost = best_cost;
  sp->best_iteration = best_iteration;
  sp->best_solution = best_solution;
  sp->max_iterations = max_iterations;
  sp->num_iterations = num_iterations;
  if (num_iterations >= max_iterations) sp->done = 1;
  if (best_id >= 0) {
    const double* m = B.models + P::kModel * best_id;
    for (int q = 0; q < P::kModel; ++q) sp->model[q] = m[q];
  }
}

// The head of a final kernel, one wavefront per selected item s: the inlier mask and count of the item's best model.
// Every lane gets the count; -1: there is no model -- the mask is cleared, the count 0 and the status 2.
template <class P>
__device__ __forceinline__ int ransac_final_inliers(const RansacBatch& B, int s, int lane,
                                                    unsigned char* __restrict__ slot_inlier,
                                                    int* __restrict__ num_inliers, signed char* __restrict__ status) {
#pragma clang fp contract(off)
  const RansacState* st = B.state + s;
  const long long o0 = B.sel_ptr[s];
  const int n = (int)(B.sel_ptr[s + 1] - o0);
  if (st->best_iteration < 0) {
    for (int q = lane; q < n; q += 64) slot_inlier[o0 + q] = 0;
    if (lane == 0) {
      num_inliers[s] = 0;
      status[s] = 2;
    }
    return -1;
  }
  const double thresh = B.threshold[s];
  int count = 0;
  for (int q = lane; q < n; q += 64) {
    const long long o = o0 + q;
    double x[P::kPlanes];
#pragma unroll
    for (int r = 0; r < P::kPlanes; ++r) x[r] = B.plane[r][o];
    const int out = P::outlier(st->model, x, thresh);
    slot_inlier[o] = (unsigned char)(1 - out);
    count += 1 - out;
  }
  count = ransac_wave_sum(count);
  if (lane == 0) num_inliers[s] = count;
  return count;
}

// ---- MLESAC scoring ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ransac_wave_sum_real(double c) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c = c + __shfl_xor(c, off, 64);
  return c;
}

template <class P>
__global__ __launch_bounds__(256) void ransac_score_mle_kernel(RansacBatch B, RansacMle E) {
#pragma clang fp contract(off)
  constexpr int G = P::kScoreSlots, kGroups = P::kSlots / G;
  static_assert(P::kSlots % G == 0, "kScoreSlots divides kSlots");
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long long id = (long long)blockIdx.x * 4 + wave;  // (active, iteration, group of slots)
  if (id >= (long long)B.num_active * B.chunk * kGroups) return;
  int any = 0;
#pragma unroll
  for (int k = 0; k < G; ++k) any |= B.has_model[G * id + k];
  if (any == 0) return;
  const int s = B.active[(int)(id / ((long long)B.chunk * kGroups))];
  const long long o0 = B.sel_ptr[s];
  const int n = (int)(B.sel_ptr[s + 1] - o0);
  const double thresh = B.threshold[s];
  const double* __restrict__ m = B.models + (long long)P::kModel * G * id;
  double c[G];
  int in[G];
#pragma unroll
  for (int k = 0; k < G; ++k) {
    c[k] = 0.0;
    in[k] = 0;
  }
  for (int q = lane; q < n; q += 64) {
    const long long o = o0 + q;
    double x[P::kPlanes];
#pragma unroll
    for (int r = 0; r < P::kPlanes; ++r) x[r] = B.plane[r][o];
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const double r = P::residual(m + P::kModel * k, x);
      const bool inlier = r < thresh;  // (a NaN residual is an outlier)
      c[k] = c[k] + (inlier ? r : thresh);
      in[k] += inlier ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < G; ++k) {
    c[k] = ransac_wave_sum_real(c[k]);
    in[k] = ransac_wave_sum(in[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < G; ++k) {
      E.cost[G * id + k] = c[k];
      E.inliers[G * id + k] = in[k];
    }
  }
}

template <class P>
__global__ __launch_bounds__(64) void ransac_replay_mle_kernel(RansacBatch B, RansacMle E) {
  const int a = blockIdx.x * 64 + threadIdx.x;
  if (a >= B.num_active) return;
  const int s = B.active[a];
  RansacState* sp = B.state + s;
  double best_cost = E.best_cost[s];
  int best_outliers = sp->best_cost, best_iteration = sp->best_iteration, best_solution = sp->best_solution;
  int max_iterations = sp->max_iterations, num_iterations = sp->num_iterations;
  const long long o0 = B.sel_ptr[s];
  const int n = (int)(B.sel_ptr[s + 1] - o0);
  const int* __restrict__ bound = B.bound_table + o0 + s;
  long long best_id = -1;
  for (int j = 0; j < B.chunk; ++j) {
    const int i = B.chunk_start + j;
    if (i >= max_iterations) break;
    const long long id0 = ((long long)a * B.chunk + j) * P::kSlots;
#pragma unroll
    for (int k = 0; k < P::kSlots; ++k) {
      const long long h = ((long long)s * B.max_iterations + i) * P::kSlots + k;
      if (B.has_model[id0 + k] != 0) {
        const double c = E.cost[id0 + k];
        const int inliers = E.inliers[id0 + k];
        if (c < best_cost) {
          best_cost = c;
          best_outliers = n - inliers;
          best_iteration = i;
          best_solution = k;
          best_id = id0 + k;
          if (inliers >= P::kSample) {  // (inlier_ratio < kSample / n skips the update of the bound)
            const int m = bound[inliers];
            if (m < max_iterations) max_iterations = m;
          }
        }
        if (B.hypothesis_cost) B.hypothesis_cost[h] = n - inliers;
        if (E.hypothesis_cost) E.hypothesis_cost[h] = c;
      } else if (B.hypothesis_cost) {
        B.hypothesis_cost[h] = -1;
      }
    }
    num_iterations = i + 1;
  }
  E.best_cost[s] = best_cost;
  sp->best_cost = best_outliers;
  sp->best_iteration = best_iteration;
  sp->best_solution = best_solution;
  sp->max_iterations = max_iterations;
  sp->num_iterations = num_iterations;
  if (num_iterations >= max_iterations) sp->done = 1;
  if (best_id >= 0) {
    const double* m = B.models + P::kModel * best_id;
    for (int q = 0; q < P::kModel; ++q) sp->model[q] = m[q];
  }
}
#endif  // __HIPCC__

}  // namespace tmi
