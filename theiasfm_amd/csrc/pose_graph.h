// The device side of what the global pose estimators share (rotation_kernels.h, position_kernels.h,
// position_nonlinear_kernels.h, rotation_nonlinear_kernels.h, rotation_linear_kernels.h): the view table and edge list
// as CSR rows (PoseGraph; pose_graph_host.h builds them, pose_graph_calls.h uploads them), the sums of fixed shape
// (pg::block_sum inside a workgroup, reduce_partials_kernel across the workgroups), the column of a free view and one
// row of the ADMM update.
//
// reduce_partials_kernel     one workgroup per quantity: thread t adds the block parts t, t + 256, ... in ascending
//                            order, then a binary LDS tree -- with the tree inside every block (pg::block_sum) a
//                            reduction of fixed shape, the same bits on every run (as translation_moments_kernel).
//
// The arithmetic written here is never contracted into FMA (#pragma clang fp contract(off) in every body), so a CPU
// model that evaluates the same expressions in the same order sees the same roundings.
#pragma once
#include <hip/hip_runtime.h>

namespace tmi {

constexpr int kRotationMaxJobs = 5;  // quantities of one reduce_partials_kernel launch

// fixed_view = num_views: no view is held and every view has a column (the nonlinear rotation estimator's gauge-free
// problem, and the linear rotation estimator).
struct PoseGraph {
  int num_views;
  int num_pairs;
  int fixed_view;
  const int* pair_view1;     // [E]
  const int* pair_view2;
  const double* edge_value;  // [3 E] TwoViewInfo::rotation_2 (the rotation estimators), the directions in the global
                             // frame (the position estimators); [9 E] the relative rotation matrices, column major
                             // (the linear rotation estimator)
  const int* row_ptr;        // [V + 1] CSR of the undirected graph
  const int2* row;           // [2 E] (neighbour, edge << 1 | (this view is the edge's view2)), ascending edge index
  const int* lap_ptr;        // [n + 1] per column: the entries whose neighbour is free
  const int2* lap_row;       // (neighbour's column, edge), ascending (neighbour, edge)
};

struct ReduceJobs {
  const double* part[kRotationMaxJobs];
  int count[kRotationMaxJobs];
};

namespace pg {

// the sum of v over the 256 threads of the workgroup by a binary tree in LDS; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* part) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  part[tid] = v;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (tid < half) part[tid] += part[tid + half];
    __syncthreads();
  }
  const double total = part[0];
  __syncthreads();  // (part is reused by the next sum)
  return total;
}

__device__ __forceinline__ double sq3(double x, double y, double z) {
#pragma clang fp contract(off)
  return (x * x + y * y) + z * z;
}

// the view of column c
__device__ __forceinline__ int view_of(int c, int fixed) { return c + (c >= fixed); }
// the column of view v (-1: the fixed view)
__device__ __forceinline__ int column_of(int v, int fixed) { return v == fixed ? -1 : v - (v > fixed); }

// One row of the ADMM update (l1_solver.h:147-156, constrained_l1_solver.cc:141-150): b its right-hand side, l1:
// shrinkage by kappa, otherwise max(., 0).
__device__ __forceinline__ void admm_row(double ax, double b, bool l1, double alpha, double kappa, double& z, double& u,
                                         double& dz, double& res) {
#pragma clang fp contract(off)
  double ax_hat = alpha * ax;
  ax_hat += (1.0 - alpha) * (z + b);
  const double v = (ax_hat - b) + u;
  const double znew = l1 ? fmax(0.0, v - kappa) - fmax(0.0, -v - kappa) : fmax(v, 0.0);
  dz = znew - z;
  u = u + ((ax_hat - znew) - b);
  res = (ax - znew) - b;
  z = znew;
}

}  // namespace pg

// blockIdx.x = the quantity: out[q] = the sum of jobs.part[q][0 .. jobs.count[q])
__global__ __launch_bounds__(256) void reduce_partials_kernel(ReduceJobs jobs, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int q = blockIdx.x;
  const double* p = jobs.part[0];
  int count = jobs.count[0];
#pragma unroll
  for (int j = 1; j < kRotationMaxJobs; ++j)  // (selects: a dynamic index into the argument would go to scratch)
    if (q == j) {
      p = jobs.part[j];
      count = jobs.count[j];
    }
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) acc += p[i];
  const double total = pg::block_sum(acc, part);
  if (threadIdx.x == 0) out[q] = total;
}

}  // namespace tmi
