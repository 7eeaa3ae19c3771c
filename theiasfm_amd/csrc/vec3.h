// Three-vectors in a fixed order of operations, never contracted into FMA: what the minimal solvers share.
#pragma once
#include <hip/hip_runtime.h>

namespace tmi {

__host__ __device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ __forceinline__ double dot3(const double a[3], const double b[3]) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
__host__ __device__ __forceinline__ void normalize3(double a[3]) {
#pragma clang fp contract(off)
  const double n = sqrt(dot3(a, a));
  a[0] = a[0] / n;
  a[1] = a[1] / n;
  a[2] = a[2] / n;
}

}  // namespace tmi
