// The sampler of the batched RANSAC calls (theiasfm_amd/csrc/ransac_core.h) on the host: the kernels' own
// __host__ __device__ text, so that tests/test_ransac_core_cpu.py can compare it with the sample function of each
// numpy model and run it under the host's sanitizers.  Compiled as HIP for the host only; no device is touched.
//
// stdin: one case per line, "N seed stream i n" in decimal (N is 3, 5 or 8).
// stdout: per case the N indices of the sample.
#include <cstdio>

#include "ransac_core.h"

template <int N>
static void print_sample(unsigned long long seed, unsigned stream, int i, int n) {
  int s[N];
  tmi::ransac_sample<N>(seed, stream, i, n, s);
  for (int k = 0; k < N; ++k) std::printf("%d%c", s[k], k + 1 < N ? ' ' : '\n');
}

int main() {
  int N, i, n, cases = 0;
  unsigned long long seed;
  unsigned stream;
  while (std::scanf("%d %llu %u %d %d", &N, &seed, &stream, &i, &n) == 5) {
    switch (N) {
      case 3: print_sample<3>(seed, stream, i, n); break;
      case 5: print_sample<5>(seed, stream, i, n); break;
      case 8: print_sample<8>(seed, stream, i, n); break;
      default: return 2;
    }
    ++cases;
  }
  std::fprintf(stderr, "ransac sample host check: %d cases\n", cases);
  return 0;
}
