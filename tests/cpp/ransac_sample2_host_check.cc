// The sampler of the batched RANSAC calls (theiasfm_amd/csrc/ransac_core.h) with a sample of two, on the host: the
// kernels' own __host__ __device__ text, so that tests/test_known_orientation_cpu.py can compare it with the sample
// function of tests/known_orientation_model.py and run it under the host's sanitizers.  Compiled as HIP for the host
// only; no device is touched.
//
// stdin: one case per line, "seed stream i n" in decimal.
// stdout: per case the two indices of the sample.
#include <cstdio>

#include "ransac_core.h"

int main() {
  int i, n, cases = 0;
  unsigned long long seed;
  unsigned stream;
  while (std::scanf("%llu %u %d %d", &seed, &stream, &i, &n) == 4) {
    int s[2];
    tmi::ransac_sample<2>(seed, stream, i, n, s);
    std::printf("%d %d\n", s[0], s[1]);
    ++cases;
  }
  std::fprintf(stderr, "ransac sample of two host check: %d cases\n", cases);
  return 0;
}
