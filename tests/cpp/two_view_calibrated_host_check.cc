// Steps 3 and 4 of tmi_ba_estimate_calibrated_relative_poses (theiasfm_amd/csrc/two_view_calibrated_kernels.h) on the
// host: the kernels' own __host__ __device__ text with a slab of stride 1, so that tests/test_two_view_calibrated_cpu.py
// can compare its bits with the numpy model's closed path and run it under the host's sanitizers.  Compiled as HIP for
// the host only; no device is touched.
//
// stdin: one sample per line, 20 hexadecimal doubles (x1[5] y1[5] x2[5] y2[5]).
// stdout: per sample "count", then count lines of 21 hexadecimal doubles (E row-major, R row-major, position).
#include <cstdio>
#include <vector>

#include "two_view_calibrated_kernels.h"

int main() {
  std::vector<double> slab(tmi::kCalibSlab), models(tmi::kCalibSlots * tmi::kTwoViewModel);
  double v[20];
  int samples = 0;
  for (;;) {
    int got = 0;
    for (; got < 20; ++got)
      if (std::scanf("%la", &v[got]) != 1) break;
    if (got == 0) break;
    if (got != 20) return 2;
    for (double& s : slab) s = 0.0;
    const int count = tmi::calib_models<1>(v, v + 5, v + 10, v + 15, slab.data(), models.data());
    std::printf("%d\n", count);
    for (int k = 0; k < count; ++k) {
      for (int q = 0; q < 21; ++q) std::printf("%a ", models[tmi::kTwoViewModel * k + q]);
      std::printf("\n");
    }
    ++samples;
  }
  std::fprintf(stderr, "two-view calibrated host check: %d samples\n", samples);
  return 0;
}
