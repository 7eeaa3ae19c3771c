// Which error the finish of a one-shot call reports (theiasfm_amd/csrc/read_back_error.h) on its own, for
// tests/test_read_back_error_cpu.py.  Compiled as HIP for the host only; of the runtime it needs the enum alone and no
// device is touched.
//
// stdout: one line "<launch> <copy> <sync> <reported>" per combination of ok / failed, where a failed launch, copy and
// synchronise carry three different errors and every word is one of ok, launch, copy, sync.
#include <cstdio>

#include <hip/hip_runtime_api.h>

#include "read_back_error.h"

int main() {
  const hipError_t failed[3] = {hipErrorLaunchFailure, hipErrorInvalidValue, hipErrorIllegalAddress};
  const char* const name[3] = {"launch", "copy", "sync"};
  auto word = [&](hipError_t e) {
    for (int k = 0; k < 3; ++k)
      if (e == failed[k]) return name[k];
    return e == hipSuccess ? "ok" : "other";
  };
  for (int bits = 0; bits < 8; ++bits) {
    hipError_t e[3];
    for (int k = 0; k < 3; ++k) e[k] = (bits >> k & 1) ? failed[k] : hipSuccess;
    std::printf("%s %s %s %s\n", word(e[0]), word(e[1]), word(e[2]), word(read_back_error(e[0], e[1], e[2])));
  }
  return 0;
}
