// Which error the finish of a one-shot call reports (ReadBack, one_shot.h): the last launch's before the copies' before
// the synchronise's; hipSuccess only if all three are.  Nothing of the HIP runtime but the enum, so that
// tests/cpp/read_back_error_check.cc runs it on the host.
#pragma once

inline hipError_t read_back_error(hipError_t launch, hipError_t copy, hipError_t sync) {
  if (launch != hipSuccess) return launch;
  if (copy != hipSuccess) return copy;
  return sync;
}
