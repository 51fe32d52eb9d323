// launch.h -- the one way a kernel that needs more than the default dynamic LDS is launched.
#pragma once
#include "common.h"
#include "dispatch.h"
#include "prof.h"

namespace gdf_amd {

// raises the kernel's dynamic-LDS limit to `lds` bytes and nothing else (a kernel launched later, or by a loop of rounds)
template <class... KArgs>
static inline gdf_error allow_lds(void (*kernel)(KArgs...), size_t lds) {
  HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return GDF_SUCCESS;
}

// allow_lds, then the launch on stream0() under `name` for the profiler (GDF_LAUNCH).  The arguments are converted to the kernel's
// parameter types by the launch itself.  No hipGetLastError(): the caller's HIP_CHECK_LAST() stays where it is.
template <class... KArgs, class... Args>
static inline gdf_error launch_lds(const char *name, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, Args &&...args) {
  GDF_TRY(allow_lds(kernel, lds));
  GDF_LAUNCH(name, kernel, grid, block, lds, stream0(), args...);
  return GDF_SUCCESS;
}

}  // namespace gdf_amd
