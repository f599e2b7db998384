// A kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize), raised before its first
// launch: once per kernel and process.
#pragma once

#include <hip/hip_runtime.h>

// K: the kernel (one cached result per instantiation).  bytes: the most K is ever launched with.
template <auto K>
hipError_t dynamic_lds_once(int bytes) {
  static const hipError_t r =
      hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return r;
}

// K<<<grid, block, lds, st>>>(args...) behind dynamic_lds_once; returns hipGetLastError() (a failed
// attribute shows there as the launch's error)
template <auto K, class... Args>
int launch_dynamic_lds(int grid, int block, int lds, hipStream_t st, const Args&... args) {
  if (lds) (void)dynamic_lds_once<K>(lds);
  K<<<grid, block, lds, st>>>(args...);
  return (int)hipGetLastError();
}
