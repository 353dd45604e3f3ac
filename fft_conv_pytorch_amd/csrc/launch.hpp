// launch.hpp -- the one place a kernel is launched from (host code only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace fc {

// Launches Kernel on `grid` workgroups of `threads` threads with `lds` bytes of dynamic LDS.
//
// More than 64 KiB of dynamic LDS needs an opt-in (gfx950: 160 KiB per workgroup).  It is made once per kernel AND
// device, with the full 160 KiB, so that nothing but the launch happens on later calls (launches may be under
// HIP-graph capture).  The attribute belongs to the function on the current device, so the "done" state is a bit per
// device ordinal (ordinals from 64 on opt in on every call).  The mask is a static of this template, i.e. one per
// kernel by construction, and atomic because plans are shared between threads (a duplicate hipFuncSetAttribute from two
// racing first calls is harmless).
template <auto Kernel, class... Args>
hipError_t launch_kernel(long long grid, unsigned threads, size_t lds, hipStream_t st, const Args&... args) {
  if (grid <= 0 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    static std::atomic<unsigned long long> opted{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool tracked = dev >= 0 && dev < 64;
    if (!tracked || !(opted.load(std::memory_order_acquire) >> dev & 1ull)) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) return e;
      if (tracked) opted.fetch_or(1ull << dev, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(threads), lds, st, args...);
  return hipGetLastError();
}

}  // namespace fc
