// wgrad_direct.hip -- the builds of wgrad_direct_kernel (wgrad_direct.hpp) and their launches: an object of its own.
#include "wgrad_direct.hpp"

#include "launch.hpp"

namespace fc {

template <int CT>
static hipError_t launch_ct(const WgradDirectArgs& a, long long grid, size_t lds, hipStream_t st) {
  if (a.io == 0) return launch_kernel<wgrad_direct_kernel<IO_F32, CT>>(grid, kWgdThreads, lds, st, a);
  if (io_is_h16(a.io)) return launch_kernel<wgrad_direct_kernel<IO_H16, CT>>(grid, kWgdThreads, lds, st, a);
  return hipErrorInvalidValue;
}

hipError_t wgrad_direct_launch(const WgradDirectArgs& a, int ct, long long grid, size_t lds, hipStream_t st) {
  if (lds > 160u * 1024u) return hipErrorInvalidValue;
  switch (ct) {
    case 1: return launch_ct<1>(a, grid, lds, st);
    case 2: return launch_ct<2>(a, grid, lds, st);
    case 4: return launch_ct<4>(a, grid, lds, st);
    case 8: return launch_ct<8>(a, grid, lds, st);
  }
  return hipErrorInvalidValue;
}

hipError_t wgrad_direct_sum_launch(const float* partial, float* dw, long long n, int slices, hipStream_t st) {
  return launch_kernel<wgrad_direct_sum_kernel<kWgdSumBlock>>((n + kWgdThreads - 1) / kWgdThreads, kWgdThreads, 0, st, partial, dw, n, slices);
}

}  // namespace fc
