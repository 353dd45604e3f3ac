// wgrad_direct_h16.hip -- the builds of wgrad_direct_h16_kernel (wgrad_direct_h16.hpp) and their launch: an object of its own.
#include "wgrad_direct_h16.hpp"

#include "launch.hpp"

namespace fc {

template <int CT>
static hipError_t launch_ct(const WgradH16Args& a, long long grid, size_t lds, hipStream_t st) {
  if (a.io == IO_CODE_BF16) return launch_kernel<wgrad_direct_h16_kernel<true, CT>>(grid, kWgdThreads, lds, st, a);
  if (a.io == IO_CODE_F16) return launch_kernel<wgrad_direct_h16_kernel<false, CT>>(grid, kWgdThreads, lds, st, a);
  return hipErrorInvalidValue;
}

hipError_t wgrad_direct_h16_launch(const WgradH16Args& a, int ct, long long grid, size_t lds, hipStream_t st) {
  if (lds > 160u * 1024u || a.RX < 1 || a.RX > kWghMaxRX || a.rows4 * a.RX > kWghMaxRuns || (a.SP & 7) || (a.rows4 & 3))
    return hipErrorInvalidValue;
  switch (ct) {
    case 1: return launch_ct<1>(a, grid, lds, st);
    case 2: return launch_ct<2>(a, grid, lds, st);
    case 4: return launch_ct<4>(a, grid, lds, st);
    case 8: return launch_ct<8>(a, grid, lds, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace fc
