// conv_direct_h16.hip -- the builds of conv_direct_h16_kernel (conv_direct_h16.hpp) and their launch: an object of its own.
#include "conv_direct_h16.hpp"

#include "launch.hpp"

namespace fc {

template <int NPT>
static hipError_t launch_npt(const ConvDirectArgs& a, long long grid, size_t lds, hipStream_t st) {
  if (a.io == IO_CODE_BF16) return launch_kernel<conv_direct_h16_kernel<true, NPT>>(grid, kCdThreads, lds, st, a);
  if (a.io == IO_CODE_F16) return launch_kernel<conv_direct_h16_kernel<false, NPT>>(grid, kCdThreads, lds, st, a);
  return hipErrorInvalidValue;
}

hipError_t conv_direct_h16_launch(const ConvDirectArgs& a, int npt, long long grid, size_t lds, hipStream_t st) {
  if (lds > 160u * 1024u || a.steps > kH16MaxSteps || a.cib % kH16Cell) return hipErrorInvalidValue;
  switch (npt) {
    case 1: return launch_npt<1>(a, grid, lds, st);
    case 2: return launch_npt<2>(a, grid, lds, st);
    case 4: return launch_npt<4>(a, grid, lds, st);
    case 8: return launch_npt<8>(a, grid, lds, st);
    case 16: return launch_npt<16>(a, grid, lds, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace fc
