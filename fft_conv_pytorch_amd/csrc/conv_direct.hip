// conv_direct.hip -- the builds of conv_direct_kernel (conv_direct.hpp) and their launch: an object of its own.
#include "conv_direct.hpp"

#include "launch.hpp"

namespace fc {

template <int NPT>
static hipError_t launch_npt(const ConvDirectArgs& a, long long grid, size_t lds, hipStream_t st) {
  if (a.io == 0) return launch_kernel<conv_direct_kernel<IO_F32, NPT>>(grid, kCdThreads, lds, st, a);
  if (io_is_h16(a.io)) return launch_kernel<conv_direct_kernel<IO_H16, NPT>>(grid, kCdThreads, lds, st, a);
  return hipErrorInvalidValue;
}

hipError_t conv_direct_launch(const ConvDirectArgs& a, int npt, long long grid, size_t lds, hipStream_t st) {
  if (lds > 160u * 1024u) return hipErrorInvalidValue;
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
