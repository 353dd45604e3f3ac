// conv_direct_tr.hip -- the builds of conv_direct_tr_kernel (conv_direct_tr.hpp) and their launch: an object of its own.
#include "conv_direct_tr.hpp"

#include "launch.hpp"

namespace fc {

template <int PH, int NPT>
static hipError_t launch_build(const ConvDirectTrArgs& a, long long grid, size_t lds, hipStream_t st) {
  if (a.io == 0) return launch_kernel<conv_direct_tr_kernel<IO_F32, PH, NPT>>(grid, kCdThreads, lds, st, a);
  if (io_is_h16(a.io)) return launch_kernel<conv_direct_tr_kernel<IO_H16, PH, NPT>>(grid, kCdThreads, lds, st, a);
  return hipErrorInvalidValue;
}

hipError_t conv_direct_tr_launch(const ConvDirectTrArgs& a, int ph, int npt, long long grid, size_t lds, hipStream_t st) {
  if (lds > 160u * 1024u) return hipErrorInvalidValue;
  switch (ph * 100 + npt) {
    case 201: return launch_build<2, 1>(a, grid, lds, st);
    case 202: return launch_build<2, 2>(a, grid, lds, st);
    case 204: return launch_build<2, 4>(a, grid, lds, st);
    case 208: return launch_build<2, 8>(a, grid, lds, st);
    case 401: return launch_build<4, 1>(a, grid, lds, st);
    case 402: return launch_build<4, 2>(a, grid, lds, st);
    case 404: return launch_build<4, 4>(a, grid, lds, st);
    case 801: return launch_build<8, 1>(a, grid, lds, st);
    case 802: return launch_build<8, 2>(a, grid, lds, st);
    case 1601: return launch_build<16, 1>(a, grid, lds, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace fc
