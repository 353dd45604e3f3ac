// conv_direct_tr_h16.hip -- the builds of conv_direct_tr_h16_kernel (conv_direct_tr_h16.hpp) and their launch: an object
// of its own.
#include "conv_direct_tr_h16.hpp"

#include <algorithm>

#include "launch.hpp"

namespace fc {

template <int PH, int NPT>
static hipError_t launch_build(const ConvDirectTrArgs& a, long long grid, size_t lds, hipStream_t st) {
  if (a.io == IO_CODE_BF16) return launch_kernel<conv_direct_tr_h16_kernel<true, PH, NPT>>(grid, kCdThreads, lds, st, a);
  if (a.io == IO_CODE_F16) return launch_kernel<conv_direct_tr_h16_kernel<false, PH, NPT>>(grid, kCdThreads, lds, st, a);
  return hipErrorInvalidValue;
}

hipError_t conv_direct_tr_h16_launch(const ConvDirectTrArgs& a, int ph, int npt, long long grid, size_t lds, hipStream_t st) {
  if (lds > 160u * 1024u || a.cib % kH16Cell || a.ppp < 1 || a.ppp > ph) return hipErrorInvalidValue;
  for (int f0 = 0; f0 < a.phases; f0 += a.ppp)      // the weights of a pass are what a thread carries
    if (a.soff[std::min(f0 + a.ppp, a.phases)] - a.soff[f0] > kTrH16MaxSteps) return hipErrorInvalidValue;
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
