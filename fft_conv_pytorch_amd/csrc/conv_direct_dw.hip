// conv_direct_dw.hip -- the builds of conv_direct_dw_kernel (conv_direct_dw.hpp) and their launch: an object of its own.
#include "conv_direct_dw.hpp"

#include "launch.hpp"

namespace fc {

// The builds: taps per block x (multiplier slots, runs per thread), forward; taps per block, transposed: 15, each in
// float32 and 16-bit.  A multiplier between two builds (3, 5, 6, 7) takes the larger one, whose spare slots multiply
// staged zeros into sums that are not stored.
#define FC_CDW_SLOTS(X, K) X(K, 1, 8, false) X(K, 2, 4, false) X(K, 4, 2, false) X(K, 8, 1, false) X(K, 1, 8, true)
#define FC_CDW_BUILDS(X) FC_CDW_SLOTS(X, 1) FC_CDW_SLOTS(X, 4) FC_CDW_SLOTS(X, 8)

template <int KXB, int M, int NR, bool TR>
static hipError_t launch_cdw(const ConvDirectDwArgs& a, long long grid, size_t lds, hipStream_t st) {
  if (a.io == 0) return launch_kernel<conv_direct_dw_kernel<IO_F32, KXB, M, NR, TR>>(grid, kCdwThreads, lds, st, a);
  if (io_is_h16(a.io)) return launch_kernel<conv_direct_dw_kernel<IO_H16, KXB, M, NR, TR>>(grid, kCdwThreads, lds, st, a);
  return hipErrorInvalidValue;
}

int conv_direct_dw_slots(int m, int transposed) {
  if (m < 1 || m > kCdwMaxMultiplier) return 0;
  return transposed || m == 1 ? 1 : m == 2 ? 2 : m <= 4 ? 4 : 8;
}

hipError_t conv_direct_dw_launch(const ConvDirectDwArgs& a, int kxb, int transposed, long long grid, size_t lds, hipStream_t st) {
  if (lds > 160u * 1024u) return hipErrorInvalidValue;
  const int slots = conv_direct_dw_slots(a.m, transposed);
  if (!slots || a.runs > kCdwThreads * (kCdwAcc / slots)) return hipErrorInvalidValue;
#define X(K, M, NR, TR) if (kxb == K && slots == M && (transposed != 0) == TR) return launch_cdw<K, M, NR, TR>(a, grid, lds, st);
  FC_CDW_BUILDS(X)
#undef X
  return hipErrorInvalidValue;
}

}  // namespace fc
