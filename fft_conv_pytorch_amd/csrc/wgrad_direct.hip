// wgrad_direct.hip -- the builds of wgrad_direct_kernel (wgrad_direct.hpp) and of wgrad_direct_dw_kernel
// (wgrad_direct_dw.hpp) and their launches: an object of its own.
#include "wgrad_direct_dw.hpp"

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

// The builds of the depthwise body: taps per block x blocks per wave.  128 taps need at most 7 blocks of 8 taps
// (5 x 5 x 5), 11 of 4 (3 x 42), 16 of 2 and 32 of 1 per wave; a count between two builds takes the larger one, whose
// spare blocks cost registers and no work.
#define FC_DW_BUILDS(X) \
  X(8, 1) X(8, 2) X(8, 4) X(8, 8) X(4, 1) X(4, 4) X(4, 16) X(2, 1) X(2, 4) X(2, 16) X(1, 1) X(1, 4) X(1, 8) X(1, 32)

template <int KXB, int NB>
static hipError_t launch_dw(const WgradDirectArgs& a, long long grid, size_t lds, hipStream_t st) {
  if (a.io == 0) return launch_kernel<wgrad_direct_dw_kernel<IO_F32, KXB, NB>>(grid, kWgdThreads, lds, st, a);
  if (io_is_h16(a.io)) return launch_kernel<wgrad_direct_dw_kernel<IO_H16, KXB, NB>>(grid, kWgdThreads, lds, st, a);
  return hipErrorInvalidValue;
}

int wgrad_direct_dw_blocks(int kxb, int nb) {
  int best = 0;
#define X(K, N) if (kxb == K && nb <= N && (best == 0 || N < best)) best = N;
  FC_DW_BUILDS(X)
#undef X
  return best;
}

hipError_t wgrad_direct_dw_launch(const WgradDirectArgs& a, int kxb, int nb, long long grid, size_t lds, hipStream_t st) {
  if (lds > 160u * 1024u) return hipErrorInvalidValue;
  const int build = wgrad_direct_dw_blocks(kxb, nb);
#define X(K, N) if (kxb == K && build == N) return launch_dw<K, N>(a, grid, lds, st);
  FC_DW_BUILDS(X)
#undef X
  return hipErrorInvalidValue;
}

hipError_t wgrad_direct_sum_launch(const float* partial, float* dw, long long n, int slices, hipStream_t st) {
  return launch_kernel<wgrad_direct_sum_kernel<kWgdSumBlock>>((n + kWgdThreads - 1) / kWgdThreads, kWgdThreads, 0, st, partial, dw, n, slices);
}

}  // namespace fc
