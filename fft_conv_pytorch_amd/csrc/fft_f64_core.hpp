// fft_f64_core.hpp -- the double-precision LDS transform shared by the float64 1-D kernels (fft_f64.hip: overlap-save
// tiles; long_f64.hip: one long transform in three passes).  Device code only; everything here inlines into its caller.
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

__device__ __forceinline__ double2 cmul_d(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}

// Stockham radix-2, T points, T/2 threads, natural order in (buffer `a`) and out (returned pointer: a or b).
// DIR = -1 forward, +1 inverse (unnormalised).  tw[k] = exp(-2 pi i k / T), k < T/2.
// Several sequences of the same length may run side by side in one workgroup, each with buffers of its own and all
// with one table: every thread of the workgroup meets the same barriers, and the returned buffer is the same one (a or
// b) for all of them.
template <int DIR>
__device__ __forceinline__ double2* fft_stockham(double2* a, double2* b, const double2* tw, int T, int t) {
  const int half = T >> 1;
  for (int ns = 1; ns < T; ns <<= 1) {
    const int k = t & (ns - 1);
    const double2 u = a[t];
    double2 v = a[t + half];
    double2 w = tw[k * (half / ns)];
    if (DIR > 0) w.y = -w.y;
    v = cmul_d(v, w);
    const int j = ((t - k) << 1) + k;
    b[j] = make_double2(u.x + v.x, u.y + v.y);
    b[j + ns] = make_double2(u.x - v.x, u.y - v.y);
    __syncthreads();
    double2* s = a; a = b; b = s;
  }
  return a;
}

__device__ __forceinline__ void build_table(double2* tw, int T, int t) {
  double s, c;
  sincospi(-2.0 * (double)t / (double)T, &s, &c);
  tw[t] = make_double2(c, s);
}

}  // namespace fc
