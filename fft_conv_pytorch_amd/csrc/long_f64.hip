// long_f64.hip -- float64 1-D convolution with a kernel longer than the 2048-point tile of fft_f64.hip takes: one cyclic
// transform of N = N1 * N2 points per row, run as two workgroup transforms with a trip through HBM between them.  The
// scheme is that of long1d.hpp; the arithmetic is plain double, the transform the Stockham one of
// fft_f64.hip (fft_f64_core.hpp), the index maps those of axis_map.hpp.
//
// The row is indexed n = n1*N2 + n2 and its bins k = k1 + N1*k2:
//
//   X[k1 + N1*k2] = sum_n2 w_N2^(n2*k2) * ( w_N^(n2*k1) * sum_n1 w_N1^(n1*k1) * x[n1*N2 + n2] )
//
//   cols_fwd   N1-point transforms along n1 (stride N2 in memory) of a block of neighbouring n2 columns, the twiddle
//              w_N^(n2*k1), W1[row][k1][n2].  Two real rows (batch items 2p and 2p+1 of one channel) ride one complex row,
//              z = x[2p] + i*x[2p+1]; the last item of an odd batch rides with zeros.  The signal is gathered through its
//              AxisMap (padding mode, left offset, the spread of a transposed plan) from the tile's first padded position;
//              the same kernel gathers the filter rows (dilated; flipped, channels exchanged for a transposed plan).
//   rows       one k1 row of N2 contiguous points: forward transform, product with H[o][i][k1][k2] summed over the input
//              channels of the group (up to 8 output channels' sums in registers), inverse transform, conjugate twiddle,
//              W2[row][k1][n2].  In its filter mode it stops after the forward half and stores conj(.) / N.
//   cols_inv   inverse N1-point transforms along k1, bias, real part -> y[2p], imaginary part -> y[2p+1]; point t of the
//              tile is sample t0 + t of the stride-1 result, stored at y[(t0 + t) / stride] where that divides and t lies
//              in the tile's window: every kept sample is written exactly once.
//
// The filter is real, so its full N-bin spectrum multiplies the complex row and the two real rows come apart as the real
// and imaginary parts of the result: there is no Hermitian untangling.  The bins stay in the order [k1][k2] on both
// operands, so the product needs no transposition.  The twiddle w_N^m comes from sincospi(2 m / N) per point: m / N is
// exact in double for every m < N <= 2^22, so it is the correctly reduced float64 value to the last ulp or two of
// sincospi, with no table.
#include <hip/hip_runtime.h>

#include "axis_map.hpp"
#include "fft_f64_core.hpp"
#include "launch.hpp"
#include "long_f64.h"

namespace fc {
namespace {

__device__ __forceinline__ int ilog2(int v) { return 31 - __clz(v); }

// w_N^(sign * m), m < N
__device__ __forceinline__ double2 long_twiddle_d(int m, double inv_n, double sign) {
  double s, c;
  sincospi(sign * 2.0 * (double)m * inv_n, &s, &c);
  return make_double2(c, s);
}

// ---- cols_fwd: workgroup = (row, block of NC neighbouring n2 columns); NC * N1/2 threads
__global__ __launch_bounds__(1024) void long_f64_cols_fwd_kernel(const LongF64Args a, const int NC) {
  extern __shared__ __attribute__((aligned(16))) double2 lds64[];
  const int N1 = a.N1, half = N1 >> 1, CS = 2 * N1 + 1, lgNC = ilog2(NC);
  double2* tw = lds64 + NC * CS;
  const int tid = threadIdx.x, NT = NC * half;
  const unsigned nblk = (unsigned)(a.N2 >> lgNC);
  const unsigned row = blockIdx.x / nblk;
  const int n20 = (int)(blockIdx.x - row * nblk) << lgNC;
  const size_t N = (size_t)N1 << a.lgN2;
  if (tid < half) build_table(tw, N1, tid);
  // lanes run over the NC neighbouring columns first, so that reads (and the stores of W1 below) run along memory
  if (a.from_kernel) {
    // transposed: the weight is (Cin, Cout/g, K) and H[g][o][i] holds the taps of w[g*Cig + i][o] back to front
    const int oi = a.row0 + (int)row;
    const int i_ = oi % a.Cig, go = oi / a.Cig;
    const double* wrow = a.src + (size_t)(a.transposed ? ((go / a.Cog) * a.Cig + i_) * a.Cog + go % a.Cog : oi) * a.K;
    const int kd = (a.K - 1) * a.dil + 1;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + u * NT, c = idx & (NC - 1), n1 = idx >> lgNC;
      const int n = (n1 << a.lgN2) + n20 + c;
      const int pp = a.transposed ? kd - 1 - n : n;
      const int tap = pp >= 0 ? tap_src(pp, a.dil, a.K) : -1;
      lds64[c * CS + n1] = make_double2(tap >= 0 ? wrow[tap] : 0.0, 0.0);
    }
  } else {
    const unsigned pr = row / (unsigned)a.C, ch = row - pr * (unsigned)a.C;
    const int b0 = 2 * (a.pair0 + (int)pr);
    const bool has1 = b0 + 1 < a.B;
    const double* xa = a.src + ((size_t)b0 * a.C + ch) * a.L;
    const double* xb = xa + (size_t)a.C * a.L;
    const AxisMap map{a.L, a.pad, a.pad_mode, a.up};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + u * NT, c = idx & (NC - 1), n1 = idx >> lgNC;
      const int q = axis_src(map, a.p0 + (n1 << a.lgN2) + n20 + c);
      lds64[c * CS + n1] = make_double2(q >= 0 ? xa[q] : 0.0, (q >= 0 && has1) ? xb[q] : 0.0);
    }
  }
  __syncthreads();
  const int sq = tid / half, t = tid - sq * half;
  double2* seq = lds64 + sq * CS;
  const int roff = (int)(fft_stockham<-1>(seq, seq + N1, tw, N1, t) - seq);
  const double inv_n = 1.0 / (double)N;
  double2* out = a.w1 + (size_t)row * N;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int idx = tid + u * NT, c = idx & (NC - 1), k1 = idx >> lgNC;
    const int n2 = n20 + c;
    const double2 w = long_twiddle_d(n2 * k1, inv_n, -1.0);
    out[((size_t)k1 << a.lgN2) + n2] = cmul_d(lds64[c * CS + roff + k1], w);
  }
}

// ---- rows: workgroup = (pair, group, out-chunk, block of NR neighbouring k1 rows), or (filter row, block) in the filter
// mode; NR * N2/2 threads
__global__ __launch_bounds__(1024) void long_f64_rows_kernel(const LongF64Args a, const int NR) {
  extern __shared__ __attribute__((aligned(16))) double2 lds64[];
  const int N2 = a.N2, half = N2 >> 1;
  const int tid = threadIdx.x, sq = tid / half, t = tid - sq * half;
  double2* bufA = lds64 + sq * 2 * N2;
  double2* bufB = bufA + N2;
  double2* tw = lds64 + NR * 2 * N2;
  const unsigned nkb = (unsigned)(a.N1 / NR);
  unsigned id = blockIdx.x / nkb;
  const int k1 = (int)(blockIdx.x - id * nkb) * NR + sq;
  const size_t N = (size_t)a.N1 << a.lgN2;
  const size_t koff = (size_t)k1 << a.lgN2;           // this k1 row inside a row of N points
  if (tid < half) build_table(tw, N2, tid);

  if (a.spec_mode) {
    // filter row `id` of this launch: transform, conjugate (cross-correlation, like rfft(kernel).conj()), 1/N
    const double2* src = a.w1 + (size_t)id * N + koff;
    bufA[t] = src[t];
    bufA[t + half] = src[t + half];
    __syncthreads();
    const double2* r = fft_stockham<-1>(bufA, bufB, tw, N2, t);
    double2* out = a.spec_out + (size_t)id * N + koff;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int f = t + h * half;
      out[f] = make_double2(r[f].x * a.scale, -r[f].y * a.scale);
    }
    return;
  }

  const int oc = (int)(id % (unsigned)a.n_ochunks); id /= (unsigned)a.n_ochunks;
  const int g = (int)(id % (unsigned)a.G);
  const size_t pr = id / (unsigned)a.G;
  const int Cin = a.G * a.Cig, Cout = a.G * a.Cog;
  const int nout = min(a.cob, a.Cog - oc * a.cob);
  double2 acc[8][2];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o][0] = acc[o][1] = make_double2(0.0, 0.0);
  for (int i = 0; i < a.Cig; ++i) {
    const double2* src = a.w1 + (pr * Cin + (size_t)g * a.Cig + i) * N + koff;
    __syncthreads();                                   // (table built / previous channel's spectrum consumed)
    bufA[t] = src[t];
    bufA[t + half] = src[t + half];
    __syncthreads();
    const double2* Z = fft_stockham<-1>(bufA, bufB, tw, N2, t);
    const double2 z0 = Z[t], z1 = Z[t + half];
    const double2* hrow = a.spec + (((size_t)g * a.Cog + (size_t)oc * a.cob) * a.Cig + i) * N + koff;
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < nout) {
        const double2* hp = hrow + (size_t)o * a.Cig * N;
        const double2 p0 = cmul_d(z0, hp[t]), p1 = cmul_d(z1, hp[t + half]);
        acc[o][0].x += p0.x; acc[o][0].y += p0.y;
        acc[o][1].x += p1.x; acc[o][1].y += p1.y;
      }
  }
  const double inv_n = 1.0 / (double)N;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    if (o >= nout) break;                              // uniform
    __syncthreads();
    bufA[t] = acc[o][0];
    bufA[t + half] = acc[o][1];
    __syncthreads();
    const double2* Y = fft_stockham<+1>(bufA, bufB, tw, N2, t);
    double2* dst = a.w2 + (pr * Cout + (size_t)g * a.Cog + (size_t)oc * a.cob + o) * N + koff;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n2 = t + h * half;
      dst[n2] = cmul_d(Y[n2], long_twiddle_d(n2 * k1, inv_n, 1.0));
    }
  }
}

// ---- cols_inv: workgroup = (row, block of NC neighbouring n2 columns); NC * N1/2 threads
__global__ __launch_bounds__(1024) void long_f64_cols_inv_kernel(const LongF64Args a, const int NC) {
  extern __shared__ __attribute__((aligned(16))) double2 lds64[];
  const int N1 = a.N1, half = N1 >> 1, CS = 2 * N1 + 1, lgNC = ilog2(NC);
  double2* tw = lds64 + NC * CS;
  const int tid = threadIdx.x, NT = NC * half;
  const unsigned nblk = (unsigned)(a.N2 >> lgNC);
  const unsigned row = blockIdx.x / nblk;
  const int n20 = (int)(blockIdx.x - row * nblk) << lgNC;
  const size_t N = (size_t)N1 << a.lgN2;
  if (tid < half) build_table(tw, N1, tid);
  const double2* src = a.w2 + (size_t)row * N;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int idx = tid + u * NT, c = idx & (NC - 1), k1 = idx >> lgNC;
    lds64[c * CS + k1] = src[((size_t)k1 << a.lgN2) + n20 + c];
  }
  __syncthreads();
  const int sq = tid / half, t = tid - sq * half;
  double2* seq = lds64 + sq * CS;
  const int roff = (int)(fft_stockham<+1>(seq, seq + N1, tw, N1, t) - seq);
  const unsigned pr = row / (unsigned)a.C, co = row - pr * (unsigned)a.C;
  const int b0 = 2 * (a.pair0 + (int)pr);
  const bool has1 = b0 + 1 < a.B;
  const double bias = a.bias ? a.bias[co] : 0.0;
  double* y0 = a.y + ((size_t)b0 * a.C + co) * a.Lout;
  double* y1 = y0 + (size_t)a.C * a.Lout;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int idx = tid + u * NT, c = idx & (NC - 1), n1 = idx >> lgNC;
    const int tt = (n1 << a.lgN2) + n20 + c;
    const int pos = a.t0 + tt, q = pos / a.stride;
    if (tt < a.limit && q * a.stride == pos && q < a.Lout) {
      const double2 v = lds64[c * CS + roff + n1];
      y0[q] = v.x + bias;
      if (has1) y1[q] = v.y + bias;
    }
  }
}

bool tile_len_ok(int v) { return v >= 64 && v <= 2048 && (v & (v - 1)) == 0; }

}  // namespace

hipError_t launch_long_f64_cols_fwd(const LongF64Args& a, long long rows, hipStream_t st) {
  if (!tile_len_ok(a.N1) || !tile_len_ok(a.N2) || (1 << a.lgN2) != a.N2) return hipErrorInvalidValue;
  const int nc = long_f64_nc(a.N1);
  return launch_kernel<long_f64_cols_fwd_kernel>(rows * (a.N2 / nc), nc * (a.N1 / 2), long_f64_cols_lds_bytes(a.N1), st, a, nc);
}

hipError_t launch_long_f64_rows(const LongF64Args& a, long long units, hipStream_t st) {
  if (!tile_len_ok(a.N1) || !tile_len_ok(a.N2) || (1 << a.lgN2) != a.N2) return hipErrorInvalidValue;
  if (!a.spec_mode && (a.cob < 1 || a.cob > 8)) return hipErrorInvalidValue;
  const int nr = long_f64_nr(a.N2);
  return launch_kernel<long_f64_rows_kernel>(units * (a.N1 / nr), nr * (a.N2 / 2), long_f64_rows_lds_bytes(a.N2), st, a, nr);
}

hipError_t launch_long_f64_cols_inv(const LongF64Args& a, long long rows, hipStream_t st) {
  if (!tile_len_ok(a.N1) || !tile_len_ok(a.N2) || (1 << a.lgN2) != a.N2 || a.stride < 1) return hipErrorInvalidValue;
  const int nc = long_f64_nc(a.N1);
  return launch_kernel<long_f64_cols_inv_kernel>(rows * (a.N2 / nc), nc * (a.N1 / 2), long_f64_cols_lds_bytes(a.N1), st, a, nc);
}

}  // namespace fc
