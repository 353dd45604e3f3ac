// fft_f64.hip -- float64 tensors through an FFT path (the reference is dtype-agnostic:
// functional.py:19-89 runs complex128 FFTs when handed float64 tensors).
//
// Round 2 served float64 callers with a direct time-domain kernel only (direct_f64.hip, O(outputs x Cin/g x taps)).
// This file is the same 1-D algorithm as the fp32 kernels -- overlap-save tiles, forward transform, per-bin channel
// contraction against the pre-transformed kernel, inverse transform, valid window + stride + bias -- written in plain
// double precision: a Stockham radix-2 transform in LDS (natural order in and out, one butterfly per thread and stage,
// twiddles from a table the workgroup builds with sincospi), two real channels per complex sequence, the output
// channels' spectra accumulated in registers over the input channels (a thread owns bins t and t + T/2).  It is not
// tuned like the packed-fp32 engine (fft_engine.hpp is written on v_pk_*_f32 pairs and 8-byte LDS slots); it exists so
// that float64 results come from the same transform-domain arithmetic as the reference's at FFT cost.  A transposed
// plan (functional.py:126-162 of the reference) runs the same kernels: its input spread over the stride's grid behind
// a left offset of kd - 1 - padding (which may be negative), its taps flipped and read with the channels exchanged.
// 2-D / 3-D float64 plans run nd_f64.hip.
#include <hip/hip_runtime.h>

#include "axis_map.hpp"
#include "fft_f64.h"
#include "fft_f64_core.hpp"
#include "launch.hpp"

namespace fc {
namespace {

// ---- kernel transform: one (o, i) pair per workgroup
__global__ __launch_bounds__(1024) void spectrum_f64_kernel(const FftF64Args a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds64[];
  const int T = a.T, t = threadIdx.x;
  double2* bufA = lds64;
  double2* bufB = lds64 + T;
  double2* tw = lds64 + 2 * T;
  const int oi = blockIdx.x;                       // o_all * Cig + i
  // transposed: the weight is (Cin, Cout/g, K) and H[g][o][i] holds the taps of w[g*Cig + i][o] back to front
  const int i_ = oi % a.Cig, go = oi / a.Cig;
  const double* wrow = a.w + (size_t)(a.transposed ? ((go / a.Cog) * a.Cig + i_) * a.Cog + go % a.Cog : oi) * a.K;
  const int kd = (a.K - 1) * a.dil + 1;
  build_table(tw, T, t);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int n = t + h * (T >> 1);
    const int pp = a.transposed ? kd - 1 - n : n;
    const int tap = pp >= 0 ? tap_src(pp, a.dil, a.K) : -1;
    bufA[n] = make_double2(tap >= 0 ? wrow[tap] : 0.0, 0.0);
  }
  __syncthreads();
  double2* r = fft_stockham<-1>(bufA, bufB, tw, T, t);
  const double sc = 1.0 / (double)T;
  double2* out = a.wspec + (size_t)oi * T;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int f = t + h * (T >> 1);
    out[f] = make_double2(r[f].x * sc, -r[f].y * sc);      // conj: cross-correlation, like rfftn(kernel).conj()
  }
}

// ---- forward: workgroup = (batch b, group g, out-chunk oc, tile)
__global__ __launch_bounds__(1024) void conv1d_f64_kernel(const FftF64Args a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds64[];
  const int T = a.T, half = T >> 1, t = threadIdx.x;
  double2* bufA = lds64;
  double2* bufB = lds64 + T;
  double2* tw = lds64 + 2 * T;
  int id = blockIdx.x;
  const int tile = id % a.ntiles; id /= a.ntiles;
  const int oc = id % a.n_ochunks; id /= a.n_ochunks;
  const int g = id % a.G;
  const int b = id / a.G;
  build_table(tw, T, t);
  const AxisMap map{a.L, a.pad, a.pad_mode, a.up};    // a.pad: left offset (padding; kd - 1 - padding transposed)
  const int p0 = tile * a.V;                           // padded position of the tile's first sample
  const int nout = min(a.cob, a.Cog - oc * a.cob);
  double2 acc[8][2];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o][0] = acc[o][1] = make_double2(0.0, 0.0);
  // two real input channels ride one complex transform (z = x_a + i x_b; X_a[f] = (Z[f] + conj Z[T-f]) / 2,
  // X_b[f] = (Z[f] - conj Z[T-f]) / 2i), two output channels one inverse transform
  for (int i = 0; i < a.Cig; i += 2) {
    const bool two = i + 1 < a.Cig;
    const double* xa = a.x + ((size_t)b * a.Cin + (size_t)g * a.Cig + i) * a.L;
    const double* xb = xa + a.L;
    __syncthreads();                                   // (table built / previous pair's spectrum consumed)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n = t + h * half;
      const int q = axis_src(map, p0 + n);
      bufA[n] = make_double2(q >= 0 ? xa[q] : 0.0, (q >= 0 && two) ? xb[q] : 0.0);
    }
    __syncthreads();
    const double2* Z = fft_stockham<-1>(bufA, bufB, tw, T, t);
    double2 xs[2][2];                                  // [bin t / t + half][channel a / b]
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int f = t + h * half;
      const double2 zf = Z[f], zg = Z[(T - f) & (T - 1)];
      xs[h][0] = make_double2(0.5 * (zf.x + zg.x), 0.5 * (zf.y - zg.y));
      xs[h][1] = make_double2(0.5 * (zf.y + zg.y), 0.5 * (zg.x - zf.x));
    }
    const double2* hrow = a.wspec + (((size_t)g * a.Cog + (size_t)oc * a.cob) * a.Cig + i) * T;
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < nout) {
        const double2* hp = hrow + (size_t)o * a.Cig * T;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int f = t + h * half;
          double2 p = cmul_d(xs[h][0], hp[f]);
          if (two) { const double2 p2 = cmul_d(xs[h][1], hp[T + f]); p.x += p2.x; p.y += p2.y; }
          acc[o][h].x += p.x; acc[o][h].y += p.y;
        }
      }
  }
  const int t0 = tile * a.V;
  const int limit = min(a.V, a.Lfull - t0);
#pragma unroll
  for (int o = 0; o < 8; o += 2) {
    if (o >= nout) break;                              // uniform
    const bool two = o + 1 < nout;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double2 ya = acc[o][h], yb = two ? acc[o + 1][h] : make_double2(0.0, 0.0);
      bufA[t + h * half] = make_double2(ya.x - yb.y, ya.y + yb.x);      // Y_a + i Y_b
    }
    __syncthreads();
    const double2* Y = fft_stockham<+1>(bufA, bufB, tw, T, t);
    const int co = g * a.Cog + oc * a.cob + o;
    const double bias_a = a.bias ? a.bias[co] : 0.0, bias_b = (a.bias && two) ? a.bias[co + 1] : 0.0;
    double* yrow = a.y + ((size_t)b * a.Cout + co) * a.Lout;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n = t + h * half;
      const int pos = t0 + n, idx = pos / a.stride;
      if (n < limit && idx * a.stride == pos) {
        yrow[idx] = Y[n].x + bias_a;
        if (two) yrow[a.Lout + idx] = Y[n].y + bias_b;
      }
    }
  }
}

}  // namespace

hipError_t launch_fft_f64(int which, const FftF64Args& a, hipStream_t st) {
  const size_t lds = fft_f64_lds_bytes(a.T);
  const int nt = a.T / 2;
  if (nt < 64 || nt > 1024 || lds > 160 * 1024) return hipErrorInvalidValue;
  // (the 2048-point tile takes 80 KiB of LDS)
  if (which == 0) return launch_kernel<spectrum_f64_kernel>((long long)a.Cout * a.Cig, nt, lds, st, a);
  return launch_kernel<conv1d_f64_kernel>((long long)a.B * a.G * a.n_ochunks * a.ntiles, nt, lds, st, a);
}

}  // namespace fc
