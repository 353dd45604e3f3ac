// nd_f64.hip -- float64 tensors of a 2-D / 3-D convolution (forward and transposed) through FFTs.
//
// The reference runs complex128 rfftn / irfftn over every spatial axis when handed float64 tensors
// (functional.py:66-75, :155-162).  This file is the separable form the fp32 N-d path uses (nd_passes.hpp), written
// in plain double precision in the style of fft_f64.hip: Stockham radix-2 transforms in LDS (natural order in and out,
// one butterfly per thread and stage), twiddles from a table each workgroup builds with sincospi, 64-bit offsets.
//
//   rows_r2c_f64   last axis, real -> half spectrum, two rows per complex sequence, sources through the x index map
//                  (padding mode, tile start, transposed spread); only rows that exist in the input are transformed
//   col_f64        complex -> complex along one axis, NS neighbouring columns per workgroup: the middle axis of a
//                  3-D problem forward (gathering padded positions through the y index map) and back (valid window,
//                  stride), and the outer passes of the kernel transform (taps dilated, flipped for a transposed plan,
//                  conjugated and scaled by 1/prod(T) on the last one)
//   fused_f64      outermost axis: forward transform, acc[o] += X[i] * H[o, i, bin] in registers over the group's input
//                  channels, inverse transform, valid window + stride; nb batch items share each read of H
//   rows_c2r_f64   last axis back: half spectrum -> real, valid window + stride + bias, store to y
//
// A T-point transform runs on T/2 threads per sequence; below 512 points several sequences share a workgroup
// (256 threads), interleaved in LDS (point n of sequence c at n * NS + c) so that butterflies are bank-conflict free.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "nd_f64.h"

namespace fc {
namespace {

__device__ __forceinline__ double2 cmul_d(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ double2 cadd_d(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }

// kernel tap at padded position p (-1: zero); flip = transposed plan (position p holds tap (kd - 1 - p) / dil)
__device__ __forceinline__ int tap_at(int p, int dil, int K, int kd, int flip) {
  const int pp = flip ? kd - 1 - p : p;
  return pp < 0 ? -1 : tap_src(pp, dil, K);
}

// tw[k] = exp(-2 pi i k / T), k < T/2
__device__ __forceinline__ void build_table_nd(double2* tw, int T) {
  for (int k = threadIdx.x; k < (T >> 1); k += blockDim.x) {
    double s, c;
    sincospi(-2.0 * (double)k / (double)T, &s, &c);
    tw[k] = make_double2(c, s);
  }
}

// Stockham radix-2 over NS interleaved sequences (point n of sequence c at n * NS + c); thread (t, c), t < T/2.
// DIR = -1 forward, +1 inverse (unnormalised).  Natural order in (a) and out (returned pointer).
template <int DIR>
__device__ __forceinline__ double2* fft_ns(double2* a, double2* b, const double2* tw, int T, int NS, int t, int c) {
  const int half = T >> 1;
  for (int ns = 1; ns < T; ns <<= 1) {
    const int k = t & (ns - 1);
    const double2 u = a[t * NS + c];
    double2 v = a[(t + half) * NS + c];
    double2 w = tw[k * (half / ns)];
    if (DIR > 0) w.y = -w.y;
    v = cmul_d(v, w);
    const int j = ((t - k) << 1) + k;
    b[j * NS + c] = make_double2(u.x + v.x, u.y + v.y);
    b[(j + ns) * NS + c] = make_double2(u.x - v.x, u.y - v.y);
    __syncthreads();
    double2* s = a; a = b; b = s;
  }
  return a;
}

__global__ __launch_bounds__(1024) void rows_r2c_f64_kernel(const RowsF64Args a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_nd[];
  const int T = a.T, half = T >> 1, NS = nd_f64_nseq(T), nthr = NS * half;
  double2* bufA = lds_nd;
  double2* bufB = lds_nd + NS * T;
  double2* tw = lds_nd + 2 * NS * T;
  build_table_nd(tw, T);
  const long long npair = (a.R + 1) >> 1;
  const long long s0 = (long long)blockIdx.x * NS;
  // load: n fastest (rows are contiguous)
  for (int idx = threadIdx.x; idx < NS * T; idx += nthr) {
    const int n = idx % T, c = idx / T;
    const long long s = s0 + c;
    double2 v = make_double2(0.0, 0.0);
    if (s < npair * a.nt) {
      const long long rp = s / a.nt;
      const int tx = (int)(s - rp * a.nt), p = tx * a.V + n;
      const int q = a.from_kernel ? tap_at(p, a.dil, a.K, a.kd, a.flip) : axis_src(a.mx, p);
      if (q >= 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const long long r = 2 * rp + h;
          if (r >= a.R) break;
          long long img = r / a.NR;
          const long long rr = r - img * a.NR;
          if (a.tw_Cig > 0) {   // transposed weight (Cin, Cout/g, ...): image (g*Cog + o)*Cig + i
            const long long i = img % a.tw_Cig, go = img / a.tw_Cig, g = go / a.tw_Cog, o = go % a.tw_Cog;
            img = (g * a.tw_Cig + i) * a.tw_Cog + o;
          }
          const double val = a.src[(size_t)(img * a.NR + rr) * a.Sx + q];
          if (h == 0) v.x = val; else v.y = val;
        }
      }
    }
    bufA[n * NS + c] = v;
  }
  __syncthreads();
  const int c = threadIdx.x % NS, t = threadIdx.x / NS;
  const double2* Z = fft_ns<-1>(bufA, bufB, tw, T, NS, t, c);
  const long long s = s0 + c;
  if (s >= npair * a.nt) return;
  const long long rp = s / a.nt;
  const int tx = (int)(s - rp * a.nt);
  const long long r0 = 2 * rp;
  const bool two = r0 + 1 < a.R;
  double2* d0 = a.dst + ((size_t)r0 * a.nt + tx) * a.Fx;
  double2* d1 = a.dst + ((size_t)(r0 + 1) * a.nt + tx) * a.Fx;
  // X_a[f] = (Z[f] + conj Z[T-f]) / 2, X_b[f] = (Z[f] - conj Z[T-f]) / 2i; thread t writes bin t, thread 0 also T/2
  for (int f = t; f <= half; f += half) {
    const double2 zf = Z[f * NS + c], zg = Z[((T - f) & (T - 1)) * NS + c];
    d0[f] = make_double2(0.5 * (zf.x + zg.x), 0.5 * (zf.y - zg.y));
    if (two) d1[f] = make_double2(0.5 * (zf.y + zg.y), 0.5 * (zg.x - zf.x));
    if (t != 0) break;
  }
}

__global__ __launch_bounds__(1024) void col_f64_kernel(const ColF64Args a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_nd[];
  const int T = a.T, half = T >> 1, NS = nd_f64_nseq(T), nthr = NS * half;
  double2* bufA = lds_nd;
  double2* bufB = lds_nd + NS * T;
  double2* tw = lds_nd + 2 * NS * T;
  build_table_nd(tw, T);
  const int ncc = (a.ncol + NS - 1) / NS;
  long long id = blockIdx.x;
  const int cc = (int)(id % ncc); id /= ncc;
  const int tile = (int)(id % a.nt);
  const long long line = id / a.nt;
  const int col0 = cc * NS;
  const double2* src = a.src + (size_t)line * a.src_line;
  // load: columns fastest (unit stride between neighbouring sequences)
  for (int idx = threadIdx.x; idx < NS * T; idx += nthr) {
    const int c = idx % NS, n = idx / NS, col = col0 + c;
    double2 v = make_double2(0.0, 0.0);
    if (col < a.ncol) {
      if (a.mode == 2) {
        v = src[(size_t)tile * a.src_tile + (size_t)n * a.src_pt + col];
      } else {
        const int p = tile * a.V + n;
        const int q = a.mode == 0 ? axis_src(a.m, p) : tap_at(p, a.dil, a.K, a.kd, a.flip);
        if (q >= 0) v = src[(size_t)q * a.src_pt + col];
      }
    }
    bufA[idx] = v;
  }
  __syncthreads();
  const int c = threadIdx.x % NS, t = threadIdx.x / NS;
  const double2* Z = a.mode == 2 ? fft_ns<+1>(bufA, bufB, tw, T, NS, t, c) : fft_ns<-1>(bufA, bufB, tw, T, NS, t, c);
  double2* dst = a.dst + (size_t)line * a.dst_line;
  for (int idx = threadIdx.x; idx < NS * T; idx += nthr) {
    const int cs = idx % NS, n = idx / NS, col = col0 + cs;
    if (col >= a.ncol) continue;
    double2 v = Z[idx];
    if (a.mode == 2) {
      const int pos = tile * a.V + n, o = pos / a.ostride;
      if (n < a.V && pos < a.Lf && o * a.ostride == pos) dst[(size_t)o * a.dst_pt + col] = v;
    } else {
      if (a.conj_scale) v = make_double2(v.x * a.scale, -v.y * a.scale);
      dst[(size_t)tile * a.dst_tile + (size_t)n * a.dst_pt + col] = v;
    }
  }
}

// NB batch items x (8 / NB) output channels of accumulators per thread and bin
template <int NB>
__global__ __launch_bounds__(1024) void fused_f64_kernel(const FusedF64Args a) {
  constexpr int COB = 8 / NB;
  extern __shared__ __attribute__((aligned(16))) double2 lds_nd[];
  const int T = a.T, half = T >> 1, NS = nd_f64_nseq(T), nthr = NS * half;
  double2* bufA = lds_nd;
  double2* bufB = lds_nd + NS * T;
  double2* tw = lds_nd + 2 * NS * T;
  build_table_nd(tw, T);
  const int ncc = (a.ncol + NS - 1) / NS;
  long long id = blockIdx.x;
  const int cc = (int)(id % ncc); id /= ncc;
  const int tile = (int)(id % a.nt); id /= a.nt;
  const int oc = (int)(id % a.n_ochunks); id /= a.n_ochunks;
  const int g = (int)(id % a.G);
  const int b0 = (int)(id / a.G) * NB;
  const int col0 = cc * NS;
  const int c = threadIdx.x % NS, t = threadIdx.x / NS, col = col0 + c;
  const bool live = col < a.ncol;
  const int hcol = live ? ((col / a.Ncol) % a.Tmid) * a.Fx + (col % a.Ncol) % a.Fx : 0;
  const int nout = min(a.cob, a.Cog - oc * a.cob);
  double2 acc[NB][COB][2];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int o = 0; o < COB; ++o) acc[j][o][0] = acc[j][o][1] = make_double2(0.0, 0.0);
  for (int i = 0; i < a.Cig; ++i) {
    double2 xs[NB][2];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int b = b0 + j;
      xs[j][0] = xs[j][1] = make_double2(0.0, 0.0);
      if (b >= a.B) continue;                          // uniform
      const double2* src = a.src + ((size_t)b * a.Cin + (size_t)g * a.Cig + i) * a.src_img;
      __syncthreads();                                 // (table built / previous transform consumed)
      for (int idx = threadIdx.x; idx < NS * T; idx += nthr) {
        const int cs = idx % NS, n = idx / NS, cl = col0 + cs;
        double2 v = make_double2(0.0, 0.0);
        if (cl < a.ncol) {
          const int q = axis_src(a.m, tile * a.V + n);
          if (q >= 0) v = src[(size_t)q * a.src_pt + cl];
        }
        bufA[idx] = v;
      }
      __syncthreads();
      const double2* Z = fft_ns<-1>(bufA, bufB, tw, T, NS, t, c);
      xs[j][0] = Z[t * NS + c];
      xs[j][1] = Z[(t + half) * NS + c];
    }
    if (!live) continue;
    const double2* hrow = a.H + (((size_t)g * a.Cog + (size_t)oc * a.cob) * a.Cig + i) * (size_t)T * a.Hcols + hcol;
#pragma unroll
    for (int o = 0; o < COB; ++o)
      if (o < nout) {
        const double2* hp = hrow + (size_t)o * a.Cig * T * a.Hcols;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double2 hv = hp[(size_t)(t + h * half) * a.Hcols];
#pragma unroll
          for (int j = 0; j < NB; ++j) acc[j][o][h] = cadd_d(acc[j][o][h], cmul_d(xs[j][h], hv));
        }
      }
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int b = b0 + j;
    if (b >= a.B) break;                               // uniform
#pragma unroll
    for (int o = 0; o < COB; ++o) {
      if (o >= nout) break;                            // uniform
      __syncthreads();
      bufA[t * NS + c] = acc[j][o][0];
      bufA[(t + half) * NS + c] = acc[j][o][1];
      __syncthreads();
      const double2* Y = fft_ns<+1>(bufA, bufB, tw, T, NS, t, c);
      double2* dst = a.dst + ((size_t)b * a.Cout + (size_t)g * a.Cog + (size_t)oc * a.cob + o) * a.dst_img;
      for (int idx = threadIdx.x; idx < NS * T; idx += nthr) {
        const int cs = idx % NS, n = idx / NS, cl = col0 + cs;
        const int pos = tile * a.V + n, q = pos / a.ostride;
        if (cl < a.ncol && n < a.V && pos < a.Lf && q * a.ostride == pos) dst[(size_t)q * a.dst_pt + cl] = Y[idx];
      }
    }
  }
}

__global__ __launch_bounds__(1024) void rows_c2r_f64_kernel(const RowsC2RF64Args a) {
  extern __shared__ __attribute__((aligned(16))) double2 lds_nd[];
  const int T = a.T, half = T >> 1, NS = nd_f64_nseq(T), nthr = NS * half;
  double2* bufA = lds_nd;
  double2* bufB = lds_nd + NS * T;
  double2* tw = lds_nd + 2 * NS * T;
  build_table_nd(tw, T);
  const long long npair = (a.R + 1) >> 1;
  const long long s0 = (long long)blockIdx.x * NS;
  // Z[n] = Y_a[n] + i Y_b[n] over the full length (Y[T-f] = conj Y[f]); n fastest
  for (int idx = threadIdx.x; idx < NS * T; idx += nthr) {
    const int n = idx % T, c = idx / T;
    const long long s = s0 + c;
    double2 v = make_double2(0.0, 0.0);
    if (s < npair * a.nt) {
      const long long rp = s / a.nt;
      const int tx = (int)(s - rp * a.nt);
      const long long r0 = 2 * rp;
      const bool mirror = n > half;
      const int f = mirror ? T - n : n;
      double2 ya = a.src[((size_t)r0 * a.nt + tx) * a.Fx + f];
      double2 yb = r0 + 1 < a.R ? a.src[((size_t)(r0 + 1) * a.nt + tx) * a.Fx + f] : make_double2(0.0, 0.0);
      if (mirror) { ya.y = -ya.y; yb.y = -yb.y; }
      v = make_double2(ya.x - yb.y, ya.y + yb.x);
    }
    bufA[n * NS + c] = v;
  }
  __syncthreads();
  const int c = threadIdx.x % NS, t = threadIdx.x / NS;
  const double2* Y = fft_ns<+1>(bufA, bufB, tw, T, NS, t, c);
  // store: n fastest again
  for (int idx = threadIdx.x; idx < NS * T; idx += nthr) {
    const int n = idx % T, cs = idx / T;
    const long long s = s0 + cs;
    if (s >= npair * a.nt || n >= a.V) continue;
    const long long rp = s / a.nt;
    const int tx = (int)(s - rp * a.nt);
    const int pos = tx * a.V + n, q = pos / a.ostride;
    if (pos >= a.Lf || q * a.ostride != pos) continue;
    const long long r0 = 2 * rp;
    const double2 v = Y[n * NS + cs];
    const int co0 = (int)((r0 / a.rows_per_co) % a.Cout);
    a.y[(size_t)r0 * a.Ox + q] = v.x + (a.bias ? a.bias[co0] : 0.0);
    if (r0 + 1 < a.R) {
      const int co1 = (int)(((r0 + 1) / a.rows_per_co) % a.Cout);
      a.y[(size_t)(r0 + 1) * a.Ox + q] = v.y + (a.bias ? a.bias[co1] : 0.0);
    }
  }
}

// T-point transforms, nd_f64_nseq(T) sequences per workgroup (the 2048-point transform takes 80 KiB of LDS)
template <auto Kernel, class Args>
hipError_t launch_nd(int T, long long grid, const Args& a, hipStream_t st) {
  const size_t lds = nd_f64_lds_bytes(T);
  if (T < 8 || T > 2048 || (T & (T - 1)) || lds > 160 * 1024) return hipErrorInvalidValue;
  return launch_kernel<Kernel>(grid, (unsigned)(nd_f64_nseq(T) * (T / 2)), lds, st, a);
}

}  // namespace

hipError_t launch_rows_r2c_f64(const RowsF64Args& a, hipStream_t st) {
  const long long seqs = ((a.R + 1) / 2) * a.nt, NS = nd_f64_nseq(a.T);
  return launch_nd<rows_r2c_f64_kernel>(a.T, (seqs + NS - 1) / NS, a, st);
}

hipError_t launch_col_f64(const ColF64Args& a, hipStream_t st) {
  const int NS = nd_f64_nseq(a.T);
  return launch_nd<col_f64_kernel>(a.T, a.nlines * a.nt * ((a.ncol + NS - 1) / NS), a, st);
}

hipError_t launch_fused_f64(const FusedF64Args& a, hipStream_t st) {
  const int NS = nd_f64_nseq(a.T);
  if ((a.nb != 1 && a.nb != 2 && a.nb != 4) || a.cob < 1 || a.cob > 8 / a.nb) return hipErrorInvalidValue;
  const long long grid = (long long)((a.B + a.nb - 1) / a.nb) * a.G * a.n_ochunks * a.nt * ((a.ncol + NS - 1) / NS);
  if (a.nb == 1) return launch_nd<fused_f64_kernel<1>>(a.T, grid, a, st);
  if (a.nb == 2) return launch_nd<fused_f64_kernel<2>>(a.T, grid, a, st);
  return launch_nd<fused_f64_kernel<4>>(a.T, grid, a, st);
}

hipError_t launch_rows_c2r_f64(const RowsC2RF64Args& a, hipStream_t st) {
  const long long seqs = ((a.R + 1) / 2) * a.nt, NS = nd_f64_nseq(a.T);
  return launch_nd<rows_c2r_f64_kernel>(a.T, (seqs + NS - 1) / NS, a, st);
}

}  // namespace fc
