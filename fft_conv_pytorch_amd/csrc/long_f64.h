// long_f64.h -- float64 1-D convolution with a kernel past the 2048-point tile (long_f64.hip): one cyclic transform of
// N = N1 * N2 points per row in three launches.  Arguments, launchers and the block geometry the planner sizes with.
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

struct LongF64Args {
  const double* src;     // signal (B, C, L), or the weight (kernel transform)
  const double* bias;    // (Cout) or null
  double* y;             // (B, Cout, Lout)
  double2* w1;           // [row][k1][n2]   rows: (pair, input channel), or the filter rows of this launch
  double2* w2;           // [row][k1][n2]   rows: (pair, output channel)
  const double2* spec;   // [(g*Cog + o)*Cig + i][k1][k2]   H = conj(FFT_N(dilated taps)) / N
  double2* spec_out;     // rows, spec_mode 1: first filter row of this launch
  int N1, N2, lgN2;
  int from_kernel;       // cols_fwd: 0 signal rows, 1 filter rows
  int row0;              // cols_fwd, filter rows: index (o_all * Cig + i) of the first row of this launch
  int spec_mode;         // rows: 1 = finish the filter spectrum
  int B, pair0;          // batch size, first batch pair of this slab
  int C;                 // channels of the source tensor (cols_fwd) / of y (cols_inv)
  int G, Cig, Cog, cob, n_ochunks;
  int L, pad, pad_mode, up;   // signal: AxisMap of the padded row (`pad` the left offset; `up` the spread of a transposed plan)
  int K, dil, transposed;     // taps: dilation; a transposed plan reads them back to front with the channels exchanged
  int p0;                // cols_fwd: padded position of the first point of the transform (tile * V)
  int t0, limit;         // cols_inv: point t < limit of the transform is sample t0 + t of the stride-1 result
  int stride, Lout;      // ... which is y[(t0 + t) / stride] where that divides
  double scale;          // 1 / N (rows, spec_mode 1)
};

// Column passes: a workgroup transforms long_f64_nc(N1) neighbouring n2 columns of one row, N1/2 threads each (at most
// 1024 in all; the sequences and the table fit 160 KiB of LDS with room for two workgroups per CU).
inline int long_f64_nc(int N1) { return N1 <= 128 ? 16 : 2048 / N1; }
// Row pass: long_f64_nr(N2) neighbouring k1 rows per workgroup, N2/2 threads each (at least two waves per workgroup).
inline int long_f64_nr(int N2) { return N2 >= 256 ? 1 : 256 / N2; }
// (each column's two buffers are followed by one spare point: neighbouring columns then start four banks apart)
inline size_t long_f64_cols_lds_bytes(int N1) { return ((size_t)long_f64_nc(N1) * (2 * N1 + 1) + N1 / 2) * 16; }
inline size_t long_f64_rows_lds_bytes(int N2) { return ((size_t)long_f64_nr(N2) * 2 * N2 + N2 / 2) * 16; }

// rows: (pair, channel) rows of the slab, or filter rows
hipError_t launch_long_f64_cols_fwd(const LongF64Args& a, long long rows, hipStream_t st);
// units: pairs * G * n_ochunks of the slab, or filter rows (spec_mode 1)
hipError_t launch_long_f64_rows(const LongF64Args& a, long long units, hipStream_t st);
hipError_t launch_long_f64_cols_inv(const LongF64Args& a, long long rows, hipStream_t st);

}  // namespace fc
