// nd_f64.h -- float64 2-D / 3-D (and their transposed form) FFT convolution (nd_f64.hip): pass arguments, launchers.
//
// Layouts (double2 elements; Fx = Tx/2 + 1 bins of the last axis, ntx / nty tiles of the last / middle axis,
// Ncol = ntx * Fx columns per row, Mcol = nty * Ty * Ncol columns per plane of a 3-D problem):
//   rows    (img, [z,] y, tx) rows of Fx bins                                        [rows][Ncol]
//   middle  3-D: (img, z) lines of nty * Ty spectra along y, Ncol columns each         [img*Sz][nty*Ty][Ncol]
//   fused   outermost axis, back in the spatial domain after the channel contraction  [b*Cout + co][O0][cols]
// The kernel spectrum is H[g][o][i][T0][(Ty,) Fx] = conj(DFT(dilated taps)) / prod(T): every x / y tile shares it.
#pragma once
#include <hip/hip_runtime.h>

#include "axis_map.hpp"

namespace fc {

// last axis, real -> half spectrum: two rows per complex sequence; sources through the x index map, or kernel taps
struct RowsF64Args {
  const double* src;
  double2* dst;               // [row][nt][Fx]
  long long R;                // rows
  int NR;                     // rows per image (the image's own, existing rows)
  int Sx;                     // source row length
  int T, V, nt, Fx;
  AxisMap mx;                 // signal
  int from_kernel, K, dil, kd, flip;   // kernel taps (flip: transposed plan)
  int tw_Cig, tw_Cog;         // > 0: the weight is (Cin, Cout/g, ...): image (g*Cog + o)*Cig + i reads (g*Cig + i)*Cog + o
};

// one axis, complex -> complex, NS neighbouring columns per workgroup (unit-stride), a sequence every `pt` elements.
// mode 0: forward, sources through the axis map; 1: forward, kernel taps; 2: inverse, valid window + stride
struct ColF64Args {
  const double2* src;
  double2* dst;
  long long nlines;
  int ncol, T, V, nt, mode;
  long long src_line, src_pt, src_tile;
  long long dst_line, dst_pt, dst_tile;
  AxisMap m;
  int K, dil, kd, flip;
  int conj_scale;             // kernel transform, last pass: conj and multiply by `scale`
  double scale;
  int Lf, ostride;            // inverse: stride-1 outputs of the axis, decimation
};

// outermost axis: forward transform, per-bin contraction over the group's input channels, inverse transform,
// valid window + stride; a workgroup serves nb batch items per read of the kernel spectrum
struct FusedF64Args {
  const double2* src;         // [b*Cin + ci][S0][ncol]
  const double2* H;           // [G*Cog][Cig][T][Hcols]
  double2* dst;               // [b*Cout + co][O0][ncol]
  long long src_img, src_pt, dst_img, dst_pt;
  int ncol, T, V, nt;
  AxisMap m;
  int B, Cin, Cout, G, Cig, Cog, cob, n_ochunks, nb;
  int Lf, ostride;
  int Ncol, Tmid, Fx, Hcols;  // kernel column of data column c: ((c / Ncol) % Tmid) * Fx + (c % Ncol) % Fx
};

// last axis back: half spectrum -> real, valid window + stride + bias, two rows per complex sequence
struct RowsC2RF64Args {
  const double2* src;         // [row][nt][Fx]
  double* y;                  // [row][Ox]
  const double* bias;
  long long R;
  int T, V, nt, Fx, Lf, ostride, Ox;
  long long rows_per_co;      // rows of one output channel (O0 [* O1])
  int Cout;
};

hipError_t launch_rows_r2c_f64(const RowsF64Args& a, hipStream_t st);
hipError_t launch_col_f64(const ColF64Args& a, hipStream_t st);
hipError_t launch_fused_f64(const FusedF64Args& a, hipStream_t st);
hipError_t launch_rows_c2r_f64(const RowsC2RF64Args& a, hipStream_t st);

// sequences per workgroup for a T-point transform: 256 threads while T <= 512, one sequence above
__host__ __device__ inline int nd_f64_nseq(int T) { return T >= 512 ? 1 : 512 / T; }
inline size_t nd_f64_lds_bytes(int T) { return (size_t)(2 * nd_f64_nseq(T) * T + T / 2) * 16; }

}  // namespace fc
