// long_inst.hip -- instantiates the three kernels of long1d.hpp (the two column kernels in nine builds each: float32,
// 16-bit, one build for float16 and bfloat16, and complex64, each plain, mapped and channels-last) for ONE tile geometry (P, S): built once per geometry
// with -DFC_P=.. -DFC_S=.. like tile_inst.hip, in an object of its own so that the two compile side by side.
#include "launch.hpp"
#include "long1d.hpp"

#ifndef FC_P
#error "compile with -DFC_P=<points per thread> -DFC_S=<lane split>"
#endif

namespace fc {
namespace {

using GG = Geo<FC_P, FC_S>;
constexpr int kT = GG::T;
// sequences per workgroup: as the c2c passes of the N-d plans (columns of a block / neighbouring k1 rows)
constexpr int kNSEQ = (8192 / kT) > 16 ? 16 : ((8192 / kT) < 2 ? 2 : (8192 / kT));
constexpr int kNT = kNSEQ * GG::TS;
constexpr int kLSEQP = SeqLayout<GG>::LSEQP;
constexpr size_t kLds = (size_t)kNSEQ * kLSEQP * sizeof(float2);
// output channels per workgroup of the row pass: 32 running sums (64 registers) per thread
constexpr int kOB = 32 / FC_P;

template <auto Kernel>
hipError_t launch(const LongArgs& a, int blocks_per_unit, long long units, hipStream_t st) {
  if (blocks_per_unit <= 0 || units <= 0) return hipErrorInvalidValue;
  LongArgs b = a;
  b.d_nblk = make_fastdiv((unsigned)blocks_per_unit);
  b.d_c = make_fastdiv((unsigned)a.C);
  b.d_nob = make_fastdiv((unsigned)a.nob);
  b.d_g = make_fastdiv((unsigned)a.G);
  return launch_kernel<Kernel>(units * blocks_per_unit, kNT, kLds, st, b);
}

hipError_t cols_fwd(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || a.src_io != 0) return hipErrorInvalidValue;
  return launch<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_fwd_h16(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || !io_is_h16(a.src_io)) return hipErrorInvalidValue;
  return launch<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t rows(const LongArgs& a, long long units, hipStream_t st) {
  if (a.N2 != kT || a.ob != kOB) return hipErrorInvalidValue;
  return launch<long_rows_kernel<FC_P, FC_S, kNSEQ, kNT, kOB>>(a, a.N1 / kNSEQ, units, st);
}
hipError_t cols_inv(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || a.y_io != 0) return hipErrorInvalidValue;
  return launch<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_inv_h16(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || !io_is_h16(a.y_io)) return hipErrorInvalidValue;
  return launch<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_fwd_map(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || a.src_io != 0) return hipErrorInvalidValue;
  return launch<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_fwd_map_h16(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || !io_is_h16(a.src_io)) return hipErrorInvalidValue;
  return launch<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16, true>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_inv_map(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || a.y_io != 0) return hipErrorInvalidValue;
  return launch<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_inv_map_h16(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || !io_is_h16(a.y_io)) return hipErrorInvalidValue;
  return launch<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16, true>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_fwd_cx(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || a.src_io != IO_CODE_C64) return hipErrorInvalidValue;
  return launch<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, false, true>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_inv_cx(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || a.y_io != IO_CODE_C64) return hipErrorInvalidValue;
  return launch<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, false, true>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_fwd_map_cx(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || a.src_io != IO_CODE_C64) return hipErrorInvalidValue;
  return launch<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true, true>>(a, a.N2 / kNSEQ, rows, st);
}
hipError_t cols_inv_map_cx(const LongArgs& a, long long rows, hipStream_t st) {
  if (a.N1 != kT || a.y_io != IO_CODE_C64) return hipErrorInvalidValue;
  return launch<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true, true>>(a, a.N2 / kNSEQ, rows, st);
}


// ---- channels-last (long1d.hpp): NC neighbouring channels x NSEQ / NC neighbouring n2 columns per workgroup.  NC makes
// a time sample's run 16 bytes long on the tensor side, as far as the NSEQ sequences go (the splits tried: DESIGN 4.7)
constexpr int nlc_nc(int es) {
  const int nc = 16 / es;
  return nc < 1 ? 1 : (nc > kNSEQ ? kNSEQ : nc);
}
constexpr int kNC32 = nlc_nc(4), kNC16 = nlc_nc(2), kNC64 = nlc_nc(8);

template <auto Kernel, int NC>
hipError_t launch_nlc(const LongArgs& a, long long pairs, hipStream_t st) {
  if (pairs <= 0 || a.C <= 0) return hipErrorInvalidValue;
  const long long ncb = (a.C + NC - 1) / NC, nblk = a.N2 / (kNSEQ / NC);
  LongArgs b = a;
  b.d_ncb = make_fastdiv((unsigned)ncb);
  b.d_nblk = make_fastdiv((unsigned)nblk);
  return launch_kernel<Kernel>(pairs * nblk * ncb, kNT, kLds, st, b);
}

hipError_t cols_fwd_nlc(const LongArgs& a, long long pairs, hipStream_t st) {
  if (a.N1 != kT || a.src_io != 0 || a.from_kernel) return hipErrorInvalidValue;
  return launch_nlc<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true, false, kNC32>, kNC32>(a, pairs, st);
}
hipError_t cols_inv_nlc(const LongArgs& a, long long pairs, hipStream_t st) {
  if (a.N1 != kT || a.y_io != 0) return hipErrorInvalidValue;
  return launch_nlc<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true, false, kNC32>, kNC32>(a, pairs, st);
}
hipError_t cols_fwd_nlc_h16(const LongArgs& a, long long pairs, hipStream_t st) {
  if (a.N1 != kT || !io_is_h16(a.src_io) || a.from_kernel) return hipErrorInvalidValue;
  return launch_nlc<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16, true, false, kNC16>, kNC16>(a, pairs, st);
}
hipError_t cols_inv_nlc_h16(const LongArgs& a, long long pairs, hipStream_t st) {
  if (a.N1 != kT || !io_is_h16(a.y_io)) return hipErrorInvalidValue;
  return launch_nlc<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16, true, false, kNC16>, kNC16>(a, pairs, st);
}
hipError_t cols_fwd_nlc_cx(const LongArgs& a, long long pairs, hipStream_t st) {
  if (a.N1 != kT || a.src_io != IO_CODE_C64 || a.from_kernel) return hipErrorInvalidValue;
  return launch_nlc<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true, true, kNC64>, kNC64>(a, pairs, st);
}
hipError_t cols_inv_nlc_cx(const LongArgs& a, long long pairs, hipStream_t st) {
  if (a.N1 != kT || a.y_io != IO_CODE_C64) return hipErrorInvalidValue;
  return launch_nlc<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true, true, kNC64>, kNC64>(a, pairs, st);
}

}  // namespace

#define FC_CAT_(a, b, c, d) a##b##c##d
#define FC_CAT(a, b, c, d) FC_CAT_(a, b, c, d)
const LongImpl* FC_CAT(get_long_P, FC_P, _S, FC_S)() {
  static const LongImpl impl = {kT, kNSEQ, kOB, cols_fwd, rows, cols_inv, cols_fwd_h16, cols_inv_h16,
                                cols_fwd_map, cols_inv_map, cols_fwd_map_h16, cols_inv_map_h16,
                                cols_fwd_cx, cols_inv_cx, cols_fwd_map_cx, cols_inv_map_cx,
                                cols_fwd_nlc, cols_inv_nlc, cols_fwd_nlc_h16, cols_inv_nlc_h16,
                                cols_fwd_nlc_cx, cols_inv_nlc_cx};
  return &impl;
}

}  // namespace fc
