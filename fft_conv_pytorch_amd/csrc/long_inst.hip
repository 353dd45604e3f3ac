// long_inst.hip -- instantiates the three kernels of long1d.hpp for ONE tile geometry (P, S) and is the one place that
// picks the build of a column launch (cols_dispatch: float32, 16-bit -- one build for float16 and bfloat16 -- or complex64
// by the launch's element code, each plain, mapped or channels-last, nine builds of each column kernel; for a phases plan,
// a.ph_s > 0, the phases builds of the filter rows and of the inverse pass, float32 and 16-bit; for a decimation plan,
// a.ph_s > 0 with a.ph_cog == 0, the decimation builds of the filter rows and of the signal rows, float32 and 16-bit; the row pass
// of the weight gradient and the float32 and 16-bit builds of its inverse pass have entries of their own, and so have the
// gated and the blocks builds of the column passes): built once per
// geometry with -DFC_P=.. -DFC_S=.. like tile_inst.hip, in an object of its own so that the two compile side by side.
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

hipError_t rows(const LongArgs& a, long long units, hipStream_t st) {
  if (a.N2 != kT || a.ob != kOB) return hipErrorInvalidValue;
  return launch<long_rows_kernel<FC_P, FC_S, kNSEQ, kNT, kOB>>(a, a.N1 / kNSEQ, units, st);
}

// ---- the weight gradient (long1d.hpp): its row pass keeps the x spectrum live across the transforms of the dY rows
constexpr int kWgOB = kOB;

hipError_t wgrad_rows(const LongArgs& a, long long units, hipStream_t st) {
  if (a.N2 != kT || a.ob != kWgOB) return hipErrorInvalidValue;
  return launch<long_wgrad_rows_kernel<FC_P, FC_S, kNSEQ, kNT, kWgOB>>(a, a.N1 / kNSEQ, units, st);
}

// ---- channels-last (long1d.hpp): NC neighbouring channels x NSEQ / NC neighbouring n2 columns per workgroup.  NC makes
// a time sample's run 16 bytes long on the tensor side, as far as the NSEQ sequences go (the splits tried: DESIGN 4.7)
constexpr int nlc_nc(int es) {
  const int nc = 16 / es;
  return nc < 1 ? 1 : (nc > kNSEQ ? kNSEQ : nc);
}

template <auto Kernel, int NC>
hipError_t launch_nlc(const LongArgs& a, long long pairs, hipStream_t st) {
  const long long ncb = (a.C + NC - 1) / NC, nblk = a.N2 / (kNSEQ / NC);
  LongArgs b = a;
  b.d_ncb = make_fastdiv((unsigned)ncb);
  b.d_nblk = make_fastdiv((unsigned)nblk);
  return launch_kernel<Kernel>(pairs * nblk * ncb, kNT, kLds, st, b);
}

// the build of a column kernel: forward or inverse, element type (IO, CX), plain / mapped, channels-last with NC > 0
template <bool INV, int IO, bool MAP, bool CX, int NC>
constexpr auto cols_kernel() {
  if constexpr (INV) return long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO, MAP, CX, NC>;
  else return long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO, MAP, CX, NC>;
}

// ... of one element type, ES bytes per sample: a channels-last build is a mapped build and serves plain launches too
template <bool INV, int IO, bool CX>
hipError_t cols_launch(const LongArgs& a, bool mapped, bool nlc, long long rows, hipStream_t st) {
  constexpr int NC = nlc_nc(CX ? 8 : (int)Io<IO>::B);
  if (nlc) return launch_nlc<cols_kernel<INV, IO, true, CX, NC>(), NC>(a, rows, st);
  if (mapped) return launch<cols_kernel<INV, IO, true, CX, 0>()>(a, a.N2 / kNSEQ, rows * a.C, st);
  return launch<cols_kernel<INV, IO, false, CX, 0>()>(a, a.N2 / kNSEQ, rows * a.C, st);
}

// ---- phases (long1d.hpp).  The filter rows of a phases plan: the plain block map, one build per element type
template <int IO>
hipError_t phs_filter_launch(const LongArgs& a, long long rows, hipStream_t st) {
  LongArgs b = a;
  b.d_ph_s = make_fastdiv((unsigned)a.ph_s);
  b.d_ph_cig = make_fastdiv((unsigned)a.Cig);
  b.d_ph_cogs = make_fastdiv((unsigned)a.ph_s * (unsigned)a.ph_cog);
  return launch<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO, false, false, 0, true>>(b, a.N2 / kNSEQ, rows * a.C, st);
}

// The inverse pass: NC phases of one filter x kNSEQ / NC neighbouring n2 columns per workgroup, a.C filters.  NC == s
// makes a workgroup's stores of one n1 contiguous (kNSEQ samples); phases past s in a filter's last block are idle slots,
// so of the two widths built the one that rounds s up by less is taken, the wider at a tie (2: s = 2, 5, 6; 4: 3, 4, 7, 8)
constexpr int kPhsWide = kNSEQ < 4 ? kNSEQ : 4;

template <int IO, int NC>
hipError_t phs_inv_launch(const LongArgs& a, long long pairs, hipStream_t st) {
  const long long npb = (a.ph_s + NC - 1) / NC, nblk = a.N2 / (kNSEQ / NC);
  const long long blocks = pairs * nblk * a.C * npb;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  LongArgs b = a;
  b.d_ncb = make_fastdiv((unsigned)npb);
  b.d_nblk = make_fastdiv((unsigned)nblk);
  b.d_c = make_fastdiv((unsigned)a.C);
  return launch_kernel<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO, true, false, NC, true>>(blocks, kNT, kLds, st, b);
}

template <int IO>
hipError_t phs_inv_pick(const LongArgs& a, long long pairs, hipStream_t st) {
  if constexpr (kPhsWide > 2) {
    if ((a.ph_s + 3) / 4 * 4 <= (a.ph_s + 1) / 2 * 2) return phs_inv_launch<IO, kPhsWide>(a, pairs, st);
  }
  return phs_inv_launch<IO, 2>(a, pairs, st);
}

// ---- decimation (long1d.hpp).  The filter rows of a decimation plan: the plain block map, one build per element type
template <int IO>
hipError_t dec_filter_launch(const LongArgs& a, long long rows, hipStream_t st) {
  LongArgs b = a;
  b.d_ph_s = make_fastdiv((unsigned)a.ph_s);
  return launch<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO, false, false, 0, false, true>>(b, a.N2 / kNSEQ, rows * a.C, st);
}

// The signal rows: NC decimated rows of one input channel x kNSEQ / NC neighbouring n2 columns per workgroup, a.C channels
// of the tensor.  The two widths and the rule that picks between them are those of the phases inverse pass above
template <int IO, int NC>
hipError_t dec_signal_launch(const LongArgs& a, long long pairs, hipStream_t st) {
  const long long npb = (a.ph_s + NC - 1) / NC, nblk = a.N2 / (kNSEQ / NC);
  const long long blocks = pairs * nblk * a.C * npb;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  LongArgs b = a;
  b.d_ncb = make_fastdiv((unsigned)npb);
  b.d_nblk = make_fastdiv((unsigned)nblk);
  b.d_c = make_fastdiv((unsigned)a.C);
  return launch_kernel<long_cols_fwd_kernel<FC_P, FC_S, kNSEQ, kNT, IO, false, false, NC, false, true>>(blocks, kNT, kLds, st, b);
}

template <int IO>
hipError_t dec_signal_pick(const LongArgs& a, long long pairs, hipStream_t st) {
  if constexpr (kPhsWide > 2) {
    if ((a.ph_s + 3) / 4 * 4 <= (a.ph_s + 1) / 2 * 2) return dec_signal_launch<IO, kPhsWide>(a, pairs, st);
  }
  return dec_signal_launch<IO, 2>(a, pairs, st);
}

// a column pass over `rows` rows of the transform per channel (LongImpl); the element type is that of the tensor the
// pass touches.  A channels-last launch never reads filter rows
template <bool INV>
hipError_t cols_dispatch(const LongArgs& a, bool mapped, bool nlc, long long rows, hipStream_t st) {
  if (a.N1 != kT || rows <= 0 || a.C <= 0 || (nlc && a.from_kernel)) return hipErrorInvalidValue;
  const int code = INV ? a.y_io : a.src_io;
  if (a.ph_s > 0 && a.ph_cog > 0 && (INV || a.from_kernel)) {      // (the signal rows of a phases plan are plain rows)
    if (mapped || nlc || a.ph_cog <= 0) return hipErrorInvalidValue;
    if constexpr (INV) {
      if (code == 0) return phs_inv_pick<IO_F32>(a, rows, st);
      if (io_is_h16(code)) return phs_inv_pick<IO_H16>(a, rows, st);
    } else {
      if (code == 0) return phs_filter_launch<IO_F32>(a, rows, st);
      if (io_is_h16(code)) return phs_filter_launch<IO_H16>(a, rows, st);
    }
    return hipErrorInvalidValue;
  }
  if constexpr (!INV) {
    if (a.ph_s > 0 && a.ph_cog == 0) {      // (a decimation plan)
      if (mapped || nlc) return hipErrorInvalidValue;
      if (code == 0) return a.from_kernel ? dec_filter_launch<IO_F32>(a, rows, st) : dec_signal_pick<IO_F32>(a, rows, st);
      if (io_is_h16(code)) return a.from_kernel ? dec_filter_launch<IO_H16>(a, rows, st) : dec_signal_pick<IO_H16>(a, rows, st);
      return hipErrorInvalidValue;
    }
  }
  if (code == 0) return cols_launch<INV, IO_F32, false>(a, mapped, nlc, rows, st);
  if (io_is_h16(code)) return cols_launch<INV, IO_H16, false>(a, mapped, nlc, rows, st);
  if (code == IO_CODE_C64) return cols_launch<INV, IO_F32, true>(a, mapped, nlc, rows, st);
  return hipErrorInvalidValue;
}

// the inverse pass of the weight gradient: one item, a.C rows of dW, the element type of dW
hipError_t wgrad_inv(const LongArgs& a, hipStream_t st) {
  if (a.N1 != kT || a.C <= 0 || a.B != 1 || a.pair0 != 0) return hipErrorInvalidValue;
  if (a.y_io == 0)
    return launch<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32, true, false, 0, false, true>>(a, a.N2 / kNSEQ, a.C, st);
  if (io_is_h16(a.y_io))
    return launch<long_cols_inv_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16, true, false, 0, false, true>>(a, a.N2 / kNSEQ, a.C, st);
  return hipErrorInvalidValue;
}

// ---- gates (long1d.hpp LongGates): the gated builds of the two column passes, float32 and 16-bit, the plain block map.
// They take the gates as a second kernel argument; every other build keeps the one it had
template <bool INV>
hipError_t cols_gated(const LongArgs& a, const LongGates& gt, long long rows, hipStream_t st) {
  if (a.N1 != kT || rows <= 0 || a.C <= 0 || a.from_kernel || a.ph_s > 0) return hipErrorInvalidValue;
  if (INV ? (gt.gate2 && !gt.y2) || (gt.y2_f32 && (gt.gate2 || !gt.y2)) : !gt.pregate) return hipErrorInvalidValue;
  LongArgs b = a;
  b.d_nblk = make_fastdiv((unsigned)(a.N2 / kNSEQ));
  b.d_c = make_fastdiv((unsigned)a.C);
  const long long grid = rows * a.C * (a.N2 / kNSEQ);
  const int code = INV ? a.y_io : a.src_io;
  if constexpr (INV) {
    if (code == 0) return launch_kernel<long_cols_inv_gated_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32>>(grid, kNT, kLds, st, b, gt);
    if (io_is_h16(code)) return launch_kernel<long_cols_inv_gated_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16>>(grid, kNT, kLds, st, b, gt);
  } else {
    if (code == 0) return launch_kernel<long_cols_fwd_gated_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32>>(grid, kNT, kLds, st, b, gt);
    if (io_is_h16(code)) return launch_kernel<long_cols_fwd_gated_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16>>(grid, kNT, kLds, st, b, gt);
  }
  return hipErrorInvalidValue;
}

// ---- blocks (long1d.hpp LongBlocks): the blocks builds of the two column passes, float32 and 16-bit, the plain block
// map over `rows` unit pairs.  They take the block map as a second kernel argument; every other build keeps the one it had
template <bool INV>
hipError_t cols_blocks(const LongArgs& a, const LongBlocks& bk, long long rows, hipStream_t st) {
  if (a.N1 != kT || rows <= 0 || a.C <= 0 || a.from_kernel || a.ph_s > 0) return hipErrorInvalidValue;
  if (bk.U <= 0 || bk.hop <= 0 || bk.d_T.d == 0 || (!INV && bk.win <= 0)) return hipErrorInvalidValue;
  const long long grid = rows * a.C * (a.N2 / kNSEQ);
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  LongArgs b = a;
  b.d_nblk = make_fastdiv((unsigned)(a.N2 / kNSEQ));
  b.d_c = make_fastdiv((unsigned)a.C);
  const int code = INV ? a.y_io : a.src_io;
  if constexpr (INV) {
    if (code == 0) return launch_kernel<long_cols_inv_blocks_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32>>(grid, kNT, kLds, st, b, bk);
    if (io_is_h16(code)) return launch_kernel<long_cols_inv_blocks_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16>>(grid, kNT, kLds, st, b, bk);
  } else {
    if (code == 0) return launch_kernel<long_cols_fwd_blocks_kernel<FC_P, FC_S, kNSEQ, kNT, IO_F32>>(grid, kNT, kLds, st, b, bk);
    if (io_is_h16(code)) return launch_kernel<long_cols_fwd_blocks_kernel<FC_P, FC_S, kNSEQ, kNT, IO_H16>>(grid, kNT, kLds, st, b, bk);
  }
  return hipErrorInvalidValue;
}

}  // namespace

#define FC_CAT_(a, b, c, d) a##b##c##d
#define FC_CAT(a, b, c, d) FC_CAT_(a, b, c, d)
const LongImpl* FC_CAT(get_long_P, FC_P, _S, FC_S)() {
  static const LongImpl impl = {kT, kOB, cols_dispatch<false>, rows, cols_dispatch<true>, kWgOB, wgrad_rows, wgrad_inv,
                                cols_gated<false>, cols_gated<true>, cols_blocks<false>, cols_blocks<true>};
  return &impl;
}

}  // namespace fc
