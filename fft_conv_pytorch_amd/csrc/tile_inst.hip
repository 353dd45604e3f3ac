// tile_inst.hip -- instantiates every kernel for ONE tile geometry (P, S).
// Built once per geometry with -DFC_P=.. -DFC_S=.. -DFC_NT=.. (see Makefile) so the
// geometries compile in parallel.
#include "fc_internal.h"
#include "launch.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#ifndef FC_P
#error "compile with -DFC_P=<points per thread> -DFC_S=<lane split> -DFC_NT=<threads of the fused 1-D kernel>"
#endif

namespace fc {
namespace {

using GG = Geo<FC_P, FC_S>;
constexpr int kT = GG::T;
constexpr int kNSEQ_C = (8192 / kT) > 16 ? 16 : ((8192 / kT) < 2 ? 2 : (8192 / kT));
#ifndef FC_ROWS_DIV
#define FC_ROWS_DIV 2
#endif
constexpr int kNSEQ_R = (kNSEQ_C / FC_ROWS_DIV) < 1 ? 1 : (kNSEQ_C / FC_ROWS_DIV);
constexpr int kLSEQP = SeqLayout<GG>::LSEQP;
constexpr int kFusedMaxCib = (8 * kLSEQP * 8 <= 160 * 1024 && 8 * GG::TS <= 1024) ? 8 : 4;

// The float32 or the 16-bit build of a kernel by a launch's `io` code: calls f with IO_F32 or IO_H16 (Io in
// fft_engine.hpp; one 16-bit build serves float16 and bfloat16) as an integral constant.  The host passes no other
// code (fc_dtype of the plan).
template <class F>
hipError_t with_io(int code, F f) {
  if (code == 0) return f(std::integral_constant<int, IO_F32>{});
  if (io_is_h16(code)) return f(std::integral_constant<int, IO_H16>{});
  return hipErrorInvalidValue;
}
#define FC_IO(io) decltype(io)::value

// (the 16-bit builds never run the chunk-by-chunk, segment or profiling launches)
hipError_t conv1d_dispatch(int cib, const Conv1dArgs& a, int grid, size_t lds, hipStream_t st) {
  return with_io(a.io, [&](auto io) {
    switch (cib) {
      case 2: return launch_kernel<conv1d_fused_kernel<FC_P, FC_S, 2, FC_NT, FC_IO(io)>>(grid, FC_NT, lds, st, a);
      case 4: return launch_kernel<conv1d_fused_kernel<FC_P, FC_S, 4, FC_NT, FC_IO(io)>>(grid, FC_NT, lds, st, a);
      case 8: return launch_kernel<conv1d_fused_kernel<FC_P, FC_S, 8, FC_NT, FC_IO(io)>>(grid, FC_NT, lds, st, a);
      default: return hipErrorInvalidValue;
    }
  });
}

hipError_t spec1d_dispatch(const Spec1dArgs& a, int grid, size_t lds, hipStream_t st) {
  return launch_kernel<spectrum1d_kernel<FC_P, FC_S, FC_NT>>(grid, FC_NT, lds, st, a);
}

// first and last pass of the N-d plans: Kernel is a build of rows_r2c_kernel (Args = RowsR2CArgs) or rows_c2r_kernel
constexpr int kNT_R = kNSEQ_R * GG::TS;
// (RB: rows per workgroup -- two per sequence in the real builds, one in the complex ones)
template <auto Kernel, class Args, int RB = 2 * kNSEQ_R>
hipError_t launch_rows(const Args& a, hipStream_t st) {
  const long long nyb = (a.NY + RB - 1) / RB;
  Args b = a;
  b.d_nyb = make_fastdiv((unsigned)nyb); b.d_nxt = make_fastdiv((unsigned)a.nxt); b.d_nc = make_fastdiv((unsigned)a.NC);
  return launch_kernel<Kernel>((long long)a.NA * a.NC * a.nxt * nyb, kNT_R, (size_t)kNSEQ_R * kLSEQP * sizeof(float2), st, b);
}
// Channels-last builds of the two (a.cl_C > 0; rows_r2c_cl_kernel / rows_c2r_cl_kernel): NCH neighbouring channels x
// kNSEQ_R / NCH row pairs per workgroup.  NCH per tile geometry and element size is the one that measured fastest for
// the two launches together (2, 4 and 8 at T = 64, 128, 512; 2 and 4 at 1024): 4, but 2 for 16-bit samples
// at T <= 128.  The 2048- and 4096-point tiles hold two and one sequence and have no such build.  -DFC_CL_NCH=<n> forces
// one count (the A/B builds of that sweep, scripts/nd_channels_last_nch.py).
template <int IO>
constexpr int nch_cl() {
  if (kNSEQ_R < 4) return 0;
#ifdef FC_CL_NCH
  return FC_CL_NCH < kNSEQ_R ? FC_CL_NCH : kNSEQ_R;
#else
  return (IO == IO_H16 && kT <= 128) ? 2 : 4;
#endif
}
constexpr int kNchCl = nch_cl<IO_F32>();      // (TileImpl: nonzero where the builds exist)
template <template <int, int> class K, class Args, int IO>
hipError_t launch_rows_cl_io(const Args& a, hipStream_t st) {
  constexpr int NCH = nch_cl<IO>();
  if constexpr (NCH == 0) {      // (no build, nothing instantiated)
    return hipErrorInvalidValue;
  } else {
    constexpr int RBC = 2 * kNSEQ_R / NCH;
    if (a.cl_C <= 0 || a.NA % a.cl_C) return hipErrorInvalidValue;
    const long long nyb = (a.NY + RBC - 1) / RBC, nchb = (a.cl_C + NCH - 1) / NCH;
    Args b = a;
    b.d_nyb = make_fastdiv((unsigned)nyb); b.d_nxt = make_fastdiv((unsigned)a.nxt); b.d_nc = make_fastdiv((unsigned)a.NC);
    b.d_chb = make_fastdiv((unsigned)nchb);
    const long long grid = (long long)(a.NA / a.cl_C) * nchb * a.NC * a.nxt * nyb;
    return launch_kernel<K<IO, NCH>::kernel>(grid, kNT_R, (size_t)kNSEQ_R * kLSEQP * sizeof(float2), st, b);
  }
}
template <template <int, int> class K, class Args>
hipError_t launch_rows_cl(const Args& a, hipStream_t st) {
  return with_io(a.io, [&](auto io) { return launch_rows_cl_io<K, Args, FC_IO(io)>(a, st); });
}
template <int IO, int NCH> struct R2CCl { static constexpr auto kernel = rows_r2c_cl_kernel<FC_P, FC_S, kNSEQ_R, kNT_R, NCH, IO>; };
template <int IO, int NCH> struct C2RCl { static constexpr auto kernel = rows_c2r_cl_kernel<FC_P, FC_S, kNSEQ_R, kNT_R, NCH, IO>; };

// io == IO_CODE_ND_C64: the complex siblings (a complex64 plan's signal and taps; no row-major pipeline, no accumulating store)
hipError_t rows_r2c_dispatch(const RowsR2CArgs& a, hipStream_t st) {
  if (a.cl_C) {
    if (a.from_kernel || a.im.on) return hipErrorInvalidValue;
    return launch_rows_cl<R2CCl>(a, st);
  }
  if (a.io == IO_CODE_ND_C64) {
    if (a.rowmajor) return hipErrorInvalidValue;
    return launch_rows<rows_c2c_fwd_kernel<FC_P, FC_S, kNSEQ_R, kNT_R>, RowsR2CArgs, kNSEQ_R>(a, st);
  }
  return with_io(a.io, [&](auto io) { return launch_rows<rows_r2c_kernel<FC_P, FC_S, kNSEQ_R, kNT_R, FC_IO(io)>>(a, st); });
}
hipError_t rows_c2r_dispatch(const RowsC2RArgs& a, hipStream_t st) {
  if (a.cl_C) {
    if (a.accum || a.im.on) return hipErrorInvalidValue;
    return launch_rows_cl<C2RCl>(a, st);
  }
  if (a.io == IO_CODE_ND_C64) {
    if (a.rowmajor || a.accum) return hipErrorInvalidValue;
    return launch_rows<rows_c2c_inv_kernel<FC_P, FC_S, kNSEQ_R, kNT_R>, RowsC2RArgs, kNSEQ_R>(a, st);
  }
  return with_io(a.io, [&](auto io) { return launch_rows<rows_c2r_kernel<FC_P, FC_S, kNSEQ_R, kNT_R, FC_IO(io)>>(a, st); });
}

template <bool INV>
hipError_t c2c_dispatch(const C2CArgs& a, hipStream_t st) {
  constexpr int NT = kNSEQ_C * GG::TS;
  const size_t lds = (size_t)kNSEQ_C * kLSEQP * sizeof(float2);
  const long long nbb = (a.NB + kNSEQ_C - 1) / kNSEQ_C;
  const long long grid = (long long)a.NA * a.NC * nbb;
  C2CArgs b = a;
  b.d_nbb = make_fastdiv((unsigned)nbb); b.d_nc = make_fastdiv((unsigned)a.NC);
  if constexpr (INV) return launch_kernel<c2c_inv_kernel<FC_P, FC_S, kNSEQ_C, NT>>(grid, NT, lds, st, b);
  else return launch_kernel<c2c_fwd_kernel<FC_P, FC_S, kNSEQ_C, NT>>(grid, NT, lds, st, b);
}

// fused column pass: NB batch items per workgroup share the spectrum loads.  NB is the largest of
// {4, 2, 1} that fits the batch, 1024 threads, the 160 KiB of LDS and 32 spectrum values per mix
// thread, and still leaves two workgroups per CU's worth of grid.
template <int CIB, int NB>
constexpr bool fusedc_fits() {
  return CIB <= kFusedMaxCib && NB * CIB * GG::TS <= 1024 && NB * CIB <= 32 &&
         (size_t)NB * CIB * kLSEQP * sizeof(float2) <= 160 * 1024;
}
template <int CIB, int NB>
hipError_t launch_fusedc_nb(const FusedCArgs& a, hipStream_t st) {
  if constexpr (!fusedc_fits<CIB, NB>()) {
    return hipErrorInvalidValue;
  } else {
    constexpr int NT = NB * CIB * GG::TS;
    const size_t lds = (size_t)(a.accumulate ? 2 : 1) * NB * CIB * kLSEQP * sizeof(float2);
    const long long nbb = (a.B + NB - 1) / NB;
    const long long grid = nbb * a.ntiles * a.n_ochunks * a.G * ((a.ncol + 7) / 8) * 8;
    FusedCArgs b = a;
    b.d_nbb = make_fastdiv((unsigned)nbb); b.d_ncb = make_fastdiv((unsigned)((a.ncol + 7) / 8));
    b.d_g = make_fastdiv((unsigned)a.G); b.d_noc = make_fastdiv((unsigned)a.n_ochunks);
    return launch_kernel<fusedc_kernel<FC_P, FC_S, CIB, NB, NT>>(grid, NT, lds, st, b);
  }
}
template <int CIB>
hipError_t launch_fusedc(const FusedCArgs& a, hipStream_t st) {
  auto ok = [&](int nb, bool fits) {
    if (!fits || nb > a.B) return false;
    const size_t lds = (size_t)(a.accumulate ? 2 : 1) * nb * CIB * kLSEQP * sizeof(float2);
    const long long grid = (long long)((a.B + nb - 1) / nb) * a.ntiles * a.n_ochunks * a.G * a.ncol;
    return lds <= 160 * 1024 && (nb == 1 || grid >= 512);
  };
  if (ok(4, fusedc_fits<CIB, 4>())) return launch_fusedc_nb<CIB, 4>(a, st);
  if (ok(2, fusedc_fits<CIB, 2>())) return launch_fusedc_nb<CIB, 2>(a, st);
  return launch_fusedc_nb<CIB, 1>(a, st);
}

hipError_t fusedc_dispatch(int cib, const FusedCArgs& a, hipStream_t st) {
  switch (cib) {
    case 2: return launch_fusedc<2>(a, st);
    case 4: return launch_fusedc<4>(a, st);
    case 8: return launch_fusedc<8>(a, st);
    default: return hipErrorInvalidValue;
  }
}

// persistent kernel: only for geometries whose twiddle table + NB*4 sequences fit in LDS
#if FC_P == 32 && FC_S == 2
constexpr int kPersNb0 = 1, kPersNb1 = 2;
#elif FC_P == 32 && FC_S == 1
constexpr int kPersNb0 = 2, kPersNb1 = 4;
#else
constexpr int kPersNb0 = 0, kPersNb1 = 0;
#endif
// (the planner's figure, table included; a build that holds the twiddles in registers is launched with pers::lds_bytes)
constexpr size_t pers_lds_bytes(int nb) { return pers::lds_with_table<FC_P, FC_S>(nb); }

// The build of the batch-sharing kernel (a mask of the pers:: features, conv1d_pers.hpp) that a launch of NB slots
// runs, float32 and 16-bit alike; kNoBuild if there is none.  In the order of precedence:
//   * 16-bit x / y have no segment and no profiling build;
//   * a segment of a long kernel is not profiled;
//   * depthwise phases are neither packed nor profiled;
//   * phases are packed in quads (ph2 == 2; four slots, not profiled: a profiled quad plan runs the pairs) or in pairs
//     (ph2 != 0), both on the P*P tiles only;
//   * the profiling build exists for the plain, the phase and the paired-phase kernel.
constexpr unsigned kNoBuild = ~0u;
unsigned pers_build(const Conv1dArgs& c, int nb) {
  const bool h16 = io_is_h16(c.io), ph = c.ph > 1, dg = c.diag != 0;
  if (c.io != 0 && (!h16 || c.segmented || c.stamps)) return kNoBuild;
  const unsigned io = h16 ? pers::half_io : 0u;
  if (c.segmented) return pers::segments | (dg ? pers::depthwise : 0u);
  if (ph && dg) return io | pers::phases | pers::depthwise;
  const unsigned st = c.stamps ? pers::stamps : 0u;
  if (ph && FC_S == 1 && c.ph2 == 2 && nb == 4 && !st) return io | pers::phases | pers::quads;
  if (ph && FC_S == 1 && c.ph2) return io | pers::phases | pers::pairs | st;
  if (ph) return io | pers::phases | st;
  if (dg) return io | pers::depthwise;
  return io | st;
}

// launches the one of BUILDS that is `build`
template <int NB, unsigned... BUILDS>
hipError_t launch_pers_among(unsigned build, const Conv1dPersArgs& a, int grid, hipStream_t st) {
  constexpr int NT = NB * 4 * GG::TS;
  hipError_t e = hipErrorInvalidValue;
  auto launch = [&](auto b) {
    constexpr unsigned B = decltype(b)::value;
    if constexpr (pers::valid(B, FC_S, 8, NB))      // (pairs: only on the P*P tiles; quads: only with four slots)
      if (build == B) e = launch_kernel<conv1d_pers_kernel<FC_P, FC_S, 8, NB, NT, B>>(grid, NT, pers::lds_bytes<FC_P, FC_S>(B, NB), st, a);
  };
  (launch(std::integral_constant<unsigned, BUILDS>{}), ...);
  return e;
}

// every build of the batch-sharing kernel the library holds
template <int NB>
hipError_t launch_pers(const Conv1dPersArgs& a, int grid, hipStream_t st) {
  if constexpr (NB == 0) {
    return hipErrorInvalidValue;
  } else {
    using namespace pers;
    return launch_pers_among<NB, 0u, stamps, depthwise, segments, segments | depthwise,
                             phases, phases | stamps, phases | depthwise,
                             phases | pairs, phases | pairs | stamps, phases | quads,
                             half_io, half_io | depthwise,
                             half_io | phases, half_io | phases | depthwise,
                             half_io | phases | pairs, half_io | phases | quads>(pers_build(a.c, NB), a, grid, st);
  }
}

hipError_t pers_dispatch(int nb, const Conv1dPersArgs& a, int grid, hipStream_t st) {
  if (nb != 0 && nb == kPersNb0) return launch_pers<kPersNb0>(a, grid, st);
  if (nb != 0 && nb == kPersNb1) return launch_pers<kPersNb1>(a, grid, st);
  return hipErrorInvalidValue;
}

#if FC_P == 32 && (FC_S == 1 || FC_S == 2)
constexpr int kWideNb = 2;
hipError_t wide_dispatch(const Conv1dPersArgs& a, int grid, hipStream_t st) {
  constexpr int NT = kWideNb * 4 * GG::TS;
  return with_io(a.c.io, [&](auto io) {
    return launch_kernel<conv1d_wide_kernel<FC_P, FC_S, kWideNb, NT, FC_IO(io)>>(grid, NT, pers_lds_bytes(kWideNb), st, a);
  });
}
#else
constexpr int kWideNb = 0;
hipError_t wide_dispatch(const Conv1dPersArgs&, int, hipStream_t) { return hipErrorInvalidValue; }
#endif

#if FC_P == 32 && FC_S == 1
constexpr int kWgradNb = 2;
// (the io code names the element type of x and dY)
hipError_t wgrad_dispatch(const WGradArgs& a, int grid, hipStream_t st) {
  constexpr int NT = kWgradNb * 4 * GG::TS;
  const size_t lds = ((size_t)FC_P * GG::N2 + (size_t)kWgradNb * 4 * GG::LSEQ) * sizeof(float2);
  return with_io(a.io, [&](auto io) {
    return launch_kernel<wgrad1d_kernel<FC_P, FC_S, kWgradNb, NT, FC_IO(io)>>(grid, NT, lds, st, a);
  });
}
hipError_t wgrad_diag_dispatch(const WGradArgs& a, int grid, hipStream_t st) {
  constexpr int NT = 8 * GG::TS;
  const size_t lds = ((size_t)FC_P * GG::N2 + (size_t)8 * GG::LSEQ) * sizeof(float2);
  return with_io(a.io, [&](auto io) { return launch_kernel<wgrad1d_diag_kernel<FC_P, FC_S, NT, FC_IO(io)>>(grid, NT, lds, st, a); });
}
#else
constexpr int kWgradNb = 0;
#endif

#if FC_P == 32 && (FC_S == 1 || FC_S == 2)
// many-channel pipeline (1024 and 2048 tiles): channel pairs per workgroup in the two transform kernels
#ifndef FC_DENSE_NSEQ
#define FC_DENSE_NSEQ 8      // measured 64->64, B 8, L 16384, k 129 (1024 tile): forward 21.1 / inverse 33.6 us at 8 (256 threads,
#endif                       // two workgroups per CU), 24.0 / 35.3 us at 16 (512 threads, one per CU); 2048 tile: 8 x 64 threads
constexpr int kDenseNseq = FC_DENSE_NSEQ;
hipError_t dense_dispatch(int which, const DenseArgs& a, hipStream_t st) {
  constexpr int NT = kDenseNseq * GG::TS;
  const size_t lds_fft = (size_t)kDenseNseq * kLSEQP * sizeof(float2);
  if (which == 0 || which == 2) {
    const int nch = which == 0 ? a.Kc : a.Nc;
    const long long ncb = (nch / 2 + kDenseNseq - 1) / kDenseNseq;
    const long long grid = (long long)a.mcount * ncb * a.G;
    return with_io(a.io, [&](auto io) {
      if (which == 0) return launch_kernel<dense_fwd_kernel<FC_P, FC_S, kDenseNseq, NT, FC_IO(io)>>(grid, NT, lds_fft, st, a);
      return launch_kernel<dense_inv_kernel<FC_P, FC_S, kDenseNseq, NT, FC_IO(io)>>(grid, NT, lds_fft, st, a);
    });
  }
  // GEMM: the widest column block that the output channels fill (8 channels per wave), the smallest K chunk that
  // covers the input channels (or 64 and several chunks)
  const int nf = kT / 2 + 1;
  const int nct = a.Nc >= 64 ? 8 : (a.Nc >= 32 ? 4 : 2);
  const int k2n = a.Kc <= 16 ? 4 : (a.Kc <= 32 ? 8 : 16);
  const int mbr = (a.mcount <= 64 && nct >= 4) ? 32 : 128;                    // rows per unit
  const size_t lds = 2 * (size_t)mbr * std::max(8 * k2n + 4, 16 * nct + 4) * sizeof(float);   // two panels (each also holds an output block)
  const long long nmb = (a.mcount + mbr - 1) / mbr, nnb = (a.Nc + 8 * nct - 1) / (8 * nct);
  const long long units = nmb * nnb * nf * a.G;
  // persistent: one workgroup per CU (two with the small unit)
  const long long grid = std::min<long long>(units, (long long)std::max(1, a.cus) * (mbr == 32 ? 2 : 1));
  if (units > 0x7fffffffffffLL) return hipErrorInvalidValue;
#define FC_DENSE_GEMM(N, K, MBR) \
  if (nct == N && k2n == K && mbr == MBR) return launch_kernel<dense_gemm_kernel<N, K, MBR>>(grid, 512, lds, st, a, nf);
  FC_DENSE_GEMM(8, 16, 128) FC_DENSE_GEMM(8, 8, 128) FC_DENSE_GEMM(8, 4, 128)
  FC_DENSE_GEMM(4, 16, 128) FC_DENSE_GEMM(4, 8, 128) FC_DENSE_GEMM(4, 4, 128)
  FC_DENSE_GEMM(2, 16, 128) FC_DENSE_GEMM(2, 8, 128) FC_DENSE_GEMM(2, 4, 128)
  FC_DENSE_GEMM(8, 16, 32) FC_DENSE_GEMM(8, 8, 32) FC_DENSE_GEMM(8, 4, 32)
  FC_DENSE_GEMM(4, 16, 32) FC_DENSE_GEMM(4, 8, 32) FC_DENSE_GEMM(4, 4, 32)
#undef FC_DENSE_GEMM
  return hipErrorInvalidValue;
}
hipError_t dense_spec_dispatch(const DenseSpecArgs& a, hipStream_t st) {
  const size_t total = (size_t)a.G * (a.T / 2 + 1) * a.Kc * a.Nc;
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(dense_spec_kernel<0>, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}
#endif

#if FC_P == 8 && FC_S == 1
// plane-major 3-D pipeline: 64-point transforms on all three axes
hipError_t planes_fwd_dispatch(const PlaneFwdArgs& a, int n_images, hipStream_t st) {
  PlaneFwdArgs b = a;
  if (b.nxt < 1) b.nxt = 1;
  if (b.nyt < 1) b.nyt = 1;
  const long long ntile = (long long)b.nxt * b.nyt;
  const long long grid = (long long)n_images * a.NZ * ntile;
  b.d_nz = make_fastdiv((unsigned)a.NZ); b.d_nt = make_fastdiv((unsigned)ntile); b.d_nx = make_fastdiv((unsigned)b.nxt);
  return with_io(a.io, [&](auto io) { return launch_kernel<planes_fwd_kernel<kPlNT, FC_IO(io)>>(grid, kPlNT, 0, st, b); });
}
hipError_t planes_inv_dispatch(const PlaneInvArgs& a, int n_images, hipStream_t st) {
  PlaneInvArgs b = a;
  if (b.nxt < 1) b.nxt = 1;
  if (b.nyt < 1) b.nyt = 1;
  if (b.nxt * b.nyt == 1) { b.Vx = a.NVx > 0 ? a.NVx : 1; b.Vy = a.NVy > 0 ? a.NVy : 1; }    // (one tile: the whole window)
  const long long ntile = (long long)b.nxt * b.nyt;
  const long long grid = (long long)n_images * a.NZo * ntile;
  b.d_nz = make_fastdiv((unsigned)a.NZo); b.d_nt = make_fastdiv((unsigned)ntile); b.d_nx = make_fastdiv((unsigned)b.nxt);
  return with_io(a.io, [&](auto io) { return launch_kernel<planes_inv_kernel<kPlNT, FC_IO(io)>>(grid, kPlNT, 0, st, b); });
}
template <int NB, bool STAMPS, int NCOLC>
hipError_t launch_colz_n(const ColZArgs& a, hipStream_t st) {
  constexpr int RING = 2;
  if (a.ncol < 16 || a.ncol % 16 || (NCOLC > 0 && a.ncol != NCOLC)) return hipErrorInvalidValue;
  const long long nbp = (a.B + NB - 1) / NB;
  const long long per = (a.ncol / 16 + 7) / 8;                  // column blocks per XCD
  const long long grid = nbp * a.ntiles * a.n_ochunks * a.G * per * 8;
  ColZArgs b = a;
  b.d_nbp = make_fastdiv((unsigned)nbp); b.d_ntiles = make_fastdiv((unsigned)a.ntiles);
  b.d_per = make_fastdiv((unsigned)per); b.d_g = make_fastdiv((unsigned)a.G);
  if (b.hcol <= 0) b.hcol = a.ncol;
  if (b.hcol % 16 || a.ncol % b.hcol) return hipErrorInvalidValue;
  b.d_hcol = make_fastdiv((unsigned)b.hcol);
  return launch_kernel<colz_kernel<NB, RING, STAMPS, NCOLC>>(grid, NB * 128, colz_lds_bytes(NB), st, b);
}
// 3-D pipeline: the column count is the compile-time kPlCols; 2-D pipeline (ncol = Tx/2): the run-time build
template <int NB, bool STAMPS = false>
hipError_t launch_colz(const ColZArgs& a, hipStream_t st) {
  if (a.ncol == kPlCols) return launch_colz_n<NB, STAMPS, kPlCols>(a, st);
  return launch_colz_n<NB, STAMPS, 0>(a, st);
}
// batch items per workgroup: 2 (two workgroups per CU).  4 (one 512-thread workgroup per CU, half the spectrum traffic)
// measured slower at cfgC: mix 28.4 against 21.2 us per workgroup -- its inputs no longer stay in registers across the
// output channels and the mix waits on LDS round trips instead (profiles/r03_experiments.md).  Two threads per sequence
// measured no faster either (112.9 against 108.3 us per forward, block 5 there).
hipError_t colz_dispatch(const ColZArgs& a, hipStream_t st) {
  if (a.B >= 2) return a.stamps ? launch_colz<2, true>(a, st) : launch_colz<2>(a, st);
  return a.stamps ? launch_colz<1, true>(a, st) : launch_colz<1>(a, st);
}
#endif

}  // namespace

#define FC_CAT_(a, b, c, d) a##b##c##d
#define FC_CAT(a, b, c, d) FC_CAT_(a, b, c, d)
const TileImpl* FC_CAT(get_tile_P, FC_P, _S, FC_S)() {
  static const TileImpl impl = {kT, FC_P, FC_S, FC_NT, GG::LSEQ, kLSEQP, kNSEQ_C, kNSEQ_R,
                                conv1d_dispatch, spec1d_dispatch, rows_r2c_dispatch, c2c_dispatch<false>,
                                c2c_dispatch<true>, rows_c2r_dispatch, fusedc_dispatch, kFusedMaxCib,
                                pers_dispatch, {kPersNb0, kPersNb1},
                                {kPersNb0 ? pers_lds_bytes(kPersNb0) : 0, kPersNb1 ? pers_lds_bytes(kPersNb1) : 0},
                                {kPersNb0 * 4 * GG::TS, kPersNb1 * 4 * GG::TS},
                                wide_dispatch, kWideNb, kWideNb ? pers_lds_bytes(kWideNb) : 0,
#if FC_P == 32 && FC_S == 1
                                wgrad_dispatch, wgrad_diag_dispatch,
#else
                                nullptr, nullptr,
#endif
                                kWgradNb,
#if FC_P == 32 && (FC_S == 1 || FC_S == 2)
                                dense_dispatch, dense_spec_dispatch,
#else
                                nullptr, nullptr,
#endif
#if FC_P == 8 && FC_S == 1
                                planes_fwd_dispatch, colz_dispatch, planes_inv_dispatch
#else
                                nullptr, nullptr, nullptr
#endif
                                , kNchCl
  };
  return &impl;
}

}  // namespace fc
