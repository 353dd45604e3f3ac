// conv1d_pers.hpp -- persistent fused 1-D FFT convolution, NB batch items per workgroup.
//
// Same arithmetic as conv1d_fused.hpp (which stays the general fallback), organised for throughput:
//   * work items come from a host-built list; an item is (tile, group, out-chunk, first batch item,
//     number of batch items <= NB).  A workgroup runs up to TWO items back to back (written out twice,
//     not as a loop: hipcc spills the FFT registers around every barrier when the body sits in a loop)
//     and requests the second item's input samples while the first is in its inverse passes, so the
//     HBM reads of one item hide behind the arithmetic of the other;
//   * the NB batch items of an item share every kernel-spectrum load of the mix step, which is what
//     bounds the one-item-per-workgroup kernel (L2 -> L1 traffic of the spectrum);
//   * the pass-A twiddle table lives in LDS for the lifetime of the workgroup -- or, in the four-slot dense builds
//     (pers::reg_twiddles), a thread's 31 entries of it in registers: no table, no copy, no barrier before the first item;
//   * the mix streams the spectrum through two register sets that are both in flight (set A holds step
//     s, set B step s+1; each is refilled with step s+2 right after use); the first two sets of an item
//     are requested before the barrier in front of the mix;
//   * in the phase builds (pers::phases) a dilation d runs as d interleaved phases on the batch-sharing axis (virtual batch
//     B*d against the undilated kernel spectrum).
// Fast-path restrictions (everything else runs conv1d_wide_kernel or conv1d_fused_kernel): a single
// input-channel chunk (Cin/groups <= CIB), full output chunks (Cout/groups a multiple of CIB), stride 1.
#pragma once
#include "conv1d_fused.hpp"

namespace fc {

struct WorkItem {
  int b0, nbc, tile, goc;   // goc = g * n_ochunks + oc
};

struct Conv1dPersArgs {
  Conv1dArgs c;
  const WorkItem* items;
  int n_items;
};

// profiling hook: lane 0 of EVERY wave records the 100 MHz wall clock, [item][wave (16 slots)][stamp (16 slots)]
__device__ __forceinline__ void stamp_item(unsigned long long* buf, int item, int slot) {
  if (buf != nullptr && (threadIdx.x & 63) == 0)
    buf[((size_t)item * 16 + (threadIdx.x >> 6)) * 16 + slot] = __builtin_amdgcn_s_memrealtime();
}
// same with the shader clock counter (slots 12 / 13 bracket an item: cycles per 100 MHz tick = the clock the CU held)
__device__ __forceinline__ void stamp_clock(unsigned long long* buf, int item, int slot) {
  if (buf != nullptr && (threadIdx.x & 63) == 0)
    buf[((size_t)item * 16 + (threadIdx.x >> 6)) * 16 + slot] = __builtin_amdgcn_s_memtime();
}

// The build of the kernel is a mask of the features below (template parameter BUILD; a launch names the features it
// switches on, `pers::phases | pers::pairs`).  The plain build (0) keeps its immediate offsets and is the only one the
// headline configuration runs.
namespace pers {
constexpr unsigned phases = 1;       // a dilation d runs as d interleaved phases on the batch-sharing axis (see above)
// pairs (with phases, an even number of phases): the two sequences of a wave are the phases 2j and 2j+1 of ONE channel
// pair instead of two channel pairs of one phase, so that a lane can load / store both phases' samples of a position
// as 8 bytes and trade halves with its partner lane (v_permlane32_swap): half the memory instructions, each
// touching half the cache lines of the 4-byte accesses at a 4*d-byte pitch.
constexpr unsigned pairs = 2;
// quads (with phases, a multiple of four phases, 8 -> 8 channel blocks, four slots): the packing is turned round -- a complex
// sequence carries two PHASES of ONE channel, a wave owns one channel and its two halves the phase pairs (0,1) and (2,3) --
// so a lane loads / stores all four phases of a position as 16 contiguous bytes (full cache lines per wave-instruction, where
// the pairs' 8 bytes at a 16-byte pitch cost partial-line write-backs and re-fetches: 1.6x the output bytes written at cfgD).
// The mix contracts the same 8 x 8 matrix per bin; its slots are phases and its steps single output channels.
constexpr unsigned quads = 4;
constexpr unsigned depthwise = 8;    // every channel meets only its own kernel (blocks of 8 channels)
constexpr unsigned segments = 16;    // a segment of the taps of a long kernel: shifted source, later segments add to y
// stamps: the profiling hook (fc_forward_stamped) is a build of its own -- compiled into the product kernel, even
// switched off, its guarded stores made hipcc put a full s_waitcnt vmcnt(0) between the two items of a workgroup
// (a pending store's registers are reused), i.e. a wait for every output store of the first item.
constexpr unsigned stamps = 32;
constexpr unsigned half_io = 64;     // x and y are 16-bit (Io<IO_H16>: float16 or bfloat16 by the launch's `io` code)
// the combinations that exist: pairs and quads are phase builds on a P*P tile with 8-channel blocks, quads fill
// a workgroup of four slots and exclude pairs
constexpr bool valid(unsigned build, int S, int CIB, int NB) {
  const bool packable = (build & phases) && !(build & (depthwise | segments)) && S == 1 && CIB == 8;
  if ((build & pairs) && !packable) return false;
  if ((build & quads) && !(packable && !(build & pairs) && NB == 4)) return false;
  return build < 2 * half_io;
}
}  // namespace pers

// LDS image of a workgroup of NB slots (four sequences each), with the pass-A twiddle table in front of the sequences.
// The four-slot dense builds on the P*P tile (batch pairs: no phases, not depthwise) run one workgroup per CU whatever
// they do -- their sequences alone are past half of the CU's 160 KB -- and have registers to spare at the two waves per
// SIMD that their 512 threads make (212 of 256): they hold the item-invariant pass-A twiddles in registers, so their
// image has no table.  (The phase builds and the 2048-point tile sit at 214 .. 236 VGPRs and would spill the 62.)
namespace pers {
template <int P, int S>
constexpr size_t lds_with_table(int nb) { return ((size_t)P * Geo<P, S>::N2 + (size_t)nb * 4 * Geo<P, S>::LSEQ) * sizeof(f2); }
template <int P, int S>
constexpr bool reg_twiddles(unsigned build, int nb) {
  return lds_with_table<P, S>(nb) > 80 * 1024 && S == 1 && nb >= 2 && !(build & (phases | depthwise));
}
template <int P, int S>
constexpr size_t lds_bytes(unsigned build, int nb) {
  return lds_with_table<P, S>(nb) - (reg_twiddles<P, S>(build, nb) ? (size_t)P * Geo<P, S>::N2 * sizeof(f2) : 0);
}
}  // namespace pers

template <int P, int S, int CIB, int NB, int NT, unsigned BUILD>
__global__ __launch_bounds__(NT, 2) void conv1d_pers_kernel(const Conv1dPersArgs pa) {
  static_assert(pers::valid(BUILD, S, CIB, NB), "no such build: see pers::valid");
  constexpr bool PHASES = (BUILD & pers::phases) != 0, PH2 = (BUILD & pers::pairs) != 0, PH4 = (BUILD & pers::quads) != 0;
  constexpr bool DIAG = (BUILD & pers::depthwise) != 0, SEG = (BUILD & pers::segments) != 0, STAMPS = (BUILD & pers::stamps) != 0;
  constexpr int IO = (BUILD & pers::half_io) ? IO_H16 : IO_F32;
  // Batch pairs (the dense builds without phases, two slots or more): a complex sequence carries ONE channel of TWO slots,
  // slot 2j in the real and slot 2j+1 in the imaginary part; sequence (pair j, channel c) at j * CIB + c.  A real kernel
  // acts on both parts alike, so the mix contracts the packed spectra as they are, Y[o][f] = sum_c H[o][c][f] Z[c][f],
  // without separating the two real spectra first and re-packing them afterwards as the channel pairs need it.
  constexpr bool BPAIR = !(BUILD & (pers::phases | pers::depthwise)) && NB >= 2;
  constexpr int RING = 2;                   // spectrum register sets of the mix
  using G = Geo<P, S>;
  constexpr int T = G::T;
  constexpr int NPI = CIB / 2;
  constexpr int NSEQ = NB * NPI;
  static_assert(NT == NSEQ * G::TS, "one thread slot per point group of every sequence");
  static_assert((T / 2) % NT == 0, "bin pairs divide evenly over the threads");
  static_assert(NPI % 2 == 0, "the spectrum pipeline alternates two register sets");
  static_assert(NB * CIB * 2 <= 64, "the self-paired bins are handled by one wave");
  constexpr int BP = (T / 2) / NT;          // bin pairs per thread
  constexpr int TWN = P * G::N2;            // pass-A twiddle table entries
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const Conv1dArgs& a = pa.c;
  const Io<IO> io(a.io);
  constexpr unsigned ES = Io<IO>::B;         // bytes per sample of x and y
  auto stampi = [&](int item, int slot) { if constexpr (STAMPS) stamp_item(a.stamps, item, slot); };
  auto stampc = [&](int item, int slot) { if constexpr (STAMPS) stamp_clock(a.stamps, item, slot); };
  const int nph = PHASES ? a.ph : 1;          // dilation phases (compile-time 1 in the plain build)

  const int tid = threadIdx.x;
  const int sq = tid / G::TS;               // sequence slot: batch slot nb, channel pair p
  const int tseq = tid % G::TS;
  static_assert(G::TS <= 64 && (NPI * G::TS) % 64 == 0, "a batch slot is a whole number of wavefronts");
  // batch slot and channel pair of this thread's sequence: slot wave-uniform, except with PH2 where the two halves of
  // a wave are slots 2j and 2j+1 (even / odd phase) of pair wave % 4
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // (PH4: nb = phase pair of this half-wave, pr = the wave's channel, sequence (pair, channel) at pair * 8 + channel)
  // (BPAIR: nb = the even slot 2j of this sequence's pair, wave-uniform too; pr = its channel; sequence j * CIB + pr)
  const int nb = PH4 ? ((tid >> 5) & 1) : (PH2 ? 2 * (wv / NPI) + ((tid >> 5) & 1)
               : (BPAIR ? 2 * __builtin_amdgcn_readfirstlane(tid / (CIB * G::TS)) : __builtin_amdgcn_readfirstlane(tid / (NPI * G::TS))));
  const int pr = PH4 ? wv : (PH2 ? wv % NPI : (BPAIR ? sq % CIB : sq % NPI));
  constexpr bool REGTW = pers::reg_twiddles<P, S>(BUILD, NB);   // pass-A twiddles in registers, no table in LDS
  f2* twl = lds;
  f2* zbuf = lds + (REGTW ? 0 : TWN);       // [NSEQ][LSEQ], sequence (slot, pair) at slot * NPI + pair
  f2* zseq = PH4 ? zbuf + (nb * 8 + pr) * G::LSEQ : zbuf + (nb * NPI + pr) * G::LSEQ;

  const PadMap pm = make_padmap(a.pad_mode, a.L);
  const BufRsrc twB = make_rsrc(a.twB, (unsigned)(S * P * 8));
  const size_t wgroup = (size_t)a.Cog_pad * (a.Cig_pad / 2) * (T / 2);   // float4 per group

  // ---- input samples of one item -> registers (unrolled buffer loads; border tiles get per-sample
  // padded / out-of-range offsets).  Only requests: nothing waits here.
  // Dilation d (stride 1) runs as d interleaved phases: y[t*d + p] = sum_k w[k] x[(t + k)*d + p] is an
  // undilated convolution of the phase-p samples, and all phases use the same spectrum -- so they ride
  // the batch-sharing axis as a virtual batch of B*d items (slot vb -> batch vb / d, phase vb % d).
  auto fetch = [&](const WorkItem& wi, f2 (&v)[P]) {
    if constexpr (BPAIR) {
      // channel pr of slot nb (real part) and of slot nb + 1 (imaginary part); a slot past the item's last one and a
      // channel past the group's last one read zeros (an offset outside the resource)
      const int g = wi.goc / a.n_ochunks;
      const int bA = a.slot_tiles ? wi.b0 : wi.b0 + nb, bB = a.slot_tiles ? bA : bA + 1;
      const int tA = a.slot_tiles ? wi.tile + nb : wi.tile, tB = a.slot_tiles ? tA + 1 : tA;
      const int bfirst = wi.b0, blast = a.slot_tiles ? bfirst : wi.b0 + wi.nbc - 1;
      const int posA = tA * a.V - a.pad + (SEG ? a.pos_shift : 0), posB = tB * a.V - a.pad + (SEG ? a.pos_shift : 0);
      const bool interior = (posA >= 0) && (posA + (T - 1) < a.L) && (posB >= 0) && (posB + (T - 1) < a.L);
      const auto* xbase = io_ptr<IO>(a.x) + ((size_t)bfirst * a.Cin + (size_t)g * a.Cig) * a.L;
      const BufRsrc xg = make_rsrc(xbase, (unsigned)(((size_t)(blast - bfirst) * a.Cin + a.Cig) * a.L * ES));
      const bool hasA = nb < wi.nbc && pr < a.Cig, hasB = nb + 1 < wi.nbc && pr < a.Cig;
      const unsigned roA = ((unsigned)(bA - bfirst) * (unsigned)a.Cin + (unsigned)pr) * (unsigned)a.L * ES;
      const unsigned roB = ((unsigned)(bB - bfirst) * (unsigned)a.Cin + (unsigned)pr) * (unsigned)a.L * ES;
      if (interior && hasB) {
        const unsigned v0 = roA + (unsigned)(posA + tseq) * ES, v1 = roB + (unsigned)(posB + tseq) * ES;
#pragma unroll
        for (int n1 = 0; n1 < P; ++n1) {
          v[n1].x = io.load(xg, v0, G::N2 * n1 * ES);
          v[n1].y = io.load(xg, v1, G::N2 * n1 * ES);
        }
      } else {
#pragma unroll
        for (int n1 = 0; n1 < P; ++n1) {
          v[n1].x = io.load(xg, padded_offset<ES>(roA, posA + G::N2 * n1 + tseq, a.L, a.pad, pm, hasA), 0);
          v[n1].y = io.load(xg, padded_offset<ES>(roB, posB + G::N2 * n1 + tseq, a.L, a.pad, pm, hasB), 0);
        }
      }
      return;
    }
    const int g = wi.goc / a.n_ochunks;
    const int vb = a.slot_tiles ? wi.b0 : wi.b0 + nb;
    const int tile = a.slot_tiles ? wi.tile + nb : wi.tile;
    const int bfirst = wi.b0 / nph, blast = a.slot_tiles ? bfirst : (wi.b0 + wi.nbc - 1) / nph;
    const int b = vb / nph, phase = vb - b * nph;
    const int pos0 = tile * a.V * nph + phase - a.pad + (SEG ? a.pos_shift : 0);   // source position of the tile's first sample
    const bool interior = (pos0 >= 0) && (pos0 + (T - 1) * nph < a.L);
    const bool act_in = nb < wi.nbc;
    const auto* xbase = io_ptr<IO>(a.x) + ((size_t)bfirst * a.Cin + (size_t)g * a.Cig) * a.L;
    const BufRsrc xg = make_rsrc(xbase, (unsigned)(((size_t)(blast - bfirst) * a.Cin + a.Cig) * a.L * ES));
    const int ci0 = 2 * pr;
    // (a depthwise plan's last block may reach past the last channel)
    const bool has0 = act_in && ci0 < a.Cig && (!DIAG || g * CIB + ci0 < a.Cin);
    const bool has1 = act_in && ci0 + 1 < a.Cig && (!DIAG || g * CIB + ci0 + 1 < a.Cin);
    const unsigned ro0 = ((unsigned)(b - bfirst) * (unsigned)a.Cin + (unsigned)ci0) * (unsigned)a.L * ES;
    const unsigned ro1 = ro0 + (unsigned)a.L * ES;
    if constexpr (PH4) {
      // wave = channel pr of batch item bA, phases phA .. phA + 3 (phA a multiple of 4: items hold four slots)
      const int bA = wi.b0 / nph, phA = wi.b0 - bA * nph;
      const int posA = wi.tile * a.V * nph + phA - a.pad;
      const bool all_in = (posA >= 0) && (posA + 3 + (T - 1) * nph < a.L);
      const bool chan = pr < a.Cig;
      const unsigned rA = ((unsigned)(bA - bfirst) * (unsigned)a.Cin + (unsigned)pr) * (unsigned)a.L * ES;
      // 4-sample accesses need the row base and the tile position on 4-sample boundaries (uniform test; else 1-sample loads)
      const bool al16 = (((size_t)xbase | ((size_t)a.L * ES) | ((size_t)(unsigned)posA * ES)) & (4 * ES - 1)) == 0;
      if (all_in && al16) {
        const unsigned q0 = chan ? rA + (unsigned)(posA + (tid & 63) * nph) * ES : 0x80000000u;
        const unsigned step4 = 64u * ES * (unsigned)nph;
#pragma unroll
        for (int m = 0; m < P / 2; ++m) {
          const f4 q = io.load4(xg, q0, step4 * m);
          v[2 * m] = q.xy; v[2 * m + 1] = q.zw;
        }
        return;        // (the halves are traded in fetch_finish)
      }
      // border tiles / unaligned rows: per-sample padded loads of this half-wave's two phases
      const unsigned ro = ((unsigned)(bA - bfirst) * (unsigned)a.Cin + (unsigned)pr) * (unsigned)a.L * ES;
#pragma unroll
      for (int n1 = 0; n1 < P; ++n1) {
        const int pos = posA + 2 * nb + (G::N2 * n1 + tseq) * nph;
        v[n1].x = io.load(xg, padded_offset<ES>(ro, pos, a.L, a.pad, pm, chan), 0);
        v[n1].y = io.load(xg, padded_offset<ES>(ro, pos + 1, a.L, a.pad, pm, chan), 0);
      }
      return;
    }
    if constexpr (PH2) {
      // even slot of this wave (wave-uniform), its batch item and (even) phase; the odd slot is the next phase
      const int vbA = wi.b0 + 2 * (wv / NPI), bA = vbA / nph, phA = vbA - bA * nph;
      const int posA = wi.tile * a.V * nph + phA - a.pad;
      const bool both_in = (posA >= 0) && (posA + 1 + (T - 1) * nph < a.L);
      if (both_in && __all(has1)) {
        // lane L of the wave asks for (phase, phase + 1) at the positions 64 m + L, m = 0 .. P/2 - 1; the swap hands
        // lanes 0-31 (even phase) the even-phase halves of both lane groups and lanes 32-63 the odd-phase halves:
        // rows n1 = 2m and 2m + 1 of this thread's sequence
        const unsigned rA = ((unsigned)(bA - bfirst) * (unsigned)a.Cin + (unsigned)ci0) * (unsigned)a.L * ES;
        const unsigned q0 = rA + (unsigned)(posA + (tid & 63) * nph) * ES, q1 = q0 + (unsigned)a.L * ES;
        const unsigned step2 = 64u * ES * (unsigned)nph;
#pragma unroll
        for (int m = 0; m < P / 2; ++m) {
          f2 cx = io.load2(xg, q0, step2 * m), cy = io.load2(xg, q1, step2 * m);
          v[2 * m].x = cx.x; v[2 * m + 1].x = cx.y; v[2 * m].y = cy.x; v[2 * m + 1].y = cy.y;
        }
        return;        // (the halves are traded in fetch_finish, when the item starts: here nothing may wait for the loads)
      }
    }
    if (interior && has1 && !PHASES) {
      const unsigned v0 = ro0 + (unsigned)(pos0 + tseq) * ES, v1 = ro1 + (unsigned)(pos0 + tseq) * ES;
#if FC_DIAG == 7
#pragma unroll
      for (int n1 = 0; n1 < P; ++n1) { v[n1] = mk2(1e-3f * n1, (float)tseq); asm volatile("" : "+v"(v[n1])); }
      (void)v0; (void)v1;
      return;
#endif
#pragma unroll
      for (int n1 = 0; n1 < P; ++n1) {
        v[n1].x = io.load(xg, v0, G::N2 * n1 * ES);
        v[n1].y = io.load(xg, v1, G::N2 * n1 * ES);
      }
    } else if (interior && has1) {
      const unsigned v0 = ro0 + (unsigned)(pos0 + tseq * nph) * ES, v1 = ro1 + (unsigned)(pos0 + tseq * nph) * ES;
      const unsigned step = (unsigned)(G::N2 * ES) * (unsigned)nph;
#pragma unroll
      for (int n1 = 0; n1 < P; ++n1) {
        v[n1].x = io.load(xg, v0, step * n1);
        v[n1].y = io.load(xg, v1, step * n1);
      }
    } else {
#pragma unroll
      for (int n1 = 0; n1 < P; ++n1) {
        const int pos = pos0 + (G::N2 * n1 + tseq) * nph;
        v[n1].x = io.load(xg, padded_offset<ES>(ro0, pos, a.L, a.pad, pm, has0), 0);
        v[n1].y = io.load(xg, padded_offset<ES>(ro1, pos, a.L, a.pad, pm, has1), 0);
      }
    }
  };

  // second half of a paired-phase fetch, run when the item starts (its loads have long landed): the partner lanes trade
  // the halves they loaded for each other.  Recomputes which path fetch() took for this item.
  auto fetch_finish = [&](const WorkItem& wi, f2 (&v)[P]) {
    if constexpr (PH4) {
      // lanes 0-31 keep (phase 0, 1) of the positions both lane groups loaded, lanes 32-63 get (phase 2, 3)
      const int bA = wi.b0 / nph, phA = wi.b0 - bA * nph;
      const int posA = wi.tile * a.V * nph + phA - a.pad;
      const int bfirst = wi.b0 / nph;
      const auto* xbase = io_ptr<IO>(a.x) + ((size_t)bfirst * a.Cin + (size_t)(wi.goc / a.n_ochunks) * a.Cig) * a.L;
      const bool all_in = (posA >= 0) && (posA + 3 + (T - 1) * nph < a.L);
      const bool al16 = (((size_t)xbase | ((size_t)a.L * ES) | ((size_t)(unsigned)posA * ES)) & (4 * ES - 1)) == 0;
      if (all_in && al16) {
#pragma unroll
        for (int m = 0; m < P / 2; ++m) { swap_halves_c<0>(v[2 * m], v[2 * m + 1]); swap_halves_c<1>(v[2 * m], v[2 * m + 1]); }
      }
    }
    if constexpr (PH2) {
      const bool has1 = nb < wi.nbc && 2 * pr + 1 < a.Cig;
      const int vbA = wi.b0 + 2 * (wv / NPI), bA = vbA / nph, phA = vbA - bA * nph;
      const int posA = wi.tile * a.V * nph + phA - a.pad;
      const bool both_in = (posA >= 0) && (posA + 1 + (T - 1) * nph < a.L);
      if (both_in && __all(has1)) {
#pragma unroll
        for (int m = 0; m < P / 2; ++m) { swap_halves_c<0>(v[2 * m], v[2 * m + 1]); swap_halves_c<1>(v[2 * m], v[2 * m + 1]); }
      }
    }
  };

  // ---- one item: forward FFT, mix, [request the next item's samples], inverse FFT, store
  f2 twr[P];                                // REGTW: twA[k1 * N2 + tseq], k1 = 1 .. P - 1, for both items and all four passes
  auto run = [&](const WorkItem& wi, int it, f2 (&v)[P], bool more, const WorkItem& wnext, f2 (&vnext)[P], auto firstc) {
    const int g = wi.goc / a.n_ochunks, oc = wi.goc % a.n_ochunks;
    const bool act_in = PH4 ? true : nb < wi.nbc;          // (phase quads: every item holds its four slots)
    // DIAG (depthwise): the spectrum is [channel pair][T/2] float4 = {H(2p)[f], H(2p+1)[f]}, 8 channels per block g
    const BufRsrc wg = DIAG ? make_rsrc(a.wspec + (size_t)g * NPI * (T / 2), (unsigned)(NPI * (T / 2) * 16))
                            : make_rsrc(a.wspec + (size_t)g * wgroup, (unsigned)(wgroup * 16));
    stampi(it, 0);
    stampc(it, 12);
    // bias of this lane's two output channels, requested now and used in the last pass
    const int cg0 = g * a.Cog + oc * a.cob + ((PH4 || BPAIR) ? pr : 2 * pr);     // (PH4: one output channel per wave, BPAIR: per sequence)
    const bool ok0 = !DIAG || cg0 < a.Cout, ok1 = !BPAIR && (!DIAG || cg0 + 1 < a.Cout);
    // (buffer loads: a missing bias is an empty resource, a missing channel an offset outside it -- no branch, so
    // nothing waits for these two values here; they are pinned as arrived after the mix, see below)
    const BufRsrc brs = make_rsrc(a.bias, a.bias ? (unsigned)a.Cout * 4u : 0u);
    float bias0 = buf_load_f32(brs, ok0 ? (unsigned)cg0 * 4u : 0xFFFFFFFFu, 0);
    float bias1 = BPAIR ? 0.f : buf_load_f32(brs, ok1 ? (unsigned)(cg0 + 1) * 4u : 0xFFFFFFFFu, 0);   // (BPAIR: both parts are channel cg0)
    // ------------------------------------------------ forward pass A
    if (STAMPS && a.stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stampi(it, 1); }
    // (act_in is wave-uniform and the two passes of a sequence only need wave-level ordering)
    if constexpr (REGTW && decltype(firstc)::value) {
      // the samples were requested first, the twiddles right behind them: both are declared arrived here, so that no
      // later use of a twiddle waits for younger memory instructions
#pragma unroll
      for (int n1 = 0; n1 < P; ++n1) asm volatile("" : "+v"(v[n1]));
#pragma unroll
      for (int k1 = 1; k1 < P; ++k1) asm volatile("" : "+v"(twr[k1]));
    }
    if (act_in) {
      fetch_finish(wi, v);
      if constexpr (REGTW) passA_fft_twiddle_store_regs<G, -1>(v, zseq, tseq, twr);
      else passA_fft_twiddle_store_lds<G, -1>(v, zseq, tseq, twl);
      stampi(it, 2);
      seq_sync<G>();
      stampi(it, 3);
      // ---------------------------------------------- forward pass B
      passB_load<G>(v, zseq, tseq);
      seq_sync<G>();
      const int j = passB_compute<G, -1>(v, tseq, twB);
      const int k1 = tseq >> G::LGS;
      f2* dst = zseq + G::nat(k1 + P * P * j);
#if FC_DIAG == 2
      { f2 sink = v[0];
#pragma unroll
        for (int k = 1; k < P; ++k) sink += v[k];
        if (sink.x == 123.456f) dst[0] = sink; }
#else
#pragma unroll
      for (int k = 0; k < P; ++k) dst[P * k] = v[k];
#endif
    }
    // ------------------------------------------------ mix, depthwise: every channel meets only its own kernel
    if constexpr (DIAG) {
      f4 wd[BP][NPI];
#pragma unroll
      for (int m = 0; m < BP; ++m)
#pragma unroll
        for (int p = 0; p < NPI; ++p) wd[m][p] = buf_load_f32x4(wg, (unsigned)(tid + m * NT) * 16u, p * (T / 2) * 16);
      // self-paired bins 0 and T/2: lane (batch b, pair p, bin) of wave 0; wspec[p][0] = {Re H_e[0], Re H_e[T/2], Re H_o[0], Re H_o[T/2]}
      const int sd_b = tid / (2 * NPI), sd_p = (tid >> 1) % NPI, sd_f = (tid & 1) ? T / 2 : 0;
      const bool sd_act = tid < NB * NPI * 2 && sd_b < wi.nbc;
      f4 sdw = {0.f, 0.f, 0.f, 0.f};
      if (sd_act) sdw = buf_load_f32x4(wg, 0u, sd_p * (T / 2) * 16);
      stampi(it, 4);
      __syncthreads();
      stampi(it, 5);
      static_for<0, BP>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int f = tid + m * NT;
        const int fm = (T - f) & (T - 1);
        f2 xe[NB][NPI], xo[NB][NPI];
        const unsigned af = lds_off(zbuf + G::nat(f)), ag = lds_off(zbuf + G::nat(fm));
        static_for<0, NB>([&](auto bc) {
          constexpr int b = decltype(bc)::value;
          const unsigned bf = af + b * NPI * G::LSEQ * 8, bg = ag + b * NPI * G::LSEQ * 8;
          static_for<0, NPI>([&](auto pc) {
            constexpr int p = decltype(pc)::value;
            xe[b][p] = lds_rd<p * G::LSEQ * 8>(bf);
            xo[b][p] = lds_rd<p * G::LSEQ * 8>(bg);
          });
        });
#pragma unroll
        for (int b = 0; b < NB; ++b) { lds_arrive(xe[b]); lds_arrive(xo[b]); }
        if (f != 0) {
#pragma unroll
          for (int b = 0; b < NB; ++b)
            if (b < wi.nbc) {
#pragma unroll
              for (int p = 0; p < NPI; ++p) {
                const f2 zf = xe[b][p], zg = xo[b][p];
                const f2 ye = cmul(add_conj(zf, zg), wd[m][p].xy);        // 2 X_even[f] * H_even[f]
                const f2 yo = cmul(sub_conj_divi(zf, zg), wd[m][p].zw);   // 2 X_odd[f]  * H_odd[f]
                f2* zb = zbuf + (b * NPI + p) * G::LSEQ;
                zb[G::nat(f)] = add_pi(ye, yo);
                zb[G::nat(fm)] = conj_add_iconj(ye, yo);
              }
            }
        }
      });
      if (sd_act) {
        f2* zp = zbuf + (sd_b * NPI + sd_p) * G::LSEQ + G::nat(sd_f);
        const f2 z = *zp;
        *zp = mk2(2.f * z.x * ((tid & 1) ? sdw.y : sdw.x), 2.f * z.y * ((tid & 1) ? sdw.w : sdw.z));
      }
    } else if constexpr (PH4) {
    // ------------------------------------------------ mix, phase quads: slots are the four phases, sequence (pair hp, channel c)
    // holds phases 2hp (re) and 2hp+1 (im) of channel c; a step is one output channel (its 8 inputs = 4 float4)
    const unsigned ostride = (unsigned)(a.Cig_pad / 2) * (T / 2) * 16u;
    const unsigned wbase = (unsigned)(oc * a.cob) * ostride;
    constexpr int R4 = 4;
    static_assert(BP == 1, "one bin pair per thread");
    const int sb_s = tid / (2 * CIB), sb_o = (tid >> 1) % CIB, sb_f = (tid & 1) ? T / 2 : 0;     // (phase, output, bin) of wave 0
    const bool sb_act = tid < 4 * CIB * 2;
    f4 sbw[NPI];
    if (sb_act) {
#pragma unroll
      for (int p = 0; p < NPI; ++p) sbw[p] = buf_load_f32x4(wg, (unsigned)sb_o * ostride, wbase + p * (T / 2) * 16);
    }
    f4 w4[R4][NPI];
    auto issue4 = [&](auto oc_) {
      constexpr int o = decltype(oc_)::value;
#pragma unroll
      for (int p = 0; p < NPI; ++p) w4[o % R4][p] = buf_load_f32x4(wg, (unsigned)tid * 16u, wbase + (unsigned)o * ostride + p * (T / 2) * 16);
    };
    static_for<0, R4>([&](auto oc_) { issue4(oc_); });
    stampi(it, 4);
    __syncthreads();
    stampi(it, 5);
    {
      float sbv[CIB];
      if (sb_act) {
#pragma unroll
        for (int c = 0; c < CIB; ++c) {
          const f2 z = zbuf[((sb_s >> 1) * 8 + c) * G::LSEQ + G::nat(sb_f)];
          sbv[c] = (sb_s & 1) ? z.y : z.x;
        }
      }
      const int f = tid, fm = (T - f) & (T - 1);
      f2 xe[2][CIB], xo[2][CIB];          // 2 * X of phase 2hp / 2hp+1 of every channel at bin f
      {
        const unsigned af = lds_off(zbuf + G::nat(f)), ag = lds_off(zbuf + G::nat(fm));
        static_for<0, 2>([&](auto hc) {
          constexpr int hp = decltype(hc)::value;
          static_for<0, CIB>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            xe[hp][c] = lds_rd_far<(hp * 8 + c) * G::LSEQ * 8>(af);
            xo[hp][c] = lds_rd_far<(hp * 8 + c) * G::LSEQ * 8>(ag);
          });
        });
#pragma unroll
        for (int hp = 0; hp < 2; ++hp) { lds_arrive(xe[hp]); lds_arrive(xo[hp]); }
#pragma unroll
        for (int hp = 0; hp < 2; ++hp)
#pragma unroll
          for (int c = 0; c < CIB; ++c) {
            const f2 zf = xe[hp][c], zg = xo[hp][c];
            xe[hp][c] = add_conj(zf, zg);
            xo[hp][c] = sub_conj_divi(zf, zg);
          }
      }
      static_for<0, CIB>([&](auto oc_) {
        constexpr int o = decltype(oc_)::value;
        const f4 (&wc)[NPI] = w4[o % R4];
#pragma unroll
        for (int hp = 0; hp < 2; ++hp) {
          f2 ya = mk2(0.f, 0.f), yb = mk2(0.f, 0.f);
#pragma unroll
          for (int p = 0; p < NPI; ++p) {
            // (ya += xe_a h_a + xe_b h_b ; yb += xo_a h_a + xo_b h_b: two chains, interleaved)
            asm("v_pk_fma_f32 %0, %2, %6, %0 op_sel_hi:[0,1,1]\n\t"
                "v_pk_fma_f32 %1, %4, %6, %1 op_sel_hi:[0,1,1]\n\t"
                "v_pk_fma_f32 %0, %2, %6, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
                "v_pk_fma_f32 %1, %4, %6, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
                "v_pk_fma_f32 %0, %3, %7, %0 op_sel_hi:[0,1,1]\n\t"
                "v_pk_fma_f32 %1, %5, %7, %1 op_sel_hi:[0,1,1]\n\t"
                "v_pk_fma_f32 %0, %3, %7, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
                "v_pk_fma_f32 %1, %5, %7, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
                : "+v"(ya), "+v"(yb)
                : "v"(xe[hp][2 * p]), "v"(xe[hp][2 * p + 1]), "v"(xo[hp][2 * p]), "v"(xo[hp][2 * p + 1]), "v"(wc[p].xy), "v"(wc[p].zw));
          }
          if (f != 0) {
            f2* zb = zbuf + (hp * 8 + o) * G::LSEQ;
            zb[G::nat(f)] = add_pi(ya, yb);
            zb[G::nat(fm)] = conj_add_iconj(ya, yb);
          }
        }
        if constexpr (o + R4 < CIB) issue4(std::integral_constant<int, o + R4>{});
      });
      if (sb_act) {
        float acc = 0.f;
#pragma unroll
        for (int p = 0; p < NPI; ++p) {
          acc = fmaf(2.f * sbv[2 * p], (tid & 1) ? sbw[p].y : sbw[p].x, acc);
          acc = fmaf(2.f * sbv[2 * p + 1], (tid & 1) ? sbw[p].w : sbw[p].z, acc);
        }
        float* dstf = reinterpret_cast<float*>(zbuf + ((sb_s >> 1) * 8 + sb_o) * G::LSEQ + G::nat(sb_f)) + (sb_s & 1);
        *dstf = acc;
      }
    }
    } else if constexpr (BPAIR) {
    // ------------------------------------------------ mix, batch pairs: sequence (pair j, channel c) holds slot 2j (re) and
    // 2j+1 (im) of channel c, and both meet the same real kernel -- the packed spectrum is contracted as it is, bin f
    // against H[f] and bin T-f against conj H[f] (= H[T-f]).  The spectrum holds H/2 (the channel pairs contract 2X):
    // the factor 2 rides on the bias add of the output stores.  Spectrum pipeline and register sets as in the mix below.
    constexpr int NJ = NB / 2;
    const unsigned ostride = (unsigned)(a.Cig_pad / 2) * (T / 2) * 16u;
    const unsigned wbase = (unsigned)(oc * a.cob) * ostride;
    // Self-paired bins 0 and T/2 (H real there; wspec[.][0] = {Re H[0], Re H[T/2]}): lane (pair j, output o, bin)
    // of wave 0 owns one complex output.
    const int sb_j = tid / (2 * CIB), sb_o = (tid >> 1) % CIB, sb_f = (tid & 1) ? T / 2 : 0;
    const bool sb_act = tid < NJ * CIB * 2 && 2 * sb_j < wi.nbc;
    f4 sbw[NPI];
    if (sb_act) {
#pragma unroll
      for (int p = 0; p < NPI; ++p) sbw[p] = buf_load_f32x4(wg, (unsigned)sb_o * ostride, wbase + p * (T / 2) * 16);
    }
    auto issue = [&](int m, int q, f4 (&dst)[2 * NPI]) {
      const unsigned vo = (unsigned)(tid + m * NT) * 16u;
      const unsigned sa = wbase + (unsigned)(2 * q) * ostride, sb = sa + ostride;
#pragma unroll
      for (int p = 0; p < NPI; ++p) {
        dst[2 * p] = buf_load_f32x4(wg, vo, sa + p * (T / 2) * 16);
        dst[2 * p + 1] = buf_load_f32x4(wg, vo, sb + p * (T / 2) * 16);
      }
    };
    f4 wr[RING][2 * NPI];
    static_for<0, RING>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      if constexpr (s < BP * NPI) issue(s / NPI, s % NPI, wr[s]);
    });
    stampi(it, 4);
    __syncthreads();
    stampi(it, 5);
    {
      f2 sbz[CIB];
      if (sb_act) {
#pragma unroll
        for (int c = 0; c < CIB; ++c) sbz[c] = zbuf[(sb_j * CIB + c) * G::LSEQ + G::nat(sb_f)];
      }
      f2 zf[NJ][CIB], zg[NJ][CIB];       // Z of every channel at bins f and T - f
      // one step: outputs 2q and 2q+1 (set entries 2p / 2p+1 hold {H(o, 2p), H(o, 2p+1)} of the even / odd output)
      auto contract = [&](int f, int fm, int q, const f4 (&wc)[2 * NPI]) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            f2 yf, yg;
            cmul2_conj(yf, yg, zf[j][0], zf[j][1], zg[j][0], zg[j][1], wc[e].xy, wc[e].zw);
#pragma unroll
            for (int p = 1; p < NPI; ++p) {
              const f4 h = wc[2 * p + e];
              cmac2_conj(yf, yg, zf[j][2 * p], zf[j][2 * p + 1], zg[j][2 * p], zg[j][2 * p + 1], h.xy, h.zw);
            }
            if (f != 0 && 2 * j < wi.nbc) {
              f2* zb = zbuf + (j * CIB + 2 * q + e) * G::LSEQ;
              zb[G::nat(f)] = yf;
              zb[G::nat(fm)] = yg;
            }
          }
      };
      static_for<0, BP>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int f = tid + m * NT;
        const int fm = (T - f) & (T - 1);
        {
          const unsigned af = lds_off(zbuf + G::nat(f)), ag = lds_off(zbuf + G::nat(fm));
          static_for<0, NJ>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const unsigned bf = af + j * CIB * G::LSEQ * 8, bg = ag + j * CIB * G::LSEQ * 8;
            static_for<0, CIB>([&](auto cc) {
              constexpr int c = decltype(cc)::value;
              zf[j][c] = lds_rd_far<c * G::LSEQ * 8>(bf);
              zg[j][c] = lds_rd_far<c * G::LSEQ * 8>(bg);
            });
          });
#pragma unroll
          for (int j = 0; j < NJ; ++j) { lds_arrive(zf[j]); lds_arrive(zg[j]); }
        }
        static_for<0, NPI>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          constexpr int s = m * NPI + q;               // this step; its set is refilled with step s + RING
          contract(f, fm, q, wr[s % RING]);
          if constexpr (s + RING < BP * NPI) issue((s + RING) / NPI, (s + RING) % NPI, wr[s % RING]);
        });
      });
      if (sb_act) {
        f2 acc = mk2(0.f, 0.f);
#pragma unroll
        for (int p = 0; p < NPI; ++p) {
          const float h0 = (tid & 1) ? sbw[p].y : sbw[p].x, h1 = (tid & 1) ? sbw[p].w : sbw[p].z;
          acc = pkfma(sbz[2 * p], mk2(h0, h0), acc);
          acc = pkfma(sbz[2 * p + 1], mk2(h1, h1), acc);
        }
        zbuf[(sb_j * CIB + sb_o) * G::LSEQ + G::nat(sb_f)] = acc;
      }
    }
    } else {
    // ------------------------------------------------ mix
    // The first two spectrum sets (and the self-paired bins' weights) do not depend on this item's
    // transforms: they are requested BEFORE the barrier and travel while the slower waves finish.
    const unsigned ostride = (unsigned)(a.Cig_pad / 2) * (T / 2) * 16u;
    const unsigned wbase = (unsigned)(oc * a.cob) * ostride;
    // Self-paired bins 0 and T/2 (both spectra real there; wspec[.][0] = {Re H[0], Re H[T/2]}):
    // lane (batch b, output o, bin) of wave 0 owns one real output.
    const int sb_b = tid / (2 * CIB), sb_o = (tid >> 1) % CIB, sb_f = (tid & 1) ? T / 2 : 0;
    const bool sb_act = tid < NB * CIB * 2 && sb_b < wi.nbc;
    f4 sbw[NPI];
    if (sb_act) {
#pragma unroll
      for (int p = 0; p < NPI; ++p) sbw[p] = buf_load_f32x4(wg, (unsigned)sb_o * ostride, wbase + p * (T / 2) * 16);
    }
    // spectrum pipeline: step = (bin pair m, output pair q); two named register sets (static
    // indices), both in flight: set A holds step s, set B step s+1, each is refilled with step s+2
    // right after it has been contracted
    auto issue = [&](int m, int q, f4 (&dst)[2 * NPI]) {
      const unsigned vo = (unsigned)(tid + m * NT) * 16u;
      const unsigned sa = wbase + (unsigned)(2 * q) * ostride, sb = sa + ostride;
#if FC_DIAG == 1
#pragma unroll
      for (int p = 0; p < 2 * NPI; ++p) { f4 c; c.x = 1e-3f * (p + q); c.y = c.x; c.z = c.x; c.w = c.x; asm volatile("" : "+v"(c)); dst[p] = c; }
      return;
#endif
#pragma unroll
      for (int p = 0; p < NPI; ++p) {
        dst[2 * p] = buf_load_f32x4(wg, vo, sa + p * (T / 2) * 16);
        dst[2 * p + 1] = buf_load_f32x4(wg, vo, sb + p * (T / 2) * 16);
      }
    };
    // RING register sets: step s lives in set s % RING; the first RING steps are requested here
    // (RING = 3 fits in 244 VGPRs at NB = 4 but measured no faster than 2: 37.4 vs 36.9 us at cfgA)
    f4 wr[RING][2 * NPI];
    static_for<0, RING>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      if constexpr (s < BP * NPI) issue(s / NPI, s % NPI, wr[s]);
    });
    stampi(it, 4);
#if FC_DIAG != 5
    __syncthreads();
#endif
    stampi(it, 5);
    {
      f2 sbz[NPI];
      if (sb_act) {
#pragma unroll
        for (int p = 0; p < NPI; ++p) sbz[p] = zbuf[(sb_b * NPI + p) * G::LSEQ + G::nat(sb_f)];
      }
      f2 xe[NB][NPI], xo[NB][NPI];       // 2*X of the even / odd channel of every pair
      auto contract = [&](int f, int fm, int q, const f4 (&wc)[2 * NPI]) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          f2 ya = mk2(0.f, 0.f), yb = mk2(0.f, 0.f);
#pragma unroll
          for (int p = 0; p < NPI; ++p) {
            const f4 ha = wc[2 * p], hb = wc[2 * p + 1];
            cmac2x2(ya, yb, xe[b][p], xo[b][p], ha.xy, ha.zw, hb.xy, hb.zw);
          }
          if (f != 0 && b < wi.nbc) {
            f2* zb = zbuf + (b * NPI + q) * G::LSEQ;
            zb[G::nat(f)] = add_pi(ya, yb);
            zb[G::nat(fm)] = conj_add_iconj(ya, yb);
          }
        }
      };
      static_for<0, BP>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int f = tid + m * NT;
        const int fm = (T - f) & (T - 1);
        {
          // all 2*NB*NPI bin reads are requested first (plain ds_read_b64), then combined
          const unsigned af = lds_off(zbuf + G::nat(f)), ag = lds_off(zbuf + G::nat(fm));
          static_for<0, NB>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            const unsigned bf = af + b * NPI * G::LSEQ * 8, bg = ag + b * NPI * G::LSEQ * 8;
            static_for<0, NPI>([&](auto pc) {
              constexpr int p = decltype(pc)::value;
              xe[b][p] = lds_rd<p * G::LSEQ * 8>(bf);
              xo[b][p] = lds_rd<p * G::LSEQ * 8>(bg);
            });
          });
#pragma unroll
          for (int b = 0; b < NB; ++b) { lds_arrive(xe[b]); lds_arrive(xo[b]); }
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int p = 0; p < NPI; ++p) {
              const f2 zf = xe[b][p], zg = xo[b][p];
              xe[b][p] = add_conj(zf, zg);
              xo[b][p] = sub_conj_divi(zf, zg);
            }
        }
        static_for<0, NPI>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          constexpr int s = m * NPI + q;               // this step; its set is refilled with step s + RING
          contract(f, fm, q, wr[s % RING]);
          if constexpr (s + RING < BP * NPI) issue((s + RING) / NPI, (s + RING) % NPI, wr[s % RING]);
        });
      });
      if (sb_act) {
        float acc = 0.f;
#pragma unroll
        for (int p = 0; p < NPI; ++p) {
          acc = fmaf(2.f * sbz[p].x, (tid & 1) ? sbw[p].y : sbw[p].x, acc);
          acc = fmaf(2.f * sbz[p].y, (tid & 1) ? sbw[p].w : sbw[p].z, acc);
        }
        float* dstf = reinterpret_cast<float*>(zbuf + (sb_b * NPI + (sb_o >> 1)) * G::LSEQ + G::nat(sb_f)) + (sb_o & 1);
        *dstf = acc;
      }
    }
    }   // dense / depthwise mix
    stampi(it, 6);
#if FC_DIAG != 5
    __syncthreads();
#endif
    stampi(it, 7);
    // gfx9 counts loads and stores in ONE vmcnt: a value first used after later memory instructions went out through
    // branches gets a full s_waitcnt vmcnt(0).  The bias is therefore declared arrived here (only this item's spectrum
    // loads are older, all consumed), and the next item's samples right before this item's output stores.
    asm volatile("" : "+v"(bias0), "+v"(bias1));
    // the next item's samples travel from HBM while this item's inverse passes run
    if (more) fetch(wnext, vnext);
    // ------------------------------------------------ inverse pass A'
    if (act_in) {
      nat_load<G>(v, zseq, tseq);
      seq_sync<G>();
      if constexpr (REGTW) passA_fft_twiddle_store_regs<G, +1>(v, zseq, tseq, twr);
      else passA_fft_twiddle_store_lds<G, +1>(v, zseq, tseq, twl);
      stampi(it, 8);
      seq_sync<G>();
      stampi(it, 9);
      // ---------------------------------------------- inverse pass B' + store
      passB_load<G>(v, zseq, tseq);
      const int j = passB_compute<G, +1>(v, tseq, twB);
      if (more) {
        // (requested a whole inverse transform ago: no stall; but behind the stores the next item would have to wait
        // for every one of them to be acknowledged before it may touch its samples)
#pragma unroll
        for (int n1 = 0; n1 < P; ++n1) asm volatile("" : "+v"(vnext[n1]));
      }
      const int o1 = tseq >> G::LGS;
      const int vb = a.slot_tiles ? wi.b0 : wi.b0 + nb;
      const int tile = a.slot_tiles ? wi.tile + nb : wi.tile;
      const int b = vb / nph, phase = vb - b * nph;
      const int t0 = tile * a.V;                                      // in samples of this phase
      const int limit = min(a.V, (a.Lfull - phase + nph - 1) / nph - t0);
      const int nbase = o1 + P * P * j;
      auto* y0 = io_ptr<IO>(a.y) + ((size_t)b * a.Cout + cg0) * a.Lout + (size_t)(t0 + nbase) * nph + phase;
      auto* y1 = y0 + a.Lout;
      if constexpr (BPAIR) {
        // v.x is slot nb (batch item b, tile `tile`), v.y slot nb + 1 (the next batch item, or with slot_tiles the next
        // tile) of channel cg0; both take that channel's bias, and the factor 2 the spectrum leaves (see the mix)
        const bool hasB = nb + 1 < wi.nbc;
        // (the float32 value is pinned before a 16-bit store rounds it: fused into one v_fma_mixlo_f16 the sum would be rounded
        // once, not to float32 and then to 16 bits as the float32 plan's result is when it is cast -- the bits the 16-bit plans promise)
        auto summed = [&](float val, float to) { float r = fmaf(2.f, val, to); asm("" : "+v"(r)); return r; };
        auto scaled = [&](float val) { return summed(val, bias0); };
        const int bB = a.slot_tiles ? b : b + 1, t0B = a.slot_tiles ? t0 + a.V : t0;
        const int limB = hasB ? min(a.V, a.Lfull - t0B) : 0;
        if (SEG && a.add_out) {
          // later segments of a long kernel accumulate into the output of the first
          auto* yB = io_ptr<IO>(a.y) + ((size_t)bB * a.Cout + cg0) * a.Lout + (size_t)(t0B + nbase);
#pragma unroll
          for (int k = 0; k < P; ++k) {
            if (nbase + P * k < limit) y0[P * k] = io.out(summed(v[k].x, io.in(y0[P * k])));
            if (nbase + P * k < limB) yB[P * k] = io.out(summed(v[k].y, io.in(yB[P * k])));
          }
        } else if (S == 1) {
          // Buffer stores in blocks of 8 rows as below; the two parts go through a resource each (an absent slot B: an
          // empty one, every store dropped), so that a dead offset stays bit 31 of an offset into ONE item's rows.
          const int limBs = hasB ? limB : limit;       // (the rows B may skip; equal to A's unless slot B is a shorter tile)
          const int ka = limit >= P ? (limit - P) / P + 1 : 0, kb = limBs >= P ? (limBs - P) / P + 1 : 0;
          const size_t crow = (size_t)(g * a.Cog + oc * a.cob);
          const unsigned ybytes = (unsigned)((size_t)a.cob * a.Lout * ES);
          const BufRsrc yrA = make_rsrc(io_ptr<IO>(a.y) + ((size_t)b * a.Cout + crow) * a.Lout, ybytes);
          const BufRsrc yrB = make_rsrc(io_ptr<IO>(a.y) + ((size_t)bB * a.Cout + crow) * a.Lout, hasB ? ybytes : 0u);
          const unsigned voA = (unsigned)((size_t)pr * a.Lout + (size_t)(t0 + nbase)) * ES;
          const unsigned voB = (unsigned)((size_t)pr * a.Lout + (size_t)(t0B + nbase)) * ES;
          static_for<0, P / 8>([&](auto bc) {
            constexpr int k0 = 8 * decltype(bc)::value;
            if (kb >= k0 + 8) {
              static_for<k0, k0 + 8>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                io.store(scaled(v[k].x), yrA, voA, P * k * ES);
                io.store(scaled(v[k].y), yrB, voB, P * k * ES);
              });
            } else if (ka >= k0) {
              static_for<k0, k0 + 8>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                if (k <= ka) {
                  io.store(scaled(v[k].x), yrA, voA | ((nbase + P * k < limit) ? 0u : 0x80000000u), P * k * ES);
                  io.store(scaled(v[k].y), yrB, voB | ((nbase + P * k < limBs) ? 0u : 0x80000000u), P * k * ES);
                }
              });
            }
          });
        } else {
          auto* yB = io_ptr<IO>(a.y) + ((size_t)bB * a.Cout + cg0) * a.Lout + (size_t)(t0B + nbase);
#pragma unroll
          for (int k = 0; k < P; ++k) {
            if (nbase + P * k < limit) y0[P * k] = io.out(scaled(v[k].x));
            if (nbase + P * k < limB) yB[P * k] = io.out(scaled(v[k].y));
          }
        }
      } else if constexpr (DIAG) {
        // depthwise: the last block may hold fewer than 8 channels, so every row is guarded
        const int ystep = P * nph;
        const bool addo = SEG && a.add_out;
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (nbase + P * k < limit) {
            if (ok0) y0[ystep * k] = io.out(v[k].x + (addo ? io.in(y0[ystep * k]) : bias0));
            if (ok1) y1[ystep * k] = io.out(v[k].y + (addo ? io.in(y1[ystep * k]) : bias1));
          }
      } else if (SEG && a.add_out) {
        // later segments of a long kernel accumulate into the output of the first
        const int ystep = P * nph;
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (nbase + P * k < limit) { y0[ystep * k] += v[k].x; y1[ystep * k] += v[k].y; }
      } else if (!PHASES && S == 1) {
        // Lane o1 holds samples o1 + P k.  For k < ka every lane is inside the valid window, k = ka is the one partly
        // valid row of stores, later k are outside for every lane (ka is wave-uniform).  Buffer stores: one 32-bit
        // offset register per output row, the step P k as the instruction's immediate.
        const int ka = limit >= P ? (limit - P) / P + 1 : 0;
        const BufRsrc yr = make_rsrc(io_ptr<IO>(a.y) + ((size_t)b * a.Cout + (size_t)(g * a.Cog + oc * a.cob)) * a.Lout, (unsigned)((size_t)a.cob * a.Lout * ES));
        const unsigned vo0 = (unsigned)((size_t)(2 * pr) * a.Lout + (size_t)(t0 + nbase)) * ES, vo1 = vo0 + (unsigned)a.Lout * ES;
        // Blocks of 8 rows: a block below ka is straight-line code behind ONE scalar branch (per-row tests, even
        // wave-uniform ones, cost more instructions than the stores they guard); only the block that holds row ka
        // tests its rows, and there the lanes past the window get an offset outside the resource (store dropped).
        static_for<0, P / 8>([&](auto bc) {
          constexpr int k0 = 8 * decltype(bc)::value;
          if (ka >= k0 + 8) {
#if FC_DIAG == 6
            { f2 sink = v[k0];
              static_for<k0 + 1, k0 + 8>([&](auto kc) { sink += v[decltype(kc)::value]; });
              if (sink.x == 123.456f) buf_store_f32(sink.x + bias0 + bias1, yr, vo0, 0); }
#else
            static_for<k0, k0 + 8>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              io.store(v[k].x + bias0, yr, vo0, P * k * ES);
              io.store(v[k].y + bias1, yr, vo1, P * k * ES);
            });
#endif
          } else if (ka >= k0) {
            static_for<k0, k0 + 8>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              if (k <= ka) {
                const unsigned dead = (nbase + P * k < limit) ? 0u : 0x80000000u;
                io.store(v[k].x + bias0, yr, vo0 | dead, P * k * ES);
                io.store(v[k].y + bias1, yr, vo1 | dead, P * k * ES);
              }
            });
          }
        });
      } else if (!PHASES) {
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (nbase + P * k < limit) { y0[P * k] = io.out(v[k].x + bias0); y1[P * k] = io.out(v[k].y + bias1); }
      } else if constexpr (PH4) {
        // all four phases of a position leave as 16 bytes: after the trade lane L of the wave holds (phases 0, 1) in
        // row 2m and (phases 2, 3) in row 2m + 1 of sample 64 m + L.  Phases past the end of the row are shorter by one.
        const int bA = wi.b0 / nph, phA = wi.b0 - bA * nph;
        int lim[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) lim[j] = min(a.V, (a.Lfull - (phA + j) + nph - 1) / nph - t0);
        const BufRsrc yr = make_rsrc(io_ptr<IO>(a.y) + ((size_t)bA * a.Cout + (size_t)(g * a.Cog + oc * a.cob)) * a.Lout, (unsigned)((size_t)a.cob * a.Lout * ES));
        const int L64 = tid & 63;
        const unsigned w0 = (unsigned)(((size_t)pr * a.Lout + (size_t)(t0 + L64) * nph + phA) * ES);
        const unsigned step4 = 64u * ES * (unsigned)nph;
        const bool al16 = (((size_t)a.y | ((size_t)a.Lout * ES)) & (4 * ES - 1)) == 0;
        const int mfull = (al16 && lim[3] >= 64) ? (lim[3] - 64) / 64 + 1 : 0;       // rows m below it: every lane, every phase valid
#pragma unroll
        for (int m = 0; m < P / 2; ++m) { swap_halves_c<0>(v[2 * m], v[2 * m + 1]); swap_halves_c<1>(v[2 * m], v[2 * m + 1]); }
        static_for<0, P / 8>([&](auto bc) {
          constexpr int m0 = 4 * decltype(bc)::value;
          if (mfull >= m0 + 4) {
            static_for<m0, m0 + 4>([&](auto mc) {
              constexpr int m = decltype(mc)::value;
              f4 d;
              d.x = v[2 * m].x + bias0; d.y = v[2 * m].y + bias0; d.z = v[2 * m + 1].x + bias0; d.w = v[2 * m + 1].y + bias0;
              io.store4(d, yr, w0, step4 * m);
            });
          } else if (64 * m0 < lim[0]) {
            static_for<m0, m0 + 4>([&](auto mc) {
              constexpr int m = decltype(mc)::value;
              if (64 * m < lim[0]) {
                const int n = 64 * m + L64;
                io.store(v[2 * m].x + bias0, yr, w0 | (n < lim[0] ? 0u : 0x80000000u), step4 * m);
                io.store(v[2 * m].y + bias0, yr, (w0 + ES) | (n < lim[1] ? 0u : 0x80000000u), step4 * m);
                io.store(v[2 * m + 1].x + bias0, yr, (w0 + 2 * ES) | (n < lim[2] ? 0u : 0x80000000u), step4 * m);
                io.store(v[2 * m + 1].y + bias0, yr, (w0 + 3 * ES) | (n < lim[3] ? 0u : 0x80000000u), step4 * m);
              }
            });
          }
        });
      } else if constexpr (PH2) {
        // both phases of a position leave as 8 bytes: rows 2m and 2m + 1 trade halves so that lane L holds (even
        // phase, odd phase) of sample 64 m + L.  The odd phase may be one sample shorter at the very end of a row.
        const int vbA = wi.b0 + 2 * (wv / NPI), bA = vbA / nph, phA = vbA - bA * nph;
        const int limA = min(a.V, (a.Lfull - phA + nph - 1) / nph - t0), limB = min(a.V, (a.Lfull - phA - 1 + nph - 1) / nph - t0);
        const BufRsrc yr = make_rsrc(io_ptr<IO>(a.y) + ((size_t)bA * a.Cout + (size_t)(g * a.Cog + oc * a.cob)) * a.Lout, (unsigned)((size_t)a.cob * a.Lout * ES));
        const int L64 = tid & 63;
        const unsigned w0 = (unsigned)(((size_t)(2 * pr) * a.Lout + (size_t)(t0 + L64) * nph + phA) * ES), w1 = w0 + (unsigned)a.Lout * ES;
        const unsigned step2 = 64u * ES * (unsigned)nph;
        const int mfull = limB >= 64 ? (limB - 64) / 64 + 1 : 0;        // rows m below it: every lane valid in both phases
#pragma unroll
        for (int m = 0; m < P / 2; ++m) { swap_halves_c<0>(v[2 * m], v[2 * m + 1]); swap_halves_c<1>(v[2 * m], v[2 * m + 1]); }
        static_for<0, P / 8>([&](auto bc) {
          constexpr int m0 = 4 * decltype(bc)::value;
          if (mfull >= m0 + 4) {
            static_for<m0, m0 + 4>([&](auto mc) {
              constexpr int m = decltype(mc)::value;
              io.store2(mk2(v[2 * m].x + bias0, v[2 * m + 1].x + bias0), yr, w0, step2 * m);
              io.store2(mk2(v[2 * m].y + bias1, v[2 * m + 1].y + bias1), yr, w1, step2 * m);
            });
          } else if (64 * m0 < limA) {
            static_for<m0, m0 + 4>([&](auto mc) {
              constexpr int m = decltype(mc)::value;
              if (64 * m < limA) {
                const int n = 64 * m + L64;
                const unsigned dA = n < limA ? 0u : 0x80000000u, dB = n < limB ? 0u : 0x80000000u;
                io.store(v[2 * m].x + bias0, yr, w0 | dA, step2 * m);
                io.store(v[2 * m + 1].x + bias0, yr, (w0 + ES) | dB, step2 * m);
                io.store(v[2 * m].y + bias1, yr, w1 | dA, step2 * m);
                io.store(v[2 * m + 1].y + bias1, yr, (w1 + ES) | dB, step2 * m);
              }
            });
          }
        });
      } else {
        const int ystep = P * nph;
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (nbase + P * k < limit) { y0[ystep * k] = io.out(v[k].x + bias0); y1[ystep * k] = io.out(v[k].y + bias1); }
      }
    }
    stampi(it, 10);
    if (STAMPS && a.stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stampi(it, 11); stampc(it, 13); }
    seq_sync<G>();     // this wave's sequences are free again (the mix barriers order the other waves)
  };

  const int it0 = blockIdx.x, it1 = blockIdx.x + gridDim.x;
  const bool two = it1 < pa.n_items;
  const WorkItem w0 = pa.items[it0];
  const WorkItem w1 = pa.items[two ? it1 : it0];
  f2 va[P], vb[P];
  fetch(w0, va);                             // first item's samples and the twiddles travel together
  if constexpr (REGTW) {
    passA_twiddle_fetch<G>(twr, tseq, make_rsrc(a.twA, (unsigned)(TWN * 8)));
  } else {
    copy_table_to_lds<TWN, NT>(twl, a.twA, tid);
    __syncthreads();
  }
  run(w0, it0, va, two, w1, vb, std::true_type{});
  if (two) run(w1, it1, vb, false, w1, va, std::false_type{});
}

}  // namespace fc
