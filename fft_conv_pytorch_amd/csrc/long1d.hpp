// long1d.hpp -- 1-D convolution with a filter as long as the row: one N-point cyclic transform per row, N = N1 * N2,
// run as two workgroup transforms with a trip through HBM between them (host_long.cpp plans it).
//
// The zero-padded row is indexed n = n1*N2 + n2 and its bins k = k1 + N1*k2:
//
//   X[k1 + N1*k2] = sum_n2 w_N2^(n2*k2) * ( w_N^(n2*k1) * sum_n1 w_N1^(n1*k1) * x[n1*N2 + n2] )
//
//   long_cols_fwd   N1-point transforms along n1 (stride N2 in memory) of a block of neighbouring n2 columns, the twiddle
//                   w_N^(n2*k1), W1[row][k1][n2].  Two real rows (batch items 2p and 2p+1 of one channel) ride one complex
//                   row, z = x[2p] + i*x[2p+1]; the same kernel reads the filter taps (imaginary part zero).
//   long_rows       one k1 row of N2 contiguous points: forward transform, product with the filter spectrum summed over the
//                   input channels of the group, inverse transform, conjugate twiddle, W2[row][k1][n2].  In its other mode it
//                   finishes the filter spectrum instead: H[o][i][k1][k2] = conj(transform) / N.
//   long_cols_inv   inverse N1-point transforms along k1, bias, real part -> y[2p], imaginary part -> y[2p+1], the
//                   kept window only.
//
// The two column kernels are the only ones that touch tensors, and they take them as float32, float16 or bfloat16
// (Io<IO>, fft_engine.hpp): the source rows of long_cols_fwd -- signal and filter taps alike -- are widened exactly as they
// are loaded, and long_cols_inv adds the bias in float32 and rounds each sample once, to nearest even, at its store.  The
// two element types of a launch are independent (src_io, y_io); W1, W2 and the spectrum are float32 always, so the result
// has the bits of: widen, run the float32 kernels, round.
//
// The two column kernels come in a plain and a mapped build (MAP).  The plain build is the zero-padded, stride-1,
// dilation-1 primitive; the mapped build of long_cols_fwd reads the signal through a padding mode (reflect / replicate /
// circular, the maps of axis_map.hpp) or spread over a grid of src_up, and the taps spread over a grid of tap_dil; the
// mapped build of long_cols_inv keeps every out_step-th sample of the stride-1 result.  The host picks per launch.
//
// Both column kernels also have a complex build (CX, plain and mapped) for complex64 tensors: a row is ONE batch item, a
// sample one 8-byte (re, im) pair, the bias Cout pairs.  The taps are conjugated as they are loaded, because long_rows
// stores conj(transform) / N and conj(FFT(conj u))[f] = U[-f] is what the unconjugated product y[t] = sum_k u[k] * z[t + k]
// needs (for real taps this is what the real builds do).  conj_src conjugates the rows of a launch once more: backward
// reads conj(x) and conj(w) that way, without a conjugated copy.  long_rows sees rows and units only and is the same.
//
// Both column kernels also have a channels-last build (NC > 0; mapped form only, which computes the plain map too; float32,
// 16-bit and complex64) for a signal / y that lies as a contiguous (B, L, C) tensor: element (b, c, t) at ((b*L + t)*C + c)
// samples.  A workgroup still runs NSEQ sequences, but they are NC neighbouring channels x NN = NSEQ / NC neighbouring n2
// columns of one batch pair; LDS slot rc*NN + rn holds (channel c0 + rc, column n20 + rn).  On the tensor side the lanes
// run over rc first (runs of NC * ES contiguous bytes per time sample), on the workspace side over rn first (NN * 8
// contiguous bytes per k1 of each of the block's rows); the transforms in between are the same code on the same slots'
// worth of data, so a row's arithmetic -- and every bit of the result -- is that of the (B, C, L) builds.  The resource of
// a row becomes that of a batch item's whole (L, C) block (so L*C*ES < 2^31, checked by the host); channels past C in the
// last block get the out-of-resource offset.  blockIdx runs over channel blocks first, then n2 blocks, then pairs.  The
// filter taps always go through the other builds.  NC = 0 compiles to what the kernels were before the parameter existed.
//
// Phases builds (PHS; float32 and 16-bit, (B, C, L) tensors) run a transposed convolution of stride s and dilation 1 as
// the s ordinary convolutions it is, y[s*t + p - padding] = sum_j w[p + s*j] * x[t - j]: the plan has s output channels per
// filter, channel o*s + p carrying phase p of filter o, on the unspread row.  long_cols_fwd in filter mode reads spectrum
// row (g, o, p, i) from row (g*Cig + i)*Cog + o of the (Cin, Cout/g, K) weight where it lies: position j of the row holds
// w[p + s*(tap0 + tstep*j)], and a tap past K - 1 (a shorter phase, or a phase with no tap at all) lies outside the row's
// resource and reads as zero.  long_cols_inv interleaves: its workgroup is laid out as a channels-last one with the
// phases of ONE filter in the place of the channels (NC phases x NN columns, the lanes over the phases first on the tensor
// side), sample t of phase p goes to y[b][o][s*t + p + ph_off] where that lies inside the row, the bias is the filter's,
// and a phase past s in the last block reads zeros and stores nothing.  long_rows sees s*Cog output channels.
//
// Decimation builds of long_cols_fwd (DEC; float32 and 16-bit, a (B, C, L) signal) run a STRIDED convolution of stride s
// and dilation 1 as the sum of s ordinary ones, the adjoint of the phases store: with k = s*m + p,
// y[j] = sum_k u[k] * xrow[s*j + k] = sum_p (u_p * x_p)[j], x_p[t] = xrow[s*t + p], u_p[m] = u[s*m + p].  The plan has s
// input channels per input channel of the tensor, channel i*s + p carrying the decimated row p of channel i, and
// ceil(K / s) taps per filter row.  The signal build (NC > 0) lays its workgroup out as a channels-last one with the
// phases of ONE input channel in the place of the channels (NC phases x NN columns; the lanes run over the phases first on
// the tensor side, so a workgroup reads runs of NC * ES contiguous bytes, and over the columns first on the workspace
// side, whose rows i*s + p0 ... are neighbours): position t of phase p reads x[b][i][s*t + p - pad_left] where that lies
// in [0, L) and p < s; front padding, positions past the data and the idle phases of a last block get the
// out-of-resource offset and read zero.  The filter build (NC == 0) reads spectrum row (g*Cog + o)*Cig*s + i*s + p from
// row (g*Cog + o)*Cig + i of the (Cout, Cin/g, K) weight where it lies: position m holds u[s*m + p], u the taps in tensor
// order or flipped; a tap past K - 1 ends a shorter phase, a phase p >= K has no tap.  long_rows sees s*Cig input
// channels per group and long_cols_inv is the unchanged one, its channels-last build included.
//
// The weight gradient (long_wgrad_rows and the WG build of long_cols_inv; host_long.cpp fc_long_wgrad) reads x and dY where
// they lie: both are signal-shaped, so long_cols_fwd transforms both with its signal builds (dY spread by the stride,
// src_up), z = x[2p] + i*x[2p+1] and w = dY[2p] + i*dY[2p+1] riding one complex row each.  The correlation theorem,
//   IFFT( FFT(z) * conj(FFT(w)) )[m] = sum_t conj(w[t]) * z[t + m],
// has the pair's contribution to dW in its real part (the cross terms are imaginary), so long_wgrad_rows sums the product
// over the batch pairs in registers, bin by bin, and transforms back once per (o, i); long_cols_inv drops the imaginary
// part (one item with no partner) and stores lag tap_dil*q at the place of tap q in the weight's own order.
//
// Gated builds of the two column kernels (long_cols_fwd_gated_kernel, long_cols_inv_gated_kernel; real rows, the plain
// form, float32 and 16-bit) multiply by elementwise gates where the tensors are touched anyway: the signal by a pregate as
// it is loaded, the result by up to two gates as up to two results are stored (LongGates, a second kernel argument of
// those builds alone).  They are kernels of their own: no build that existed changes by an instruction.
//
// The bins stay in the order [k1][k2] on both operands, so the product needs no transposition.  The filter is real,
// hence conj(H) is the spectrum of the correlation and y[t] = sum_k u[k] * z[t + k] comes out in place.
#pragma once
#include "axis_map.hpp"
#include "nd_passes.hpp"

namespace fc {

constexpr int kLongLoBits = 12;      // w_N^m = thi[m >> 12] * tlo[m & 4095]

struct LongArgs {
  const float* src;      // signal (B, C, L) or filter taps (rows of K samples); element type src_io
  const float* bias;     // float32
  float* y;              // (B, Cout, nout); element type y_io
  f2* w1;                // [row][k1][n2]   rows: (pair, input channel) or filter rows of this launch
  f2* w2;                // [row][k1][n2]   rows: (pair, output channel)
  const f2* spec;        // [(g*Cog + o)*Cig + i][k1][k2]   (long_wgrad_rows: W1 of dY, rows (pair, output channel))
  f2* spec_out;          // rows mode 1: first filter row of this launch
  const f2* thi;         // [N >> 12]  w_N^(a * 4096)
  const f2* tlo;         // [4096]     w_N^b
  const f2* twA1; const f2* twB1;    // engine tables of the N1-point tile
  const f2* twA2; const f2* twB2;    // ... of the N2-point tile
  int N1, N2, lgN2;
  int from_kernel;       // cols_fwd: 0 signal rows, 1 filter rows
  int spec_mode;         // rows: 1 = finish the filter spectrum   (long_wgrad_rows: 1 = add to what W2 holds, a later slab)
  int B, pair0;          // batch size, first pair of this slab   (long_wgrad_rows: B = the batch pairs of this slab)
  int C;                 // channels of the source tensor (signal) / of y
  int G, Cig, Cog, ob, nob;
  int L, padl;           // signal: row position p holds x[p - padl]
  int tap0, tstep, keff; // filter: row position p < keff holds taps[tap0 + tstep*p]
  int K;                 // filter row length in memory
  int nout;              // kept output samples
  float scale;           // 1 / N (rows mode 1)
  FastDiv d_nblk, d_c, d_nob, d_g;   // unit maps (filled by the dispatcher)
  int src_io, y_io;      // element types of src and of y (fc_dtype: 0 float32, 2 float16, 3 bfloat16; wave-uniform, Io<IO>)
  // the mapped builds only (wave-uniform):
  int pad_mode;          // PadMode of the signal row
  int mpadl, mpadr;      // positions before / behind the data that the mode fills (0 with PAD_CONSTANT)
  int src_up;            // signal: row position p holds x[(p - padl) / src_up] where that divides
  int kpos;              // filter: positions of the row that hold taps, tap_dil * (keff - 1) + 1
  FastDiv d_up, d_tdil;  // src_up and tap_dil: position p of a filter row holds taps[tap0 + tstep * (p / tap_dil)]
  FastDiv d_ostep;       // out_step: sample t of the stride-1 result is y[t / out_step] where that divides
  // the complex builds only (wave-uniform):
  int conj_src;          // cols_fwd: the rows of this launch are read conjugated (signal: conj(x); taps: u = conj(w))
  // the channels-last builds only:
  FastDiv d_ncb;         // channel blocks of NC channels, ceil(C / NC) (filled by the dispatcher; d_nblk: blocks of NN columns)
  // the phases builds only (wave-uniform; ph_s == 0: not a phases plan):
  int ph_s;              // stride s: output channel o*s + p of the plan carries phase p of filter o (Cog == s * ph_cog)
  int ph_cog;            // filters per group, Cout/g of the transposed convolution
  int ph_row0;           // cols_fwd: the first filter row of this launch, in the spectrum's order
  int ph_off;            // cols_inv: sample t of phase p is y[s*t + p + ph_off] where that lies in [0, nout)
  FastDiv d_ph_s, d_ph_cig, d_ph_cogs;   // s, Cig and s * ph_cog: spectrum row -> (g, o, p, i)
  // A decimation plan is no phases plan and lends the words above other meanings (the struct keeps its size, and with it
  // every build that existed its registers): ph_s > 0 with ph_cog == 0 says decimation, ph_s = stride s (input channel
  // i*s + p of the plan carries the decimated row p of channel i), d_ph_s: spectrum row -> (weight row, p), ph_row0 as
  // above, ph_off = the phase origin: position t of phase p of a signal row holds x[s*t + p - ph_off] where that lies in
  // [0, L).  Position m < keff of a filter row holds taps[tap0 + tstep*(s*m + p)] where s*m + p < K: tap0, tstep = 0, 1
  // (tensor order) or K - 1, -1 (flipped)
};

constexpr int IO_CODE_C64 = 4;       // fc_dtype code of a launch of a complex build (src_io / y_io)

// The second kernel argument of the gated builds of the two column kernels (fc_long_forward_gated).  The builds without
// gates do not take it: LongArgs, and with it their arguments and registers, stay what they were.
struct LongGates {
  const float* pregate;  // cols_fwd: (B, C, L) like the signal, element type src_io; the row is pregate * x
  const float* gate;     // cols_inv: (B, Cout, nout) like y, element type y_io, or null: y = gate * c, c = z + bias
  float* y2;             // cols_inv: a second result of y's shape, or null: y2 = gate2 * c
  const float* gate2;    // cols_inv: like gate, or null (y2 = c)
  int y2_f32;            // cols_inv, 16-bit build: y2 is float32 (c unrounded) and gate2 null
};

__device__ __forceinline__ f2 long_twiddle(BufRsrc thi, BufRsrc tlo, unsigned m) {
  const f2 hi = buf_load_f32x2(thi, (m >> kLongLoBits) * 8u, 0);
  const f2 lo = buf_load_f32x2(tlo, (m & ((1u << kLongLoBits) - 1u)) * 8u, 0);
  return cmul(hi, lo);
}

// ------------------------------------------------------------------------------------------ long_cols_fwd
// (long_cols_fwd_gated_kernel below repeats the plain signal path of this kernel -- offsets, LDS staging, transform, twiddle
// and store: a fix to any of those here is a fix there too)
template <int P, int S, int NSEQ, int NT, int IO = IO_F32, bool MAP = false, bool CX = false, int NC = 0, bool PHS = false,
          bool DEC = false>
__global__ __launch_bounds__(NT) void long_cols_fwd_kernel(const LongArgs a) {
  using G = Geo<P, S>;
  static_assert(!CX || IO == IO_F32, "a complex sample is a pair of float32");
  static_assert(!PHS || (!MAP && !CX && NC == 0), "phases: the filter rows of a real plan, dilation 1");
  static_assert(!DEC || (!MAP && !CX && !PHS), "decimation: the rows of a real plan, zero padding, dilation 1");
  constexpr bool BLK = NC > 0;                  // the workgroup is NC rows x NN columns (channels-last, decimated signal)
  constexpr bool NLC = BLK && !DEC;             // channels-last signal (header); never a launch of filter rows
  constexpr bool DSIG = BLK && DEC;             // decimated signal rows: the phases of one channel for the channels
  constexpr bool DFIL = DEC && !BLK;            // the filter rows of a decimation plan
  constexpr int M = BLK ? NC : 1;               // neighbouring channels (phases) of the workgroup ...
  constexpr int NN = NSEQ / M;                  // ... and neighbouring n2 columns of each
  static_assert(!NLC || MAP, "channels-last: the mapped form");
  static_assert(!BLK || (NC <= NSEQ && (NC & (NC - 1)) == 0), "a block of NC rows: NC * NN == NSEQ");
  const Io<IO> io(a.src_io);
  constexpr unsigned ES = CX ? 8u : Io<IO>::B;  // bytes per sample of the source rows
  constexpr int EW = CX ? 2 : 1;                // elements of Io<IO>::T per sample
  constexpr int T = G::T;                       // == a.N1
  constexpr int LSEQP = SeqLayout<G>::LSEQP;
  static_assert(NT == NSEQ * G::TS && (NSEQ & (NSEQ - 1)) == 0, "one thread slot per point group, column block a power of two");
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const BufRsrc twA = make_rsrc(a.twA1, (unsigned)(P * G::N2 * 8));
  const BufRsrc twB = make_rsrc(a.twB1, (unsigned)(S * P * 8));
  const int tid = threadIdx.x, sq = tid / G::TS, tseq = tid % G::TS;
  unsigned row;                                 // (channels-last: the workspace row of the block's first channel)
  int n20;
  [[maybe_unused]] unsigned c0 = 0, pr_nlc = 0, dph0 = 0;
  if constexpr (!BLK) {
    n20 = (int)fdivmod(blockIdx.x, a.d_nblk, &row) * NSEQ;
  } else if constexpr (DSIG) {
    // the phase block of a channel varies fastest, then the channel (a.C of them), then the n2 block, then the pair; the
    // workspace rows of a channel's phases are neighbours, c * s + p
    unsigned q, q2;
    dph0 = fdivmod(blockIdx.x, a.d_ncb, &q) * NC;
    c0 = fdivmod(q, a.d_c, &q2);
    n20 = (int)fdivmod(q2, a.d_nblk, &pr_nlc) * NN;
    row = (pr_nlc * (unsigned)a.C + c0) * (unsigned)a.ph_s + dph0;
  } else {
    // the channel block varies fastest, then the n2 block, then the pair
    unsigned q;
    c0 = fdivmod(blockIdx.x, a.d_ncb, &q) * NC;
    n20 = (int)fdivmod(q, a.d_nblk, &pr_nlc) * NN;
    row = pr_nlc * (unsigned)a.C + c0;
  }
  const size_t N = (size_t)a.N1 << a.lgN2;

  // the two real rows of the pair (filter rows: one, the imaginary part stays zero); complex build: the one row of item
  // pair0 + pr.  Channels-last: the (L, C) blocks of the pair's two batch items
  const typename Io<IO>::T* r0;
  bool has1 = false;
  unsigned len;
  [[maybe_unused]] unsigned ph = 0;             // phases build: the phase this filter row carries
  if constexpr (DFIL) {
    // (always a launch of filter rows) spectrum row wr * s + p reads row wr of the (Cout, Cin/g, K) weight where it lies
    unsigned wr;
    ph = fdivmod((unsigned)a.ph_row0 + row, a.d_ph_s, &wr);
    r0 = io_ptr<IO>(a.src) + (size_t)wr * a.K;
    len = (unsigned)a.K;
  } else if constexpr (DSIG) {
    const int b0 = 2 * (a.pair0 + (int)pr_nlc);
    r0 = io_ptr<IO>(a.src) + ((size_t)b0 * a.C + c0) * a.L;
    has1 = b0 + 1 < a.B;
    len = (unsigned)a.L;
  } else if constexpr (PHS) {
    // (always a launch of filter rows) spectrum row (g, o, p, i) reads weight row (g*Cig + i)*Cog + o where it lies
    unsigned q, g, o;
    const unsigned i = fdivmod((unsigned)a.ph_row0 + row, a.d_ph_cig, &q);
    const unsigned op = fdivmod(q, a.d_ph_cogs, &g);
    ph = fdivmod(op, a.d_ph_s, &o);
    r0 = io_ptr<IO>(a.src) + ((size_t)(g * (unsigned)a.Cig + i) * a.ph_cog + o) * a.K;
    len = (unsigned)a.K;
  } else if constexpr (NLC) {
    const int b0 = CX ? a.pair0 + (int)pr_nlc : 2 * (a.pair0 + (int)pr_nlc);
    r0 = io_ptr<IO>(a.src) + (size_t)b0 * a.C * a.L * EW;
    has1 = !CX && b0 + 1 < a.B;
    len = (unsigned)a.L;
  } else if (a.from_kernel) {
    r0 = io_ptr<IO>(a.src) + (size_t)row * a.K * EW;
    len = (unsigned)a.K;
  } else {
    unsigned pr;
    const unsigned c = fdivmod(row, a.d_c, &pr);
    const int b0 = CX ? a.pair0 + (int)pr : 2 * (a.pair0 + (int)pr);
    r0 = io_ptr<IO>(a.src) + ((size_t)b0 * a.C + c) * a.L * EW;
    has1 = !CX && b0 + 1 < a.B;
    len = (unsigned)a.L;
  }
  const unsigned sbytes = NLC ? len * (unsigned)a.C * ES : len * ES;
  const BufRsrc s0 = make_rsrc(r0, sbytes);
  const BufRsrc s1 = make_rsrc(has1 ? r0 + (size_t)a.C * a.L : r0, sbytes);
  {
    // lanes run over the NSEQ neighbouring columns first (channels-last: over the NC channels first, then the NN
    // columns); every sample of the thread is requested before the first is stored; positions outside the data -- and
    // the channels past C of the last channel block -- get an offset outside the resource and read as zero
    f2 val[P];
    const auto offset = [&](int u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
      const int p = (n1 << a.lgN2) + n20 + (BLK ? r / M : r);
      if constexpr (DSIG) {
        // position p of phase q holds x[s*p + q - ph_off]; padding, positions past the data and idle phases read as zero
        const unsigned q = dph0 + (unsigned)(r & (M - 1));
        const unsigned e = (unsigned)(p * a.ph_s + (int)q - a.ph_off);
        return q < (unsigned)a.ph_s && e < len ? e * ES : 0x80000000u;
      } else if constexpr (DFIL) {
        // position p < keff holds u[s*p + ph], u = the taps in tensor order or flipped; a tap past K - 1 reads as zero
        const unsigned e = ph + (unsigned)a.ph_s * (unsigned)p;
        return p < a.keff && e < len ? (unsigned)(a.tap0 + a.tstep * (int)e) * ES : 0x80000000u;
      } else if constexpr (PHS) {
        // position p < keff holds w[ph + s*(tap0 + tstep*p)]; a tap past K - 1 reads as zero (the resource says so too)
        const unsigned e = ph + (unsigned)a.ph_s * (unsigned)(a.tap0 + a.tstep * p);
        return p < a.keff && e < len ? e * ES : 0x80000000u;
      } else if constexpr (!MAP) {
        const int s = a.from_kernel ? a.tap0 + a.tstep * p : p - a.padl;
        const bool ok = a.from_kernel ? p < a.keff : (unsigned)s < len;
        return ok ? (unsigned)s * ES : 0x80000000u;
      } else {
        // (every branch below is wave-uniform: it tests launch arguments)
        int s;
        bool ok;
        if (!NLC && a.from_kernel) {               // (a channels-last launch never reads filter rows)
          const unsigned q = fdiv((unsigned)p, a.d_tdil);
          ok = p < a.kpos && q * a.d_tdil.d == (unsigned)p;
          s = a.tap0 + a.tstep * (int)q;
        } else if (a.src_up > 1) {
          const int pos = p - a.padl;
          const unsigned q = fdiv((unsigned)pos, a.d_up);
          ok = pos >= 0 && q * a.d_up.d == (unsigned)pos && q < len;
          s = (int)q;
        } else {
          const int pos = p - a.padl, n = (int)len;
          ok = pos >= -a.mpadl && pos < n + a.mpadr;
          s = pos;
          if (a.pad_mode == PAD_REFLECT) s = pos < 0 ? -pos : (pos >= n ? 2 * (n - 1) - pos : pos);
          else if (a.pad_mode == PAD_REPLICATE) s = pos < 0 ? 0 : (pos >= n ? n - 1 : pos);
          else if (a.pad_mode == PAD_CIRCULAR) s = pos < 0 ? pos + n : (pos >= n ? pos - n : pos);
        }
        if constexpr (NLC) {                       // sample s of channel c0 + rc lies at s * C + c samples
          const unsigned c = c0 + (unsigned)(r & (M - 1));
          return ok && c < (unsigned)a.C ? ((unsigned)s * (unsigned)a.C + c) * ES : 0x80000000u;
        } else {
          return ok ? (unsigned)s * ES : 0x80000000u;
        }
      }
    };
    if constexpr (CX) {
      // taps are conjugated on load (header), conj_src conjugates the rows of the launch once more: a sign-bit flip
      const unsigned sign = ((a.from_kernel != 0) != (a.conj_src != 0)) ? 0x80000000u : 0u;
#pragma unroll
      for (int u = 0; u < P; ++u) val[u] = buf_load_f32x2(s0, offset(u), 0);
#pragma unroll
      for (int u = 0; u < P; ++u) val[u].y = __uint_as_float(__float_as_uint(val[u].y) ^ sign);
    } else if constexpr (IO == IO_F32) {
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const unsigned off = offset(u);
        val[u].x = buf_load_f32(s0, off, 0);
        val[u].y = buf_load_f32(s1, has1 ? off : 0x80000000u, 0);
      }
    } else {
      // 16-bit rows: all 2 P loads are issued before the first sample is widened (a conversion right behind its load
      // makes the compiler wait for that load before it issues the next, wgrad1d.hpp load_pairs_h16)
      unsigned h0[P], h1[P];
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const unsigned off = offset(u);
        h0[u] = __builtin_amdgcn_raw_buffer_load_b16(s0, off, 0, 0);
        h1[u] = __builtin_amdgcn_raw_buffer_load_b16(s1, has1 ? off : 0x80000000u, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < P; ++u) val[u] = mk2(io.in(h0[u]), io.in(h1[u]));
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
      if constexpr (BLK) {                       // slot (rc, rn) = rc * NN + rn
        lds[((r & (M - 1)) * NN + r / M) * LSEQP + G::nat(n1)] = val[u];
      } else {
        lds[r * LSEQP + G::nat(n1)] = val[u];
      }
    }
  }
  __syncthreads();
  f2 v[P];
  f2* lseq = lds + sq * LSEQP;
  nat_load<G>(v, lseq, tseq);
  seq_sync<G>();
  fwd_from_regs<G>(v, lseq, tseq, true, twA, twB);
  __syncthreads();
  // twiddle w_N^(n2*k1) and store: NSEQ neighbouring n2 per k1
  const BufRsrc thi = make_rsrc(a.thi, (unsigned)((N >> kLongLoBits) * 8));
  const BufRsrc tlo = make_rsrc(a.tlo, (unsigned)(8u << kLongLoBits));
  // (channels-last: one resource over the block's workspace rows, the NC of them or those up to channel C - 1; the
  // lanes run over the NN columns first, slot r = (r / NN, r % NN).  NC * N <= 8192 * 4096 points: 2^28 bytes)
  // (decimated signal: the rows of the block's phases, those up to phase s - 1)
  const unsigned wrows = DSIG ? min((unsigned)M, (unsigned)a.ph_s - dph0) : NLC ? min((unsigned)M, (unsigned)a.C - c0) : 1u;
  const BufRsrc orr = make_rsrc(a.w1 + (size_t)row * N, (unsigned)(N * 8) * wrows);
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
    const unsigned n2 = (unsigned)(n20 + (BLK ? r & (NN - 1) : r));
    const f2 w = long_twiddle(thi, tlo, n2 * (unsigned)k1);
    const f2 z = lds[r * LSEQP + G::nat(k1)];
    const unsigned wrow = BLK ? (unsigned)(r / NN) * (unsigned)N : 0u;
    buf_store_f32x2(cmul(z, w), orr, (wrow + ((unsigned)k1 << a.lgN2) + n2) * 8u, 0);
  }
}

// The gated build of long_cols_fwd: the signal rows of a real plan in the plain form ((B, C, L) tensors, zero padding, no
// spread; float32 or 16-bit), each sample times its pregate as it is loaded.  The pregate rows of the pair's two items are
// read at the offsets of the signal's through resources of the same size, so a position that reads the signal as zero
// reads the gate as zero too.  The product is one float32 multiply of the widened operands (of two 16-bit values: exact),
// the bits of torch's pregate * x on float32 tensors; transform, twiddle and store are those of the kernel above on those
// values.  It is a kernel of its own, so that every build above keeps its code: filter rows never come here.
template <int P, int S, int NSEQ, int NT, int IO>
__global__ __launch_bounds__(NT) void long_cols_fwd_gated_kernel(const LongArgs a, const LongGates gt) {
  using G = Geo<P, S>;
  const Io<IO> io(a.src_io);
  constexpr unsigned ES = Io<IO>::B;
  constexpr int LSEQP = SeqLayout<G>::LSEQP;
  static_assert(NT == NSEQ * G::TS && (NSEQ & (NSEQ - 1)) == 0, "one thread slot per point group, column block a power of two");
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const BufRsrc twA = make_rsrc(a.twA1, (unsigned)(P * G::N2 * 8));
  const BufRsrc twB = make_rsrc(a.twB1, (unsigned)(S * P * 8));
  const int tid = threadIdx.x, sq = tid / G::TS, tseq = tid % G::TS;
  unsigned row, pr;
  const int n20 = (int)fdivmod(blockIdx.x, a.d_nblk, &row) * NSEQ;
  const size_t N = (size_t)a.N1 << a.lgN2;
  const unsigned c = fdivmod(row, a.d_c, &pr);
  const int b0 = 2 * (a.pair0 + (int)pr);
  const bool has1 = b0 + 1 < a.B;
  const size_t first = ((size_t)b0 * a.C + c) * a.L, next = has1 ? (size_t)a.C * a.L : 0;
  const unsigned len = (unsigned)a.L, sbytes = len * ES;
  const BufRsrc s0 = make_rsrc(io_ptr<IO>(a.src) + first, sbytes), s1 = make_rsrc(io_ptr<IO>(a.src) + first + next, sbytes);
  const BufRsrc g0 = make_rsrc(io_ptr<IO>(gt.pregate) + first, sbytes), g1 = make_rsrc(io_ptr<IO>(gt.pregate) + first + next, sbytes);
  {
    // all 4 P loads are issued before the first sample is widened or multiplied (as the 16-bit build above)
    f2 val[P];
    const auto offset = [&](int u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
      const int s = (n1 << a.lgN2) + n20 + r - a.padl;
      return (unsigned)s < len ? (unsigned)s * ES : 0x80000000u;
    };
    if constexpr (IO == IO_F32) {
      f2 gv[P];
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const unsigned off = offset(u), off1 = has1 ? off : 0x80000000u;
        val[u] = mk2(buf_load_f32(s0, off, 0), buf_load_f32(s1, off1, 0));
        gv[u] = mk2(buf_load_f32(g0, off, 0), buf_load_f32(g1, off1, 0));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < P; ++u) val[u] = mk2(__fmul_rn(gv[u].x, val[u].x), __fmul_rn(gv[u].y, val[u].y));
    } else {
      unsigned h0[P], h1[P], q0[P], q1[P];
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const unsigned off = offset(u), off1 = has1 ? off : 0x80000000u;
        h0[u] = __builtin_amdgcn_raw_buffer_load_b16(s0, off, 0, 0);
        h1[u] = __builtin_amdgcn_raw_buffer_load_b16(s1, off1, 0, 0);
        q0[u] = __builtin_amdgcn_raw_buffer_load_b16(g0, off, 0, 0);
        q1[u] = __builtin_amdgcn_raw_buffer_load_b16(g1, off1, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < P; ++u) val[u] = mk2(__fmul_rn(io.in(q0[u]), io.in(h0[u])), __fmul_rn(io.in(q1[u]), io.in(h1[u])));
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
      lds[r * LSEQP + G::nat(n1)] = val[u];
    }
  }
  __syncthreads();
  f2 v[P];
  f2* lseq = lds + sq * LSEQP;
  nat_load<G>(v, lseq, tseq);
  seq_sync<G>();
  fwd_from_regs<G>(v, lseq, tseq, true, twA, twB);
  __syncthreads();
  const BufRsrc thi = make_rsrc(a.thi, (unsigned)((N >> kLongLoBits) * 8));
  const BufRsrc tlo = make_rsrc(a.tlo, (unsigned)(8u << kLongLoBits));
  const BufRsrc orr = make_rsrc(a.w1 + (size_t)row * N, (unsigned)(N * 8));
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
    const unsigned n2 = (unsigned)(n20 + r);
    const f2 w = long_twiddle(thi, tlo, n2 * (unsigned)k1);
    const f2 z = lds[r * LSEQP + G::nat(k1)];
    buf_store_f32x2(cmul(z, w), orr, (((unsigned)k1 << a.lgN2) + n2) * 8u, 0);
  }
}

// ------------------------------------------------------------------------------------------ long_rows
// NSEQ neighbouring k1 rows per workgroup, one sequence each; OB output channels of one group per workgroup, their
// running sums in registers in the order the inverse transform starts from (bins N2e*i1 + tseq of the thread).
template <int P, int S, int NSEQ, int NT, int OB>
__global__ __launch_bounds__(NT) void long_rows_kernel(const LongArgs a) {
  using G = Geo<P, S>;
  constexpr int T = G::T;                       // == a.N2
  constexpr int LSEQP = SeqLayout<G>::LSEQP;
  static_assert(NT == NSEQ * G::TS, "one thread slot per point group");
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const BufRsrc twA = make_rsrc(a.twA2, (unsigned)(P * G::N2 * 8));
  const BufRsrc twB = make_rsrc(a.twB2, (unsigned)(S * P * 8));
  const int tid = threadIdx.x, sq = tid / G::TS, tseq = tid % G::TS;
  f2* lseq = lds + sq * LSEQP;
  unsigned q;
  const int k1 = (int)fdivmod(blockIdx.x, a.d_nblk, &q) * NSEQ + sq;
  const size_t N = (size_t)a.N1 * T;
  const unsigned rowoff = (unsigned)k1 * (unsigned)(T * 8);      // byte offset of this k1 row inside a row of N points
  const unsigned toff = rowoff + (unsigned)tseq * 8u;

  if (a.spec_mode) {
    // filter row q of this launch: transform, conjugate, 1/N
    const BufRsrc sr = make_rsrc(a.w1 + (size_t)q * N, (unsigned)(N * 8));
    f2 v[P];
#pragma unroll
    for (int n1 = 0; n1 < P; ++n1) v[n1] = buf_load_f32x2(sr, toff, G::N2 * n1 * 8);
    fwd_from_regs<G>(v, lseq, tseq, true, twA, twB);
    seq_sync<G>();
    nat_load<G>(v, lseq, tseq);
    const BufRsrc orr = make_rsrc(a.spec_out + (size_t)q * N, (unsigned)(N * 8));
#pragma unroll
    for (int i1 = 0; i1 < P; ++i1) buf_store_f32x2(mk2(v[i1].x * a.scale, -v[i1].y * a.scale), orr, toff, G::N2 * i1 * 8);
    return;
  }

  const int ob0 = (int)fdivmod(q, a.d_nob, &q) * OB;
  const int g = (int)fdivmod(q, a.d_g, &q);
  const int pr = (int)q;
  const int Cin = a.G * a.Cig, Cout = a.G * a.Cog;
  f2 acc[OB][P];
#pragma unroll
  for (int o = 0; o < OB; ++o)
#pragma unroll
    for (int i1 = 0; i1 < P; ++i1) acc[o][i1] = mk2(0.f, 0.f);

#pragma unroll 1
  for (int i = 0; i < a.Cig; ++i) {
    const BufRsrc sr = make_rsrc(a.w1 + ((size_t)pr * Cin + (size_t)g * a.Cig + i) * N, (unsigned)(N * 8));
    f2 v[P], h[P];
#pragma unroll
    for (int n1 = 0; n1 < P; ++n1) v[n1] = buf_load_f32x2(sr, toff, G::N2 * n1 * 8);
    {
      // spectrum of the first output channel: requested before the transform, used after it
      const BufRsrc hr = make_rsrc(a.spec + (((size_t)g * a.Cog + ob0) * a.Cig + i) * N, (unsigned)(N * 8));
#pragma unroll
      for (int i1 = 0; i1 < P; ++i1) h[i1] = buf_load_f32x2(hr, toff, G::N2 * i1 * 8);
    }
    fwd_from_regs<G>(v, lseq, tseq, true, twA, twB);
    seq_sync<G>();
    nat_load<G>(v, lseq, tseq);
    seq_sync<G>();                       // the next transform writes this sequence's slots
    static_for<0, OB>([&](auto oc) {
      constexpr int o = decltype(oc)::value;
      if (ob0 + o < a.Cog) {             // (workgroup-uniform)
        if constexpr (o > 0) {
          const BufRsrc hr = make_rsrc(a.spec + (((size_t)g * a.Cog + ob0 + o) * a.Cig + i) * N, (unsigned)(N * 8));
#pragma unroll
          for (int i1 = 0; i1 < P; ++i1) h[i1] = buf_load_f32x2(hr, toff, G::N2 * i1 * 8);
        }
#pragma unroll
        for (int i1 = 0; i1 < P; ++i1) cmac(acc[o][i1], v[i1], h[i1]);
      }
    });
  }

  const BufRsrc thi = make_rsrc(a.thi, (unsigned)((N >> kLongLoBits) * 8));
  const BufRsrc tlo = make_rsrc(a.tlo, (unsigned)(8u << kLongLoBits));
  static_for<0, OB>([&](auto oc) {
    constexpr int o = decltype(oc)::value;
    if (ob0 + o < a.Cog) {               // (workgroup-uniform, so the barriers inside are met by all)
      passA_fft_twiddle_store<G, +1>(acc[o], lseq, tseq, twA);
      seq_sync<G>();
      f2 v[P];
      passB_load<G>(v, lseq, tseq);
      const int j = passB_compute<G, +1>(v, tseq, twB);
      seq_sync<G>();
      const int nbase = (tseq >> G::LGS) + P * P * j;
      const BufRsrc orr = make_rsrc(a.w2 + ((size_t)pr * Cout + (size_t)g * a.Cog + ob0 + o) * N, (unsigned)(N * 8));
#pragma unroll
      for (int k = 0; k < P; ++k) {
        const unsigned n2 = (unsigned)(nbase + P * k);
        const f2 w = long_twiddle(thi, tlo, n2 * (unsigned)k1);
        buf_store_f32x2(cmulc(v[k], w), orr, rowoff + n2 * 8u, 0);
      }
    }
  });
}

// ------------------------------------------------------------------------------------------ long_wgrad_rows
// acc += x * conj(d)
__device__ __forceinline__ void cmac_conj(f2& acc, f2 x, f2 d) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]\n\t"
      "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_hi:[0,1,0]" : "+v"(acc) : "v"(d), "v"(x));
}

// The middle pass of the weight gradient.  NSEQ neighbouring k1 rows per workgroup, one sequence each; ONE input channel
// i of a group and OB output channels of that group per workgroup.  For every batch pair of the slab (a.B of them) the
// W1 row of x (pair, (g, i)) and the W1 rows of dY (pair, (g, o)), a.spec, are transformed and X * conj(D) is summed in
// registers, in the order the inverse transform starts from; then, per output channel, the inverse transform, 1 / N and
// the conjugate twiddle as in long_rows, into W2 row (g*Cog + o)*Cig + i -- the row order of the weight.  With
// a.spec_mode the result is added to what W2 holds (the pairs of an earlier slab).
template <int P, int S, int NSEQ, int NT, int OB>
__global__ __launch_bounds__(NT) void long_wgrad_rows_kernel(const LongArgs a) {
  using G = Geo<P, S>;
  constexpr int T = G::T;                       // == a.N2
  constexpr int LSEQP = SeqLayout<G>::LSEQP;
  static_assert(NT == NSEQ * G::TS, "one thread slot per point group");
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const BufRsrc twA = make_rsrc(a.twA2, (unsigned)(P * G::N2 * 8));
  const BufRsrc twB = make_rsrc(a.twB2, (unsigned)(S * P * 8));
  const int tid = threadIdx.x, sq = tid / G::TS, tseq = tid % G::TS;
  f2* lseq = lds + sq * LSEQP;
  unsigned q;
  const int k1 = (int)fdivmod(blockIdx.x, a.d_nblk, &q) * NSEQ + sq;
  const size_t N = (size_t)a.N1 * T;
  const unsigned rowoff = (unsigned)k1 * (unsigned)(T * 8);      // byte offset of this k1 row inside a row of N points
  const unsigned toff = rowoff + (unsigned)tseq * 8u;
  const int ob0 = (int)fdivmod(q, a.d_nob, &q) * OB;
  const int g = (int)fdivmod(q, a.d_g, &q);
  const int i = (int)q;
  const int Cin = a.G * a.Cig, Cout = a.G * a.Cog;
  f2 acc[OB][P];
#pragma unroll
  for (int o = 0; o < OB; ++o)
#pragma unroll
    for (int i1 = 0; i1 < P; ++i1) acc[o][i1] = mk2(0.f, 0.f);

  const unsigned rbytes = (unsigned)(N * 8);
  // (ONE transform in the code for the row of x, h == 0, and the rows of dY, h - 1 == o: the scalar registers hold the
  // constants of one)
  const int nrows = 1 + min(OB, a.Cog - ob0);
#pragma unroll 1
  for (int pr = 0; pr < a.B; ++pr) {
    f2 v[P];
#pragma unroll 1
    for (int h = 0; h < nrows; ++h) {    // (workgroup-uniform, so the barriers inside are met by all)
      // the W1 row of x (pair, (g, i)), or of dY (pair, (g, ob0 + h - 1))
      const size_t row = h ? (size_t)pr * Cout + (size_t)(g * a.Cog + ob0 + h - 1) : (size_t)pr * Cin + (size_t)(g * a.Cig + i);
      const BufRsrc sr = make_rsrc((h ? a.spec : a.w1) + row * N, rbytes);
      f2 d[P];
#pragma unroll
      for (int n1 = 0; n1 < P; ++n1) d[n1] = buf_load_f32x2(sr, toff, G::N2 * n1 * 8);
      fwd_from_regs<G>(d, lseq, tseq, true, twA, twB);
      seq_sync<G>();
      nat_load<G>(d, lseq, tseq);
      seq_sync<G>();                     // the next transform writes this sequence's slots
      if (h == 0) {
#pragma unroll
        for (int i1 = 0; i1 < P; ++i1) v[i1] = d[i1];
      }
      static_for<0, OB>([&](auto oc) {
        constexpr int o = decltype(oc)::value;
        if (h == o + 1) {
#pragma unroll
          for (int i1 = 0; i1 < P; ++i1) cmac_conj(acc[o][i1], v[i1], d[i1]);
        }
      });
    }
  }

  const BufRsrc thi = make_rsrc(a.thi, (unsigned)((N >> kLongLoBits) * 8));
  const BufRsrc tlo = make_rsrc(a.tlo, (unsigned)(8u << kLongLoBits));
  static_for<0, OB>([&](auto oc) {
    constexpr int o = decltype(oc)::value;
    if (ob0 + o < a.Cog) {               // (workgroup-uniform, so the barriers inside are met by all)
      passA_fft_twiddle_store<G, +1>(acc[o], lseq, tseq, twA);
      seq_sync<G>();
      f2 v[P];
      passB_load<G>(v, lseq, tseq);
      const int j = passB_compute<G, +1>(v, tseq, twB);
      seq_sync<G>();
      const int nbase = (tseq >> G::LGS) + P * P * j;
      const BufRsrc orr = make_rsrc(a.w2 + (((size_t)g * a.Cog + ob0 + o) * a.Cig + i) * N, (unsigned)(N * 8));
      // (the first slab reads what W2 holds at an offset outside the resource, that is as zero; a later slab adds to it)
      const unsigned poff = a.spec_mode ? 0u : 0x80000000u;
#pragma unroll
      for (int k = 0; k < P; ++k) {
        const unsigned n2 = (unsigned)(nbase + P * k);
        const f2 w = long_twiddle(thi, tlo, n2 * (unsigned)k1);
        const f2 prev = buf_load_f32x2(orr, poff + rowoff + n2 * 8u, 0);
        const f2 r = cmulc(v[k], w);
        buf_store_f32x2(mk2(prev.x + r.x * a.scale, prev.y + r.y * a.scale), orr, rowoff + n2 * 8u, 0);
      }
    }
  });
}

// ------------------------------------------------------------------------------------------ long_cols_inv
// The weight-gradient build (WG; mapped form, real rows, (rows, K) weight): a launch of ONE item (a.B == 1, so the
// imaginary part is dropped) whose "channels" are the a.C = Cout * Cin/g rows of dW, each a.K elements long: sample
// out_step * q of the row, q < a.keff, is the lag of tap q and goes where long_cols_fwd reads that tap of a filter row,
// element a.tap0 + a.tstep * q (tensor order or flipped); the elements no kept lag reaches are not touched (the host
// zeroes them).
// (long_cols_inv_gated_kernel below repeats the plain real path of this kernel -- W2 loads, inverse transform, the trip
// through LDS, bias and store offsets: a fix to any of those here is a fix there too)
template <int P, int S, int NSEQ, int NT, int IO = IO_F32, bool MAP = false, bool CX = false, int NC = 0, bool PHS = false,
          bool WG = false>
__global__ __launch_bounds__(NT) void long_cols_inv_kernel(const LongArgs a) {
  using G = Geo<P, S>;
  static_assert(!CX || IO == IO_F32, "a complex sample is a pair of float32");
  static_assert(!PHS || (NC > 0 && !CX), "phases: the block layout of the channels-last build, real rows");
  static_assert(!WG || (MAP && !CX && NC == 0 && !PHS), "weight gradient: the mapped form, real rows, no block layout");
  constexpr bool NLC = NC > 0;                  // channels-last y, the block map of long_cols_fwd (PHS: phases for channels)
  constexpr int M = NLC ? NC : 1;
  constexpr int NN = NSEQ / M;
  static_assert(!NLC || (MAP && NC <= NSEQ && (NC & (NC - 1)) == 0), "channels-last: the mapped form, NC * NN == NSEQ");
  const Io<IO> io(a.y_io);
  constexpr unsigned ES = CX ? 8u : Io<IO>::B;  // bytes per sample of y
  constexpr int EW = CX ? 2 : 1;                // elements of Io<IO>::T per sample
  constexpr int T = G::T;                       // == a.N1
  constexpr int LSEQP = SeqLayout<G>::LSEQP;
  static_assert(NT == NSEQ * G::TS && (NSEQ & (NSEQ - 1)) == 0, "one thread slot per point group, column block a power of two");
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const BufRsrc twA = make_rsrc(a.twA1, (unsigned)(P * G::N2 * 8));
  const BufRsrc twB = make_rsrc(a.twB1, (unsigned)(S * P * 8));
  const int tid = threadIdx.x, sq = tid / G::TS, tseq = tid % G::TS;
  unsigned row;                                 // (channels-last: row and o of the block's first channel)
  int n20;
  [[maybe_unused]] unsigned o_nlc = 0, pr_nlc = 0, ph0 = 0;
  if constexpr (!NLC) {
    n20 = (int)fdivmod(blockIdx.x, a.d_nblk, &row) * NSEQ;
  } else if constexpr (PHS) {
    // the phase block of a filter varies fastest, then the filter (a.C of them), then the n2 block, then the pair; the
    // workspace rows of a filter's phases are neighbours, o * s + p
    unsigned q, q2;
    ph0 = fdivmod(blockIdx.x, a.d_ncb, &q) * NC;
    o_nlc = fdivmod(q, a.d_c, &q2);
    n20 = (int)fdivmod(q2, a.d_nblk, &pr_nlc) * NN;
    row = (pr_nlc * (unsigned)a.C + o_nlc) * (unsigned)a.ph_s + ph0;
  } else {
    unsigned q;
    o_nlc = fdivmod(blockIdx.x, a.d_ncb, &q) * NC;
    n20 = (int)fdivmod(q, a.d_nblk, &pr_nlc) * NN;
    row = pr_nlc * (unsigned)a.C + o_nlc;
  }
  const size_t N = (size_t)a.N1 << a.lgN2;
  unsigned pr;
  unsigned o;
  if constexpr (!NLC) {
    o = fdivmod(row, a.d_c, &pr);
  } else {
    o = o_nlc;
    pr = pr_nlc;
  }
  const int b0 = CX ? a.pair0 + (int)pr : 2 * (a.pair0 + (int)pr);      // (complex build: one batch item per row)
  const bool has1 = !CX && b0 + 1 < a.B;
  f2 wtw[P];
  passA_twiddle_fetch<G>(wtw, tseq, twA);
  {
    // (channels-last: the block's workspace rows behind one resource, rows of channels past C read as zero)
    unsigned wbytes = (unsigned)(N * 8);
    if constexpr (PHS) wbytes *= min((unsigned)M, (unsigned)a.ph_s - ph0);      // (rows of phases past s read as zero)
    else if constexpr (NLC) wbytes *= min((unsigned)M, (unsigned)a.C - o);
    const BufRsrc sr = make_rsrc(a.w2 + (size_t)row * N, wbytes);
    f2 val[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
      if constexpr (NLC)
        val[u] = buf_load_f32x2(sr, ((unsigned)(r / NN) * (unsigned)N + ((unsigned)k1 << a.lgN2) + (unsigned)(n20 + (r & (NN - 1)))) * 8u, 0);
      else
        val[u] = buf_load_f32x2(sr, (((unsigned)k1 << a.lgN2) + (unsigned)(n20 + r)) * 8u, 0);
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
      lds[r * LSEQP + G::nat(k1)] = val[u];
    }
  }
  __syncthreads();
  f2 v[P];
  f2* lseq = lds + sq * LSEQP;
  const int j = inv_to_regs_pre<G>(v, wtw, lseq, tseq, true, twB);
  seq_sync<G>();
  {
    // back through LDS so that the stores run along n2 (the samples of one thread are N2 apart in y)
    const int nbase = (tseq >> G::LGS) + P * P * j;
#pragma unroll
    for (int k = 0; k < P; ++k) lseq[G::nat(nbase + P * k)] = v[k];
  }
  __syncthreads();
  // (channels-last: the lanes run over the channels first and NT is a multiple of NSEQ, so a thread stores to one
  // channel, o + tid % NC, and holds that channel's bias; a channel past C reads the last one's and stores nothing)
  unsigned oc = o;
  if constexpr (NLC && !PHS) oc = min(o + (unsigned)(tid & (M - 1)), (unsigned)a.C - 1u);      // (phases share the filter's)
  float b = a.bias ? a.bias[oc * EW] : 0.f;
  asm volatile("" : "+v"(b));
  [[maybe_unused]] float bi = 0.f;              // complex build: the bias is Cout (re, im) pairs
  if constexpr (CX) {
    bi = a.bias ? a.bias[oc * 2 + 1] : 0.f;
    asm volatile("" : "+v"(bi));
  }
  // (the bias is added in float32; a 16-bit y is rounded once, at the store)
  typename Io<IO>::T* y0;                       // (channels-last: the (nout, C) blocks of the pair's two batch items)
  unsigned ybytes;
  if constexpr (NLC && !PHS) {
    y0 = io_ptr<IO>(a.y) + (size_t)b0 * a.C * a.nout * EW;
    ybytes = (unsigned)a.nout * (unsigned)a.C * ES;
  } else if constexpr (WG) {
    y0 = io_ptr<IO>(a.y) + (size_t)o * a.K;
    ybytes = (unsigned)a.K * ES;
  } else {
    y0 = io_ptr<IO>(a.y) + ((size_t)b0 * a.C + o) * a.nout * EW;
    ybytes = (unsigned)a.nout * ES;
  }
  const BufRsrc o0 = make_rsrc(y0, ybytes);
  const BufRsrc o1 = make_rsrc(has1 ? y0 + (size_t)a.C * a.nout : y0, ybytes);
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
    const f2 z = lds[(NLC ? (r & (M - 1)) * NN + r / M : r) * LSEQP + G::nat(n1)];
    const unsigned t = ((unsigned)n1 << a.lgN2) + (unsigned)(n20 + (NLC ? r / M : r));
    unsigned off;
    if constexpr (PHS) {
      // sample t of phase p is y[s*t + p + ph_off]: the lanes run over the phases first, runs of NC * ES bytes per t
      // (of NSEQ * ES where NC == s); samples in front of y, behind it, and of phases past s are dropped
      const unsigned p = ph0 + (unsigned)(r & (M - 1));
      const int n = (int)(t * (unsigned)a.ph_s + p) + a.ph_off;
      off = (p < (unsigned)a.ph_s && (unsigned)n < (unsigned)a.nout) ? (unsigned)n * ES : 0x80000000u;
    } else if constexpr (NLC) {
      const unsigned q = fdiv(t, a.d_ostep), c = o + (unsigned)(r & (M - 1));
      off = (q * a.d_ostep.d == t && q < (unsigned)a.nout && c < (unsigned)a.C) ? (q * (unsigned)a.C + c) * ES : 0x80000000u;
    } else if constexpr (WG) {
      const unsigned q = fdiv(t, a.d_ostep);                 // (lag out_step * q -> the element of tap q)
      off = (q * a.d_ostep.d == t && q < (unsigned)a.keff) ? (unsigned)(a.tap0 + a.tstep * (int)q) * ES : 0x80000000u;
    } else if constexpr (!MAP) {
      off = t < (unsigned)a.nout ? t * ES : 0x80000000u;     // (samples past the kept window: dropped)
    } else {
      const unsigned q = fdiv(t, a.d_ostep);                 // (and those between the kept ones)
      off = (q * a.d_ostep.d == t && q < (unsigned)a.nout) ? q * ES : 0x80000000u;
    }
    if constexpr (CX) {
      buf_store_f32x2(mk2(z.x + b, z.y + bi), o0, off, 0);
    } else {
      io.store(z.x + b, o0, off, 0);
      io.store(z.y + b, o1, has1 ? off : 0x80000000u, 0);
    }
  }
}

// The gated build of long_cols_inv: real rows, the plain form, (B, C, L) tensors, float32 or 16-bit.  Up to two results
// from the one value c = z + bias it holds per sample: y = gate * c and y2 = gate2 * c, a null gate being all ones and a
// null y2 not stored.  The gates lie as y does and are loaded at the offset of the store through resources of y's row;
// the product is one float32 multiply -- (z + b) * gate, never fused with the bias add -- and is rounded once, at the
// store.  With y2_f32 a 16-bit launch stores c itself, unrounded, into a float32 y2.  A kernel of its own, as the gated
// build of long_cols_fwd is.
template <int P, int S, int NSEQ, int NT, int IO>
__global__ __launch_bounds__(NT) void long_cols_inv_gated_kernel(const LongArgs a, const LongGates gt) {
  using G = Geo<P, S>;
  const Io<IO> io(a.y_io);
  constexpr unsigned ES = Io<IO>::B;
  constexpr int LSEQP = SeqLayout<G>::LSEQP;
  static_assert(NT == NSEQ * G::TS && (NSEQ & (NSEQ - 1)) == 0, "one thread slot per point group, column block a power of two");
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const BufRsrc twA = make_rsrc(a.twA1, (unsigned)(P * G::N2 * 8));
  const BufRsrc twB = make_rsrc(a.twB1, (unsigned)(S * P * 8));
  const int tid = threadIdx.x, sq = tid / G::TS, tseq = tid % G::TS;
  unsigned row, pr;
  const int n20 = (int)fdivmod(blockIdx.x, a.d_nblk, &row) * NSEQ;
  const size_t N = (size_t)a.N1 << a.lgN2;
  const unsigned o = fdivmod(row, a.d_c, &pr);
  const int b0 = 2 * (a.pair0 + (int)pr);
  const bool has1 = b0 + 1 < a.B;
  f2 wtw[P];
  passA_twiddle_fetch<G>(wtw, tseq, twA);
  {
    const BufRsrc sr = make_rsrc(a.w2 + (size_t)row * N, (unsigned)(N * 8));
    f2 val[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
      val[u] = buf_load_f32x2(sr, (((unsigned)k1 << a.lgN2) + (unsigned)(n20 + r)) * 8u, 0);
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
      lds[r * LSEQP + G::nat(k1)] = val[u];
    }
  }
  __syncthreads();
  f2 v[P];
  f2* lseq = lds + sq * LSEQP;
  const int j = inv_to_regs_pre<G>(v, wtw, lseq, tseq, true, twB);
  seq_sync<G>();
  {
    const int nbase = (tseq >> G::LGS) + P * P * j;
#pragma unroll
    for (int k = 0; k < P; ++k) lseq[G::nat(nbase + P * k)] = v[k];
  }
  __syncthreads();
  float b = a.bias ? a.bias[o] : 0.f;
  asm volatile("" : "+v"(b));
  // the rows of the pair's two items in y and in every tensor that lies as y does; an absent tensor gets y's address and
  // is never touched (every branch on gt below is wave-uniform)
  const size_t first = ((size_t)b0 * a.C + o) * a.nout, next = has1 ? (size_t)a.C * a.nout : 0;
  const unsigned ybytes = (unsigned)a.nout * ES;
  const auto like_y = [&](const float* p, size_t at) { return make_rsrc(io_ptr<IO>(p ? p : a.y) + at, ybytes); };
  const bool wide2 = IO != IO_F32 && gt.y2_f32;
  const BufRsrc o0 = like_y(a.y, first), o1 = like_y(a.y, first + next);
  const BufRsrc ga0 = like_y(gt.gate, first), ga1 = like_y(gt.gate, first + next);
  const BufRsrc gb0 = like_y(gt.gate2, first), gb1 = like_y(gt.gate2, first + next);
  const BufRsrc p0 = wide2 ? make_rsrc(gt.y2 + first, (unsigned)a.nout * 4u) : like_y(gt.y2, first);
  const BufRsrc p1 = wide2 ? make_rsrc(gt.y2 + first + next, (unsigned)a.nout * 4u) : like_y(gt.y2, first + next);
  // every gate sample of the thread is requested before the first is widened or used (as the loads of long_cols_fwd)
  const auto raw = [&](const BufRsrc& g, unsigned at) {
    if constexpr (IO == IO_F32) return __builtin_amdgcn_raw_buffer_load_b32(g, at, 0, 0);
    else return (unsigned)__builtin_amdgcn_raw_buffer_load_b16(g, at, 0, 0);
  };
  const auto widen = [&](unsigned h) {
    if constexpr (IO == IO_F32) return __uint_as_float(h);
    else return io.in(h);
  };
  const auto place = [&](int u, unsigned* t) {
    const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
    *t = ((unsigned)n1 << a.lgN2) + (unsigned)(n20 + r);
    return *t < (unsigned)a.nout ? *t * ES : 0x80000000u;       // (samples past the kept window: dropped)
  };
  unsigned ra0[P], ra1[P], rb0[P], rb1[P];
#pragma unroll
  for (int u = 0; u < P; ++u) {
    unsigned t;
    const unsigned off = place(u, &t), off1 = has1 ? off : 0x80000000u;
    ra0[u] = gt.gate ? raw(ga0, off) : 0u;
    ra1[u] = gt.gate ? raw(ga1, off1) : 0u;
    rb0[u] = gt.gate2 ? raw(gb0, off) : 0u;
    rb1[u] = gt.gate2 ? raw(gb1, off1) : 0u;
  }
  __builtin_amdgcn_sched_barrier(0);
  // gate * c as a float32 value of its own: the empty asm keeps the compiler from folding the multiply into the 16-bit
  // conversion of the store (v_fma_mixlo_f16 rounds the exact product once; torch rounds to float32, then to 16 bits)
  const auto times = [&](unsigned h, float c) {
    float p = __fmul_rn(widen(h), c);
    asm volatile("" : "+v"(p));
    return p;
  };
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
    const f2 z = lds[r * LSEQP + G::nat(n1)];
    unsigned t;
    const unsigned off = place(u, &t), off1 = has1 ? off : 0x80000000u;
    const bool keep = off != 0x80000000u;
    const float c0 = z.x + b, c1 = z.y + b;
    io.store(gt.gate ? times(ra0[u], c0) : c0, o0, off, 0);
    io.store(gt.gate ? times(ra1[u], c1) : c1, o1, off1, 0);
    if (gt.y2) {
      if (wide2) {
        buf_store_f32(c0, p0, keep ? t * 4u : 0x80000000u, 0);
        buf_store_f32(c1, p1, keep && has1 ? t * 4u : 0x80000000u, 0);
      } else {
        io.store(gt.gate2 ? times(rb0[u], c0) : c0, p0, off, 0);
        io.store(gt.gate2 ? times(rb1[u], c1) : c1, p1, off1, 0);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ blocks (overlap-save)
// The blocks builds of the two column kernels (long_cols_fwd_blocks_kernel, long_cols_inv_blocks_kernel; real rows, the
// plain form, (B, C, L) tensors, float32 and 16-bit) run a row that is longer than the transform as overlap-save blocks of
// N points against ONE filter spectrum of N bins: block t of a row starts hop = N - keff + 1 samples behind block t - 1
// and keeps its first hop results.  The block index is a batch-like index: unit u = b*T + t, T blocks per row, and the
// complex row of pair p carries units 2p and 2p + 1, which may lie in different rows of the tensor -- each unit has a
// row resource and a sample origin of its own.  Everything between the two tensor sides (W1, long_rows, W2) sees pairs
// and channels as ever.  LongBlocks is a second kernel argument of these builds alone, as LongGates is of the gated ones.
struct LongBlocks {
  FastDiv d_T;           // blocks per row: unit u -> (b, t)
  int U;                 // units, B * T; a last odd unit has no partner
  int hop;               // V = N - keff + 1: block t starts at sample t * hop of the padded row / of y
  int win;               // cols_fwd: positions q < win of a block hold samples, the rest reads zero (N for x; hop for the
                         // dY of the weight gradient)
};

// The blocks build of long_cols_fwd: position q of unit (b, t) of channel c holds x[b][c][t*hop + q - padl] where q < win
// and that index lies in [0, L), zero elsewhere.  The index is compared with the row length in SAMPLES and only then
// scaled to bytes: t*hop + q passes 2^29 on long rows (the host keeps it below 2^31), and a scaled value must not wrap
// onto an offset that is read.  Lane order, LDS staging, transform, twiddle and store are those of the plain build.
template <int P, int S, int NSEQ, int NT, int IO>
__global__ __launch_bounds__(NT) void long_cols_fwd_blocks_kernel(const LongArgs a, const LongBlocks bk) {
  using G = Geo<P, S>;
  const Io<IO> io(a.src_io);
  constexpr unsigned ES = Io<IO>::B;
  constexpr int LSEQP = SeqLayout<G>::LSEQP;
  static_assert(NT == NSEQ * G::TS && (NSEQ & (NSEQ - 1)) == 0, "one thread slot per point group, column block a power of two");
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const BufRsrc twA = make_rsrc(a.twA1, (unsigned)(P * G::N2 * 8));
  const BufRsrc twB = make_rsrc(a.twB1, (unsigned)(S * P * 8));
  const int tid = threadIdx.x, sq = tid / G::TS, tseq = tid % G::TS;
  unsigned row, pr;
  const int n20 = (int)fdivmod(blockIdx.x, a.d_nblk, &row) * NSEQ;
  const size_t N = (size_t)a.N1 << a.lgN2;
  const unsigned c = fdivmod(row, a.d_c, &pr);
  // the pair's two units: batch item, block and the row of the tensor each reads
  const unsigned u0 = 2u * ((unsigned)a.pair0 + pr);
  const bool has1 = u0 + 1u < (unsigned)bk.U;
  unsigned bt0, bt1;
  const unsigned t0 = fdivmod(u0, bk.d_T, &bt0), t1 = fdivmod(has1 ? u0 + 1u : u0, bk.d_T, &bt1);
  const unsigned len = (unsigned)a.L, sbytes = len * ES;
  const BufRsrc s0 = make_rsrc(io_ptr<IO>(a.src) + ((size_t)bt0 * a.C + c) * a.L, sbytes);
  const BufRsrc s1 = make_rsrc(io_ptr<IO>(a.src) + ((size_t)bt1 * a.C + c) * a.L, sbytes);
  const int org0 = (int)(t0 * (unsigned)bk.hop) - a.padl, org1 = (int)(t1 * (unsigned)bk.hop) - a.padl;
  {
    f2 val[P];
    const auto place = [&](int u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
      return (n1 << a.lgN2) + n20 + r;
    };
    const auto offset = [&](int q, int org, bool on) {
      const unsigned e = (unsigned)(q + org);
      return on && q < bk.win && e < len ? e * ES : 0x80000000u;
    };
    if constexpr (IO == IO_F32) {
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const int q = place(u);
        val[u].x = buf_load_f32(s0, offset(q, org0, true), 0);
        val[u].y = buf_load_f32(s1, offset(q, org1, has1), 0);
      }
    } else {
      // (all 2 P loads are issued before the first sample is widened, as in the plain build)
      unsigned h0[P], h1[P];
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const int q = place(u);
        h0[u] = __builtin_amdgcn_raw_buffer_load_b16(s0, offset(q, org0, true), 0, 0);
        h1[u] = __builtin_amdgcn_raw_buffer_load_b16(s1, offset(q, org1, has1), 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < P; ++u) val[u] = mk2(io.in(h0[u]), io.in(h1[u]));
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
      lds[r * LSEQP + G::nat(n1)] = val[u];
    }
  }
  __syncthreads();
  f2 v[P];
  f2* lseq = lds + sq * LSEQP;
  nat_load<G>(v, lseq, tseq);
  seq_sync<G>();
  fwd_from_regs<G>(v, lseq, tseq, true, twA, twB);
  __syncthreads();
  const BufRsrc thi = make_rsrc(a.thi, (unsigned)((N >> kLongLoBits) * 8));
  const BufRsrc tlo = make_rsrc(a.tlo, (unsigned)(8u << kLongLoBits));
  const BufRsrc orr = make_rsrc(a.w1 + (size_t)row * N, (unsigned)(N * 8));
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
    const unsigned n2 = (unsigned)(n20 + r);
    const f2 w = long_twiddle(thi, tlo, n2 * (unsigned)k1);
    const f2 z = lds[r * LSEQP + G::nat(k1)];
    buf_store_f32x2(cmul(z, w), orr, (((unsigned)k1 << a.lgN2) + n2) * 8u, 0);
  }
}

// The blocks build of long_cols_inv: the real part is unit 2p, the imaginary part unit 2p + 1; sample j < hop of unit
// (b, t) goes to y[b][o][t*hop + j] where that lies below nout, everything else is dropped (the wrapped-around samples
// behind the hop, and the tail of a row's last block).  The index is compared in samples before it is scaled to bytes.
// W2 loads, inverse transform, the trip through LDS and the bias are those of the plain build.
template <int P, int S, int NSEQ, int NT, int IO>
__global__ __launch_bounds__(NT) void long_cols_inv_blocks_kernel(const LongArgs a, const LongBlocks bk) {
  using G = Geo<P, S>;
  const Io<IO> io(a.y_io);
  constexpr unsigned ES = Io<IO>::B;
  constexpr int LSEQP = SeqLayout<G>::LSEQP;
  static_assert(NT == NSEQ * G::TS && (NSEQ & (NSEQ - 1)) == 0, "one thread slot per point group, column block a power of two");
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const BufRsrc twA = make_rsrc(a.twA1, (unsigned)(P * G::N2 * 8));
  const BufRsrc twB = make_rsrc(a.twB1, (unsigned)(S * P * 8));
  const int tid = threadIdx.x, sq = tid / G::TS, tseq = tid % G::TS;
  unsigned row, pr;
  const int n20 = (int)fdivmod(blockIdx.x, a.d_nblk, &row) * NSEQ;
  const size_t N = (size_t)a.N1 << a.lgN2;
  const unsigned o = fdivmod(row, a.d_c, &pr);
  const unsigned u0 = 2u * ((unsigned)a.pair0 + pr);
  const bool has1 = u0 + 1u < (unsigned)bk.U;
  unsigned bt0, bt1;
  const unsigned t0 = fdivmod(u0, bk.d_T, &bt0), t1 = fdivmod(has1 ? u0 + 1u : u0, bk.d_T, &bt1);
  f2 wtw[P];
  passA_twiddle_fetch<G>(wtw, tseq, twA);
  {
    const BufRsrc sr = make_rsrc(a.w2 + (size_t)row * N, (unsigned)(N * 8));
    f2 val[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
      val[u] = buf_load_f32x2(sr, (((unsigned)k1 << a.lgN2) + (unsigned)(n20 + r)) * 8u, 0);
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int idx = tid + u * NT, r = idx & (NSEQ - 1), k1 = idx / NSEQ;
      lds[r * LSEQP + G::nat(k1)] = val[u];
    }
  }
  __syncthreads();
  f2 v[P];
  f2* lseq = lds + sq * LSEQP;
  const int j = inv_to_regs_pre<G>(v, wtw, lseq, tseq, true, twB);
  seq_sync<G>();
  {
    const int nbase = (tseq >> G::LGS) + P * P * j;
#pragma unroll
    for (int k = 0; k < P; ++k) lseq[G::nat(nbase + P * k)] = v[k];
  }
  __syncthreads();
  float b = a.bias ? a.bias[o] : 0.f;
  asm volatile("" : "+v"(b));
  // (the bias is added in float32; a 16-bit y is rounded once, at the store)
  const unsigned nout = (unsigned)a.nout, ybytes = nout * ES;
  const BufRsrc o0 = make_rsrc(io_ptr<IO>(a.y) + ((size_t)bt0 * a.C + o) * a.nout, ybytes);
  const BufRsrc o1 = make_rsrc(io_ptr<IO>(a.y) + ((size_t)bt1 * a.C + o) * a.nout, ybytes);
  const unsigned at0 = t0 * (unsigned)bk.hop, at1 = t1 * (unsigned)bk.hop;
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int idx = tid + u * NT, r = idx & (NSEQ - 1), n1 = idx / NSEQ;
    const f2 z = lds[r * LSEQP + G::nat(n1)];
    const unsigned s = ((unsigned)n1 << a.lgN2) + (unsigned)(n20 + r);
    const bool kept = s < (unsigned)bk.hop;
    const unsigned e0 = at0 + s, e1 = at1 + s;
    io.store(z.x + b, o0, kept && e0 < nout ? e0 * ES : 0x80000000u, 0);
    io.store(z.y + b, o1, kept && has1 && e1 < nout ? e1 * ES : 0x80000000u, 0);
  }
}

// what one tile geometry contributes: the column passes of an N1 = T plan and the row pass of an N2 = T plan.  The host
// states facts and long_inst.hip picks the build of a column pass: the element type by a.src_io (cols_fwd) / a.y_io
// (cols_inv), the mapped build where `mapped` (padding mode, src_up, tap_dil / out_step), the channels-last build where
// `nlc`, the phases builds for the filter rows and the inverse pass of a launch with a.ph_s > 0, the decimation builds for
// the filter rows and the signal rows of a launch with a.ph_s > 0 and a.ph_cog == 0.  `rows`: rows of the transform per channel in this launch -- batch pairs, batch items of a complex plan, or
// filter rows with a.C == 1 -- which makes rows * a.C workgroup units, or `rows` units of a channels-last launch
struct LongImpl {
  int T, ob;
  hipError_t (*cols_fwd)(const LongArgs& a, bool mapped, bool nlc, long long rows, hipStream_t st);
  hipError_t (*rows)(const LongArgs& a, long long units, hipStream_t st);     // units: filter rows, or pairs * G * nob
  hipError_t (*cols_inv)(const LongArgs& a, bool mapped, bool nlc, long long rows, hipStream_t st);
  // the weight gradient: its row pass (units: G * Cig * ceil(Cog / wg_ob)) and its inverse pass over a.C rows of dW
  int wg_ob;
  hipError_t (*wgrad_rows)(const LongArgs& a, long long units, hipStream_t st);
  hipError_t (*wgrad_inv)(const LongArgs& a, hipStream_t st);
  // the gated builds of the column passes (float32 and 16-bit, plain form): `rows` batch pairs
  hipError_t (*cols_fwd_gated)(const LongArgs& a, const LongGates& gt, long long rows, hipStream_t st);
  hipError_t (*cols_inv_gated)(const LongArgs& a, const LongGates& gt, long long rows, hipStream_t st);
  // the blocks builds of the column passes (float32 and 16-bit, plain form): `rows` unit pairs
  hipError_t (*cols_fwd_blocks)(const LongArgs& a, const LongBlocks& bk, long long rows, hipStream_t st);
  hipError_t (*cols_inv_blocks)(const LongArgs& a, const LongBlocks& bk, long long rows, hipStream_t st);
};

#define FC_DECLARE_LONG(P, S) const LongImpl* get_long_P##P##_S##S();
FC_DECLARE_LONG(8, 1)
FC_DECLARE_LONG(8, 2)
FC_DECLARE_LONG(16, 1)
FC_DECLARE_LONG(16, 2)
FC_DECLARE_LONG(32, 1)
FC_DECLARE_LONG(32, 2)
FC_DECLARE_LONG(32, 4)

}  // namespace fc
