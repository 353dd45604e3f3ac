// long_spec.hpp -- up to `head` draft tokens of a causal long filter verified in one launch WITHOUT the accumulator being
// touched (include/fftconv_amd.h "Token-by-token decoding", fc_long_spec): long_push_kernel (long_push.hpp) for tokens
// that may be rejected.
//
// For the columns t = t0 ... t0 + count - 1 (count <= U = head), the chunk tensors indexed by j = t - t0:
//   z[c][t] = pregate[b][c][j] * x[b][c][j]                                     stored to hist[b][c][t]
//   y[o][j] = postgate[b][o][j] * (acc[b][o][t] + bias[o] + head(o, t) + late(o, t))
//   head(o, t) = sum_c sum_{k < U, t - k >= first} taps[o][c][k] * z[c][t - k]                    (the push kernel's sum)
//   late(o, t) = sum_c sum_{n} sum_{e} filter[o][c][t - M + n - e] * hist[c][M - n + e]            (only for t >= M)
// M is the one multiple of U inside (t0, t0 + count) -- none: no column has a late sum.  The blocks that a step or a push
// would run at M (functional._long_stream_blocks) have not been run: late(o, t) is what they would have put on column t.
// n runs over the levels U, 2U, 4U, ... below K that divide M, e over 0 ... t - M, and a pair counts when its sample
// M - n + e >= first and its tap t - M + n - e < min(2n, K).  Every such sample lies below t0 (t - n < t0 because
// t - t0 < U <= n) and at or past 0 (n divides M): an old sample of hist, never a column this launch writes.
//
// The index prologue, the staging, the stores of hist, the head chain and the epilogue ARE the push kernel's: both kernels
// run LongChunk (long_push.hpp; one workgroup per (batch item, group, tile of 64 columns), one lane per column, one wave
// per output channel at a time).  The epilogue combines as r = acc; r += bias; r += head: a column below M has the bits a
// push gives it.  Then r += late (columns at or past M only), r *= postgate, rounded once.  This kernel's own are d, dmax
// and `late`, the late chain, and the late term it hands to the epilogue.
// The late sum of an output is ONE chain of fused multiply-adds of its own, in an order fixed by (t, M, U, K, first):
//   c ascending (all input channels of the group), then the level n ascending, then e ascending (samples ascending, taps
//   descending); pairs outside the conditions above are skipped, not added as zeros.
// No atomics, no cross-lane reduction: two launches on the same state return the same bits.  For a fixed (c, n, e) the
// sample is the same for every lane (a broadcast read of hist) and the tap index falls by one per lane, so the taps are
// read from the flipped filter (tap k of (o, c) at K - 1 - k), whose addresses rise with the lane: 64 consecutive words.
// The loop over e runs to the tile's last column (workgroup-uniform), lanes select.  At most (count - 1) * levels * Cin/g
// multiply-adds per output; the late sum uses no LDS (staging the old samples there measured no faster: DESIGN 4.7).
// All global indices are 64-bit; the LDS image is the push kernel's.
#pragma once
#include "long_push.hpp"

namespace fc {

struct LongSpecArgs {
  LongPushArgs p;         // as the push: x, gates, head taps, bias, hist, acc, y, t0, count, first, max_len, tiles, cblock ...
  const float* flipped;   // (Cout, Cig, K) the whole filter, flipped: tap k at K - 1 - k
  long long M;            // the multiple of U inside (t0, t0 + count) whose blocks are due, below max_len; unused if levels == 0
  long long K;            // taps of the filter
  int levels;             // levels U << 0 ... U << (levels - 1) divide M and lie below K; 0: no late sum
};

template <int IO>
__global__ __launch_bounds__(64 * kLongPushWaves) void long_spec_kernel(const LongSpecArgs s) {
  const LongPushArgs& a = s.p;
  const LongChunk<IO> t(a);
  const int U = t.U, Cig = t.Cig, Cog = t.Cog;
  // (read once into registers: with these left as loads of `s` inside the chain, the compiler keeps the pair conditions
  // as branches and the eight loads of an unrolled round no longer overlap -- measured 14 to 25 % slower on dense layers)
  const long long first = a.first, K = s.K, M = s.M;
  const int levels = s.levels;
  // the late sum: d = t - M of this lane (negative: none), dmax that of the tile's last live column (workgroup-uniform)
  const long long d = a.t0 + t.j - M;
  const long long dmax = a.t0 + min(t.j0 + 63, a.count - 1) - M;
  const bool late = levels > 0 && t.live && d >= 0;
  for (int o0 = 0; o0 < Cog; o0 += t.nwaves) {
    const int o = o0 + t.wave;                           // wave-uniform
    const float sh = t.head(o0);
    float sl = 0.f;
    if (o < Cog && levels > 0 && dmax >= 0) {            // (wave-uniform)
      for (int c = 0; c < Cig; ++c) {
        const float* hc = t.hist + (size_t)c * (size_t)a.max_len;
        // tap k of (o, c) is fk[-k]
        const float* fk = s.flipped + (((size_t)t.g * Cog + o) * (size_t)Cig + (size_t)c) * (size_t)K + (size_t)(K - 1);
        for (int lv = 0; lv < levels; ++lv) {
          const long long n = (long long)U << lv;
          const long long tap1 = min(2 * n, K);
          const long long s0 = M - n;                    // the block's first sample, >= 0; s0 + dmax < t0
          // Both loads are unconditional, so that the loads of several e are in flight at once (the chain itself is
          // serial): hc[s0 + e] is in range for every e <= dmax, the tap index is clamped into [0, K) where the pair does
          // not count.  A pair that does not count is skipped by a select, never added: dead values cannot reach `sl`.
#pragma unroll 8
          for (long long e = 0; e <= dmax; ++e) {
            const long long k = d + n - e;               // >= n when e <= d
            const bool on = late && e <= d && s0 + e >= first && k < tap1;
            const float wk = fk[-min(max(k, 0LL), K - 1)], zs = hc[s0 + e];
            const float next = __builtin_fmaf(wk, zs, sl);
            sl = on ? next : sl;
          }
        }
      }
    }
    t.store(o, sh, late, sl);
  }
}

// the float32 or the 16-bit build by the fc_dtype code of s.p.io; grid = B * groups * tiles workgroups of `waves` waves
hipError_t long_spec_launch(const LongSpecArgs& s, long long grid, int waves, size_t lds, hipStream_t st);

}  // namespace fc
