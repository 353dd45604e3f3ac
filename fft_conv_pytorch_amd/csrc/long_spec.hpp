// long_spec.hpp -- up to `head` draft tokens of a causal long filter verified in one launch WITHOUT the accumulator being
// touched (include/fftconv_amd.h "Token-by-token decoding", fc_long_spec): the sibling of long_push_kernel (long_push.hpp)
// for tokens that may be rejected.
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
// The staging, the head chain and the stores of hist are the push kernel's (one workgroup per (batch item, group, tile of
// 64 columns), one lane per column, one wave per output channel at a time; see long_push.hpp), and the head chain
// combines as r = acc; r += bias; r += head: a column below M has the bits a push gives it.  Then r += late (columns at or
// past M only), r *= postgate, rounded once.
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
  using T = typename Io<IO>::T;
  extern __shared__ float lds_spec[];
  const LongPushArgs& a = s.p;
  const Io<IO> io(a.io);
  const int tile = blockIdx.x % a.tiles;
  const int bg = blockIdx.x / a.tiles;
  const int g = bg % a.groups, b = bg / a.groups;
  const int Cig = a.Cin / a.groups, Cog = a.Cout / a.groups;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthreads >> 6;
  const int U = 1 << a.ulog, W = 64 + U - 1;
  const long long j0 = (long long)tile * 64;             // first chunk column of the tile
  const long long base = a.t0 + j0 - (U - 1);            // row position of staged sample 0 (may be negative)
  const size_t xrow = (size_t)b * a.Cin + (size_t)g * Cig, yrow = (size_t)b * a.Cout + (size_t)g * Cog;
  const T* x = static_cast<const T*>(a.x) + xrow * (size_t)a.count;
  const T* pre = a.pregate ? static_cast<const T*>(a.pregate) + xrow * (size_t)a.count : nullptr;
  float* hist = a.hist + xrow * (size_t)a.max_len;
  const long long j = j0 + lane;                         // this lane's column of the chunk
  const bool live = j < a.count;
  const int nblocks = (Cig + a.cblock - 1) / a.cblock;
  // the late sum: d = t - M of this lane (negative: none), dmax that of the tile's last live column (workgroup-uniform)
  const long long d = a.t0 + j - s.M;
  const long long dmax = a.t0 + min(j0 + 63, a.count - 1) - s.M;
  const bool late = s.levels > 0 && live && d >= 0;
  for (int o0 = 0; o0 < Cog; o0 += nwaves) {
    const int o = o0 + wave;                             // wave-uniform
    float sh = 0.f;
    for (int c0 = 0; c0 < Cig; c0 += a.cblock) {
      const int nc = min(a.cblock, Cig - c0);
      if (nblocks > 1 || o0 == 0) {                      // (workgroup-uniform: every wave meets the barriers)
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
          const size_t ch = (size_t)(c0 + c);
          for (int i = tid; i < W; i += nthreads) {
            const long long pos = base + i;
            float z = 0.f;
            if (pos >= a.first) {
              const long long jj = pos - a.t0;
              if (jj < 0) {
                z = hist[ch * (size_t)a.max_len + (size_t)pos];
              } else if (jj < a.count) {
                z = io.in(x[ch * (size_t)a.count + (size_t)jj]);
                if (pre) z *= io.in(pre[ch * (size_t)a.count + (size_t)jj]);
                if (o0 == 0 && i >= U - 1) hist[ch * (size_t)a.max_len + (size_t)pos] = z;      // the tile's own column
              }
            }
            lds_spec[c * W + i] = z;
          }
        }
        __syncthreads();
      }
      if (o < Cog) {
        const float* w = a.taps + (((size_t)g * Cog + o) * (size_t)Cig + (size_t)c0) * (size_t)U;
        for (int c = 0; c < nc; ++c) {
          const float* zc = lds_spec + c * W + lane + (U - 1);
          const float* wc = w + (size_t)c * U;
#pragma unroll 8
          for (int k = 0; k < U; ++k) sh = __builtin_fmaf(wc[k], zc[-k], sh);
        }
      }
    }
    float sl = 0.f;
    if (o < Cog && s.levels > 0 && dmax >= 0) {          // (wave-uniform)
      for (int c = 0; c < Cig; ++c) {
        const float* hc = hist + (size_t)c * (size_t)a.max_len;
        // tap k of (o, c) is fk[-k]
        const float* fk = s.flipped + (((size_t)g * Cog + o) * (size_t)Cig + (size_t)c) * (size_t)s.K + (size_t)(s.K - 1);
        for (int lv = 0; lv < s.levels; ++lv) {
          const long long n = (long long)U << lv;
          const long long tap1 = min(2 * n, s.K);
          const long long s0 = s.M - n;                  // the block's first sample, >= 0; s0 + dmax < t0
          // Both loads are unconditional, so that the loads of several e are in flight at once (the chain itself is
          // serial): hc[s0 + e] is in range for every e <= dmax, the tap index is clamped into [0, K) where the pair does
          // not count.  A pair that does not count is skipped by a select, never added: dead values cannot reach `sl`.
#pragma unroll 8
          for (long long e = 0; e <= dmax; ++e) {
            const long long k = d + n - e;               // >= n when e <= d
            const bool on = late && e <= d && s0 + e >= a.first && k < tap1;
            const float wk = fk[-min(max(k, 0LL), s.K - 1)], zs = hc[s0 + e];
            const float next = __builtin_fmaf(wk, zs, sl);
            sl = on ? next : sl;
          }
        }
      }
    }
    if (o < Cog && live) {
      float r = a.acc[(yrow + o) * (size_t)a.max_len + (size_t)(a.t0 + j)];
      if (a.bias) r += a.bias[g * Cog + o];
      r += sh;
      if (late) r += sl;
      const size_t at = (yrow + o) * (size_t)a.count + (size_t)j;
      if (a.postgate) r *= io.in(static_cast<const T*>(a.postgate)[at]);
      static_cast<T*>(a.y)[at] = io.out(r);
    }
  }
}

// the float32 or the 16-bit build by the fc_dtype code of s.p.io; grid = B * groups * tiles workgroups of `waves` waves
hipError_t long_spec_launch(const LongSpecArgs& s, long long grid, int waves, size_t lds, hipStream_t st);

}  // namespace fc
