// long_push.hpp -- `count` consecutive decoding steps of a causal long filter in one launch (include/fftconv_amd.h
// "Token-by-token decoding", fc_long_push): the sibling of long_step_kernel (long_step.hpp) for a chunk of tokens.
//
// For the columns t = t0 ... t0 + count - 1, the chunk tensors indexed by j = t - t0:
//   z[c][t] = pregate[b][c][j] * x[b][c][j]                                     stored to hist[b][c][t]
//   y[o][j] = postgate[b][o][j] * (bias[o] + acc[b][o][t] + sum_c sum_{k < U, t - k >= first} taps[o][c][k] * z[c][t - k])
// One workgroup per (batch item, group, tile of 64 columns), one lane per column, one wave per output channel at a time.
// The tile's 64 + U - 1 samples of a block of input channels are staged as float32 in LDS: a sample at or past t0 is the
// chunk's (the product is formed again -- another workgroup may be the one that stores it, so hist is never read there), a
// sample below t0 is read from hist, one below `first` is zero.  The workgroup stores the hist columns of its own tile as
// it stages them, once.  The taps of (o, c) are wave-uniform reads (the wave index goes through readfirstlane), the LDS
// reads of a wave are 64 consecutive words.  Every output is ONE chain of fused multiply-adds over c ascending, then k
// ascending, whatever the tile or the chunk: the bits of a column do not depend on how a row was cut into launches.
// When a group's input channels pass one LDS block, the blocks are staged again for every round of output channels (the
// chain of an output stays in one register); with one block -- depthwise layers, and dense ones up to 64 channels per
// group at U = 64 -- staging happens once.  All global indices are 64-bit; the LDS image is at most kLongPushLds bytes.
#pragma once
#include "fft_engine.hpp"

namespace fc {

struct LongPushArgs {
  const void* x;          // (B, Cin, count) samples of the chunk, Io<IO>::T
  const void* pregate;    // like x, or null: all ones
  const void* postgate;   // (B, Cout, count), or null: all ones
  const float* taps;      // (Cout, Cig, U) head taps, zero past K
  const float* bias;      // (Cout) or null
  float* hist;            // (B, Cin, max_len): columns t0 ... t0 + count - 1 are written, earlier ones read
  const float* acc;       // (B, Cout, max_len): columns t0 ... t0 + count - 1 are read
  void* y;                // (B, Cout, count), Io<IO>::T
  long long t0, count, first, max_len;
  int tiles;              // ceil(count / 64)
  int cblock;             // input channels staged at a time: cblock * (64 + U - 1) * 4 <= kLongPushLds
  int Cin, Cout, groups, ulog, io;
};

constexpr int kLongPushWaves = 4;
constexpr int kLongPushLds = 32 * 1024;

// One workgroup's tile of 64 chunk columns: the index prologue, the staging with the hist stores, the head chain and the
// epilogue described above, for long_push_kernel and for long_spec_kernel (long_spec.hpp).  A draft column without a late
// sum has the bits a push gives it because both kernels run THIS code; every member is inlined.
template <int IO>
struct LongChunk {
  using T = typename Io<IO>::T;
  const LongPushArgs& a;
  const Io<IO> io;
  int g, Cig, Cog, tid, nthreads, lane, wave, nwaves, U, W, nblocks;
  long long j0, base, j;
  size_t yrow;
  const T *x, *pre;
  float* hist;            // row 0 of the group's input channels
  bool live;

  __device__ __forceinline__ explicit LongChunk(const LongPushArgs& args) : a(args), io(args.io) {
    const int tile = blockIdx.x % a.tiles;
    const int bg = blockIdx.x / a.tiles;
    g = bg % a.groups;
    const int b = bg / a.groups;
    Cig = a.Cin / a.groups, Cog = a.Cout / a.groups;
    tid = threadIdx.x, nthreads = blockDim.x;
    lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthreads >> 6;
    U = 1 << a.ulog, W = 64 + U - 1;
    j0 = (long long)tile * 64;                           // first chunk column of the tile
    base = a.t0 + j0 - (U - 1);                          // row position of staged sample 0 (may be negative)
    const size_t xrow = (size_t)b * a.Cin + (size_t)g * Cig;
    yrow = (size_t)b * a.Cout + (size_t)g * Cog;
    x = static_cast<const T*>(a.x) + xrow * (size_t)a.count;
    pre = a.pregate ? static_cast<const T*>(a.pregate) + xrow * (size_t)a.count : nullptr;
    hist = a.hist + xrow * (size_t)a.max_len;
    j = j0 + lane;                                       // this lane's column of the chunk
    live = j < a.count;
    nblocks = (Cig + a.cblock - 1) / a.cblock;
  }

  // The head chain of output channel o0 + wave of the group (0 for a wave past Cog); every wave of the workgroup calls it
  // for the same o0, ascending from 0: the round o0 == 0 stores the tile's hist columns.
  __device__ __forceinline__ float head(int o0) const {
    extern __shared__ float lds_chunk[];
    const int o = o0 + wave;                             // wave-uniform
    float s = 0.f;
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
            lds_chunk[c * W + i] = z;
          }
        }
        __syncthreads();
      }
      if (o < Cog) {
        const float* w = a.taps + (((size_t)g * Cog + o) * (size_t)Cig + (size_t)c0) * (size_t)U;
        for (int c = 0; c < nc; ++c) {
          const float* zc = lds_chunk + c * W + lane + (U - 1);
          const float* wc = w + (size_t)c * U;
#pragma unroll 8
          for (int k = 0; k < U; ++k) s = __builtin_fmaf(wc[k], zc[-k], s);
        }
      }
    }
    return s;
  }

  // y of output channel o at this lane's column: r = acc; r += bias; r += head; [r += late;] r *= postgate, rounded once
  __device__ __forceinline__ void store(int o, float head, bool has_late = false, float late = 0.f) const {
    if (o < Cog && live) {
      float r = a.acc[(yrow + o) * (size_t)a.max_len + (size_t)(a.t0 + j)];
      if (a.bias) r += a.bias[g * Cog + o];
      r += head;
      if (has_late) r += late;
      const size_t at = (yrow + o) * (size_t)a.count + (size_t)j;
      if (a.postgate) r *= io.in(static_cast<const T*>(a.postgate)[at]);
      static_cast<T*>(a.y)[at] = io.out(r);
    }
  }
};

template <int IO>
__global__ __launch_bounds__(64 * kLongPushWaves) void long_push_kernel(const LongPushArgs a) {
  const LongChunk<IO> t(a);
  for (int o0 = 0; o0 < t.Cog; o0 += t.nwaves) t.store(o0 + t.wave, t.head(o0));
}

// the float32 or the 16-bit build by the fc_dtype code of a.io; grid = B * groups * tiles workgroups of `waves` waves
hipError_t long_push_launch(const LongPushArgs& a, long long grid, int waves, size_t lds, hipStream_t st);

}  // namespace fc
