// long_step.hpp -- one decoding step of a causal long filter (include/fftconv_amd.h "Token-by-token decoding").
//
// The stream of functional.FFTLongConvStream cuts a causal convolution into power-of-two blocks that land on future
// positions of a float32 accumulator `acc`; what is left for the step at position t are the U head taps:
//   z[c]  = pregate[b][c] * x_t[b][c]                                         stored to hist[b][c][t]
//   y[o]  = postgate[b][o] * (bias[o] + acc[b][o][t] + sum_c sum_{k < U, t - k >= first} taps[o][c][k] * z[c][t - k])
// One workgroup per (batch item, group), one wave per output channel at a time.  The lanes of a wave run over the
// flattened (input channel, tap) index j = c * U + k, so U >= 64 gives a lane one contiguous run of history per channel
// and U < 64 puts 64 / U channels side by side; the taps of an output channel (Cig * U float32, zero past K) are one
// contiguous row read in j order.  Tap 0 comes from the registers that hold z, never from hist: the store of column t is
// another lane's (wave 0's, as it works on the group's first output).  The history of the group lies behind one buffer
// resource whose base is advanced in 64 bits; a position below `first` gets the out-of-resource offset and reads as zero.
// The wave sum is a butterfly of __shfl_xor, no LDS memory and no atomics.
#pragma once
#include "fft_engine.hpp"

namespace fc {

struct LongStepArgs {
  const void* x;          // (B, Cin) samples of this step, Io<IO>::T
  const void* pregate;    // like x, or null: all ones
  const void* postgate;   // (B, Cout), or null: all ones
  const float* taps;      // (Cout, Cig, U) head taps, zero past K
  const float* bias;      // (Cout) or null
  float* hist;            // (B, Cin, max_len): column t is written
  const float* acc;       // (B, Cout, max_len): column t is read
  void* y;                // (B, Cout), Io<IO>::T
  long long t, max_len;
  int reach;              // taps 1 ... reach lie at or behind `first`: min(U - 1, t - first)
  int Cin, Cout, groups, ulog, io;
};

constexpr int kLongStepWaves = 4;

template <int IO>
__global__ __launch_bounds__(64 * kLongStepWaves) void long_step_kernel(const LongStepArgs a) {
  using T = typename Io<IO>::T;
  const Io<IO> io(a.io);
  const int g = blockIdx.x % a.groups, b = blockIdx.x / a.groups;
  const int Cig = a.Cin / a.groups, Cog = a.Cout / a.groups;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const size_t xrow = (size_t)b * a.Cin + (size_t)g * Cig, yrow = (size_t)b * a.Cout + (size_t)g * Cog;
  const T* x = static_cast<const T*>(a.x) + xrow;
  const T* pre = a.pregate ? static_cast<const T*>(a.pregate) + xrow : nullptr;
  // (the host keeps Cig * max_len * 4 below 2^31: every offset fits, and 0x80000000 lies outside)
  const BufRsrc hr = make_rsrc(a.hist + xrow * (size_t)a.max_len, (unsigned)((size_t)Cig * a.max_len * 4));
  const unsigned row = (unsigned)a.max_len, t = (unsigned)a.t;
  const int n = Cig << a.ulog, umask = (1 << a.ulog) - 1;
  for (int o = wave; o < Cog; o += nwaves) {
    const float* w = a.taps + ((size_t)g * Cog + o) * (size_t)n;
    float s = 0.f;
#pragma unroll 4
    for (int j = lane; j < n; j += 64) {
      const int c = j >> a.ulog, k = j & umask;
      const unsigned at = ((unsigned)c * row + t) * 4u;
      float z;
      if (k == 0) {
        z = io.in(x[c]);
        if (pre) z *= io.in(pre[c]);
        if (o == 0) buf_store_f32(z, hr, at, 0);
      } else {
        z = buf_load_f32(hr, k <= a.reach ? at - 4u * (unsigned)k : 0x80000000u, 0);
      }
      s += w[j] * z;
    }
#pragma unroll
    for (int m = 32; m; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) {
      float r = a.acc[(yrow + o) * (size_t)a.max_len + (size_t)a.t];
      if (a.bias) r += a.bias[g * Cog + o];
      r += s;
      if (a.postgate) r *= io.in(static_cast<const T*>(a.postgate)[yrow + o]);
      static_cast<T*>(a.y)[yrow + o] = io.out(r);
    }
  }
}

// the float32 or the 16-bit build by the fc_dtype code of a.io; grid = B * groups workgroups of `waves` waves
hipError_t long_step_launch(const LongStepArgs& a, long long grid, int waves, hipStream_t st);

}  // namespace fc
