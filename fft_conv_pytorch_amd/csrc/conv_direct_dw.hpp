// conv_direct_dw.hpp -- time-domain forward of a depthwise 2-D / 3-D convolution with a small kernel: a
// weight with one input channel per group and a channel multiplier m = Cout/g of 1 .. 8, the layers conv_direct.hpp
// refuses,
//   y[b][g*m + j][t] = bias[g*m + j] + sum_k W[g*m + j][0][k] * Xpad[b][g][t*stride + k*dilation - pad]
// on the vector ALU in float32.  With `transposed` the stride-1 transposed convolution, which is the dX of a stride-1
// zero-padded depthwise layer: the weight is read where it lies, the taps flipped, the planner passes d*(k-1) - p,
//   out[b][g][t] = bias[g] + sum_j sum_k W[g*m + j][0][K-1-k] * Ypad[b][g*m + j][t + k*dilation - pad'].
//
// Work split.  A workgroup (4 waves) owns one batch item, one group and one spatial output tile.  Forward it produces
// all m output channels of the group from one staged x halo; transposed it stages the m dY halos of the group and
// produces the one channel.  Every output sample is written exactly once, by one thread, bias added, rounded once
// (Io<>).  Nothing else is written, no workspace, no atomics: the bits of y are a function of the geometry alone.
//
// Positions go to lanes.  A tile row is cut into runs of kDwR = 4 consecutive outputs; thread t owns the runs
// t, t + 256, ..., NR of them at most, and keeps acc[NR][M][4] sums in registers with compile-time indices: M is the
// build's multiplier slot count (forward; a slot past m multiplies staged zeros into sums nobody stores) or 1 (transposed), and
// NR * M = 8 in every build.  A run past the tile computes on the first run's window and stores nothing; a whole round
// of runs past the tile is skipped by a wave-uniform branch.
//
// Data movement.  Staged once per workgroup, widened to float32 as loaded:
//   wl[j][row][kxp]  the m * taps weights of the group, a (kz, ky) tap row padded to whole blocks of KXB taps;
//   xl[halo]         the halo (wgd_stage_halo of wgrad_direct.hpp, as it is), rows padded to a pitch in which every
//                    run's window starts on a 16-byte boundary and stays inside its row (transposed: m halos).
// Per tap row and block of KXB taps the weights of the block are read once for all runs of the thread (wave-uniform
// addresses: broadcast reads), then per run the 4 + KXB - 1 word window as 16-byte reads for 4 * KXB * M FMAs.  Stride
// or dilation other than 1 on the last axis takes the general KXB = 1 build, one read per product.
//
// Dead taps and positions.  A ragged last block takes the straight-line copy of the products for its count of live
// taps, chosen by a wave-uniform branch (the block index is wave-uniform): a dead tap forms no product at all, so none
// is 0 * x, and whole blocks pay nothing.  A dead position is computed from staged samples of its row's padding and
// never stored.
//
// Summation.  One chain per output sample over the taps in tensor order, <= 128 terms; transposed: acc1 per channel,
// acc2 += acc1 over the m channels.
//
// Addressing: size_t into global memory, int for LDS and positions.
#pragma once
#include "wgrad_direct_dw.hpp"

namespace fc {

constexpr int kCdwThreads = kWgdThreads;
constexpr int kCdwMaxMultiplier = 8;      // channel multiplier: slots of the largest build
constexpr int kCdwAcc = 8;                // NR * M of every build: 32 accumulators per thread

struct ConvDirectDwArgs {
  const void* x;        // (B, Cin, *S)
  const void* w;        // (G * m, 1, *k), forward and transposed
  const void* bias;     // (Cout) or null
  void* y;              // (B, Cout, *O)
  AxisMap map[3];       // per axis (z, y, x; a 2-D layer has a z axis of one sample)
  int S[3], O[3];
  int k[3], stride[3], dil[3];
  int tile[3], ntile[3];
  int halo[3];          // halo[2]: the padded pitch of a halo row
  FastDiv fd_hx, fd_hy; // of wgd_stage_halo
  FastDiv fd_rx, fd_ty; // runs per tile row, rows per tile plane
  int Cin, Cout, G, m, taps;
  int runs;             // runs of a tile
  int nbx, kxp, wp;     // tap blocks per kernel row, floats per staged tap row and per staged channel
  int wl;               // floats of the staged weights, a multiple of 4
  int vec;              // y, O[2] and tile[2] let a live run be stored as one 4-sample access
  int io;               // fc_dtype code of x, weight, bias and y
};

// One block of KXB taps, the first KLIVE of them live, of one tap row into the sums of the thread's runs.  wrow: the
// block's weights of channel slot 0 (slot j: wp floats on); xl + xo[i] + toff: the window of run i.  Straight-line but for
// the rounds of runs: a dead tap is left out at compile time, a dead slot multiplies staged zeros into sums nobody stores.
template <int KXB, int KLIVE, int M, int NR>
__device__ __forceinline__ void cdw_block(float (&acc)[NR][M][kDwR], const float* xl, const float* wrow, int wp, const int (&xo)[NR],
                                          int toff, int nrw, int sx) {
  float wv[M][KXB];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    if constexpr (KXB >= 4) {
#pragma unroll
      for (int q = 0; q < (KLIVE + 3) / 4; ++q) {
        const dw_v4f t = reinterpret_cast<const dw_v4f*>(wrow + j * wp)[q];
        wv[j][4 * q] = t[0]; wv[j][4 * q + 1] = t[1]; wv[j][4 * q + 2] = t[2]; wv[j][4 * q + 3] = t[3];
      }
    } else {
      wv[j][0] = wrow[j * wp];
    }
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    if (i >= nrw) break;      // wave-uniform
    const float* xp = xl + xo[i] + toff;
    if constexpr (KXB == 1) {
      float xv[kDwR];
#pragma unroll
      for (int r = 0; r < kDwR; ++r) xv[r] = xp[r * sx];
#pragma unroll
      for (int j = 0; j < M; ++j)
#pragma unroll
        for (int r = 0; r < kDwR; ++r) acc[i][j][r] = __builtin_fmaf(wv[j][0], xv[r], acc[i][j][r]);
    } else {
      constexpr int W4 = dw_window4(KLIVE);      // (the words the live taps reach, in whole reads)
      float xw[4 * W4];
#pragma unroll
      for (int q = 0; q < W4; ++q) {
        const dw_v4f t = reinterpret_cast<const dw_v4f*>(xp)[q];
        xw[4 * q] = t[0]; xw[4 * q + 1] = t[1]; xw[4 * q + 2] = t[2]; xw[4 * q + 3] = t[3];
      }
#pragma unroll
      for (int j = 0; j < M; ++j)
#pragma unroll
        for (int k = 0; k < KLIVE; ++k)
#pragma unroll
          for (int r = 0; r < kDwR; ++r) acc[i][j][r] = __builtin_fmaf(wv[j][k], xw[r + k], acc[i][j][r]);
    }
  }
}

// the block with `klive` live taps: one straight-line copy per count
template <int KXB, int M, int NR, int KLIVE = KXB>
__device__ __forceinline__ void cdw_block_of(float (&acc)[NR][M][kDwR], const float* xl, const float* wrow, int wp, const int (&xo)[NR],
                                             int toff, int klive, int nrw, int sx) {
  if constexpr (KLIVE == 1) {
    cdw_block<KXB, 1, M, NR>(acc, xl, wrow, wp, xo, toff, nrw, sx);
  } else {
    if (klive == KLIVE) cdw_block<KXB, KLIVE, M, NR>(acc, xl, wrow, wp, xo, toff, nrw, sx);      // wave-uniform
    else cdw_block_of<KXB, M, NR, KLIVE - 1>(acc, xl, wrow, wp, xo, toff, klive, nrw, sx);
  }
}

// Every tap of one staged halo into the sums of the thread's runs: tap rows in tensor order, blocks along the row.
template <int KXB, int M, int NR>
__device__ __forceinline__ void cdw_accumulate(float (&acc)[NR][M][kDwR], const ConvDirectDwArgs& a, const float* xl, const float* wl,
                                               const int (&xo)[NR], int nrw, int HyHx, int hxp) {
#pragma unroll 1
  for (int kz = 0; kz < a.k[0]; ++kz)
#pragma unroll 1
    for (int ky = 0; ky < a.k[1]; ++ky) {
      const int rowoff = kz * a.dil[0] * HyHx + ky * a.dil[1] * hxp;
      const float* wrow = wl + (kz * a.k[1] + ky) * a.kxp;
#pragma unroll 1
      for (int bx = 0; bx < a.nbx; ++bx)
        cdw_block_of<KXB, M, NR>(acc, xl, wrow + bx * KXB, a.wp, xo, rowoff + bx * KXB * a.dil[2], min(KXB, a.k[2] - bx * KXB), nrw,
                                 a.stride[2]);
    }
}

// run q of the tile -> its first position in the tile
__device__ __forceinline__ void cdw_run(const ConvDirectDwArgs& a, int q, int& pz, int& py, int& px) {
  unsigned t, z;
  px = (int)fdivmod((unsigned)q, a.fd_rx, &t) * kDwR;
  py = (int)fdivmod(t, a.fd_ty, &z);
  pz = (int)z;
}

template <int IO, int KXB, int M, int NR, bool TR>
__global__ __launch_bounds__(kCdwThreads) void conv_direct_dw_kernel(const ConvDirectDwArgs a) {
  static_assert(M * NR == kCdwAcc && (!TR || M == 1), "32 accumulators per thread; the transposed form sums into one channel");
  using T = typename Io<IO>::T;
  extern __shared__ __attribute__((aligned(16))) float cdw_lds[];
  float* wl = cdw_lds;
  float* xl = cdw_lds + a.wl;
  const Io<IO> io(a.io);
  const T* xg = static_cast<const T*>(a.x);
  const T* wg = static_cast<const T*>(a.w);
  const T* bg = static_cast<const T*>(a.bias);
  T* yg = static_cast<T*>(a.y);
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6);

  // workgroup -> (batch item, group, tile): the tiles of one channel run next to each other and share their halos in L2
  unsigned bid = blockIdx.x;
  const int tiles = a.ntile[0] * a.ntile[1] * a.ntile[2];
  int t = bid % tiles; bid /= tiles;
  const int g = bid % a.G, b = bid / a.G;
  const int o0x = (t % a.ntile[2]) * a.tile[2]; t /= a.ntile[2];
  const int o0y = (t % a.ntile[1]) * a.tile[1], o0z = (t / a.ntile[1]) * a.tile[0];
  const int hxp = a.halo[2], HyHx = a.halo[1] * hxp, HV = a.halo[0] * HyHx;
  const size_t Ovol = (size_t)a.O[0] * a.O[1] * a.O[2], Svol = (size_t)a.S[0] * a.S[1] * a.S[2];

  // the weights of the group, tap rows padded to whole blocks (a dead tap: a zero that no product reads)
  for (int e = tid; e < a.wl; e += kCdwThreads) {
    const int j = e / a.wp, rem = e - j * a.wp, row = rem / a.kxp, kx = rem - row * a.kxp;
    const int tap = row * a.k[2] + kx;
    const bool live = j < a.m && kx < a.k[2] && tap < a.taps;
    wl[e] = live ? io.in(wg[(size_t)(g * a.m + j) * a.taps + (TR ? a.taps - 1 - tap : tap)]) : 0.f;
  }
  // forward: the one x halo of the group; transposed: the m dY halos
  wgd_stage_halo(a, io, xg + ((size_t)b * a.Cin + (TR ? g * a.m : g)) * Svol, xl, TR ? a.m : 1, HV, Svol, o0z, o0y, o0x, tid);

  // the halo offset of the first position of each of this thread's runs (a run past the tile: the first run's)
  int xo[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    int pz, py, px;
    const int q = tid + i * kCdwThreads;
    cdw_run(a, q < a.runs ? q : 0, pz, py, px);
    xo[i] = pz * a.stride[0] * HyHx + py * a.stride[1] * hxp + px * a.stride[2];
  }
  // rounds of runs in which this wave has a live one
  const int nrw = max(0, min(NR, (a.runs - w * 64 + kCdwThreads - 1) / kCdwThreads));
  __syncthreads();

  float acc[NR][M][kDwR];
#pragma unroll
  for (int i = 0; i < NR; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
      for (int r = 0; r < kDwR; ++r) acc[i][j][r] = 0.f;
  if constexpr (TR) {
#pragma unroll 1
    for (int j = 0; j < a.m; ++j) {
      float acc1[NR][M][kDwR];
#pragma unroll
      for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int r = 0; r < kDwR; ++r) acc1[i][0][r] = 0.f;
      cdw_accumulate<KXB, 1, NR>(acc1, a, xl + j * HV, wl + j * a.wp, xo, nrw, HyHx, hxp);
#pragma unroll
      for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int r = 0; r < kDwR; ++r) acc[i][0][r] += acc1[i][0][r];
    }
  } else {
    cdw_accumulate<KXB, M, NR>(acc, a, xl, wl, xo, nrw, HyHx, hxp);
  }

  const int nco = TR ? 1 : a.m, co0 = TR ? g : g * a.m;
  float bv[M];
#pragma unroll
  for (int j = 0; j < M; ++j) bv[j] = (bg && j < nco) ? io.in(bg[co0 + min(j, nco - 1)]) : 0.f;
  T* ydst = yg + ((size_t)b * a.Cout + co0) * Ovol;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int q = tid + i * kCdwThreads;
    if (q >= a.runs) continue;
    int pz, py, px;
    cdw_run(a, q, pz, py, px);
    const int oz = o0z + pz, oy = o0y + py, ox = o0x + px;
    if (oz >= a.O[0] || oy >= a.O[1]) continue;
    const size_t off = ((size_t)oz * a.O[1] + oy) * a.O[2] + ox;
    const int nlive = min(kDwR, min(a.tile[2] - px, a.O[2] - ox));      // the run's live positions come first
#pragma unroll
    for (int j = 0; j < M; ++j) {
      if (j >= nco) break;
      T* dst = ydst + j * Ovol + off;
      if (a.vec && nlive == kDwR) {
        typedef T out_v4 __attribute__((ext_vector_type(4)));
        out_v4 v;
#pragma unroll
        for (int r = 0; r < kDwR; ++r) v[r] = io.out(acc[i][j][r] + bv[j]);
        *reinterpret_cast<out_v4*>(dst) = v;
      } else {
#pragma unroll
        for (int r = 0; r < kDwR; ++r)
          if (r < nlive) dst[r] = io.out(acc[i][j][r] + bv[j]);
      }
    }
  }
}

// (conv_direct_dw.hip) kxb: taps per block, 1 (the general build), 4 or 8; m: channel multiplier
int conv_direct_dw_slots(int m, int transposed);      // the M of the build that serves the layer (NR = 8 / M), 0 if none
hipError_t conv_direct_dw_launch(const ConvDirectDwArgs& a, int kxb, int transposed, long long grid, size_t lds, hipStream_t st);

}  // namespace fc
