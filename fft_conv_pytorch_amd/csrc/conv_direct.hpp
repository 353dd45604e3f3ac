// conv_direct.hpp -- time-domain forward of a 2-D / 3-D convolution with a small kernel:
//   y[b][(g,o)][t] = bias[(g,o)] + sum_i sum_k W[(g,o)][i][k] * Xpad[b][(g,i)][t*stride + k*dilation - pad]
// as a GEMM y = W . im2col(x) of (Cout/g) x (Cin/g * taps) with B * prod(out) columns on v_mfma_f32_16x16x4_f32.  With
// `transposed` the same sum runs a stride-1 transposed convolution, which is the dX of a stride-1 layer: the weight
// (Cin, Cout/g, *k) is read where it lies with the channel roles exchanged and the taps flipped, the planner passes the
// padding d*(k-1) - p.
//
// Work split.  A workgroup (4 waves) owns one unit (batch item, spatial output tile of <= 1024 positions), one group and
// a block of <= 16 output channels (the MFMA rows).  The reduction is not split: every output sample is written exactly
// once, by one workgroup, bias added, rounded once (Io<>).  Nothing else is written, no workspace, no atomics: the bits
// of y are a function of the geometry alone.
//
// Data movement.  The workgroup loops over blocks of `cib` input channels of the group, cib * taps <= 512.  Per block:
//   xl[ci][halo]   the x samples the tile reaches through every tap, (tile-1)*stride + (k-1)*dilation + 1 per axis, read
//                  through axis_src in the layer's padding mode by wgd_stage_halo (wgrad_direct.hpp): each global sample
//                  once per workgroup and block;
//   wl[step][68]   the weight block, the 16 x 4 floats of one MFMA step together at i * 4 + k.  The pitch of 68 floats
//                  spreads the staging stores of one row (consecutive columns) over all banks; the A operand of a step
//                  is one conflict-free read.  Rows past the block and columns past it are zeros;
//   cbl[j]         the halo offset of column j = (ci, tap): ci * halo + the tap's dilated offset.
// The weights of the NEXT block are loaded into registers (2 columns x 16 rows per thread, coalesced along the row of
// the weight tensor) before the MFMAs of this block start and stored to LDS after them, so that their latency is under
// the multiplies.  There is no im2col buffer: the B operand of (column j, position p) is xl[cbl[j] + posoff[p]], posoff in
// a register per position tile.  A dead column or position reads as zero by a select, never as 0 * x.
//
// MFMA operands (dense1d.hpp): A[i][k] in lane 16 k + i, B[k][j] in lane 16 k + j, D[4 (lane / 16) + r][lane % 16] in
// register r.  Here i = output channel, k = one of 4 consecutive columns (ci, tap), j = one of 16 output positions.  The
// position tiles of the unit are dealt to the waves in turn, NPT (1 .. 16) per wave; a step reads A and the column offset
// once for all of them.  The MFMAs are unconditional.
//
// Summation.  Two levels: acc1 is the chain of one input-channel block (<= 128 steps of 4 products), acc2 += acc1 after
// every block.
//
// Addressing.  x, weight, bias and y are plain pointers indexed with size_t; LDS indices and positions are int (the
// planner bounds the extents).
#pragma once
#include "wgrad_direct.hpp"

namespace fc {

constexpr int kCdThreads = kWgdThreads, kCdWaves = 4;
constexpr int kCdRows = 16;               // output channels per workgroup: the rows of one MFMA
constexpr int kCdMaxCols = 512;           // columns (input channel, tap) of one block: a first-level chain of 128 steps
constexpr int kCdMaxPos = 1024;           // positions per unit
constexpr int kCdMaxPT = 16;              // position tiles per wave: 4 * 16 * 16 = 1024 positions per workgroup
constexpr int kCdWPitch = 68;             // floats per MFMA step of the staged weight block
constexpr int kCdWCols = kCdMaxCols / kCdThreads;      // weight columns a thread carries to the next block
constexpr int kCdDead = -(1 << 30);       // posoff / column offset of a position / column that does not exist

struct ConvDirectArgs {
  const void* x;        // (B, Cin, *S)
  const void* w;        // (Cout, Cin/g, *k); transposed: (Cin, Cout/g, *k)
  const void* bias;     // (Cout) or null
  void* y;              // (B, Cout, *O)
  AxisMap map[3];       // per axis (z, y, x; a 2-D layer has a z axis of one sample)
  int S[3], O[3];
  int k[3], stride[3], dil[3];
  int tile[3], ntile[3], halo[3];
  FastDiv fd_tx, fd_ty, fd_hx, fd_hy;
  int Cin, Cout, Cig, Cog, G, taps;
  int cib, nib, nob;    // input channels per block, blocks of them, blocks of 16 output channels
  int P;                // positions of a tile
  int steps;            // MFMA steps of a whole block: ceil(cib * taps / 4)
  int io;               // fc_dtype code of x, weight, bias and y
  int transposed;
};

// position p of the tile at (o0z, o0y, o0x) -> its coordinates in the tile; whether it exists
__device__ __forceinline__ bool cd_position(const ConvDirectArgs& a, int p, int o0z, int o0y, int o0x, int& pz, int& py, int& px) {
  unsigned q, z;
  px = (int)fdivmod((unsigned)p, a.fd_tx, &q);
  py = (int)fdivmod(q, a.fd_ty, &z);
  pz = (int)z;
  return p < a.P && o0z + pz < a.O[0] && o0y + py < a.O[1] && o0x + px < a.O[2];
}

// The weights of rows co0 .. co0 + nco - 1 of group g and input channels ci0 .. ci0 + nci - 1 into registers: thread tid
// carries columns tid and tid + 256 of the block, 16 rows each; zeros past the block.
template <class IoT, class T>
__device__ __forceinline__ void cd_load_weights(const ConvDirectArgs& a, const IoT& io, const T* wg, int g, int co0, int nco,
                                                int ci0, int nci, int tid, float (&wr)[kCdWCols][kCdRows]) {
  const int ncols = nci * a.taps;
#pragma unroll
  for (int q = 0; q < kCdWCols; ++q) {
    const int j = tid + q * kCdThreads;
    const bool live = j < ncols;
    const int ci = j / a.taps, tap = j - ci * a.taps;
    // forward: W[(g, co)][ci][tap]; transposed: W[(g, ci)][co][taps - 1 - tap] (the flip of every axis at once)
    const size_t base = a.transposed ? ((size_t)(g * a.Cig + ci0 + ci) * a.Cog + co0) * a.taps + (a.taps - 1 - tap)
                                     : ((size_t)(g * a.Cog + co0) * a.Cig + ci0 + ci) * a.taps + tap;
    const size_t row = a.transposed ? (size_t)a.taps : (size_t)a.Cig * a.taps;
#pragma unroll
    for (int i = 0; i < kCdRows; ++i) wr[q][i] = (live && i < nco) ? io.in(wg[base + i * row]) : 0.f;
  }
}

__device__ __forceinline__ void cd_store_weights(const ConvDirectArgs& a, float* wl, int tid, const float (&wr)[kCdWCols][kCdRows]) {
#pragma unroll
  for (int q = 0; q < kCdWCols; ++q) {
    const int j = tid + q * kCdThreads;
    if (j >= a.steps * 4) continue;
#pragma unroll
    for (int i = 0; i < kCdRows; ++i) wl[(j >> 2) * kCdWPitch + i * 4 + (j & 3)] = wr[q][i];
  }
}

template <int IO, int NPT>
__global__ __launch_bounds__(kCdThreads) void conv_direct_kernel(const ConvDirectArgs a) {
  using T = typename Io<IO>::T;
  extern __shared__ __attribute__((aligned(16))) float cd_lds[];
  float* wl = cd_lds;
  int* cbl = reinterpret_cast<int*>(wl + a.steps * kCdWPitch);
  float* xl = reinterpret_cast<float*>(cbl + a.steps * 4);
  const Io<IO> io(a.io);
  const T* xg = static_cast<const T*>(a.x);
  const T* wg = static_cast<const T*>(a.w);
  const T* bg = static_cast<const T*>(a.bias);
  T* yg = static_cast<T*>(a.y);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;

  // workgroup -> (unit, group, block of output channels): the blocks of one unit run next to each other and share its
  // halo in L2
  unsigned bid = blockIdx.x;
  const int ob = bid % a.nob; bid /= a.nob;
  const int g = bid % a.G, u = bid / a.G;
  const int co0 = ob * kCdRows, nco = min(kCdRows, a.Cog - co0);
  const int tiles = a.ntile[0] * a.ntile[1] * a.ntile[2];
  const int b = u / tiles;
  int t = u - b * tiles;
  const int o0x = (t % a.ntile[2]) * a.tile[2]; t /= a.ntile[2];
  const int o0y = (t % a.ntile[1]) * a.tile[1], o0z = (t / a.ntile[1]) * a.tile[0];
  const int HyHx = a.halo[1] * a.halo[2], HV = a.halo[0] * HyHx;
  const size_t Ovol = (size_t)a.O[0] * a.O[1] * a.O[2], Svol = (size_t)a.S[0] * a.S[1] * a.S[2];

  for (int j = tid; j < a.steps * 4; j += kCdThreads) {
    const int ci = j / a.taps, tap = j - ci * a.taps;
    const int kx = tap % a.k[2], kyz = tap / a.k[2], ky = kyz % a.k[1], kz = kyz / a.k[1];
    cbl[j] = ci < a.cib ? ci * HV + kz * a.dil[0] * HyHx + ky * a.dil[1] * a.halo[2] + kx * a.dil[2] : kCdDead;
  }

  // wave w owns the position tiles w, w + 4, ...: the halo offset of this lane's position in each
  int po[NPT];
#pragma unroll
  for (int c = 0; c < NPT; ++c) {
    int pz, py, px;
    const bool live = cd_position(a, ((c * kCdWaves + w) * 16) + i16, o0z, o0y, o0x, pz, py, px);
    po[c] = live ? pz * a.stride[0] * HyHx + py * a.stride[1] * a.halo[2] + px * a.stride[2] : kCdDead;
  }

  wgd_v4f acc2[NPT];
#pragma unroll
  for (int c = 0; c < NPT; ++c) acc2[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};

  float wr[kCdWCols][kCdRows];
  cd_load_weights(a, io, wg, g, co0, nco, 0, min(a.cib, a.Cig), tid, wr);
  for (int ib = 0; ib < a.nib; ++ib) {
    const int ci0 = ib * a.cib, nci = min(a.cib, a.Cig - ci0);
    const int ncols = nci * a.taps;
    __syncthreads();      // the MFMA loop of the block before has read its last sample
    cd_store_weights(a, wl, tid, wr);
    wgd_stage_halo(a, io, xg + ((size_t)b * a.Cin + g * a.Cig + ci0) * Svol, xl, nci, HV, Svol, o0z, o0y, o0x, tid);
    __syncthreads();
    // the next block's weights travel under the multiplies of this one
    if (ib + 1 < a.nib) cd_load_weights(a, io, wg, g, co0, nco, ci0 + a.cib, min(a.cib, a.Cig - ci0 - a.cib), tid, wr);

    wgd_v4f acc1[NPT];
#pragma unroll
    for (int c = 0; c < NPT; ++c) acc1[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (ncols + 3) >> 2;
    for (int s = 0; s < nsteps; ++s) {
      const float av = wl[s * kCdWPitch + i16 * 4 + kq];
      const int j = 4 * s + kq;
      const int cb = j < ncols ? cbl[j] : kCdDead;
#pragma unroll
      for (int c = 0; c < NPT; ++c) {
        const int e = cb + po[c];      // (dead + dead = -2^31: still negative)
        const float v = xl[max(e, 0)];
        acc1[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, e < 0 ? 0.f : v, acc1[c], 0, 0, 0);
      }
    }
#pragma unroll
    for (int c = 0; c < NPT; ++c) acc2[c] += acc1[c];
  }

  float bv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bv[r] = (bg && 4 * kq + r < nco) ? io.in(bg[g * a.Cog + co0 + 4 * kq + r]) : 0.f;
  T* ydst = yg + ((size_t)b * a.Cout + g * a.Cog + co0) * Ovol;
#pragma unroll
  for (int c = 0; c < NPT; ++c) {
    int pz, py, px;
    if (!cd_position(a, ((c * kCdWaves + w) * 16) + i16, o0z, o0y, o0x, pz, py, px)) continue;
    const size_t off = ((size_t)(o0z + pz) * a.O[1] + (o0y + py)) * a.O[2] + (o0x + px);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * kq + r < nco) ydst[(4 * kq + r) * Ovol + off] = io.out(acc2[c][r] + bv[r]);
  }
}

// (conv_direct.hip) npt: position tiles per wave, 1, 2, 4, 8 or 16; the build by a.io
hipError_t conv_direct_launch(const ConvDirectArgs& a, int npt, long long grid, size_t lds, hipStream_t st);

}  // namespace fc
