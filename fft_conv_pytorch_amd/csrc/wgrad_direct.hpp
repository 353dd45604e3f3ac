// wgrad_direct.hpp -- time-domain weight gradient of a 2-D / 3-D convolution with a small kernel:
//   dW[(g,o)][i][k] = sum_b sum_t dY[b][(g,o)][t] * Xpad[b][(g,i)][t*stride + k*dilation - pad]
// as a GEMM of (Cout/g) x (Cin/g * taps) with the reduction over B * prod(out) on v_mfma_f32_16x16x4_f32.
//
// Work split.  A workgroup (4 waves) owns one group g, a block of <= 16 output channels (the MFMA rows), a block of
// `cib` input channels of the group and one slice: a contiguous range of units (batch item, spatial output tile) --
// split-K.  It writes its (<= 16) x (cib * taps) block of partial[slice] completely; wgrad_direct_sum_kernel adds the
// slices in a fixed order.  No atomics anywhere: the bits of dW are a function of the geometry alone.
//
// Per unit the workgroup stages, widened to float32 as they are loaded (Io<>):
//   dyl[p][16]      the dY tile, position-major with a pitch of 17 floats (rows past Cout/g and positions past the tensor
//                   or past the tile are zero), so that the A operand of lane (k, i) is one conflict-free LDS read;
//   xl[ci][halo]    the x samples the tile reaches through every tap, (tile-1)*stride + (k-1)*dilation + 1 per axis, read
//                   through axis_src (axis_map.hpp) in the layer's padding mode -- a zero where that says -1;
//   posoff[p]       the halo offset of output position p, or kWgdDead for a position that does not exist.
// Every global sample is read once per workgroup and unit.  There is no im2col buffer: column j = (ci, tap) of the B
// operand at position p is xl[colbase_j + posoff[p]], colbase_j = ci * halo + the tap's dilated offset, held in a
// register per column tile.  A dead column or position reads as zero (one select), never as 0 * x.
//
// MFMA operands (dense1d.hpp): A[i][k] in lane 16 k + i, B[k][j] in lane 16 k + j, D[4 (lane / 16) + r][lane % 16] in
// register r.  Here i = output channel, k = one of 4 consecutive positions, j = column.  Wave w owns the column tiles
// w*CT .. w*CT + CT - 1; CT (1, 2, 4, 8) is the smallest that covers cib * taps <= 512 columns, so the accumulators are
// at most 2 x 32 registers.  The MFMAs are unconditional (a guarded MFMA makes hipcc copy the accumulator).
//
// Summation.  Three levels: acc1 sums one unit (<= 1024 positions, 256 MFMA steps of 4 products), acc2 += acc1 after
// every unit, and the slices are summed in blocks of 16 by the second launch.
//
// Addressing.  x, dY and partial are plain pointers indexed with size_t; LDS indices and positions are int (the planner
// bounds the extents).  Nothing here forms a 32-bit global offset.
#pragma once
#include "axis_map.hpp"
#include "fft_engine.hpp"

namespace fc {

constexpr int kWgdThreads = 256, kWgdWaves = 4;
constexpr int kWgdRows = 16;              // output channels per workgroup: the rows of one MFMA
constexpr int kWgdDyPitch = 17;           // floats per position of the staged dY tile
constexpr int kWgdMaxCT = 8;              // column tiles per wave: 4 * 8 * 16 = 512 columns per workgroup
constexpr int kWgdMaxPos = 1024;          // positions per unit: the length of a first-level chain
constexpr int kWgdDead = -(1 << 30);      // posoff / colbase of a position / column that does not exist
constexpr int kWgdSumBlock = 16;          // slices per inner sum of the second launch

struct WgradDirectArgs {
  const void* x;        // (B, Cin, *S)
  const void* dy;       // (B, Cout, *O)
  float* partial;       // (slices, Cout, Cig, taps)
  AxisMap map[3];       // per axis (z, y, x; a 2-D layer has a z axis of one sample)
  int S[3], O[3];       // input / output extent
  int k[3], stride[3], dil[3];
  int tile[3], ntile[3], halo[3];
  FastDiv fd_tx, fd_ty, fd_hx, fd_hy;
  int Cin, Cout, Cig, Cog, taps;
  int cib, nib, nob;    // input channels per block, blocks of them, blocks of 16 output channels
  int slices, units;    // units = B * ntile[0] * ntile[1] * ntile[2]
  int P, P4;            // positions of a tile, rounded up to the 4 of an MFMA step
  int io;               // fc_dtype code of x and dY
  // the depthwise body (wgrad_direct_dw.hpp); there halo[2] is the padded pitch of a halo row
  FastDiv fd_rx;        // runs of 4 output columns per tile row
  int runs, runs64;     // runs of a tile, rounded up to whole waves
  int nbx, nblk;        // tap blocks per kernel row, tap blocks in all
};

typedef float wgd_v4f __attribute__((ext_vector_type(4)));

// unit u -> its batch item and the first output position of its tile
__device__ __forceinline__ void wgd_unit_origin(const WgradDirectArgs& a, int u, int& b, int& o0z, int& o0y, int& o0x) {
  const int tiles = a.ntile[0] * a.ntile[1] * a.ntile[2];
  b = u / tiles;
  int t = u - b * tiles;
  const int tix = t % a.ntile[2]; t /= a.ntile[2];
  o0x = tix * a.tile[2]; o0y = (t % a.ntile[1]) * a.tile[1]; o0z = (t / a.ntile[1]) * a.tile[0];
}

// The x halo of nci input channels (xsrc: the first, Svol samples apart) of the tile at (o0z, o0y, o0x) into
// xl[ci][HV], through the padding mode: a zero where axis_src says -1.  Each global sample is read once.  Args: the
// argument struct of a kernel of 256 threads with map, stride, S, fd_hx and fd_hy (conv_direct.hpp stages its halo here too).
template <class Args, class IoT, class T>
__device__ __forceinline__ void wgd_stage_halo(const Args& a, const IoT& io, const T* xsrc, float* xl, int nci,
                                               int HV, size_t Svol, int o0z, int o0y, int o0x, int tid) {
  for (int e = tid; e < HV; e += kWgdThreads) {
    unsigned q, hz;
    const int hx = (int)fdivmod((unsigned)e, a.fd_hx, &q);
    const int hy = (int)fdivmod(q, a.fd_hy, &hz);
    const int sz = axis_src(a.map[0], o0z * a.stride[0] + (int)hz);
    const int sy = axis_src(a.map[1], o0y * a.stride[1] + hy);
    const int sx = axis_src(a.map[2], o0x * a.stride[2] + hx);
    const bool live = (sz | sy | sx) >= 0;
    const size_t off = ((size_t)max(sz, 0) * a.S[1] + max(sy, 0)) * a.S[2] + max(sx, 0);
    for (int ci = 0; ci < nci; ++ci) xl[ci * HV + e] = live ? io.in(xsrc[ci * Svol + off]) : 0.f;
  }
}

template <int IO, int CT>
__global__ __launch_bounds__(kWgdThreads) void wgrad_direct_kernel(const WgradDirectArgs a) {
  using T = typename Io<IO>::T;
  extern __shared__ __attribute__((aligned(16))) float wgd_lds[];
  int* posoff = reinterpret_cast<int*>(wgd_lds);
  float* dyl = wgd_lds + a.P4;
  float* xl = dyl + a.P4 * kWgdDyPitch;
  const Io<IO> io(a.io);
  const T* xg = static_cast<const T*>(a.x);
  const T* dyg = static_cast<const T*>(a.dy);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;

  // workgroup -> (group, block of output channels, slice, block of input channels): the input-channel blocks of one
  // slice run next to each other and share their dY tiles in L2
  unsigned bid = blockIdx.x;
  const int ib = bid % a.nib; bid /= a.nib;
  const int slice = bid % a.slices; bid /= a.slices;
  const int ob = bid % a.nob, g = bid / a.nob;
  const int co0 = g * a.Cog + ob * kWgdRows, nco = min(kWgdRows, a.Cog - ob * kWgdRows);
  const int ci0 = ib * a.cib, nci = min(a.cib, a.Cig - ci0);
  const int ncols = nci * a.taps;
  const int HyHx = a.halo[1] * a.halo[2], HV = a.halo[0] * HyHx;
  const size_t Ovol = (size_t)a.O[0] * a.O[1] * a.O[2], Svol = (size_t)a.S[0] * a.S[1] * a.S[2];

  int colbase[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int col = (w * CT + c) * 16 + i16;
    colbase[c] = kWgdDead;
    if (col < ncols) {
      const int ci = col / a.taps, tap = col - ci * a.taps;
      const int kx = tap % a.k[2], kyz = tap / a.k[2], ky = kyz % a.k[1], kz = kyz / a.k[1];
      colbase[c] = ci * HV + kz * a.dil[0] * HyHx + ky * a.dil[1] * a.halo[2] + kx * a.dil[2];
    }
  }

  wgd_v4f acc2[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc2[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};

  const int u0 = (int)((long long)slice * a.units / a.slices), u1 = (int)((long long)(slice + 1) * a.units / a.slices);
  for (int u = u0; u < u1; ++u) {
    int b, o0z, o0y, o0x;
    wgd_unit_origin(a, u, b, o0z, o0y, o0x);
    __syncthreads();      // the MFMA loop of the unit before has read its last sample

    // dY tile and the halo offsets of its positions
    const T* dsrc = dyg + ((size_t)b * a.Cout + co0) * Ovol;
    for (int p = tid; p < a.P4; p += kWgdThreads) {
      unsigned q, pz;
      const int px = (int)fdivmod((unsigned)p, a.fd_tx, &q);
      const int py = (int)fdivmod(q, a.fd_ty, &pz);
      const bool live = p < a.P && o0z + (int)pz < a.O[0] && o0y + py < a.O[1] && o0x + px < a.O[2];
      posoff[p] = live ? (int)pz * a.stride[0] * HyHx + py * a.stride[1] * a.halo[2] + px * a.stride[2] : kWgdDead;
      const size_t off = ((size_t)(o0z + (int)pz) * a.O[1] + (o0y + py)) * a.O[2] + (o0x + px);
#pragma unroll
      for (int i = 0; i < kWgdRows; ++i) dyl[p * kWgdDyPitch + i] = (live && i < nco) ? io.in(dsrc[i * Ovol + off]) : 0.f;
    }
    // x halo of the block's input channels, through the padding mode
    wgd_stage_halo(a, io, xg + ((size_t)b * a.Cin + g * a.Cig + ci0) * Svol, xl, nci, HV, Svol, o0z, o0y, o0x, tid);
    __syncthreads();

    wgd_v4f acc1[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc1[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};
    for (int p = kq; p < a.P4; p += 4) {
      const int po = posoff[p];
      const float av = dyl[p * kWgdDyPitch + i16];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int s = colbase[c] + po;      // (dead + dead = -2^31: still negative)
        const float v = xl[max(s, 0)];
        acc1[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s < 0 ? 0.f : v, acc1[c], 0, 0, 0);
      }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) acc2[c] += acc1[c];
  }

  float* out = a.partial + (size_t)slice * a.Cout * a.Cig * a.taps;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int col = (w * CT + c) * 16 + i16;
    if (col >= ncols) continue;
    const int ci = col / a.taps, tap = col - ci * a.taps;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * kq + r;
      if (row < nco) out[((size_t)(co0 + row) * a.Cig + ci0 + ci) * a.taps + tap] = acc2[c][r];
    }
  }
}

// dw[e] = the slices of partial[.][e], blocks of BLOCK slices summed first, block after block: a fixed order
template <int BLOCK>
__global__ __launch_bounds__(kWgdThreads) void wgrad_direct_sum_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                                                       long long n, int slices) {
  const long long e = (long long)blockIdx.x * kWgdThreads + threadIdx.x;
  if (e >= n) return;
  float total = 0.f;
  for (int s0 = 0; s0 < slices; s0 += BLOCK) {
    float part = 0.f;
    const int s1 = min(slices, s0 + BLOCK);
    for (int s = s0; s < s1; ++s) part += partial[(size_t)s * n + e];
    total += part;
  }
  dw[e] = total;
}

// (wgrad_direct.hip) ct: column tiles per wave, 1, 2, 4 or 8; the build by a.io
hipError_t wgrad_direct_launch(const WgradDirectArgs& a, int ct, long long grid, size_t lds, hipStream_t st);
hipError_t wgrad_direct_sum_launch(const float* partial, float* dw, long long n, int slices, hipStream_t st);

}  // namespace fc
