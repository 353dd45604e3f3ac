// conv_direct_h16.hpp -- the direct small-kernel forward of conv_direct.hpp for float16 / bfloat16 tensors on the 16-bit
// matrix instructions of gfx950, v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x32_f16:
//   y[b][(g,o)][t] = bias[(g,o)] + sum_i sum_k W[(g,o)][i][k] * Xpad[b][(g,i)][t*stride + k*dilation - pad]
// The contract is conv_direct_kernel's: one launch, no workspace, no atomics; a workgroup (4 waves) owns one unit (batch
// item, spatial output tile of <= 1024 positions), one group and a block of <= 16 output channels; the reduction is not
// split, every output sample is written exactly once, bias added, rounded once; `transposed` reads the weight
// (Cin, Cout/g, *k) where it lies with the channel roles exchanged and the taps flipped.  Nothing is widened: a product of
// two bfloat16 (16 significant bits) or two float16 (22) is exact in the float32 accumulator, so the sum is that of
// "widen, multiply in float32" in another order.
//
// Data movement.  The workgroup loops over blocks of `cib` input channels of the group, whole cells of 8 channels,
// cib * taps <= 1024.  Per block:
//   xl[cell][halo]      the x halo as 16-byte cells of 8 consecutive channels in the tensors' own 16-bit format.  A thread
//                       owns a halo position: it resolves the padding mode (axis_src) once, loads the 8 channels of every
//                       cell (each load coalesced across the lanes along x) and writes the cell with one 16-byte store.
//                       Channels past the group and positions in zero padding are zero cells;
//   wl[step][68 cells]  the weight block, the 16 rows x 4 columns x 8 channels of one MFMA step together, cell i * 4 + q.
//                       The pitch of 68 cells puts the 4 steps that 16 consecutive staging lanes touch on disjoint
//                       banks; the A operand of a step is one contiguous KiB: a conflict-free 16-byte read per lane;
//   cbl[j]              the halo offset (in cells) of column j = (cell, tap): cell * halo + the tap's dilated offset.
// A column is a pair (channel cell, tap), cell-major, so that the table of a whole block serves a ragged last block and
// the weight gather runs along the taps as they lie in memory.  The B operand of (column, position) is the aligned
// 16-byte read xl[cbl[j] + posoff[p]]: stride and dilation only change offsets, one build covers them all.  A dead column
// or position reads as a zero cell by a select, never as 0 * x.  The weights of the NEXT block travel in registers (8
// cells per thread: column tid % 128, rows 8 (tid / 128) .. + 7) under the MFMAs of this one.
//
// MFMA operands: A[i][8 q .. 8 q + 7] in lane 16 q + i, B[8 q .. 8 q + 7][j] in lane 16 q + j, D[4 (lane / 16) + r][lane % 16]
// in register r.  Here i = output channel, q = one of 4 consecutive columns whose 8 channels are the lane's k, j = one of
// 16 output positions.  Output channels stay on the rows: the A read of a step then serves all NPT position tiles of the
// wave and posoff stays one register per tile; y goes out as 2-byte stores coalesced along the positions, as
// conv_direct_kernel's.
//
// Summation.  Two levels: acc1 is the chain of one input-channel block (<= 32 steps of 32 products), acc2 += acc1 after
// every block.
#pragma once
#include "conv_direct.hpp"

namespace fc {

constexpr int kH16Cell = 8;               // channels per LDS cell: the k of one lane of an MFMA step
constexpr int kH16MaxCols = 1024;         // (input channel, tap) pairs of one block, zero channels of a ragged cell included
constexpr int kH16MaxSteps = kH16MaxCols / (4 * kH16Cell);      // the first-level chain: 32 steps of 32 products
constexpr int kH16WPitch = 68;            // cells per MFMA step of the staged weight block (64 live)
constexpr int kH16WCols = 4 * kH16MaxSteps;                     // columns (cell, tap) of a block: 128
constexpr int kH16WRows = kCdRows * kH16WCols / kCdThreads;     // weight cells a thread carries to the next block: 8

typedef unsigned h16_cell __attribute__((ext_vector_type(4)));  // 8 x 16 bits
typedef __bf16 h16_v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 h16_v8h __attribute__((ext_vector_type(8)));

template <bool BF>
__device__ __forceinline__ wgd_v4f h16_mfma(h16_cell av, h16_cell bv, wgd_v4f acc) {
  if constexpr (BF)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(h16_v8bf, av), __builtin_bit_cast(h16_v8bf, bv), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16_v8h, av), __builtin_bit_cast(h16_v8h, bv), acc, 0, 0, 0);
}

__device__ __forceinline__ h16_cell h16_pack(const unsigned (&h)[kH16Cell]) {
  return h16_cell{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
}

// The x halo of nci input channels (xsrc: the first, Svol samples apart) of the tile at (o0z, o0y, o0x) into
// xl[cell][HV], through the padding mode: the padding mode is resolved once per position, a zero cell where axis_src
// says -1, zero channels past nci.  Each global sample is read once.
__device__ __forceinline__ void h16_stage_halo(const ConvDirectArgs& a, const unsigned short* xsrc, h16_cell* xl, int nci,
                                               int HV, size_t Svol, int o0z, int o0y, int o0x, int tid) {
  const int ncell = (nci + kH16Cell - 1) / kH16Cell;
  for (int e = tid; e < HV; e += kCdThreads) {
    unsigned q, hz;
    const int hx = (int)fdivmod((unsigned)e, a.fd_hx, &q);
    const int hy = (int)fdivmod(q, a.fd_hy, &hz);
    const int sz = axis_src(a.map[0], o0z * a.stride[0] + (int)hz);
    const int sy = axis_src(a.map[1], o0y * a.stride[1] + hy);
    const int sx = axis_src(a.map[2], o0x * a.stride[2] + hx);
    const bool live = (sz | sy | sx) >= 0;
    const size_t off = ((size_t)max(sz, 0) * a.S[1] + max(sy, 0)) * a.S[2] + max(sx, 0);
    for (int cell = 0; cell < ncell; ++cell) {
      unsigned h[kH16Cell];
#pragma unroll
      for (int c = 0; c < kH16Cell; ++c) {
        const int ci = cell * kH16Cell + c;
        h[c] = (live && ci < nci) ? xsrc[ci * Svol + off] : 0u;
      }
      xl[cell * HV + e] = h16_pack(h);
    }
  }
}

// The weights of rows co0 .. co0 + nco - 1 of group g and input channels ci0 .. ci0 + nci - 1 into registers: thread tid
// carries column tid % 128 = (cell, tap) of the block, rows 8 (tid / 128) .. + 7, the 8 channels of the cell each; zeros
// past the block.
__device__ __forceinline__ void h16_load_weights(const ConvDirectArgs& a, const unsigned short* wg, int g, int co0, int nco,
                                                 int ci0, int nci, int tid, h16_cell (&wr)[kH16WRows]) {
  const int j = tid & (kH16WCols - 1), i0 = (tid / kH16WCols) * kH16WRows;
  const int cell = j / a.taps, tap = j - cell * a.taps;
  const bool livej = cell * kH16Cell < nci;
  // forward: W[(g, co)][ci][tap]; transposed: W[(g, ci)][co][taps - 1 - tap] (the flip of every axis at once)
  const size_t base = a.transposed ? ((size_t)(g * a.Cig + ci0 + cell * kH16Cell) * a.Cog + co0) * a.taps + (a.taps - 1 - tap)
                                   : ((size_t)(g * a.Cog + co0) * a.Cig + ci0 + cell * kH16Cell) * a.taps + tap;
  const size_t row = a.transposed ? (size_t)a.taps : (size_t)a.Cig * a.taps;
  const size_t chan = a.transposed ? (size_t)a.Cog * a.taps : (size_t)a.taps;
#pragma unroll
  for (int r = 0; r < kH16WRows; ++r) {
    unsigned h[kH16Cell];
#pragma unroll
    for (int c = 0; c < kH16Cell; ++c)
      h[c] = (livej && i0 + r < nco && cell * kH16Cell + c < nci) ? wg[base + (i0 + r) * row + c * chan] : 0u;
    wr[r] = h16_pack(h);
  }
}

__device__ __forceinline__ void h16_store_weights(const ConvDirectArgs& a, h16_cell* wl, int tid, const h16_cell (&wr)[kH16WRows]) {
  const int j = tid & (kH16WCols - 1), i0 = (tid / kH16WCols) * kH16WRows;
  if (j >= a.steps * 4) return;
#pragma unroll
  for (int r = 0; r < kH16WRows; ++r) wl[(j >> 2) * kH16WPitch + (i0 + r) * 4 + (j & 3)] = wr[r];
}

template <bool BF, int NPT>
__global__ __launch_bounds__(kCdThreads) void conv_direct_h16_kernel(const ConvDirectArgs a) {
  using T = unsigned short;
  extern __shared__ __attribute__((aligned(16))) h16_cell h16_lds[];
  h16_cell* wl = h16_lds;
  int* cbl = reinterpret_cast<int*>(wl + a.steps * kH16WPitch);
  h16_cell* xl = reinterpret_cast<h16_cell*>(cbl + a.steps * 4);
  const Io<IO_H16> io(BF ? IO_CODE_BF16 : IO_CODE_F16);
  const T* xg = static_cast<const T*>(a.x);
  const T* wg = static_cast<const T*>(a.w);
  const T* bg = static_cast<const T*>(a.bias);
  T* yg = static_cast<T*>(a.y);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;

  // workgroup -> (unit, group, block of output channels), as conv_direct_kernel
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
    const int cell = j / a.taps, tap = j - cell * a.taps;
    const int kx = tap % a.k[2], kyz = tap / a.k[2], ky = kyz % a.k[1], kz = kyz / a.k[1];
    cbl[j] = cell * kH16Cell < a.cib ? cell * HV + kz * a.dil[0] * HyHx + ky * a.dil[1] * a.halo[2] + kx * a.dil[2] : kCdDead;
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

  h16_cell wr[kH16WRows];
  h16_load_weights(a, wg, g, co0, nco, 0, min(a.cib, a.Cig), tid, wr);
  for (int ib = 0; ib < a.nib; ++ib) {
    const int ci0 = ib * a.cib, nci = min(a.cib, a.Cig - ci0);
    const int ncols = (nci + kH16Cell - 1) / kH16Cell * a.taps;
    __syncthreads();      // the MFMA loop of the block before has read its last cell
    h16_store_weights(a, wl, tid, wr);
    h16_stage_halo(a, xg + ((size_t)b * a.Cin + g * a.Cig + ci0) * Svol, xl, nci, HV, Svol, o0z, o0y, o0x, tid);
    __syncthreads();
    // the next block's weights travel under the multiplies of this one
    if (ib + 1 < a.nib) h16_load_weights(a, wg, g, co0, nco, ci0 + a.cib, min(a.cib, a.Cig - ci0 - a.cib), tid, wr);

    wgd_v4f acc1[NPT];
#pragma unroll
    for (int c = 0; c < NPT; ++c) acc1[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (ncols + 3) >> 2;
    for (int s = 0; s < nsteps; ++s) {
      const h16_cell av = wl[s * kH16WPitch + i16 * 4 + kq];
      const int j = 4 * s + kq;
      const int cb = j < ncols ? cbl[j] : kCdDead;
#pragma unroll
      for (int c = 0; c < NPT; ++c) {
        const int e = cb + po[c];      // (dead + dead = -2^31: still negative)
        const h16_cell v = xl[max(e, 0)];
        acc1[c] = h16_mfma<BF>(av, e < 0 ? h16_cell{0u, 0u, 0u, 0u} : v, acc1[c]);
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

// (conv_direct_h16.hip) npt: position tiles per wave, 1, 2, 4, 8 or 16; the build by a.io (float16 or bfloat16)
hipError_t conv_direct_h16_launch(const ConvDirectArgs& a, int npt, long long grid, size_t lds, hipStream_t st);

}  // namespace fc
