// conv_direct_tr_h16.hpp -- the strided transposed convolution by output phases of conv_direct_tr.hpp for float16 /
// bfloat16 tensors on the 16-bit matrix instructions of gfx950, v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x32_f16
// (DESIGN 4.5i): the phase decomposition of 4.5h on the cell layout of 4.5f.
//   y[b][(g,o)][t] = bias[(g,o)] + sum_i sum_k W[(g,i)][o][k] * x[b][(g,i)][(t + p - k*d) / s]
// The contract is conv_direct_tr_kernel's: one launch, no workspace, no atomics; a workgroup (4 waves) owns one unit
// (batch item, tile of <= 1024 base positions q), one group and a block of <= 16 output channels; the reduction is not
// split, every output sample is written exactly once from registers, bias added, rounded once; a phase without a live
// tap writes the bias; the bits of y are a function of the geometry alone.  Nothing is widened: a product of two
// bfloat16 or two float16 is exact in the float32 accumulator (conv_direct_h16.hpp).
//
// Data movement.  The workgroup loops over blocks of `cib` input channels of the group, whole cells of 8 channels.  Per
// block:
//   xl[cell][halo]      x[q0 - M .. q0 + tile - 1] per axis as 16-byte cells of 8 consecutive channels in the tensors' own
//                       16-bit format, zero cells outside [0, S), zero channels past the group: staged once per block (of
//                       a layer of one block: by the first pass only), read by every phase.  A thread owns a halo
//                       position: it resolves it once, loads the 8 channels of every cell and writes one 16-byte store;
//   wl[step][68 cells]  the weights of the pass in MFMA-step order, cell i * 4 + q (conv_direct_h16.hpp): the A operand of
//                       a step is one conflict-free 16-byte read per lane.  The 8 channels of a cell are gathered from
//                       W[(g,ci)][co][tap], Cog * taps apart;
//   cbl[j], cwl[j]      of column j = (cell, live tap), the columns sorted by phase and each phase padded to whole steps of
//                       4 columns = 32 products, built as cdt_column_tables builds them, cells in the place of channels: the halo
//                       offset in cells (kCdDead for padding) and cell * 128 + tap, where the weight gather finds it.
// The weights of the NEXT block travel in registers (16 cells per thread: columns tid % 128 and + 128 of the pass, rows
// 8 (tid / 128) .. + 7) under the MFMAs of this one.  The B operand of (column, position) is the aligned 16-byte read
// xl[cbl[j] + po[c]]; a dead column or position is selected to a zero cell, never multiplied as 0 * x.
//
// Phases in registers, MFMA operands and the two-level summation (acc1 over one phase of one block, acc2 += acc1 per
// block) are conv_direct_tr_kernel's and conv_direct_h16_kernel's.  y goes out as 2-byte stores, a lane holding the s_x
// neighbouring outputs of a row.
#pragma once
#include "conv_direct_h16.hpp"
#include "conv_direct_tr.hpp"

namespace fc {

constexpr int kTrH16WSlots = 2;           // weight columns of a pass a thread carries to the next block, 8 rows each
constexpr int kTrH16MaxSteps = kTrH16WSlots * kH16MaxSteps;     // steps of one pass of one block: 64 (256 columns)

// cbl and cwl of every column (cell, live tap) of a whole block: cdt_column_tables with cells in the place of channels
// (a function of its own so that the device code of conv_direct_tr.o stays what it was)
__device__ __forceinline__ void cdth_column_tables(const ConvDirectTrArgs& a, int* cbl, int* cwl, int HV, int tid) {
  const int cells = a.cib / kH16Cell;
  for (int j = tid; j < a.steps * 4; j += kCdThreads) {
    int f = 0;
    while (f + 1 < a.phases && (j >> 2) >= a.soff[f + 1]) ++f;
    int r[3];
    cdt_phase(a, f, r);
    const int nz = a.nk[0][r[0]], ny = a.nk[1][r[1]], nx = a.nk[2][r[2]], n = nz * ny * nx;
    const int l = j - 4 * a.soff[f];
    int cb = kCdDead, cw = -1;
    if (n > 0 && l < cells * n) {
      const int cell = l / n;
      int t = l - cell * n;
      const int ix = t % nx; t /= nx;
      const int iy = t % ny, iz = t / ny;
      const int kz = a.k0[0][r[0]] + iz * a.kstep[0], ky = a.k0[1][r[1]] + iy * a.kstep[1], kx = a.k0[2][r[2]] + ix * a.kstep[2];
      const int mz = a.m0[0][r[0]] + iz * a.mstep[0], my = a.m0[1][r[1]] + iy * a.mstep[1], mx = a.m0[2][r[2]] + ix * a.mstep[2];
      cb = cell * HV + ((a.M[0] - mz) * a.halo[1] + (a.M[1] - my)) * a.halo[2] + (a.M[2] - mx);
      cw = cell * 128 + (kz * a.k[1] + ky) * a.k[2] + kx;
    }
    cbl[j] = cb; cwl[j] = cw;
  }
}

// The weights of rows co0 .. co0 + nco - 1 of group g, input channels ci0 .. ci0 + nci - 1 and the columns from j0 up to
// j1 into registers: thread tid carries columns j0 + tid % 128 and + 128, rows 8 (tid / 128) .. + 7, the 8 channels of
// the column's cell each; zeros where there is none.
__device__ __forceinline__ void cdth_load_weights(const ConvDirectTrArgs& a, const unsigned short* wg, const int* cwl, int g,
                                                  int co0, int nco, int ci0, int nci, int j0, int j1, int tid,
                                                  h16_cell (&wr)[kTrH16WSlots][kH16WRows]) {
  const int i0 = (tid / kH16WCols) * kH16WRows;
  const size_t chan = (size_t)a.Cog * a.taps;
#pragma unroll
  for (int q = 0; q < kTrH16WSlots; ++q) {
    const int j = j0 + (tid & (kH16WCols - 1)) + q * kH16WCols;
    const int cw = j < j1 ? cwl[j] : -1;
    const int c0 = max(cw >> 7, 0) * kH16Cell, tap = cw & 127;
    const bool live = cw >= 0 && c0 < nci;
    const size_t base = ((size_t)(g * a.Cig + ci0 + c0) * a.Cog + co0) * a.taps + tap;
#pragma unroll
    for (int r = 0; r < kH16WRows; ++r) wr[q][r] = h16_cell{0u, 0u, 0u, 0u};
    if (j0 + q * kH16WCols >= j1) continue;      // (the whole second slot of most layers: no load is issued)
#pragma unroll
    for (int r = 0; r < kH16WRows; ++r) {
      unsigned h[kH16Cell];
#pragma unroll
      for (int c = 0; c < kH16Cell; ++c)
        h[c] = (live && i0 + r < nco && c0 + c < nci) ? wg[base + (size_t)(i0 + r) * a.taps + c * chan] : 0u;
      wr[q][r] = h16_pack(h);
    }
  }
}

__device__ __forceinline__ void cdth_store_weights(h16_cell* wl, int ncols, int tid, const h16_cell (&wr)[kTrH16WSlots][kH16WRows]) {
  const int i0 = (tid / kH16WCols) * kH16WRows;
#pragma unroll
  for (int q = 0; q < kTrH16WSlots; ++q) {
    const int j = (tid & (kH16WCols - 1)) + q * kH16WCols;
    if (j >= ncols) continue;
#pragma unroll
    for (int r = 0; r < kH16WRows; ++r) wl[(j >> 2) * kH16WPitch + (i0 + r) * 4 + (j & 3)] = wr[q][r];
  }
}

// x[q0 - M + h] per axis of nci input channels (xsrc: the first, Svol samples apart) into xl[cell][HV]: zero cells
// outside x, zero channels past nci.  Each global sample is read once.
__device__ __forceinline__ void cdth_stage_halo(const ConvDirectTrArgs& a, const unsigned short* xsrc, h16_cell* xl, int nci, int HV,
                                                size_t Svol, const int (&x0)[3], int tid) {
  const int ncell = (nci + kH16Cell - 1) / kH16Cell;
  for (int e = tid; e < HV; e += kCdThreads) {
    unsigned q, hz;
    const int hx = (int)fdivmod((unsigned)e, a.fd_hx, &q);
    const int hy = (int)fdivmod(q, a.fd_hy, &hz);
    const int sz = x0[0] + (int)hz, sy = x0[1] + hy, sx = x0[2] + hx;
    const bool live = (unsigned)sz < (unsigned)a.S[0] && (unsigned)sy < (unsigned)a.S[1] && (unsigned)sx < (unsigned)a.S[2];
    const size_t off = live ? ((size_t)sz * a.S[1] + sy) * a.S[2] + sx : 0;
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

template <bool BF, int PH, int NPT>
__global__ __launch_bounds__(kCdThreads) void conv_direct_tr_h16_kernel(const ConvDirectTrArgs a) {
  static_assert(PH * NPT <= 16, "accumulators of a pass: 2 x 64 registers");
  using T = unsigned short;
  extern __shared__ __attribute__((aligned(16))) h16_cell cdth_lds[];
  h16_cell* wl = cdth_lds;
  int* cbl = reinterpret_cast<int*>(wl + a.steps * kH16WPitch);
  int* cwl = cbl + a.steps * 4;
  h16_cell* xl = reinterpret_cast<h16_cell*>(cwl + a.steps * 4);
  const Io<IO_H16> io(BF ? IO_CODE_BF16 : IO_CODE_F16);
  const T* xg = static_cast<const T*>(a.x);
  const T* wg = static_cast<const T*>(a.w);
  const T* bg = static_cast<const T*>(a.bias);
  T* yg = static_cast<T*>(a.y);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;

  // workgroup -> (unit, group, block of output channels), as conv_direct_tr_kernel
  unsigned bid = blockIdx.x;
  const int ob = bid % a.nob; bid /= a.nob;
  const int g = bid % a.G, u = bid / a.G;
  const int co0 = ob * kCdRows, nco = min(kCdRows, a.Cog - co0);
  const int tiles = a.ntile[0] * a.ntile[1] * a.ntile[2];
  const int b = u / tiles;
  int t = u - b * tiles;
  int o0[3];            // the tile's first base position, counted from qlo
  o0[2] = (t % a.ntile[2]) * a.tile[2]; t /= a.ntile[2];
  o0[1] = (t % a.ntile[1]) * a.tile[1]; o0[0] = (t / a.ntile[1]) * a.tile[0];
  const int x0[3] = {a.qlo[0] + o0[0] - a.M[0], a.qlo[1] + o0[1] - a.M[1], a.qlo[2] + o0[2] - a.M[2]};
  const int HyHx = a.halo[1] * a.halo[2], HV = a.halo[0] * HyHx;
  const size_t Ovol = (size_t)a.O[0] * a.O[1] * a.O[2], Svol = (size_t)a.S[0] * a.S[1] * a.S[2];

  cdth_column_tables(a, cbl, cwl, HV, tid);

  // wave w owns the position tiles w, w + 4, ...: the halo offset of this lane's base position in each
  int po[NPT];
#pragma unroll
  for (int c = 0; c < NPT; ++c) {
    int pq[3];
    const bool live = cdt_position(a, ((c * kCdWaves + w) * 16) + i16, o0, pq);
    po[c] = live ? pq[0] * HyHx + pq[1] * a.halo[2] + pq[2] : kCdDead;
  }
  float bv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bv[r] = (bg && 4 * kq + r < nco) ? io.in(bg[g * a.Cog + co0 + 4 * kq + r]) : 0.f;
  T* ydst = yg + ((size_t)b * a.Cout + g * a.Cog + co0) * Ovol;
  __syncthreads();      // cwl is read by the first weight load

  for (int pass = 0; pass < a.npass; ++pass) {
    const int f0 = pass * a.ppp, nph = min(a.ppp, a.phases - f0);
    const int s0 = a.soff[f0], s1 = a.soff[f0 + nph];      // the steps of this pass
    wgd_v4f acc2[PH][NPT];
#pragma unroll
    for (int h = 0; h < PH; ++h)
#pragma unroll
      for (int c = 0; c < NPT; ++c) acc2[h][c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};

    h16_cell wr[kTrH16WSlots][kH16WRows];
    cdth_load_weights(a, wg, cwl, g, co0, nco, 0, min(a.cib, a.Cig), 4 * s0, 4 * s1, tid, wr);
    for (int ib = 0; ib < a.nib; ++ib) {
      const int ci0 = ib * a.cib, nci = min(a.cib, a.Cig - ci0);
      const int live_end = (nci + kH16Cell - 1) / kH16Cell * HV;      // a column of a cell past the block: dead
      __syncthreads();      // the MFMA loop of the block before has read its last cell
      cdth_store_weights(wl, 4 * (s1 - s0), tid, wr);
      if (a.nib > 1 || pass == 0)
        cdth_stage_halo(a, xg + ((size_t)b * a.Cin + g * a.Cig + ci0) * Svol, xl, nci, HV, Svol, x0, tid);
      __syncthreads();
      // the next block's weights travel under the multiplies of this one
      if (ib + 1 < a.nib)
        cdth_load_weights(a, wg, cwl, g, co0, nco, ci0 + a.cib, min(a.cib, a.Cig - ci0 - a.cib), 4 * s0, 4 * s1, tid, wr);

#pragma unroll
      for (int h = 0; h < PH; ++h) {
        if (h >= nph) continue;
        wgd_v4f acc1[NPT];
#pragma unroll
        for (int c = 0; c < NPT; ++c) acc1[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};
        const int e0 = a.soff[f0 + h], e1 = a.soff[f0 + h + 1];
        for (int s = e0; s < e1; ++s) {
          const h16_cell av = wl[(s - s0) * kH16WPitch + i16 * 4 + kq];
          const int cj = cbl[4 * s + kq];
          const int cb = cj < live_end ? cj : kCdDead;
#pragma unroll
          for (int c = 0; c < NPT; ++c) {
            const int e = cb + po[c];      // (dead + dead = -2^31: still negative)
            const h16_cell v = xl[max(e, 0)];
            acc1[c] = h16_mfma<BF>(av, e < 0 ? h16_cell{0u, 0u, 0u, 0u} : v, acc1[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < NPT; ++c) acc2[h][c] += acc1[c];
      }
    }

    // slot h is phase f0 + h: output t = s * q + r - p per axis, where that lies in [0, O)
#pragma unroll
    for (int c = 0; c < NPT; ++c) {
      int pq[3];
      const bool there = cdt_position(a, ((c * kCdWaves + w) * 16) + i16, o0, pq);
#pragma unroll
      for (int h = 0; h < PH; ++h) {
        if (h >= nph) continue;
        int r[3];
        cdt_phase(a, f0 + h, r);
        const int tz = (a.qlo[0] + o0[0] + pq[0]) * a.up[0] + r[0] - a.pad[0];
        const int ty = (a.qlo[1] + o0[1] + pq[1]) * a.up[1] + r[1] - a.pad[1];
        const int tx = (a.qlo[2] + o0[2] + pq[2]) * a.up[2] + r[2] - a.pad[2];
        if (!there || (unsigned)tz >= (unsigned)a.O[0] || (unsigned)ty >= (unsigned)a.O[1] || (unsigned)tx >= (unsigned)a.O[2])
          continue;
        const size_t off = ((size_t)tz * a.O[1] + ty) * a.O[2] + tx;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          if (4 * kq + rr < nco) ydst[(4 * kq + rr) * Ovol + off] = io.out(acc2[h][c][rr] + bv[rr]);
      }
    }
  }
}

// (conv_direct_tr_h16.hip) ph, npt as conv_direct_tr_launch; the build by a.io (float16 or bfloat16)
hipError_t conv_direct_tr_h16_launch(const ConvDirectTrArgs& a, int ph, int npt, long long grid, size_t lds, hipStream_t st);

}  // namespace fc
