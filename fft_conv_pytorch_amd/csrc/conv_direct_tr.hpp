// conv_direct_tr.hpp -- time-domain strided transposed convolution of a 2-D / 3-D layer with a small kernel, by output
// phases.  Weight (Cin, Cout/g, *k), stride s, dilation d, padding p, output padding op per axis:
//   y[b][(g,o)][t] = bias[(g,o)] + sum_i sum_k W[(g,i)][o][k] * x[b][(g,i)][(t + p - k*d) / s]
// over the taps for which the division is exact and the index lies in [0, S).  This is fft_conv_transpose at stride >= 2
// and the dX of every strided layer with zero padding.
//
// Phases.  Per axis t + p = s*q + r, r in [0, s) the phase, q the base position.  Tap k is live for phase r iff
// k*d = r (mod s); it reads x[q - m], m = (k*d - r) / s in [0, M], M = (k - 1)*d / s.  The live taps of a phase are an
// arithmetic progression k0[r], k0[r] + kstep, ... (kstep = s / gcd(d, s); none where gcd(d, s) does not divide r).  One
// phase (rz, ry, rx) is a stride-1 correlation of x with the sub-kernel of its live taps: no structural zero is
// multiplied, and all prod(s) phases read the same x halo of tile + M samples per axis.
//
// Work split.  A workgroup (4 waves) owns one unit (batch item, tile of <= 1024 base positions q), one group and a block
// of <= 16 output channels (the MFMA rows).  The reduction is not split: every output sample is written exactly once, by
// one workgroup, bias added, rounded once (Io<>).  No workspace, no atomics: the bits of y are a function of the
// geometry alone.  A position whose t = s*q + r - p falls outside [0, O) is dead for that phase only.
//
// Data movement.  The workgroup loops over blocks of `cib` input channels of the group.  Per block:
//   xl[ci][halo]   x[q0 - M .. q0 + tile - 1] per axis in float32, zeros outside [0, S): staged once, read by every phase;
//   wl[step][68]   the weight block in MFMA-step order (conv_direct.hpp), its columns (ci, tap) sorted by phase, each
//                  phase padded to whole steps of 4 (soff[phase]: its first step): a phase's chain runs over its live
//                  taps only.  Columns past a phase, channels past the block and rows past it are zeros;
//   cbl[j]         the halo offset of column j: ci * halo + sum over the axes of (M - m) * pitch; kCdDead for padding;
//   cwl[j]         its (ci, tap) as ci * 128 + tap, where the staging finds its weights; -1 for padding.
// cbl and cwl depend on the geometry alone and are built once per workgroup.  The weights of the NEXT block travel in
// registers under the MFMAs of this one.  A dead column or position reads as zero by a select, never as 0 * x.
//
// Phases in registers.  A pass keeps PH phase slots x NPT position tiles of accumulators per wave (PH * NPT <= 16).  The
// slots hold whole rows of last-axis phases, ppp = (PH / s_x) * s_x phases of them live, so a lane holds the s_x
// neighbouring outputs of a row and the stores of one accumulator row of a wave cover 16 * s_x consecutive samples,
// straight from registers.  A layer with more phases runs further passes over the input-channel blocks (the halo of a
// layer of one block is staged by the first pass only).  A phase without a live tap still writes its outputs: the bias.
//
// MFMA operands as conv_direct.hpp: i = output channel, k = one of 4 consecutive columns, j = one of 16 base positions.
// Summation.  Two levels: acc1 is the chain of one phase over one input-channel block, acc2 += acc1 after every block.
// Addressing.  x, weight, bias and y are indexed with size_t; LDS indices and positions are int.
#pragma once
#include "conv_direct.hpp"

namespace fc {

constexpr int kCdtMaxStride = 8, kCdtMaxPhases = 64;

struct ConvDirectTrArgs {
  const void* x;        // (B, Cin, *S)
  const void* w;        // (Cin, Cout/g, *k)
  const void* bias;     // (Cout) or null
  void* y;              // (B, Cout, *O)
  int S[3], O[3];       // per axis (z, y, x; a 2-D layer has a z axis of one sample)
  int k[3], up[3], pad[3];
  int qlo[3], Q[3], M[3];            // first base position, base positions, deepest reach of a tap
  int tile[3], ntile[3], halo[3];    // in q space; halo = tile + M
  FastDiv fd_tx, fd_ty, fd_hx, fd_hy;
  int Cin, Cout, Cig, Cog, G, taps;
  int cib, nib, nob;    // input channels per block, blocks of them, blocks of 16 output channels
  int P;                // base positions of a tile
  int phases, ppp, npass;            // prod(up); live phases of a pass; passes
  int steps;            // MFMA steps of all phases of a whole block: soff[phases]
  int k0[3][kCdtMaxStride], nk[3][kCdtMaxStride], m0[3][kCdtMaxStride];   // per axis and phase: first live tap, live taps, m of the first
  int kstep[3], mstep[3];            // tap and m distance of neighbouring live taps
  unsigned short soff[kCdtMaxPhases + 1];
  int io;               // fc_dtype code of x, weight, bias and y
};

// phase f -> (rz, ry, rx), the last axis fastest
__device__ __forceinline__ void cdt_phase(const ConvDirectTrArgs& a, int f, int (&r)[3]) {
  r[2] = f % a.up[2]; f /= a.up[2];
  r[1] = f % a.up[1]; r[0] = f / a.up[1];
}

// position p of the tile whose first base position is o0 -> its coordinates in the tile; whether its base position exists
__device__ __forceinline__ bool cdt_position(const ConvDirectTrArgs& a, int p, const int (&o0)[3], int (&pq)[3]) {
  unsigned q, z;
  pq[2] = (int)fdivmod((unsigned)p, a.fd_tx, &q);
  pq[1] = (int)fdivmod(q, a.fd_ty, &z);
  pq[0] = (int)z;
  return p < a.P && o0[0] + pq[0] < a.Q[0] && o0[1] + pq[1] < a.Q[1] && o0[2] + pq[2] < a.Q[2];
}

// cbl and cwl of every column of a whole block
__device__ __forceinline__ void cdt_column_tables(const ConvDirectTrArgs& a, int* cbl, int* cwl, int HV, int tid) {
  for (int j = tid; j < a.steps * 4; j += kCdThreads) {
    int f = 0;
    while (f + 1 < a.phases && (j >> 2) >= a.soff[f + 1]) ++f;
    int r[3];
    cdt_phase(a, f, r);
    const int nz = a.nk[0][r[0]], ny = a.nk[1][r[1]], nx = a.nk[2][r[2]], n = nz * ny * nx;
    const int l = j - 4 * a.soff[f];
    int cb = kCdDead, cw = -1;
    if (n > 0 && l < a.cib * n) {
      const int ci = l / n;
      int t = l - ci * n;
      const int ix = t % nx; t /= nx;
      const int iy = t % ny, iz = t / ny;
      const int kz = a.k0[0][r[0]] + iz * a.kstep[0], ky = a.k0[1][r[1]] + iy * a.kstep[1], kx = a.k0[2][r[2]] + ix * a.kstep[2];
      const int mz = a.m0[0][r[0]] + iz * a.mstep[0], my = a.m0[1][r[1]] + iy * a.mstep[1], mx = a.m0[2][r[2]] + ix * a.mstep[2];
      cb = ci * HV + ((a.M[0] - mz) * a.halo[1] + (a.M[1] - my)) * a.halo[2] + (a.M[2] - mx);
      cw = ci * 128 + (kz * a.k[1] + ky) * a.k[2] + kx;
    }
    cbl[j] = cb; cwl[j] = cw;
  }
}

// The weights of rows co0 .. co0 + nco - 1 of group g, input channels ci0 .. ci0 + nci - 1 and the columns from j0 up to
// j1 into registers: thread tid carries columns j0 + tid and j0 + tid + 256, 16 rows each; zeros where there is none.
template <class IoT, class T>
__device__ __forceinline__ void cdt_load_weights(const ConvDirectTrArgs& a, const IoT& io, const T* wg, const int* cwl, int g,
                                                 int co0, int nco, int ci0, int nci, int j0, int j1, int tid,
                                                 float (&wr)[kCdWCols][kCdRows]) {
#pragma unroll
  for (int q = 0; q < kCdWCols; ++q) {
    const int j = j0 + tid + q * kCdThreads;
    const int cw = j < j1 ? cwl[j] : -1;
    const int ci = cw >> 7, tap = cw & 127;
    const bool live = cw >= 0 && ci < nci;
    const size_t base = ((size_t)(g * a.Cig + ci0 + max(ci, 0)) * a.Cog + co0) * a.taps + tap;
#pragma unroll
    for (int i = 0; i < kCdRows; ++i) wr[q][i] = (live && i < nco) ? io.in(wg[base + (size_t)i * a.taps]) : 0.f;
  }
}

__device__ __forceinline__ void cdt_store_weights(float* wl, int ncols, int tid, const float (&wr)[kCdWCols][kCdRows]) {
#pragma unroll
  for (int q = 0; q < kCdWCols; ++q) {
    const int j = tid + q * kCdThreads;
    if (j >= ncols) continue;
#pragma unroll
    for (int i = 0; i < kCdRows; ++i) wl[(j >> 2) * kCdWPitch + i * 4 + (j & 3)] = wr[q][i];
  }
}

// x[q0 - M + h] per axis of nci input channels (xsrc: the first, Svol samples apart) into xl[ci][HV]; zeros outside x
template <class IoT, class T>
__device__ __forceinline__ void cdt_stage_halo(const ConvDirectTrArgs& a, const IoT& io, const T* xsrc, float* xl, int nci, int HV,
                                               size_t Svol, const int (&x0)[3], int tid) {
  for (int e = tid; e < HV; e += kCdThreads) {
    unsigned q, hz;
    const int hx = (int)fdivmod((unsigned)e, a.fd_hx, &q);
    const int hy = (int)fdivmod(q, a.fd_hy, &hz);
    const int sz = x0[0] + (int)hz, sy = x0[1] + hy, sx = x0[2] + hx;
    const bool live = (unsigned)sz < (unsigned)a.S[0] && (unsigned)sy < (unsigned)a.S[1] && (unsigned)sx < (unsigned)a.S[2];
    const size_t off = live ? ((size_t)sz * a.S[1] + sy) * a.S[2] + sx : 0;
    for (int ci = 0; ci < nci; ++ci) xl[ci * HV + e] = live ? io.in(xsrc[ci * Svol + off]) : 0.f;
  }
}

template <int IO, int PH, int NPT>
__global__ __launch_bounds__(kCdThreads) void conv_direct_tr_kernel(const ConvDirectTrArgs a) {
  static_assert(PH * NPT <= 16, "accumulators of a pass: 2 x 64 registers");
  using T = typename Io<IO>::T;
  extern __shared__ __attribute__((aligned(16))) float cdt_lds[];
  float* wl = cdt_lds;
  int* cbl = reinterpret_cast<int*>(wl + a.steps * kCdWPitch);
  int* cwl = cbl + a.steps * 4;
  float* xl = reinterpret_cast<float*>(cwl + a.steps * 4);
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
  int o0[3];            // the tile's first base position, counted from qlo
  o0[2] = (t % a.ntile[2]) * a.tile[2]; t /= a.ntile[2];
  o0[1] = (t % a.ntile[1]) * a.tile[1]; o0[0] = (t / a.ntile[1]) * a.tile[0];
  const int x0[3] = {a.qlo[0] + o0[0] - a.M[0], a.qlo[1] + o0[1] - a.M[1], a.qlo[2] + o0[2] - a.M[2]};
  const int HyHx = a.halo[1] * a.halo[2], HV = a.halo[0] * HyHx;
  const size_t Ovol = (size_t)a.O[0] * a.O[1] * a.O[2], Svol = (size_t)a.S[0] * a.S[1] * a.S[2];

  cdt_column_tables(a, cbl, cwl, HV, tid);

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

    float wr[kCdWCols][kCdRows];
    cdt_load_weights(a, io, wg, cwl, g, co0, nco, 0, min(a.cib, a.Cig), 4 * s0, 4 * s1, tid, wr);
    for (int ib = 0; ib < a.nib; ++ib) {
      const int ci0 = ib * a.cib, nci = min(a.cib, a.Cig - ci0);
      const int live_end = nci * HV;      // a column of a channel past the block: dead
      __syncthreads();      // the MFMA loop of the block before has read its last sample
      cdt_store_weights(wl, 4 * (s1 - s0), tid, wr);
      if (a.nib > 1 || pass == 0)
        cdt_stage_halo(a, io, xg + ((size_t)b * a.Cin + g * a.Cig + ci0) * Svol, xl, nci, HV, Svol, x0, tid);
      __syncthreads();
      // the next block's weights travel under the multiplies of this one
      if (ib + 1 < a.nib)
        cdt_load_weights(a, io, wg, cwl, g, co0, nco, ci0 + a.cib, min(a.cib, a.Cig - ci0 - a.cib), 4 * s0, 4 * s1, tid, wr);

#pragma unroll
      for (int h = 0; h < PH; ++h) {
        if (h >= nph) continue;
        wgd_v4f acc1[NPT];
#pragma unroll
        for (int c = 0; c < NPT; ++c) acc1[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};
        const int e0 = a.soff[f0 + h], e1 = a.soff[f0 + h + 1];
        for (int s = e0; s < e1; ++s) {
          const float av = wl[(s - s0) * kCdWPitch + i16 * 4 + kq];
          const int cj = cbl[4 * s + kq];
          const int cb = cj < live_end ? cj : kCdDead;
#pragma unroll
          for (int c = 0; c < NPT; ++c) {
            const int e = cb + po[c];      // (dead + dead = -2^31: still negative)
            const float v = xl[max(e, 0)];
            acc1[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, e < 0 ? 0.f : v, acc1[c], 0, 0, 0);
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

// (conv_direct_tr.hip) ph: phase slots of a pass, 2, 4, 8 or 16; npt: position tiles per wave, 1, 2, 4 or 8, ph * npt <= 16;
// the build by a.io
hipError_t conv_direct_tr_launch(const ConvDirectTrArgs& a, int ph, int npt, long long grid, size_t lds, hipStream_t st);

}  // namespace fc
