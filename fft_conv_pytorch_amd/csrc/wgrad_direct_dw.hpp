// wgrad_direct_dw.hpp -- the depthwise body of the direct weight gradient: layers with one input channel
// per group (any channel multiplier Cout/g),
//   dW[o][0][k] = sum_b sum_t dY[b][o][t] * Xpad[b][g(o)][t*stride + k*dilation - pad]
// on the vector ALU in float32.  The MFMA body (wgrad_direct.hpp) gives such a layer one live row of 16.
//
// Work split.  A workgroup (4 waves) owns one output channel and one slice of the (batch item, output tile) units, and
// writes its `taps` sums to partial[slice][o][0][:]; wgrad_direct_sum_kernel adds the slices.  No atomics, nothing
// cleared, nothing uninitialised read: the bits of dW are a function of the geometry alone.
//
// Positions go to lanes, taps to waves and registers.  A tile row is cut into runs of kDwR = 4 consecutive output
// columns (the tile's last axis is padded to whole runs); lane l of every wave owns the runs l, l + 64, ...  The taps
// are cut into blocks of KXB consecutive taps of the last axis within one (kz, ky) row; wave w owns the blocks
// w, w + 4, ..., NB of them at most, and keeps their NB * KXB sums in registers with compile-time indices: acc1 over one
// unit, acc2 += acc1 after every unit.  A block past the last one is skipped by a wave-uniform branch.
//
// Per unit the workgroup stages, widened to float32 as they are loaded (Io<>):
//   dyl[run][4]   the dY tile, run-major: a dead position (past the tensor, or the padding of the tile to a whole run)
//                 is a zero by a select;
//   info[run]     the halo offset of the run's first position, and above bit 20 which of its 4 positions are live;
//   xl[halo]      the x halo of the channel (wgd_stage_halo, shared with the MFMA body), rows padded to hxp floats so
//                 that the window of the last run and the dead tail of the last tap block stay inside their row.
// Per run a lane reads its 4 dY once (one 16-byte LDS read) and per tap block the x window of the tap row: with stride
// and dilation 1 on the last axis 4 + KXB - 1 contiguous words as 16-byte reads (the planner makes every window base a
// multiple of 4 words) for 4 * KXB FMAs; the KXB == 1 builds are the general ones and read x[p * stride] per product,
// the taps' dilated offsets riding in the block offset.  A run with a dead position takes a second copy of the
// products that selects the dead ones to zero (never 0 * x); the choice is a wave vote, so interior tiles never take it.
//
// Once per workgroup every sum is reduced over the 64 lanes by a fixed xor butterfly and lane 0 writes it.
//
// Addressing as in wgrad_direct.hpp: size_t into global memory, int for positions and LDS.
#pragma once
#include "wgrad_direct.hpp"

namespace fc {

constexpr int kDwR = 4;                   // output columns of a run
constexpr int kDwLiveShift = 20;          // info word: halo offset below this bit (LDS holds < 2^16 floats), live bits above
constexpr int kDwMaxAcc = 64;             // NB * KXB of the largest build

typedef float dw_v4f __attribute__((ext_vector_type(4)));

// words of x one run reads through a block of KXB taps, in whole 16-byte reads
constexpr int dw_window4(int kxb) { return (kDwR + kxb - 1 + 3) / 4; }

template <int KXB, int NB, bool SEL>
__device__ __forceinline__ void dw_products(float (&acc)[NB * KXB], const float* xl, const int (&toff)[NB], int xo, int live,
                                            const dw_v4f dy, int w, int nblk, int sx) {
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    if (w + kWgdWaves * j >= nblk) break;      // wave-uniform
    const float* xp = xl + xo + toff[j];
    if constexpr (KXB == 1) {
#pragma unroll
      for (int r = 0; r < kDwR; ++r) {
        float v = xp[r * sx];
        if (SEL) v = (live >> r & 1) ? v : 0.f;
        acc[j] = __builtin_fmaf(dy[r], v, acc[j]);
      }
    } else {
      constexpr int W4 = dw_window4(KXB);
      float xw[4 * W4];
#pragma unroll
      for (int i = 0; i < W4; ++i) {
        const dw_v4f t = reinterpret_cast<const dw_v4f*>(xp)[i];
        xw[4 * i] = t[0]; xw[4 * i + 1] = t[1]; xw[4 * i + 2] = t[2]; xw[4 * i + 3] = t[3];
      }
#pragma unroll
      for (int r = 0; r < kDwR; ++r)
#pragma unroll
        for (int k = 0; k < KXB; ++k) {
          float v = xw[r + k];
          if (SEL) v = (live >> r & 1) ? v : 0.f;
          acc[j * KXB + k] = __builtin_fmaf(dy[r], v, acc[j * KXB + k]);
        }
    }
  }
}

template <int IO, int KXB, int NB>
__global__ __launch_bounds__(kWgdThreads) void wgrad_direct_dw_kernel(const WgradDirectArgs a) {
  static_assert(NB * KXB <= kDwMaxAcc, "at most 64 sums per lane and level");
  using T = typename Io<IO>::T;
  extern __shared__ __attribute__((aligned(16))) float wgd_lds[];
  int* info = reinterpret_cast<int*>(wgd_lds);
  float* dyl = wgd_lds + a.runs64;
  float* xl = dyl + a.runs64 * kDwR;
  const Io<IO> io(a.io);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);

  // workgroup -> (group, slice, output channel of the group): the channels of a group run next to each other and
  // share their x halo in L2
  unsigned bid = blockIdx.x;
  const int om = bid % a.Cog; bid /= a.Cog;
  const int slice = bid % a.slices, g = bid / a.slices;
  const int o = g * a.Cog + om;
  const int hxp = a.halo[2], HyHx = a.halo[1] * hxp, HV = a.halo[0] * HyHx;
  const size_t Ovol = (size_t)a.O[0] * a.O[1] * a.O[2], Svol = (size_t)a.S[0] * a.S[1] * a.S[2];
  const T* xg = static_cast<const T*>(a.x);
  const T* dyg = static_cast<const T*>(a.dy);

  int toff[NB];      // halo offset of the first tap of block w + 4 j
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int blk = min(w + kWgdWaves * j, a.nblk - 1);
    const int row = blk / a.nbx, bx = blk - row * a.nbx;
    const int ky = row % a.k[1], kz = row / a.k[1];
    toff[j] = kz * a.dil[0] * HyHx + ky * a.dil[1] * hxp + bx * KXB * a.dil[2];
  }

  float acc2[NB * KXB];
#pragma unroll
  for (int i = 0; i < NB * KXB; ++i) acc2[i] = 0.f;

  const int u0 = (int)((long long)slice * a.units / a.slices), u1 = (int)((long long)(slice + 1) * a.units / a.slices);
  for (int u = u0; u < u1; ++u) {
    int b, o0z, o0y, o0x;
    wgd_unit_origin(a, u, b, o0z, o0y, o0x);
    __syncthreads();      // the products of the unit before have read their last sample

    // dY tile, run by run, with the halo offset and the live bits of each run
    const T* dsrc = dyg + ((size_t)b * a.Cout + o) * Ovol;
    for (int q = tid; q < a.runs64; q += kWgdThreads) {
      dw_v4f v = {0.f, 0.f, 0.f, 0.f};
      int word = 0;
      if (q < a.runs) {
        unsigned t, pz;
        const int px = (int)fdivmod((unsigned)q, a.fd_rx, &t) * kDwR;
        const int py = (int)fdivmod(t, a.fd_ty, &pz);
        const bool rowlive = o0z + (int)pz < a.O[0] && o0y + py < a.O[1];
        const size_t off = ((size_t)(o0z + (int)pz) * a.O[1] + (o0y + py)) * a.O[2] + (o0x + px);
        int live = 0;
#pragma unroll
        for (int r = 0; r < kDwR; ++r) {
          const bool l = rowlive && px + r < a.tile[2] && o0x + px + r < a.O[2];
          if (l) v[r] = io.in(dsrc[off + r]);
          live |= (int)l << r;
        }
        word = ((int)pz * a.stride[0] * HyHx + py * a.stride[1] * hxp + px * a.stride[2]) | live << kDwLiveShift;
      }
      info[q] = word;
      reinterpret_cast<dw_v4f*>(dyl)[q] = v;
    }
    wgd_stage_halo(a, io, xg + ((size_t)b * a.Cin + g) * Svol, xl, 1, HV, Svol, o0z, o0y, o0x, tid);
    __syncthreads();

    float acc1[NB * KXB];
#pragma unroll
    for (int i = 0; i < NB * KXB; ++i) acc1[i] = 0.f;
    for (int q = lane; q < a.runs64; q += 64) {
      const int word = info[q], live = word >> kDwLiveShift, xo = word & ((1 << kDwLiveShift) - 1);
      const dw_v4f dy = reinterpret_cast<const dw_v4f*>(dyl)[q];
      const bool ragged = live != 0 && live != (1 << kDwR) - 1;
      if (__builtin_amdgcn_ballot_w64(ragged) == 0) {
        if (live) dw_products<KXB, NB, false>(acc1, xl, toff, xo, live, dy, w, a.nblk, a.stride[2]);
      } else {
        dw_products<KXB, NB, true>(acc1, xl, toff, xo, live, dy, w, a.nblk, a.stride[2]);
      }
    }
#pragma unroll
    for (int i = 0; i < NB * KXB; ++i) acc2[i] += acc1[i];
  }

  // every sum over the 64 lanes, a fixed butterfly; lane 0 writes the live taps
  float* out = a.partial + ((size_t)slice * a.Cout + o) * a.taps;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int blk = w + kWgdWaves * j;
    if (blk >= a.nblk) break;
    const int row = blk / a.nbx, k0 = (blk - row * a.nbx) * KXB;
#pragma unroll
    for (int k = 0; k < KXB; ++k) {
      float s = acc2[j * KXB + k];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
      if (lane == 0 && k0 + k < a.k[2]) out[row * a.k[2] + k0 + k] = s;
    }
  }
}

// (wgrad_direct.hip) kxb: taps per block, 1 (the general build), 2, 4 or 8; nb: blocks per wave, rounded up to a build
int wgrad_direct_dw_blocks(int kxb, int nb);      // the NB of the build that serves nb blocks per wave, 0 if none
hipError_t wgrad_direct_dw_launch(const WgradDirectArgs& a, int kxb, int nb, long long grid, size_t lds, hipStream_t st);

}  // namespace fc
