// wgrad_direct_h16.hpp -- the direct weight gradient of wgrad_direct.hpp for float16 / bfloat16 x and dY on the 16-bit
// matrix instructions of gfx950, v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x32_f16:
//   dW[(g,o)][i][k] = sum_b sum_t dY[b][(g,o)][t] * Xpad[b][(g,i)][t*stride + k*dilation - pad]
// The contract is wgrad_direct_kernel's: a workgroup (4 waves) owns one group, a block of <= 16 output channels, a block
// of `cib` input channels and one slice of the units (batch item, spatial output tile); it writes its block of
// partial[slice] completely and wgrad_direct_sum_kernel adds the slices in its fixed order.  No atomics.  Nothing is
// widened: a product of two bfloat16 or two float16 values is exact in the float32 accumulator, so the sum is that of
// "widen, multiply in float32" in another order.
//
// Operands.  The reduction index of the instruction is the output position: lane 16 q + i holds A[i][8 q .. 8 q + 7],
// lane 16 q + j holds B[8 q .. 8 q + 7][j], D[4 (lane / 16) + r][lane % 16] is register r.  i = output channel, j = column
// (input channel, tap), and the 8 k values of a lane are a RUN of 8 consecutive output positions along the last axis.
// A tile is `rows` = tz * ty rows of RX runs; a step takes the same run rx of 4 rows (q = the row), so one unit is
// rows4 / 4 * RX steps of 32 products.  Wave w owns the column tiles w * CT .. w * CT + CT - 1 as wgrad_direct_kernel.
//
// LDS, all in the tensors' own 16-bit format:
//   mask[n]          9 cells: the first n of 8 samples kept -- the B mask of a run with n live positions;
//   zero             8 zero cells: what a column past the block reads;
//   rowl[row]        the halo offset (samples) of a tile row, -1 for a row past the tile or the tensor;
//   dyl[16][dyp]     the dY tile, channel-major, a row of the tile after another, each RX whole runs: nearly a copy of
//                    dY, which is contiguous along x.  Rows past Cout/g and dead positions are zero.  dyp = 8 (runs + 1)
//                    is an odd number of cells, so the A operands of the 16 channels of a run, one aligned 16-byte read
//                    per lane shared by all column tiles, fall on 16 different 16-byte bank groups;
//   x0[ci][halo]     the x halo through the padding mode (axis_src).  A halo row has stride[2] PHASES of SP slots, SP a
//                    multiple of 8: sample hx lies in phase hx % s, slot hx / s, so that the 8 positions of a run read 8
//                    consecutive samples for every stride; a tap's dilated offset kx * d picks phase (kx d) % s and
//                    shifts the slot by (kx d) / s.  Every pitch is a multiple of 8 samples;
//   x1               the same halo one sample to the left: x1[t] = x0[t + 1].
// The B operand of (column, run) is 8 consecutive samples at colbase + rowl[row] + 8 rx.  Everything but colbase is a
// multiple of 8 samples, so the misalignment is a constant of the lane: a column with an even colbase reads x0, one with
// an odd colbase reads x1 one sample lower, and either read starts on a 4-byte boundary -- one address, no shifts.  The
// operand is ANDed with mask[live positions of the run]: a dead position contributes exactly zero whatever x holds
// there (an Inf that only the dead tail of a rounded-up run reaches never meets a multiply).
//
// Prefetch.  The samples of the NEXT unit are requested from global memory before the MFMA loop of this one and stay in
// registers under it (the first kWghXItems x 2 halo samples and kWghDyItems x 8 dY samples of a thread; what a large
// tile has beyond that is staged in place); after the loop they go to LDS between two barriers.
//
// Summation.  Three levels as wgrad_direct_kernel: acc1 sums one unit (<= 1024 positions, 32 steps of 32 products),
// acc2 += acc1 after every unit, the slices are summed in blocks of 16 by the second launch.
//
// Addressing.  x, dY and partial are plain pointers indexed with size_t; LDS offsets and positions are int.
#pragma once
#include "wgrad_direct.hpp"

namespace fc {

constexpr int kWghRun = 8;                // output positions per lane of an MFMA step
constexpr int kWghMaxRX = 8;              // runs per tile row: the zero cells a dead column reads
constexpr int kWghMaxRuns = kWgdMaxPos / kWghRun;      // runs per unit, rows rounded up to 4
constexpr int kWghXItems = 24;            // halo sample pairs a thread carries to the next unit
constexpr int kWghDyItems = 4;            // dY runs a thread carries to the next unit
constexpr int kWghMaskBytes = 9 * 16, kWghZeroBytes = kWghMaxRX * 16;
constexpr int kWghHeadBytes = kWghMaskBytes + kWghZeroBytes;      // rowl starts here

struct WgradH16Args {
  const void* x;        // (B, Cin, *S)
  const void* dy;       // (B, Cout, *O)
  float* partial;       // (slices, Cout, Cig, taps)
  AxisMap map[3];
  int S[3], O[3];
  int k[3], stride[3], dil[3];
  int tile[3], ntile[3];
  int halo[3];          // halo[2]: the pitch of a halo row, stride[2] * SP
  int SP;               // slots per phase
  int RX, rows, rows4;  // runs per tile row; rows of a tile (tz * ty), rounded up to 4
  int dyp;              // samples per channel of the staged dY tile
  FastDiv fd_ty, fd_rx, fd_runs, fd_sp2, fd_s, fd_hy, fd_hz;
  int Cin, Cout, Cig, Cog, taps;
  int cib, nib, nob;
  int slices, units;
  int off_dy, off_x0, off_x1;      // byte offsets in LDS
  int io;
};

typedef unsigned wgh_cell __attribute__((ext_vector_type(4)));      // 8 x 16 bits
typedef wgh_cell wgh_cell_a4 __attribute__((aligned(4)));           // the same on a 4-byte boundary
typedef __bf16 wgh_v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 wgh_v8h __attribute__((ext_vector_type(8)));

template <bool BF>
__device__ __forceinline__ wgd_v4f wgh_mfma(wgh_cell av, wgh_cell bv, wgd_v4f acc) {
  if constexpr (BF)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(wgh_v8bf, av), __builtin_bit_cast(wgh_v8bf, bv), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(wgh_v8h, av), __builtin_bit_cast(wgh_v8h, bv), acc, 0, 0, 0);
}

struct WghUnit { int b, o0z, o0y, o0x, lim; };      // lim: live positions of a tile row along x

__device__ __forceinline__ WghUnit wgh_unit(const WgradH16Args& a, int u) {
  const int tiles = a.ntile[0] * a.ntile[1] * a.ntile[2];
  WghUnit n;
  n.b = u / tiles;
  int t = u - n.b * tiles;
  n.o0x = (t % a.ntile[2]) * a.tile[2]; t /= a.ntile[2];
  n.o0y = (t % a.ntile[1]) * a.tile[1]; n.o0z = (t / a.ntile[1]) * a.tile[0];
  n.lim = min(a.tile[2], a.O[2] - n.o0x);
  return n;
}

// Halo item e = (ci, hz, hy, phase, slot pair): the dword x0[e].  Its two samples through the padding mode, zero where
// axis_src says -1.  Each global sample is read once per workgroup and unit.
__device__ __forceinline__ void wgh_load_x(const WgradH16Args& a, const WghUnit& n, const unsigned short* xsrc, size_t Svol,
                                           int e, unsigned& v0, unsigned& v1) {
  unsigned q, ph, hy, hz, ci;
  const int sl = 2 * (int)fdivmod((unsigned)e, a.fd_sp2, &q);
  ph = fdivmod(q, a.fd_s, &q);
  hy = fdivmod(q, a.fd_hy, &q);
  hz = fdivmod(q, a.fd_hz, &ci);
  const int hx = sl * a.stride[2] + (int)ph;
  const int sz = axis_src(a.map[0], n.o0z * a.stride[0] + (int)hz);
  const int sy = axis_src(a.map[1], n.o0y * a.stride[1] + (int)hy);
  const int sx0 = axis_src(a.map[2], n.o0x * a.stride[2] + hx);
  const int sx1 = axis_src(a.map[2], n.o0x * a.stride[2] + hx + a.stride[2]);
  const bool live = (sz | sy) >= 0;
  const unsigned short* row = xsrc + ci * Svol + ((size_t)max(sz, 0) * a.S[1] + max(sy, 0)) * a.S[2];
  v0 = (live && sx0 >= 0) ? row[sx0] : 0u;
  v1 = (live && sx1 >= 0) ? row[sx1] : 0u;
}

// x0[2 e], x0[2 e + 1] as one dword; x1[2 e - 1], x1[2 e] as two halves (16 spare bytes lie in front of x1)
__device__ __forceinline__ void wgh_store_x(unsigned char* lds, const WgradH16Args& a, int e, unsigned v0, unsigned v1) {
  reinterpret_cast<unsigned*>(lds + a.off_x0)[e] = v0 | (v1 << 16);
  unsigned short* x1 = reinterpret_cast<unsigned short*>(lds + a.off_x1);
  x1[2 * e - 1] = (unsigned short)v0;
  x1[2 * e] = (unsigned short)v1;
}

// dY item e = (channel i, run r of the tile): 8 samples along x, zero past the tile, the tensor or the block's channels
__device__ __forceinline__ void wgh_load_dy(const WgradH16Args& a, const WghUnit& n, const unsigned short* dsrc, size_t Ovol,
                                            int nco, int e, unsigned (&v)[kWghRun]) {
  unsigned i, row, pz;
  const unsigned r = fdivmod((unsigned)e, a.fd_runs, &i);
  const int rx = (int)fdivmod(r, a.fd_rx, &row);
  const int py = (int)fdivmod(row, a.fd_ty, &pz);
  const bool live = (int)i < nco && (int)row < a.rows && n.o0z + (int)pz < a.O[0] && n.o0y + py < a.O[1];
  const unsigned short* src = dsrc + i * Ovol + ((size_t)(n.o0z + (int)pz) * a.O[1] + (n.o0y + py)) * a.O[2] + n.o0x + rx * kWghRun;
#pragma unroll
  for (int t = 0; t < kWghRun; ++t) v[t] = (live && rx * kWghRun + t < n.lim) ? src[t] : 0u;
}

__device__ __forceinline__ void wgh_store_dy(unsigned char* lds, const WgradH16Args& a, int e, const unsigned (&v)[kWghRun]) {
  unsigned i;
  const unsigned r = fdivmod((unsigned)e, a.fd_runs, &i);
  *reinterpret_cast<wgh_cell*>(lds + a.off_dy + ((int)i * a.dyp + (int)r * kWghRun) * 2) =
      wgh_cell{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
}

template <bool BF, int CT>
__global__ __launch_bounds__(kWgdThreads) void wgrad_direct_h16_kernel(const WgradH16Args a) {
  using T = unsigned short;
  extern __shared__ __attribute__((aligned(16))) unsigned char wgh_lds[];
  int* rowl = reinterpret_cast<int*>(wgh_lds + kWghHeadBytes);
  const T* xg = static_cast<const T*>(a.x);
  const T* dyg = static_cast<const T*>(a.dy);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kq = lane >> 4;

  // workgroup -> (group, block of output channels, slice, block of input channels), as wgrad_direct_kernel
  unsigned bid = blockIdx.x;
  const int ib = bid % a.nib; bid /= a.nib;
  const int slice = bid % a.slices; bid /= a.slices;
  const int ob = bid % a.nob, g = bid / a.nob;
  const int co0 = g * a.Cog + ob * kWgdRows, nco = min(kWgdRows, a.Cog - ob * kWgdRows);
  const int ci0 = ib * a.cib, nci = min(a.cib, a.Cig - ci0);
  const int ncols = nci * a.taps;
  const int HyP = a.halo[1] * a.halo[2], HV = a.halo[0] * HyP;
  const size_t Ovol = (size_t)a.O[0] * a.O[1] * a.O[2], Svol = (size_t)a.S[0] * a.S[1] * a.S[2];
  const int nxi = nci * (HV / 2), ndi = kWgdRows * a.rows4 * a.RX;      // items of a unit

  // the mask cells and the zero cells
  if (tid < (kWghMaskBytes + kWghZeroBytes) / 4) {
    const int n = tid >> 2, d = tid & 3;
    reinterpret_cast<unsigned*>(wgh_lds)[tid] = tid >= kWghMaskBytes / 4 ? 0u : n >= 2 * d + 2 ? ~0u : n == 2 * d + 1 ? 0xFFFFu : 0u;
  }

  // the LDS byte address of this lane's column in each tile: x0 for an even colbase, x1 one sample lower for an odd one
  unsigned base[CT], colive[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int col = (w * CT + c) * 16 + i16;
    base[c] = kWghMaskBytes; colive[c] = 0u;      // (a column past the block reads the zero cells)
    if (col < ncols) {
      const int ci = col / a.taps, tap = col - ci * a.taps;
      const int kx = tap % a.k[2], kyz = tap / a.k[2], ky = kyz % a.k[1], kz = kyz / a.k[1];
      const int t = kx * a.dil[2], ph = t % a.stride[2], sl = t / a.stride[2];
      const int cb = ci * HV + kz * a.dil[0] * HyP + ky * a.dil[1] * a.halo[2] + ph * a.SP + sl;
      base[c] = (cb & 1) ? a.off_x1 + (cb - 1) * 2 : a.off_x0 + cb * 2;
      colive[c] = 1u;
    }
  }

  wgd_v4f acc2[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc2[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};

  const int u0 = (int)((long long)slice * a.units / a.slices), u1 = (int)((long long)(slice + 1) * a.units / a.slices);
  const T* xblk = xg + ((size_t)g * a.Cig + ci0) * Svol;
  const T* dyblk = dyg + (size_t)co0 * Ovol;

  unsigned xr[kWghXItems][2], dr[kWghDyItems][kWghRun];
  auto request = [&](int u) {      // the loads of unit u, into registers; nothing waits for them here
    const WghUnit n = wgh_unit(a, u);
    const T* xsrc = xblk + (size_t)n.b * a.Cin * Svol;
    const T* dsrc = dyblk + (size_t)n.b * a.Cout * Ovol;
#pragma unroll
    for (int t = 0; t < kWghDyItems; ++t) {
      const int e = tid + t * kWgdThreads;
      if (e < ndi) wgh_load_dy(a, n, dsrc, Ovol, nco, e, dr[t]);
    }
#pragma unroll
    for (int t = 0; t < kWghXItems; ++t) {
      const int e = tid + t * kWgdThreads;
      if (e < nxi) wgh_load_x(a, n, xsrc, Svol, e, xr[t][0], xr[t][1]);
    }
  };

  if (u0 < u1) request(u0);
  for (int u = u0; u < u1; ++u) {
    const WghUnit n = wgh_unit(a, u);
    __syncthreads();      // the MFMA loop of the unit before has read its last sample
    for (int row = tid; row < a.rows4; row += kWgdThreads) {
      unsigned pz;
      const int py = (int)fdivmod((unsigned)row, a.fd_ty, &pz);
      const bool live = row < a.rows && n.o0z + (int)pz < a.O[0] && n.o0y + py < a.O[1];
      rowl[row] = live ? (int)pz * a.stride[0] * HyP + py * a.stride[1] * a.halo[2] : -1;
    }
#pragma unroll
    for (int t = 0; t < kWghDyItems; ++t) {
      const int e = tid + t * kWgdThreads;
      if (e < ndi) wgh_store_dy(wgh_lds, a, e, dr[t]);
    }
#pragma unroll
    for (int t = 0; t < kWghXItems; ++t) {
      const int e = tid + t * kWgdThreads;
      if (e < nxi) wgh_store_x(wgh_lds, a, e, xr[t][0], xr[t][1]);
    }
    // what a large tile has beyond the registers, in place
    {
      const T* xsrc = xblk + (size_t)n.b * a.Cin * Svol;
      const T* dsrc = dyblk + (size_t)n.b * a.Cout * Ovol;
      for (int e = tid + kWghDyItems * kWgdThreads; e < ndi; e += kWgdThreads) {
        unsigned v[kWghRun];
        wgh_load_dy(a, n, dsrc, Ovol, nco, e, v);
        wgh_store_dy(wgh_lds, a, e, v);
      }
      for (int e = tid + kWghXItems * kWgdThreads; e < nxi; e += kWgdThreads) {
        unsigned v0, v1;
        wgh_load_x(a, n, xsrc, Svol, e, v0, v1);
        wgh_store_x(wgh_lds, a, e, v0, v1);
      }
    }
    __syncthreads();
    // the next unit's samples travel under the multiplies of this one
    if (u + 1 < u1) request(u + 1);

    wgd_v4f acc1[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc1[c] = wgd_v4f{0.f, 0.f, 0.f, 0.f};
    for (int row = kq; row < a.rows4; row += 4) {
      const int ro = rowl[row];
      const int limq = ro >= 0 ? n.lim : 0;
      const unsigned rb = (unsigned)max(ro, 0) * 2u;
      unsigned ad[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) ad[c] = base[c] + rb * colive[c];
      const unsigned dya = a.off_dy + (i16 * a.dyp + row * a.RX * kWghRun) * 2;
      for (int rx = 0; rx < a.RX; ++rx) {
        const wgh_cell av = *reinterpret_cast<const wgh_cell*>(wgh_lds + dya + rx * 16);
        const int live = min(max(limq - rx * kWghRun, 0), kWghRun);
        const wgh_cell mk = *reinterpret_cast<const wgh_cell*>(wgh_lds + live * 16);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const wgh_cell v = *reinterpret_cast<const wgh_cell_a4*>(wgh_lds + ad[c] + rx * 16);
          acc1[c] = wgh_mfma<BF>(av, v & mk, acc1[c]);
        }
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

// (wgrad_direct_h16.hip) ct: column tiles per wave, 1, 2, 4 or 8; the build by a.io (float16 or bfloat16)
hipError_t wgrad_direct_h16_launch(const WgradH16Args& a, int ct, long long grid, size_t lds, hipStream_t st);

}  // namespace fc
