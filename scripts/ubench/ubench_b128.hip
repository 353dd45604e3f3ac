// ubench_b128.hip -- what does the in-sequence exchange of the batch-sharing kernel (pass A -> pass B of one work item's 16
// sequences) cost with 16-byte row stores?  512-thread workgroups, two waves per SIMD, one workgroup per CU.
//   rows       today's layout: thread n2 stores A[k1][n2] at seq[k1 * 33 + n2], 32 ds_write_b64; lane k1 reads row k1,
//              32 ds_read_b64
//   transposed thread n2 owns a row: it stores (k1, k1 + 1) at seq[n2 * RS + k1] as one ds_write_b128, 16 of them; lane k1
//              reads seq[n2 * RS + k1], 32 ds_read_b64 of consecutive lanes.  RS = 34, 36, 40.
// Both move the same values (a 32 x 32 transpose inside each sequence), which main() checks after an even number of
// repetitions.  'stores' / 'reads' time one side alone.  Prints the median shader cycles per repetition over the waves of all
// workgroups, for a single workgroup and for one per CU, three launches each (the spread between them is the noise).
// Counters (SQ_LDS_BANK_CONFLICT, SQ_INSTS_LDS) are collected per kernel name by a profiler run of its own: `ubench_b128 pmc`
// launches every kernel once, one workgroup.  Diagnostic only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../fft_conv_pytorch_amd/csrc/fft_engine.hpp"

using namespace fc;

constexpr int kMaxRS = 40;

template <int BYTES>
__device__ __forceinline__ void st64(unsigned addr, f2 a) {
  asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(a), "n"(BYTES) : "memory");
}
template <int BYTES>
__device__ __forceinline__ void st128(unsigned addr, f2 a, f2 b) {
  f4 q; q.xy = a; q.zw = b;
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(q), "n"(BYTES) : "memory");
}
__device__ __forceinline__ void wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// MODE: 0 exchange, 1 stores only, 2 reads only
template <int MODE>
__device__ __forceinline__ void rows_exchange(f2 (&v)[32], f2* seq, int lane) {
  if constexpr (MODE != 2) {
    const unsigned addr = lds_off(seq + lane);
    static_for<0, 32>([&](auto kc) { constexpr int k1 = decltype(kc)::value; st64<k1 * 33 * 8>(addr, v[k1]); });
    wave_sync();
  }
  if constexpr (MODE != 1) {
    lds_read_strided<32, 1>(v, seq + lane * 33);
    lds_arrive(v);
    __builtin_amdgcn_wave_barrier();
  }
}
template <int RS, int MODE>
__device__ __forceinline__ void transposed_exchange(f2 (&v)[32], f2* seq, int lane) {
  static_assert(RS % 2 == 0 && RS <= kMaxRS, "16-byte stores need even rows");
  if constexpr (MODE != 2) {
    const unsigned addr = lds_off(seq + lane * RS);
    static_for<0, 16>([&](auto kc) { constexpr int k1 = 2 * decltype(kc)::value; st128<k1 * 8>(addr, v[k1], v[k1 + 1]); });
    wave_sync();
  }
  if constexpr (MODE != 1) {
    lds_read_strided<32, RS>(v, seq + lane);
    lds_arrive(v);
    __builtin_amdgcn_wave_barrier();
  }
}

// RS = 0: today's rows
template <int RS, int MODE>
__global__ __launch_bounds__(512, 2) void k(const f2* __restrict__ in, f2* __restrict__ out, unsigned long long* cyc, int R) {
  extern __shared__ __attribute__((aligned(16))) f2 lds[];
  const int tid = threadIdx.x;
  f2 v[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) v[i] = in[(size_t)i * 512 + tid];
  constexpr int LSEQ = RS ? 32 * RS : 32 * 33;
  f2* seq = lds + (tid / 32) * LSEQ;
  const int lane = tid % 32;
  if (MODE == 2) {      // (reads only: defined values)
#pragma unroll
    for (int i = 0; i < 32; ++i) seq[i * (LSEQ / 32) + lane] = v[i];
  }
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < R; ++r) {
    if constexpr (RS == 0) rows_exchange<MODE>(v, seq, lane);
    else transposed_exchange<RS, MODE>(v, seq, lane);
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
#pragma unroll
  for (int i = 0; i < 32; ++i) out[((size_t)blockIdx.x * 32 + i) * 512 + tid] = v[i];
  if ((tid & 63) == 0) cyc[(size_t)blockIdx.x * 8 + tid / 64] = t1 - t0;
}

int main(int argc, char** argv) {
  const bool pmc = argc > 1 && !strcmp(argv[1], "pmc");
  const int NWG = 256;
  f2 *in, *out;
  unsigned long long* cyc;
  hipMalloc(&in, 32 * 512 * sizeof(f2));
  hipMalloc(&out, (size_t)NWG * 32 * 512 * sizeof(f2));
  hipMalloc(&cyc, NWG * 8 * sizeof(unsigned long long));
  std::vector<f2> h(32 * 512), ho(32 * 512);
  for (size_t i = 0; i < h.size(); ++i) h[i] = f2{(float)(rand() % 1000) / 1000.f - 0.5f, (float)(rand() % 1000) / 1000.f - 0.5f};
  hipMemcpy(in, h.data(), h.size() * sizeof(f2), hipMemcpyHostToDevice);
  const size_t lds = (size_t)16 * 32 * kMaxRS * sizeof(f2);      // 163,840 bytes: one workgroup per CU in every variant
  const int R = pmc ? 16 : 64;
  auto run = [&](auto kern, const char* name, int mode) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      printf("%s: no %zu bytes of LDS\n", name, lds);
      return;
    }
    for (int grid : {1, NWG}) {
      if (pmc && grid != 1) continue;
      double med[3];
      for (int rep = 0; rep < (pmc ? 1 : 3); ++rep) {
        kern<<<grid, 512, lds>>>(in, out, cyc, R);
        if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); exit(1); }
        std::vector<unsigned long long> hc(grid * 8);
        hipMemcpy(hc.data(), cyc, hc.size() * 8, hipMemcpyDeviceToHost);
        std::sort(hc.begin(), hc.end());
        med[rep] = (double)hc[hc.size() / 2] / R;
      }
      if (pmc) { printf("%-28s R %d, one workgroup\n", name, R); continue; }
      // an even number of exchanges is the identity
      long bad = 0;
      if (mode == 0) {
        hipMemcpy(ho.data(), out, ho.size() * sizeof(f2), hipMemcpyDeviceToHost);
        for (size_t i = 0; i < h.size(); ++i) bad += (ho[i].x != h[i].x) || (ho[i].y != h[i].y);
      }
      printf("%-28s %3d workgroup(s): %7.1f %7.1f %7.1f cycles per repetition and wave%s\n", name, grid, med[0], med[1], med[2],
             mode ? "" : (bad ? "   VALUES WRONG" : "   values ok"));
    }
  };
  run(k<0, 0>, "rows b64 exchange", 0);
  run(k<34, 0>, "transposed RS 34 exchange", 0);
  run(k<36, 0>, "transposed RS 36 exchange", 0);
  run(k<40, 0>, "transposed RS 40 exchange", 0);
  run(k<0, 1>, "rows b64 stores", 1);
  run(k<34, 1>, "transposed RS 34 stores", 1);
  run(k<36, 1>, "transposed RS 36 stores", 1);
  run(k<0, 2>, "rows b64 reads", 2);
  run(k<34, 2>, "transposed RS 34 reads", 2);
  return 0;
}
