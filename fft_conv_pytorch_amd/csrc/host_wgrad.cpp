// host_wgrad.cpp -- fc_wgrad_direct_geometry and fc_wgrad_direct (include/fftconv_amd.h "Direct weight gradient"): the
// planner of wgrad_direct_kernel (wgrad_direct.hpp) and its two launches.  The planner is pure arithmetic on the
// descriptor, the CU count and FFTCONV_WGRAD_DIRECT_SLICES; the launch call plans again for the current device (the last
// answer is remembered per thread), allocates nothing and synchronises nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "fc_plan.h"
#include "wgrad_direct.hpp"

using namespace fc;

namespace {

constexpr int64_t kLdsShared = 64 * 1024;       // up to here two workgroups share a CU
constexpr int64_t kLdsBudget = 160 * 1024;
constexpr int kMaxTaps = 128;
constexpr int kMaxCols = kWgdWaves * kWgdMaxCT * 16;      // columns (input channel, tap) of one workgroup

struct Geom {
  int ax0;                   // first axis of the descriptor in the kernel's (z, y, x): 1 for a 2-D layer
  int O[3], S[3], k[3], stride[3], dil[3], pad[3];
  int tile[3], ntile[3], halo[3];
  int Cig, Cog, taps, cib, nib, nob, ct;
  int P, P4, slices;
  int64_t units, lds, ws;
};

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

int lds_bytes(int p4, int cib, int64_t hv, int64_t* out) {
  *out = 4 * ((int64_t)p4 * (1 + kWgdDyPitch) + cib * hv);
  return *out <= kLdsBudget;
}

// Validates the descriptor and chooses input-channel block, tile and slices.  The tile and the channel block minimise a
// cycle estimate of the whole launch: per unit the MFMA steps of a wave (P4/4 steps x CT instructions x 32 cycles), a
// fixed cost for the exposed latency of its loads, and half a cycle per staged sample; among the candidates that fit
// 64 KiB of LDS, else among those that fit the 160 KiB budget.
int plan(const fc_desc& c, int cus, Geom& g) {
  if (c.ndim == 1) return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct covers 2-D and 3-D convolutions (1-D: fc_wgrad1d)");
  if (c.ndim < 1 || c.ndim > 3) return fail(FC_ERR_INVALID, "ndim must be 1, 2 or 3 (got %d)", c.ndim);
  if (c.dtype == FC_F64 || c.dtype == FC_C64)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct takes float32, float16 or bfloat16 x and dY (no %s)",
                c.dtype == FC_F64 ? "float64" : "complex64");
  if (c.dtype != FC_F32 && c.dtype != FC_F16 && c.dtype != FC_BF16) return fail(FC_ERR_INVALID, "unknown dtype %d", c.dtype);
  if (c.transposed) return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct takes the descriptor of a forward convolution");
  if (c.batch < 1 || c.in_channels < 1 || c.out_channels < 1 || c.groups < 1 || c.in_channels % c.groups || c.out_channels % c.groups)
    return fail(FC_ERR_INVALID, "batch, channels and groups must be positive and the channels divisible by groups");
  if (c.padding_mode < 0 || c.padding_mode > 3) return fail(FC_ERR_INVALID, "unknown padding_mode %d", c.padding_mode);
  if (cus < 1) return fail(FC_ERR_INVALID, "compute_units must be positive (got %d)", cus);
  g.ax0 = 3 - c.ndim;
  for (int a = 0; a < 3; ++a) { g.O[a] = g.S[a] = g.k[a] = g.stride[a] = g.dil[a] = 1; g.pad[a] = 0; }
  int64_t taps = 1, xs = c.batch * c.in_channels, ys = c.batch * c.out_channels;
  for (int i = 0; i < c.ndim; ++i) {
    const int a = g.ax0 + i;
    if (c.spatial[i] < 1 || c.kernel[i] < 1 || c.stride[i] < 1 || c.dilation[i] < 1 || c.padding[i] < 0)
      return fail(FC_ERR_INVALID, "axis %d: spatial/kernel/stride/dilation must be >= 1 and padding >= 0", i);
    if (c.kernel[i] > kMaxTaps || c.dilation[i] >= (1 << 20) || c.stride[i] >= (1 << 20))
      return fail(FC_ERR_UNSUPPORTED, "axis %d: fc_wgrad_direct covers kernels of at most %d taps in all", i, kMaxTaps);
    if (c.spatial[i] + 2 * c.padding[i] >= ((int64_t)1 << 31))
      return fail(FC_ERR_UNSUPPORTED, "axis %d: padded extent %lld exceeds 32-bit positions (must be < 2^31 samples)", i,
                  (long long)(c.spatial[i] + 2 * c.padding[i]));
    const int64_t kd = (c.kernel[i] - 1) * c.dilation[i] + 1, span = c.spatial[i] + 2 * c.padding[i] - kd;
    if (span < 0) return fail(FC_ERR_INVALID, "axis %d: dilated kernel extent %lld is larger than the padded input", i, (long long)kd);
    if (c.padding_mode == FC_PAD_REFLECT && c.padding[i] >= c.spatial[i])
      return fail(FC_ERR_INVALID, "axis %d: reflect padding (%lld) must be smaller than the input size (%lld)", i,
                  (long long)c.padding[i], (long long)c.spatial[i]);
    if (c.padding_mode == FC_PAD_CIRCULAR && c.padding[i] > c.spatial[i])
      return fail(FC_ERR_INVALID, "axis %d: circular padding (%lld) must not exceed the input size (%lld)", i,
                  (long long)c.padding[i], (long long)c.spatial[i]);
    g.S[a] = (int)c.spatial[i]; g.O[a] = (int)(span / c.stride[i] + 1); g.k[a] = (int)c.kernel[i];
    g.stride[a] = (int)c.stride[i]; g.dil[a] = (int)c.dilation[i]; g.pad[a] = (int)c.padding[i];
    taps *= c.kernel[i];
    xs *= c.spatial[i]; ys *= g.O[a];
    if (xs >= ((int64_t)1 << 40) || ys >= ((int64_t)1 << 40))
      return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct indexes x and dY in 64 bits but takes fewer than 2^40 samples each");
  }
  if (taps > kMaxTaps)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct covers kernels of at most %d taps in all (got %lld): the accumulators of a "
                "workgroup hold %d columns", kMaxTaps, (long long)taps, kMaxCols);
  g.taps = (int)taps;
  g.Cig = (int)(c.in_channels / c.groups); g.Cog = (int)(c.out_channels / c.groups);
  if (c.in_channels >= (1 << 30) || c.out_channels >= (1 << 30)) return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: fewer than 2^30 channels");
  g.nob = (int)cdiv(g.Cog, kWgdRows);

  // candidates: the largest channel blocks of the first 8 even splits of the group, tiles of powers of two clipped to the output
  double best = -1.0;
  bool best_shared = false;
  const int cibmax = std::min<int>(g.Cig, kMaxCols / g.taps);
  int last_cib = 0, tried = 0;
  for (int n = (int)cdiv(g.Cig, cibmax); n <= g.Cig && tried < 8; ++n) {
    const int cib = (int)cdiv(g.Cig, n);
    if (cib == last_cib) continue;
    last_cib = cib; ++tried;
    const int nib = (int)cdiv(g.Cig, cib);
    int ct = 1;
    while (kWgdWaves * ct * 16 < cib * g.taps) ct *= 2;
    for (int tz = 1; tz <= 8; tz *= 2)
      for (int ty = 1; ty <= 16; ty *= 2)
        for (int tx = 1; tx <= 64; tx *= 2) {
          const int t[3] = {std::min(tz, g.O[0]), std::min(ty, g.O[1]), std::min(tx, g.O[2])};
          if ((tz > 1 && t[0] < tz && tz / 2 >= g.O[0]) || (ty > 1 && t[1] < ty && ty / 2 >= g.O[1]) ||
              (tx > 1 && t[2] < tx && tx / 2 >= g.O[2]))
            continue;      // (the same clipped tile as a smaller candidate)
          const int P = t[0] * t[1] * t[2];
          if (P > kWgdMaxPos) continue;
          const int P4 = (P + 3) & ~3;
          int64_t hv = 1, ntiles = 1, lds;
          for (int a = 0; a < 3; ++a) {
            hv *= (int64_t)(t[a] - 1) * g.stride[a] + (int64_t)(g.k[a] - 1) * g.dil[a] + 1;
            ntiles *= cdiv(g.O[a], t[a]);
            if (hv > kLdsBudget) break;
          }
          if (hv > kLdsBudget || !lds_bytes(P4, cib, hv, &lds)) continue;
          const bool shared = lds <= kLdsShared;
          if (best_shared && !shared) continue;
          const double cost = (double)nib * (double)ntiles * (8.0 * P4 * ct + 3000.0 + 0.5 * (cib * (double)hv + 16.0 * P4));
          if (best < 0 || (shared && !best_shared) || cost < best) {
            best = cost; best_shared = shared;
            g.cib = cib; g.nib = nib; g.ct = ct; g.P = P; g.P4 = P4; g.lds = lds;
            for (int a = 0; a < 3; ++a) {
              g.tile[a] = t[a]; g.ntile[a] = (int)cdiv(g.O[a], t[a]);
              g.halo[a] = (t[a] - 1) * g.stride[a] + (g.k[a] - 1) * g.dil[a] + 1;
            }
          }
        }
  }
  if (best < 0)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: the x samples that one output position reaches through every tap do not "
                "fit %lld bytes of LDS", (long long)kLdsBudget);
  g.units = c.batch * g.ntile[0] * g.ntile[1] * g.ntile[2];
  const int64_t blocks = c.groups * g.nob * g.nib;
  if (g.units >= ((int64_t)1 << 31))
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: %lld (batch item, tile) units exceed 2^31", (long long)g.units);
  int64_t slices = std::max<int64_t>(1, ((g.lds <= kLdsShared ? 2 : 1) * (int64_t)cus + blocks / 2) / blocks);
  if (const char* env = getenv("FFTCONV_WGRAD_DIRECT_SLICES")) {
    const long long forced = atoll(env);
    if (forced >= 1) slices = forced;
  }
  slices = std::min<int64_t>(slices, g.units);
  if (blocks * slices > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: %lld workgroups exceed the 2^31 of one launch", (long long)(blocks * slices));
  g.slices = (int)slices;
  g.ws = slices * c.out_channels * g.Cig * g.taps * 4;
  return FC_OK;
}

}  // namespace

extern "C" int fc_wgrad_direct_geometry(const fc_desc* conv_desc, int compute_units, int64_t info[8]) {
  if (!conv_desc || !info) return fail(FC_ERR_INVALID, "null argument");
  Geom g;
  if (int st = plan(*conv_desc, compute_units, g)) return st;
  for (int i = 0; i < 3; ++i) info[i] = i < conv_desc->ndim ? g.tile[g.ax0 + i] : 0;
  info[3] = std::min(g.Cog, kWgdRows); info[4] = g.cib; info[5] = g.slices; info[6] = g.lds; info[7] = g.ws;
  return FC_OK;
}

extern "C" int fc_wgrad_direct(const fc_desc* conv_desc, const void* x, const void* dy, float* dw, void* workspace,
                               void* hip_stream) {
  if (!conv_desc || !x || !dy || !dw || !workspace) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // (as fc_forward: a stale sticky error of an earlier call is not this call's)
  int cus = 0;
  if (!current_device_cus(&cus) || cus < 1) return fail(FC_ERR_HIP, "the CU count of the current device is not available");
  // the plan of the last call of this thread, while descriptor, CU count and the knob are what they were
  struct Last { fc_desc d; int cus; long long knob; Geom g; bool set; };
  static thread_local Last last = {};
  const char* env = getenv("FFTCONV_WGRAD_DIRECT_SLICES");
  const long long knob = env ? atoll(env) : 0;
  if (!last.set || std::memcmp(&last.d, conv_desc, sizeof(fc_desc)) || last.cus != cus || last.knob != knob) {
    last.set = false;
    if (int st = plan(*conv_desc, cus, last.g)) return st;
    last.d = *conv_desc; last.cus = cus; last.knob = knob; last.set = true;
  }
  const Geom& g = last.g;
  const fc_desc& c = *conv_desc;
  WgradDirectArgs a;
  std::memset(&a, 0, sizeof a);
  a.x = x; a.dy = dy; a.partial = static_cast<float*>(workspace);
  for (int i = 0; i < 3; ++i) {
    a.map[i] = AxisMap{g.S[i], g.pad[i], c.padding_mode, 1};
    a.S[i] = g.S[i]; a.O[i] = g.O[i]; a.k[i] = g.k[i]; a.stride[i] = g.stride[i]; a.dil[i] = g.dil[i];
    a.tile[i] = g.tile[i]; a.ntile[i] = g.ntile[i]; a.halo[i] = g.halo[i];
  }
  a.fd_tx = make_fastdiv(g.tile[2]); a.fd_ty = make_fastdiv(g.tile[1]);
  a.fd_hx = make_fastdiv(g.halo[2]); a.fd_hy = make_fastdiv(g.halo[1]);
  a.Cin = (int)c.in_channels; a.Cout = (int)c.out_channels; a.Cig = g.Cig; a.Cog = g.Cog; a.taps = g.taps;
  a.cib = g.cib; a.nib = g.nib; a.nob = g.nob;
  a.slices = g.slices; a.units = (int)g.units; a.P = g.P; a.P4 = g.P4;
  a.io = c.dtype;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  FC_HIP(wgrad_direct_launch(a, g.ct, c.groups * g.nob * g.nib * g.slices, (size_t)g.lds, st));
  FC_HIP(wgrad_direct_sum_launch(a.partial, dw, (long long)c.out_channels * g.Cig * g.taps, g.slices, st));
  return FC_OK;
}
