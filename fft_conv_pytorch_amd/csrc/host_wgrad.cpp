// host_wgrad.cpp -- fc_wgrad_direct_geometry, fc_wgrad_direct_body and fc_wgrad_direct (include/fftconv_amd.h "Direct
// weight gradient"): the planner of wgrad_direct_kernel (wgrad_direct.hpp), of wgrad_direct_dw_kernel
// (wgrad_direct_dw.hpp) and of wgrad_direct_h16_kernel (wgrad_direct_h16.hpp), and their two launches.  The planner is pure arithmetic on the descriptor, the CU count,
// FFTCONV_WGRAD_DIRECT_SLICES and FFTCONV_WGRAD_DIRECT_BODY; the launch call plans again for the current device (the
// last answer is remembered per thread), allocates nothing and synchronises nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "fc_plan.h"
#include "wgrad_direct_dw.hpp"
#include "wgrad_direct_h16.hpp"

using namespace fc;

namespace {

constexpr int64_t kLdsShared = 64 * 1024;       // up to here two workgroups share a CU
constexpr int64_t kLdsBudget = 160 * 1024;
constexpr int kMaxTaps = 128;
constexpr int kMaxCols = kWgdWaves * kWgdMaxCT * 16;      // columns (input channel, tap) of one workgroup
enum Body { BODY_MFMA = 0, BODY_VALU = 1, BODY_H16 = 2 };
// The largest channel multiplier Cout/g of a layer with Cin/g == 1 that the automatic rule gives to the depthwise
// body: the largest of 1, 2, 4, 8, 16 at which it was faster than the MFMA body by more than three spreads on
// B8 C256 56^2 k7 bfloat16 (profiles/wgrad_direct_dw.jsonl).
constexpr int kDwMaxMultiplier = 8;
constexpr int kDwGroupsPerCu = 4;               // workgroups the slices aim at per CU, while LDS allows
constexpr int64_t kDwLdsShared = kLdsBudget / kDwGroupsPerCu;

struct Geom {
  int ax0;                   // first axis of the descriptor in the kernel's (z, y, x): 1 for a 2-D layer
  int O[3], S[3], k[3], stride[3], dil[3], pad[3];
  int tile[3], ntile[3], halo[3];
  int Cig, Cog, taps, cib, nib, nob, ct;
  int P, P4, slices;
  int64_t units, lds, ws;
  int body;                  // Body; the depthwise body besides:
  int kxb, nb, nbx, nblk;    // taps per block, blocks of the busiest wave, blocks per kernel row and in all
  int runs, runs64;          // runs of kDwR positions per tile, rounded up to whole waves
  // the 16-bit MFMA body: slots per phase of a halo row, runs per tile row, rows of a tile and rounded up to 4, samples
  // per channel of the dY tile, LDS byte offsets
  int SP, RX, rows, rows4, dyp, off_dy, off_x0, off_x1;
};

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

int lds_bytes(int p4, int cib, int64_t hv, int64_t* out) {
  *out = 4 * ((int64_t)p4 * (1 + kWgdDyPitch) + cib * hv);
  return *out <= kLdsBudget;
}

// FFTCONV_WGRAD_DIRECT_BODY: 1 "mfma", 2 "valu", 3 "h16" (the automatic rule, and the 16-bit MFMA body where that gives a
// float16 / bfloat16 layer to the MFMA body), 0 unset or anything else (the automatic rule)
int body_knob() {
  const char* env = getenv("FFTCONV_WGRAD_DIRECT_BODY");
  return !env ? 0 : !std::strcmp(env, "mfma") ? 1 : !std::strcmp(env, "valu") ? 2 : !std::strcmp(env, "h16") ? 3 : 0;
}

int64_t forced_slices() {
  const char* env = getenv("FFTCONV_WGRAD_DIRECT_SLICES");
  return env ? std::max<long long>(atoll(env), 0) : 0;
}

// Tile and slices of the depthwise body for a validated layer with Cin/g == 1.  Tiles are powers of two clipped to
// the output, the last axis in whole runs; the one with the smallest cycle estimate of the launch wins among those whose
// LDS (one dY tile with its run words, one halo) lets kDwGroupsPerCu workgroups share a CU, else among those that fit.
// Per unit the estimate counts the FMAs of the busiest wave (4 cycles each), its LDS reads, half a cycle per staged
// sample and a fixed cost for the exposed latency of the loads.
int plan_dw(const fc_desc& c, int cus, Geom& g) {
  const bool unit = g.stride[2] == 1 && g.dil[2] == 1;      // else the general build, a tap per block
  g.kxb = !unit || g.k[2] == 1 ? 1 : g.k[2] == 2 ? 2 : g.k[2] <= 4 ? 4 : 8;
  g.nbx = (int)cdiv(g.k[2], g.kxb); g.nblk = g.k[0] * g.k[1] * g.nbx; g.nb = (int)cdiv(g.nblk, kWgdWaves);
  if (!wgrad_direct_dw_blocks(g.kxb, g.nb)) return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: no depthwise build of %d x %d", g.kxb, g.nb);
  g.cib = 1; g.nib = 1; g.nob = g.Cog; g.ct = 0; g.P4 = 0;
  double best = -1.0;
  bool best_shared = false;
  for (int tz = 1; tz <= 8; tz *= 2)
    for (int ty = 1; ty <= 16; ty *= 2)
      for (int tx = kDwR; tx <= 64; tx *= 2) {
        const int t[3] = {std::min(tz, g.O[0]), std::min(ty, g.O[1]), std::min(tx, g.O[2])};
        if ((tz > 1 && tz / 2 >= g.O[0]) || (ty > 1 && ty / 2 >= g.O[1]) || (tx > kDwR && tx / 2 >= g.O[2]))
          continue;      // (the same clipped tile as a smaller candidate)
        const int txr = (t[2] + kDwR - 1) / kDwR * kDwR, runs = t[0] * t[1] * (txr / kDwR);
        if (runs * kDwR > kWgdMaxPos) continue;
        const int runs64 = (runs + 63) & ~63;
        int64_t halo[3], ntiles = 1;
        for (int a = 0; a < 3; ++a) {
          halo[a] = (int64_t)(t[a] - 1) * g.stride[a] + (int64_t)(g.k[a] - 1) * g.dil[a] + 1;
          ntiles *= cdiv(g.O[a], t[a]);
        }
        // the row pitch: the window of the last run through the last tap block, dead tail included, in whole reads
        halo[2] = unit ? (txr - kDwR) + (g.nbx - 1) * g.kxb + (g.kxb == 1 ? kDwR : 4 * dw_window4(g.kxb))
                       : (int64_t)(txr - 1) * g.stride[2] + (int64_t)(g.k[2] - 1) * g.dil[2] + 1;
        halo[2] = (halo[2] + 3) & ~(int64_t)3;
        if (halo[0] > kLdsBudget || halo[1] > kLdsBudget || halo[2] > kLdsBudget || halo[0] * halo[1] > kLdsBudget) continue;
        const int64_t hv = halo[0] * halo[1] * halo[2], lds = 4 * ((int64_t)runs64 * (1 + kDwR) + hv);
        if (lds > kLdsBudget) continue;
        const bool shared = lds <= kDwLdsShared;
        if (best_shared && !shared) continue;
        const double per_run = g.nb * (4.0 * g.kxb * kDwR + (g.kxb == 1 ? 8.0 * kDwR : 8.0 * dw_window4(g.kxb))) + 24.0;
        const double cost = (double)ntiles * (runs64 / 64 * per_run + 3000.0 + 0.5 * ((double)hv + kDwR * runs64));
        if (best < 0 || (shared && !best_shared) || cost < best) {
          best = cost; best_shared = shared;
          g.runs = runs; g.runs64 = runs64; g.P = runs * kDwR; g.lds = lds;
          for (int a = 0; a < 3; ++a) { g.tile[a] = t[a]; g.ntile[a] = (int)cdiv(g.O[a], t[a]); g.halo[a] = (int)halo[a]; }
        }
      }
  if (best < 0)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: the x samples that one run of output positions reaches through every tap "
                "do not fit %lld bytes of LDS", (long long)kLdsBudget);
  g.units = c.batch * g.ntile[0] * g.ntile[1] * g.ntile[2];
  if (g.units >= ((int64_t)1 << 31))
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: %lld (batch item, tile) units exceed 2^31", (long long)g.units);
  // channels x slices fill the device kDwGroupsPerCu workgroups deep
  int64_t slices = std::max<int64_t>(1, ((int64_t)kDwGroupsPerCu * cus + c.out_channels / 2) / c.out_channels);
  if (const int64_t forced = forced_slices()) slices = forced;
  slices = std::min<int64_t>(slices, g.units);
  if (c.out_channels * slices > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: %lld workgroups exceed the 2^31 of one launch", (long long)(c.out_channels * slices));
  g.slices = (int)slices;
  g.ws = slices * c.out_channels * g.taps * 4;
  return FC_OK;
}

// Input-channel block, tile and slices of the 16-bit MFMA body (wgrad_direct_h16.hpp) for a validated float16 /
// bfloat16 layer that plan() gave to the MFMA body; false where no tile fits, and the layer keeps that body.  A tile is
// tz x ty rows (rounded up to 4: the rows of one MFMA step) of RX whole runs of 8 positions, at most kWghMaxRuns runs.
// LDS is counted in 16-bit samples: the dY tile of 16 channels with a pitch of 8 (runs + 1), and the halo twice (x0 and
// the copy one sample to the left), its rows stride[2] phases of SP slots, SP the tile row and the farthest tap's slot
// shift rounded up to 8.  The cycle estimate has the form and the constants of plan()'s (32 cycles per MFMA, 3000 of
// exposed latency per unit, half a cycle per staged sample); they were measured for wgrad_direct_kernel, not for this
// kernel.  Among the candidates that fit 64 KiB, else among those that fit the 160 KiB budget.
bool plan_h16(const fc_desc& c, int cus, Geom& g) {
  double best = -1.0;
  bool best_shared = false;
  Geom b = g;
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
        for (int rx = 1; rx <= kWghMaxRX; rx *= 2) {
          const int txr = rx * kWghRun;
          const int t[3] = {std::min(tz, g.O[0]), std::min(ty, g.O[1]), std::min(txr, g.O[2])};
          if ((tz > 1 && tz / 2 >= g.O[0]) || (ty > 1 && ty / 2 >= g.O[1]) || (rx > 1 && txr / 2 >= g.O[2]))
            continue;      // (the same clipped tile as a smaller candidate)
          const int rows = t[0] * t[1], rows4 = (rows + 3) & ~3, runs = rows4 * rx;
          if (runs > kWghMaxRuns) continue;
          const int64_t sp = ((int64_t)txr + (int64_t)(g.k[2] - 1) * g.dil[2] / g.stride[2] + 7) & ~(int64_t)7;
          int64_t halo[3], ntiles = 1;
          for (int a = 0; a < 3; ++a) {
            halo[a] = (int64_t)(t[a] - 1) * g.stride[a] + (int64_t)(g.k[a] - 1) * g.dil[a] + 1;
            ntiles *= cdiv(g.O[a], t[a]);
          }
          halo[2] = sp * g.stride[2];
          if (halo[0] > kLdsBudget || halo[1] > kLdsBudget || halo[2] > kLdsBudget || halo[0] * halo[1] > kLdsBudget) continue;
          const int64_t hv = halo[0] * halo[1] * halo[2], dyp = (int64_t)kWghRun * (runs + 1);
          if (hv > kLdsBudget) continue;
          const int64_t off_dy = kWghHeadBytes + 4 * rows4, off_x0 = off_dy + 2 * kWgdRows * dyp;
          const int64_t off_x1 = off_x0 + 2 * cib * hv + 16, lds = off_x1 + 2 * cib * hv + 16;
          if (lds > kLdsBudget) continue;
          const bool shared = lds <= kLdsShared;
          if (best_shared && !shared) continue;
          const double cost = (double)nib * (double)ntiles * (32.0 * (runs / 4) * ct + 3000.0 + 0.5 * (cib * (double)hv + 16.0 * kWghRun * runs));
          if (best < 0 || (shared && !best_shared) || cost < best) {
            best = cost; best_shared = shared;
            b.cib = cib; b.nib = nib; b.ct = ct; b.P = rows * txr; b.P4 = runs * kWghRun; b.lds = lds;
            b.SP = (int)sp; b.RX = rx; b.rows = rows; b.rows4 = rows4; b.dyp = (int)dyp;
            b.off_dy = (int)off_dy; b.off_x0 = (int)off_x0; b.off_x1 = (int)off_x1;
            for (int a = 0; a < 3; ++a) { b.tile[a] = t[a]; b.ntile[a] = (int)cdiv(g.O[a], t[a]); b.halo[a] = (int)halo[a]; }
          }
        }
  }
  if (best < 0) return false;
  b.units = c.batch * b.ntile[0] * b.ntile[1] * b.ntile[2];
  const int64_t blocks = c.groups * b.nob * b.nib;
  if (b.units >= ((int64_t)1 << 31)) return false;
  int64_t slices = std::max<int64_t>(1, ((b.lds <= kLdsShared ? 2 : 1) * (int64_t)cus + blocks / 2) / blocks);
  if (const int64_t forced = forced_slices()) slices = forced;
  slices = std::min<int64_t>(slices, b.units);
  if (blocks * slices > 0x7fffffffLL) return false;
  b.slices = (int)slices;
  b.ws = slices * c.out_channels * b.Cig * b.taps * 4;
  b.body = BODY_H16;
  g = b;
  return true;
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
  const int knob = body_knob();
  g.body = g.Cig == 1 && knob != 1 && (knob == 2 || g.Cog <= kDwMaxMultiplier) ? BODY_VALU : BODY_MFMA;
  if (g.body == BODY_VALU) return plan_dw(c, cus, g);

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
  if (const int64_t forced = forced_slices()) slices = forced;
  slices = std::min<int64_t>(slices, g.units);
  if (blocks * slices > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_direct: %lld workgroups exceed the 2^31 of one launch", (long long)(blocks * slices));
  g.slices = (int)slices;
  g.ws = slices * c.out_channels * g.Cig * g.taps * 4;
  if (knob == 3 && (c.dtype == FC_F16 || c.dtype == FC_BF16)) plan_h16(c, cus, g);
  return FC_OK;
}

}  // namespace

extern "C" int fc_wgrad_direct_geometry(const fc_desc* conv_desc, int compute_units, int64_t info[8]) {
  if (!conv_desc || !info) return fail(FC_ERR_INVALID, "null argument");
  Geom g;
  if (int st = plan(*conv_desc, compute_units, g)) return st;
  for (int i = 0; i < 3; ++i) info[i] = i < conv_desc->ndim ? g.tile[g.ax0 + i] : 0;
  info[3] = g.body == BODY_VALU ? 1 : std::min(g.Cog, kWgdRows); info[4] = g.cib; info[5] = g.slices; info[6] = g.lds; info[7] = g.ws;
  return FC_OK;
}

extern "C" int fc_wgrad_direct_body(const fc_desc* conv_desc, int compute_units, int* body) {
  if (!conv_desc || !body) return fail(FC_ERR_INVALID, "null argument");
  Geom g;
  if (int st = plan(*conv_desc, compute_units, g)) return st;
  *body = g.body;
  return FC_OK;
}

extern "C" int fc_wgrad_direct(const fc_desc* conv_desc, const void* x, const void* dy, float* dw, void* workspace,
                               void* hip_stream) {
  if (!conv_desc || !x || !dy || !dw || !workspace) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // (as fc_forward: a stale sticky error of an earlier call is not this call's)
  int cus = 0;
  if (!current_device_cus(&cus) || cus < 1) return fail(FC_ERR_HIP, "the CU count of the current device is not available");
  // the plan of the last call of this thread, while descriptor, CU count and the knob are what they were
  struct Last { fc_desc d; int cus; long long knob; int body; Geom g; bool set; };
  static thread_local Last last = {};
  const long long knob = forced_slices();
  const int body = body_knob();
  if (!last.set || std::memcmp(&last.d, conv_desc, sizeof(fc_desc)) || last.cus != cus || last.knob != knob || last.body != body) {
    last.set = false;
    if (int st = plan(*conv_desc, cus, last.g)) return st;
    last.d = *conv_desc; last.cus = cus; last.knob = knob; last.body = body; last.set = true;
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
  if (g.body == BODY_H16) {
    WgradH16Args h;
    std::memset(&h, 0, sizeof h);
    h.x = x; h.dy = dy; h.partial = a.partial;
    for (int i = 0; i < 3; ++i) {
      h.map[i] = a.map[i];
      h.S[i] = g.S[i]; h.O[i] = g.O[i]; h.k[i] = g.k[i]; h.stride[i] = g.stride[i]; h.dil[i] = g.dil[i];
      h.tile[i] = g.tile[i]; h.ntile[i] = g.ntile[i]; h.halo[i] = g.halo[i];
    }
    h.SP = g.SP; h.RX = g.RX; h.rows = g.rows; h.rows4 = g.rows4; h.dyp = g.dyp;
    h.fd_ty = make_fastdiv(g.tile[1]); h.fd_rx = make_fastdiv(g.RX); h.fd_runs = make_fastdiv(g.rows4 * g.RX);
    h.fd_sp2 = make_fastdiv(g.SP / 2); h.fd_s = make_fastdiv(g.stride[2]);
    h.fd_hy = make_fastdiv(g.halo[1]); h.fd_hz = make_fastdiv(g.halo[0]);
    h.Cin = a.Cin; h.Cout = a.Cout; h.Cig = g.Cig; h.Cog = g.Cog; h.taps = g.taps;
    h.cib = g.cib; h.nib = g.nib; h.nob = g.nob; h.slices = g.slices; h.units = (int)g.units;
    h.off_dy = g.off_dy; h.off_x0 = g.off_x0; h.off_x1 = g.off_x1; h.io = c.dtype;
    FC_HIP(wgrad_direct_h16_launch(h, g.ct, c.groups * g.nob * g.nib * g.slices, (size_t)g.lds, st));
  } else if (g.body == BODY_VALU) {
    a.fd_rx = make_fastdiv(g.runs / (g.tile[0] * g.tile[1]));
    a.runs = g.runs; a.runs64 = g.runs64; a.nbx = g.nbx; a.nblk = g.nblk;
    FC_HIP(wgrad_direct_dw_launch(a, g.kxb, g.nb, c.out_channels * g.slices, (size_t)g.lds, st));
  } else {
    FC_HIP(wgrad_direct_launch(a, g.ct, c.groups * g.nob * g.nib * g.slices, (size_t)g.lds, st));
  }
  FC_HIP(wgrad_direct_sum_launch(a.partial, dw, (long long)c.out_channels * g.Cig * g.taps, g.slices, st));
  return FC_OK;
}
