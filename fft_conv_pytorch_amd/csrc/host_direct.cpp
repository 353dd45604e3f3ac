// host_direct.cpp -- fc_conv_direct_geometry and fc_conv_direct (include/fftconv_amd.h "Direct forward"): the planner of
// conv_direct_kernel (conv_direct.hpp) and its launch; fc_conv_direct_dw_geometry and fc_conv_direct_dw ("Direct
// depthwise forward"): those of conv_direct_dw_kernel (conv_direct_dw.hpp), and fc_conv_direct_h16_geometry and
// fc_conv_direct_h16 ("Direct forward on the 16-bit matrix instructions"): those of conv_direct_h16_kernel
// (conv_direct_h16.hpp), behind the same validation; fc_conv_direct_tr_geometry and fc_conv_direct_tr ("Direct strided
// transposed convolution"): those of conv_direct_tr_kernel (conv_direct_tr.hpp), validation extended, and
// fc_conv_direct_tr_h16_geometry and fc_conv_direct_tr_h16 ("... on the 16-bit matrix instructions"): those of
// conv_direct_tr_h16_kernel (conv_direct_tr_h16.hpp).  The planners
// are pure arithmetic on the descriptor and the CU count; a launch call plans again for the current device (the last
// answer is remembered per thread), allocates nothing and synchronises nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "conv_direct.hpp"
#include "conv_direct_dw.hpp"
#include "conv_direct_h16.hpp"
#include "conv_direct_tr.hpp"
#include "conv_direct_tr_h16.hpp"
#include "fc_plan.h"

using namespace fc;

namespace {

constexpr int64_t kLdsShared = 64 * 1024;       // up to here two workgroups share a CU
constexpr int64_t kLdsBudget = 160 * 1024;
constexpr int kMaxTaps = 128;
constexpr int kDepthwiseMaxMultiplier = 8;      // Cin/g == 1 and Cout/g up to here: of the layer's weight: refused

struct Geom {
  int ax0;                   // first axis of the descriptor in the kernel's (z, y, x): 1 for a 2-D layer
  int O[3], S[3], k[3], stride[3], dil[3], pad[3];
  int tile[3], ntile[3], halo[3];
  int Cig, Cog, taps, cib, nib, nob, npt, steps, P;
  int64_t units, lds;
  // the depthwise kernel (plan_dw); there halo[2] is the padded pitch of a halo row
  int m, slots, nr;          // channel multiplier, multiplier slots and runs per thread of the build
  int kxb, nbx, kxp, wp, wl; // taps per block, blocks per kernel row, floats per staged tap row / channel / group
  int runs;                  // runs of kDwR positions per tile
};

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The descriptor of a layer either direct forward covers, into g: extents, taps and channels per group.  `who` names the
// entry point in the refusals, `why_taps` ends the one of a kernel past 128 taps.  `by_phases` (plan_tr): a transposed
// descriptor may have any stride up to 8, an output padding and any padding that leaves an output; g.pad is then the
// descriptor's padding and g.O the extent of the transposed convolution.
int validate(const fc_desc& c, int cus, const char* who, const char* why_taps, Geom& g, bool by_phases = false) {
  if (c.ndim == 1) return fail(FC_ERR_UNSUPPORTED, "%s covers 2-D and 3-D convolutions (no 1-D)", who);
  if (c.ndim < 1 || c.ndim > 3) return fail(FC_ERR_INVALID, "ndim must be 1, 2 or 3 (got %d)", c.ndim);
  if (c.dtype == FC_F64 || c.dtype == FC_C64)
    return fail(FC_ERR_UNSUPPORTED, "%s takes float32, float16 or bfloat16 tensors (no %s)", who,
                c.dtype == FC_F64 ? "float64" : "complex64");
  if (c.dtype != FC_F32 && c.dtype != FC_F16 && c.dtype != FC_BF16) return fail(FC_ERR_INVALID, "unknown dtype %d", c.dtype);
  if (c.batch < 1 || c.in_channels < 1 || c.out_channels < 1 || c.groups < 1 || c.in_channels % c.groups || c.out_channels % c.groups)
    return fail(FC_ERR_INVALID, "batch, channels and groups must be positive and the channels divisible by groups");
  if (c.padding_mode < 0 || c.padding_mode > 3) return fail(FC_ERR_INVALID, "unknown padding_mode %d", c.padding_mode);
  if (c.transposed && c.padding_mode != FC_PAD_CONSTANT) return fail(FC_ERR_INVALID, "a transposed convolution pads with zeros");
  if (cus < 1) return fail(FC_ERR_INVALID, "compute_units must be positive (got %d)", cus);
  g.ax0 = 3 - c.ndim;
  for (int a = 0; a < 3; ++a) { g.O[a] = g.S[a] = g.k[a] = g.stride[a] = g.dil[a] = 1; g.pad[a] = 0; }
  int64_t taps = 1, xs = c.batch * c.in_channels, ys = c.batch * c.out_channels;
  for (int i = 0; i < c.ndim; ++i) {
    const int a = g.ax0 + i;
    if (c.spatial[i] < 1 || c.kernel[i] < 1 || c.stride[i] < 1 || c.dilation[i] < 1 || c.padding[i] < 0)
      return fail(FC_ERR_INVALID, "axis %d: spatial/kernel/stride/dilation must be >= 1 and padding >= 0", i);
    if (c.kernel[i] > kMaxTaps || c.dilation[i] >= (1 << 20) || c.stride[i] >= (1 << 20))
      return fail(FC_ERR_UNSUPPORTED, "axis %d: %s covers kernels of at most %d taps in all", i, who, kMaxTaps);
    int64_t pad = c.padding[i];
    if (c.transposed && by_phases) {
      if (c.stride[i] > kCdtMaxStride)
        return fail(FC_ERR_UNSUPPORTED, "axis %d: %s covers a stride of at most %d (got %lld)", i, who, kCdtMaxStride,
                    (long long)c.stride[i]);
      if (c.output_padding[i] < 0 || c.output_padding[i] >= std::max(c.stride[i], c.dilation[i]))
        return fail(FC_ERR_INVALID, "axis %d: output_padding must be >= 0 and smaller than stride or dilation", i);
      if (c.spatial[i] >= (1 << 26) || pad >= ((int64_t)1 << 30))
        return fail(FC_ERR_UNSUPPORTED, "axis %d: extent %lld times the stride exceeds 32-bit positions", i, (long long)c.spatial[i]);
      const int64_t out = (c.spatial[i] - 1) * c.stride[i] - 2 * pad + (c.kernel[i] - 1) * c.dilation[i] + c.output_padding[i] + 1;
      if (out < 1) return fail(FC_ERR_INVALID, "axis %d: the padding %lld leaves no output sample", i, (long long)pad);
      if (out >= ((int64_t)1 << 30))
        return fail(FC_ERR_UNSUPPORTED, "axis %d: output extent %lld exceeds 32-bit positions", i, (long long)out);
      g.S[a] = (int)c.spatial[i]; g.O[a] = (int)out; g.k[a] = (int)c.kernel[i];
      g.stride[a] = (int)c.stride[i]; g.dil[a] = (int)c.dilation[i]; g.pad[a] = (int)pad;
      taps *= c.kernel[i];
      xs *= c.spatial[i]; ys *= out;
      if (xs >= ((int64_t)1 << 40) || ys >= ((int64_t)1 << 40))
        return fail(FC_ERR_UNSUPPORTED, "%s indexes x and y in 64 bits but takes fewer than 2^40 samples each", who);
      continue;
    }
    if (c.transposed) {
      // the stride-1 transposed convolution is the forward one with the taps flipped and a padding of d * (k - 1) - p
      if (c.stride[i] != 1)
        return fail(FC_ERR_UNSUPPORTED, "axis %d: %s runs a transposed convolution at stride 1 only (got stride %lld)", i, who,
                    (long long)c.stride[i]);
      if (c.output_padding[i] != 0)
        return fail(FC_ERR_UNSUPPORTED, "axis %d: %s runs a transposed convolution without output padding", i, who);
      pad = (c.kernel[i] - 1) * c.dilation[i] - c.padding[i];
      if (pad < 0)
        return fail(FC_ERR_UNSUPPORTED, "axis %d: the padding %lld of a transposed convolution exceeds d * (k - 1) = %lld: a crop, "
                    "which %s does not run", i, (long long)c.padding[i], (long long)((c.kernel[i] - 1) * c.dilation[i]), who);
    }
    if (c.spatial[i] + 2 * pad >= ((int64_t)1 << 31))
      return fail(FC_ERR_UNSUPPORTED, "axis %d: padded extent %lld exceeds 32-bit positions (must be < 2^31 samples)", i,
                  (long long)(c.spatial[i] + 2 * pad));
    const int64_t kd = (c.kernel[i] - 1) * c.dilation[i] + 1, span = c.spatial[i] + 2 * pad - kd;
    if (span < 0) return fail(FC_ERR_INVALID, "axis %d: dilated kernel extent %lld is larger than the padded input", i, (long long)kd);
    if (c.padding_mode == FC_PAD_REFLECT && pad >= c.spatial[i])
      return fail(FC_ERR_INVALID, "axis %d: reflect padding (%lld) must be smaller than the input size (%lld)", i, (long long)pad,
                  (long long)c.spatial[i]);
    if (c.padding_mode == FC_PAD_CIRCULAR && pad > c.spatial[i])
      return fail(FC_ERR_INVALID, "axis %d: circular padding (%lld) must not exceed the input size (%lld)", i, (long long)pad,
                  (long long)c.spatial[i]);
    g.S[a] = (int)c.spatial[i]; g.O[a] = (int)(span / c.stride[i] + 1); g.k[a] = (int)c.kernel[i];
    g.stride[a] = (int)c.stride[i]; g.dil[a] = (int)c.dilation[i]; g.pad[a] = (int)pad;
    taps *= c.kernel[i];
    xs *= c.spatial[i]; ys *= g.O[a];
    if (xs >= ((int64_t)1 << 40) || ys >= ((int64_t)1 << 40))
      return fail(FC_ERR_UNSUPPORTED, "%s indexes x and y in 64 bits but takes fewer than 2^40 samples each", who);
  }
  if (taps > kMaxTaps)
    return fail(FC_ERR_UNSUPPORTED, "%s covers kernels of at most %d taps in all (got %lld): %s", who, kMaxTaps, (long long)taps, why_taps);
  g.taps = (int)taps;
  g.Cig = (int)(c.in_channels / c.groups); g.Cog = (int)(c.out_channels / c.groups);
  if (c.in_channels >= (1 << 30) || c.out_channels >= (1 << 30)) return fail(FC_ERR_UNSUPPORTED, "%s: fewer than 2^30 channels", who);
  return FC_OK;
}

// Validates the descriptor and chooses input-channel block and tile.  Both minimise a cycle estimate of the whole
// launch: per workgroup and input-channel block the MFMAs of a wave (steps x NPT instructions x 32 cycles), a fixed
// cost for the exposed latency of its loads, and half a cycle per staged sample; among the candidates of which two
// workgroups share a CU (64 KiB of LDS, fewer than 16 position tiles per wave), else among those that fit the 160 KiB budget.  (The constants are those of the weight gradient's planner,
// host_wgrad.cpp; DESIGN 4.5d says what the benchmark showed of them.)
int plan(const fc_desc& c, int cus, Geom& g) {
  static_assert(kCdMaxCols == 512, "the text below");
  if (int st = validate(c, cus, "fc_conv_direct", "a block of 512 columns holds whole input channels", g)) return st;
  g.nob = (int)cdiv(g.Cog, kCdRows);

  // candidates: the largest channel blocks of the first 8 even splits of the group, tiles of powers of two clipped to the output
  double best = -1.0;
  bool best_shared = false;
  const int cibmax = std::min<int>(g.Cig, kCdMaxCols / g.taps);
  int last_cib = 0, tried = 0;
  for (int n = (int)cdiv(g.Cig, cibmax); n <= g.Cig && tried < 8; ++n) {
    const int cib = (int)cdiv(g.Cig, n);
    if (cib == last_cib) continue;
    last_cib = cib; ++tried;
    const int nib = (int)cdiv(g.Cig, cib), steps = (int)cdiv(cib * g.taps, 4);
    for (int tz = 1; tz <= 8; tz *= 2)
      for (int ty = 1; ty <= 16; ty *= 2)
        for (int tx = 1; tx <= 64; tx *= 2) {
          const int t[3] = {std::min(tz, g.O[0]), std::min(ty, g.O[1]), std::min(tx, g.O[2])};
          if ((tz > 1 && t[0] < tz && tz / 2 >= g.O[0]) || (ty > 1 && t[1] < ty && ty / 2 >= g.O[1]) ||
              (tx > 1 && t[2] < tx && tx / 2 >= g.O[2]))
            continue;      // (the same clipped tile as a smaller candidate)
          const int P = t[0] * t[1] * t[2];
          if (P > kCdMaxPos) continue;
          int npt = 1;
          while (kCdWaves * npt * 16 < P) npt *= 2;
          int64_t hv = 1, ntiles = 1;
          for (int a = 0; a < 3; ++a) {
            hv *= (int64_t)(t[a] - 1) * g.stride[a] + (int64_t)(g.k[a] - 1) * g.dil[a] + 1;
            ntiles *= cdiv(g.O[a], t[a]);
            if (hv > kLdsBudget) break;
          }
          if (hv > kLdsBudget) continue;
          const int64_t lds = 4 * ((int64_t)steps * (kCdWPitch + 4) + cib * hv);
          if (lds > kLdsBudget) continue;
          const bool shared = lds <= kLdsShared && npt < kCdMaxPT;      // (the build of 16 tiles per wave: 312 VGPRs, one workgroup per CU)
          if (best_shared && !shared) continue;
          const double cost = (double)nib * (double)ntiles * (32.0 * steps * npt + 3000.0 + 0.5 * (cib * (double)hv + 64.0 * steps));
          if (best < 0 || (shared && !best_shared) || cost < best) {
            best = cost; best_shared = shared;
            g.cib = cib; g.nib = nib; g.npt = npt; g.steps = steps; g.P = P; g.lds = lds;
            for (int a = 0; a < 3; ++a) {
              g.tile[a] = t[a]; g.ntile[a] = (int)cdiv(g.O[a], t[a]);
              g.halo[a] = (t[a] - 1) * g.stride[a] + (g.k[a] - 1) * g.dil[a] + 1;
            }
          }
        }
  }
  if (best < 0)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct: the x samples that one output position reaches through every tap do not "
                "fit %lld bytes of LDS", (long long)kLdsBudget);
  // (the layer whose weight this is: a transposed descriptor carries the weight of the layer it is the input gradient of)
  if ((c.transposed ? g.Cog : g.Cig) == 1 && (c.transposed ? g.Cig : g.Cog) <= kDepthwiseMaxMultiplier)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct does not run depthwise layers (a weight with one input channel per group and "
                "%d output channels per group: one live reduction column in four, at most 8 live rows in 16), forward or "
                "transposed; they keep the FFT plan", c.transposed ? g.Cig : g.Cog);
  g.units = c.batch * g.ntile[0] * g.ntile[1] * g.ntile[2];
  if (g.units >= ((int64_t)1 << 31))
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct: %lld (batch item, tile) units exceed 2^31", (long long)g.units);
  if (g.units * c.groups * g.nob > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct: %lld workgroups exceed the 2^31 of one launch", (long long)(g.units * c.groups * g.nob));
  return FC_OK;
}

// The planner of conv_direct_h16_kernel: plan() with input-channel blocks of whole cells of 8 channels, at most
// kH16MaxCols = 1024 (channel, tap) pairs each (the 16-bit halo is half the size, the first-level chain kH16MaxSteps = 32
// steps of 32 products), the same candidates, the same preference for two workgroups per CU and the same refusals,
// float32 tensors besides.  The cycle estimate keeps plan()'s shape and constants, 32 cycles per MFMA among them (the
// instruction itself is shorter, but its B operand is a KiB of LDS per wave): none of them is measured for this kernel.
int plan_h16(const fc_desc& c, int cus, Geom& g) {
  static_assert(kH16MaxCols == 1024 && kH16Cell == 8, "the text below");
  if (c.dtype == FC_F32 || c.dtype == FC_F64 || c.dtype == FC_C64)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_h16 takes float16 or bfloat16 tensors (no %s)",
                c.dtype == FC_F32 ? "float32: fc_conv_direct covers it" : c.dtype == FC_F64 ? "float64" : "complex64");
  if (int st = validate(c, cus, "fc_conv_direct_h16", "a block of 1024 columns holds whole cells of 8 input channels", g)) return st;
  g.nob = (int)cdiv(g.Cog, kCdRows);

  // candidates: the largest cell blocks of the first 8 even splits of the group's cells, tiles as plan()
  double best = -1.0;
  bool best_shared = false;
  const int cells = (int)cdiv(g.Cig, kH16Cell), cellmax = std::min<int>(cells, kH16MaxCols / kH16Cell / g.taps);
  int last_cb = 0, tried = 0;
  for (int n = (int)cdiv(cells, cellmax); n <= cells && tried < 8; ++n) {
    const int cb = (int)cdiv(cells, n);
    if (cb == last_cb) continue;
    last_cb = cb; ++tried;
    const int cib = cb * kH16Cell, nib = (int)cdiv(g.Cig, cib), steps = (int)cdiv(cb * g.taps, 4);
    for (int tz = 1; tz <= 8; tz *= 2)
      for (int ty = 1; ty <= 16; ty *= 2)
        for (int tx = 1; tx <= 64; tx *= 2) {
          const int t[3] = {std::min(tz, g.O[0]), std::min(ty, g.O[1]), std::min(tx, g.O[2])};
          if ((tz > 1 && t[0] < tz && tz / 2 >= g.O[0]) || (ty > 1 && t[1] < ty && ty / 2 >= g.O[1]) ||
              (tx > 1 && t[2] < tx && tx / 2 >= g.O[2]))
            continue;      // (the same clipped tile as a smaller candidate)
          const int P = t[0] * t[1] * t[2];
          if (P > kCdMaxPos) continue;
          int npt = 1;
          while (kCdWaves * npt * 16 < P) npt *= 2;
          int64_t hv = 1, ntiles = 1;
          for (int a = 0; a < 3; ++a) {
            hv *= (int64_t)(t[a] - 1) * g.stride[a] + (int64_t)(g.k[a] - 1) * g.dil[a] + 1;
            ntiles *= cdiv(g.O[a], t[a]);
            if (hv > kLdsBudget) break;
          }
          if (hv > kLdsBudget) continue;
          const int64_t lds = 16 * ((int64_t)steps * (kH16WPitch + 1) + cb * hv);      // wl, cbl (4 ints a step), xl
          if (lds > kLdsBudget) continue;
          const bool shared = lds <= kLdsShared && npt < kCdMaxPT;      // (the build of 16 tiles per wave: 316 VGPRs, one workgroup per CU)
          if (best_shared && !shared) continue;
          const double cost = (double)nib * (double)ntiles * (32.0 * steps * npt + 3000.0 + 0.5 * (cb * (double)hv + 64.0 * steps));
          if (best < 0 || (shared && !best_shared) || cost < best) {
            best = cost; best_shared = shared;
            g.cib = cib; g.nib = nib; g.npt = npt; g.steps = steps; g.P = P; g.lds = lds;
            for (int a = 0; a < 3; ++a) {
              g.tile[a] = t[a]; g.ntile[a] = (int)cdiv(g.O[a], t[a]);
              g.halo[a] = (t[a] - 1) * g.stride[a] + (g.k[a] - 1) * g.dil[a] + 1;
            }
          }
        }
  }
  if (best < 0)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_h16: the x samples that one output position reaches through every tap (of a "
                "cell of 8 channels) do not fit %lld bytes of LDS", (long long)kLdsBudget);
  if ((c.transposed ? g.Cog : g.Cig) == 1 && (c.transposed ? g.Cig : g.Cog) <= kDepthwiseMaxMultiplier)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_h16 does not run depthwise layers (a weight with one input channel per group "
                "and %d output channels per group), forward or transposed, as fc_conv_direct", c.transposed ? g.Cig : g.Cog);
  g.units = c.batch * g.ntile[0] * g.ntile[1] * g.ntile[2];
  if (g.units >= ((int64_t)1 << 31))
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_h16: %lld (batch item, tile) units exceed 2^31", (long long)g.units);
  if (g.units * c.groups * g.nob > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_h16: %lld workgroups exceed the 2^31 of one launch", (long long)(g.units * c.groups * g.nob));
  return FC_OK;
}

// The depthwise planner: the layer's weight must have one input channel per group and a multiplier of at most 8, the
// set plan() refuses.  Tiles are powers of two clipped to the output, at most 256 * NR runs of 4 outputs (NR: runs per
// thread of the build, 8 / multiplier slots).  The one with the smallest cycle estimate of the launch wins among those
// whose LDS lets two workgroups share a CU, else among those that fit: rounds of workgroups over 2 x CUs, times per
// workgroup the FMAs of a thread (4 cycles each), its 16-byte LDS reads (8 cycles each; the weights once per block, the
// window once per run), half a cycle per staged sample and a fixed cost for the exposed latency of the loads.
int plan_dw(const fc_desc& c, int cus, Geom& g) {
  if (int st = validate(c, cus, "fc_conv_direct_dw", "the sums of one output sample are one chain", g)) return st;
  const int wci = c.transposed ? g.Cog : g.Cig;      // (of the layer whose weight this is, as plan() reads it)
  g.m = c.transposed ? g.Cig : g.Cog;
  if (wci != 1)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_dw runs depthwise layers only: this weight has %d input channels per group, "
                "not one (fc_conv_direct covers it)", wci);
  if (g.m > kDepthwiseMaxMultiplier)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_dw runs channel multipliers of at most %d (got %d output channels per group; "
                "fc_conv_direct covers it)", kDepthwiseMaxMultiplier, g.m);
  g.slots = conv_direct_dw_slots(g.m, c.transposed);
  g.nr = kCdwAcc / g.slots;
  const bool unit = g.stride[2] == 1 && g.dil[2] == 1;      // else the general build, a tap per block
  g.kxb = !unit ? 1 : g.k[2] <= 4 ? 4 : 8;
  g.nbx = (int)cdiv(g.k[2], g.kxb); g.kxp = g.nbx * g.kxb; g.wp = g.k[0] * g.k[1] * g.kxp;
  g.wl = (std::max(g.slots, g.m) * g.wp + 3) & ~3;      // (a slot past m: staged zeros)
  const int nh = c.transposed ? g.m : 1, mlive = g.slots;      // staged halos; channels a block of taps feeds
  const int64_t groups = c.batch * c.groups;
  double best = -1.0;
  bool best_shared = false;
  for (int tz = 1; tz <= 8; tz *= 2)
    for (int ty = 1; ty <= 64; ty *= 2)
      for (int tx = kDwR; tx <= 128; tx *= 2) {
        const int t[3] = {std::min(tz, g.O[0]), std::min(ty, g.O[1]), std::min(tx, g.O[2])};
        if ((tz > 1 && tz / 2 >= g.O[0]) || (ty > 1 && ty / 2 >= g.O[1]) || (tx > kDwR && tx / 2 >= g.O[2]))
          continue;      // (the same clipped tile as a smaller candidate)
        const int txr = (t[2] + kDwR - 1) / kDwR * kDwR, runs = t[0] * t[1] * (txr / kDwR);
        if (runs > kCdwThreads * g.nr) continue;
        int64_t halo[3], ntiles = 1;
        for (int a = 0; a < 3; ++a) {
          halo[a] = (int64_t)(t[a] - 1) * g.stride[a] + (int64_t)(g.k[a] - 1) * g.dil[a] + 1;
          ntiles *= cdiv(g.O[a], t[a]);
        }
        // the row pitch: the window of the last run through the last tap block, dead tail included, in whole reads
        halo[2] = unit ? (txr - kDwR) + (g.nbx - 1) * g.kxb + 4 * dw_window4(g.kxb)
                       : (int64_t)(txr - 1) * g.stride[2] + (int64_t)(g.k[2] - 1) * g.dil[2] + 1;
        halo[2] = (halo[2] + 3) & ~(int64_t)3;
        if (halo[0] > kLdsBudget || halo[1] > kLdsBudget || halo[2] > kLdsBudget || halo[0] * halo[1] > kLdsBudget) continue;
        const int64_t hv = halo[0] * halo[1] * halo[2], lds = 4 * (g.wl + nh * hv);
        if (lds > kLdsBudget) continue;
        const bool shared = lds <= kLdsShared;
        if (best_shared && !shared) continue;
        const double rounds = (double)cdiv(runs, kCdwThreads), blocks = (double)nh * g.k[0] * g.k[1] * g.nbx;
        const double reads = unit ? dw_window4(g.kxb) : kDwR;
        const double work = blocks * (rounds * (4.0 * kDwR * g.kxb * mlive + 8.0 * reads) + 8.0 * mlive * std::max(1, g.kxb / 4));
        const double cost = (double)cdiv(groups * ntiles, 2 * (int64_t)cus) * (work + 3000.0 + 0.5 * (nh * (double)hv + g.wl));
        if (best < 0 || (shared && !best_shared) || cost < best) {
          best = cost; best_shared = shared;
          g.runs = runs; g.lds = lds;
          for (int a = 0; a < 3; ++a) { g.tile[a] = t[a]; g.ntile[a] = (int)cdiv(g.O[a], t[a]); g.halo[a] = (int)halo[a]; }
        }
      }
  if (best < 0)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_dw: the samples that one run of output positions reaches through every tap "
                "(of %d channels) do not fit %lld bytes of LDS", nh, (long long)kLdsBudget);
  g.units = c.batch * g.ntile[0] * g.ntile[1] * g.ntile[2];
  if (g.units >= ((int64_t)1 << 31))
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_dw: %lld (batch item, tile) units exceed 2^31", (long long)g.units);
  if (g.units * c.groups > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_dw: %lld workgroups exceed the 2^31 of one launch", (long long)(g.units * c.groups));
  return FC_OK;
}

// What plan_tr adds to a Geom (tile, ntile and halo of which are in the space of base positions q)
struct TrPlan {
  Geom g;
  int qlo[3], Q[3], M[3];
  int phases, ppp, ph, npass;      // prod(stride); live phases and phase slots of a pass; passes
  int k0[3][kCdtMaxStride], nk[3][kCdtMaxStride], m0[3][kCdtMaxStride], kstep[3], mstep[3];
  unsigned short soff[kCdtMaxPhases + 1];
};

// MFMA steps of the phases of a block of nc input channels (plan_tr_h16: nc cells of 8 channels; a column is then (cell,
// tap) and a step 32 products), each phase padded to whole steps: soff[f] is the first step of phase f (the last axis
// fastest), the return value soff[phases]
int tr_steps(const TrPlan& t, int nc, unsigned short* soff) {
  const int* s = t.g.stride;
  int total = 0, f = 0;
  for (int rz = 0; rz < s[0]; ++rz)
    for (int ry = 0; ry < s[1]; ++ry)
      for (int rx = 0; rx < s[2]; ++rx, ++f) {
        if (soff) soff[f] = (unsigned short)total;
        total += (int)cdiv((int64_t)nc * t.nk[0][rz] * t.nk[1][ry] * t.nk[2][rx], 4);
      }
  if (soff) soff[f] = (unsigned short)total;
  return total;
}

// The planner of conv_direct_tr_kernel: validate() in its by_phases form, the live taps of every phase, then plan()'s
// search with three changes.  The tiles are tiles of base positions q (t + p = s q + r), their halo is tile + M; the
// candidates carry the phase slots of a pass (2 .. 16, whole rows of last-axis phases) times the position tiles per wave
// (<= 16 together); and the cycle estimate counts the MFMAs over the live steps of all phases and the staging once per
// pass.  The constants are plan()'s, inherited: none of them is measured for this kernel.
//
// `h16`: the planner of conv_direct_tr_h16_kernel (plan_tr_h16).  The input-channel blocks are whole cells of 8 channels
// and a column is (cell, tap); the steps of a whole block are capped at kTrH16MaxSteps = 64, those of a pass being what
// a thread carries to the next block (a block of one cell may have more, up to (128 + 3 * 64) / 4 = 80, but a pass of at
// most 16 phases of it no more than (128 + 3 * 16) / 4 = 44); the LDS is plan_h16's, 16-byte cells at kH16WPitch, with
// cwl.  Same candidates, same refusals, float32 tensors besides.  The cycle estimate is unchanged, 32 cycles per MFMA
// among its constants, as plan_h16 keeps plan()'s: none of them is measured for this kernel either.
int plan_tr(const fc_desc& c, int cus, TrPlan& t, bool h16 = false) {
  static_assert(kCdMaxCols == 512 && kCdtMaxStride == 8 && kCdtMaxPhases == 64, "the text below");
  static_assert(kTrH16MaxSteps == 64 && kH16Cell == 8, "the text above and below");
  Geom& g = t.g;
  const char* who = h16 ? "fc_conv_direct_tr_h16" : "fc_conv_direct_tr";
  if (h16 && (c.dtype == FC_F32 || c.dtype == FC_F64 || c.dtype == FC_C64))
    return fail(FC_ERR_UNSUPPORTED, "fc_conv_direct_tr_h16 takes float16 or bfloat16 tensors (no %s)",
                c.dtype == FC_F32 ? "float32: fc_conv_direct_tr covers it" : c.dtype == FC_F64 ? "float64" : "complex64");
  if (int st = validate(c, cus, who, h16 ? "a block of 256 columns holds whole cells of 8 input channels"
                                         : "a block of 512 columns holds whole input channels", g, true)) return st;
  if (!c.transposed || (g.stride[0] == 1 && g.stride[1] == 1 && g.stride[2] == 1))
    return fail(FC_ERR_UNSUPPORTED, "%s runs transposed convolutions with a stride above 1 on some axis (this one "
                "is %s: fc_conv_direct covers it)", who, c.transposed ? "at stride 1" : "not transposed");
  t.phases = g.stride[0] * g.stride[1] * g.stride[2];
  if (t.phases > kCdtMaxPhases)
    return fail(FC_ERR_UNSUPPORTED, "%s covers at most %d phases (the product of the strides; got %d)", who, kCdtMaxPhases,
                t.phases);
  if (g.Cog == 1 && g.Cig <= kDepthwiseMaxMultiplier)
    return fail(FC_ERR_UNSUPPORTED, "%s does not run depthwise layers (a weight with one input channel per group and "
                "%d output channels per group), as fc_conv_direct; they keep the FFT plan", who, g.Cig);
  g.nob = (int)cdiv(g.Cog, kCdRows);
  for (int a = 0; a < 3; ++a) {
    const int s = g.stride[a], d = g.dil[a], k = g.k[a];
    t.qlo[a] = g.pad[a] / s; t.Q[a] = (g.O[a] - 1 + g.pad[a]) / s - t.qlo[a] + 1;
    t.M[a] = (int)((int64_t)(k - 1) * d / s);
    int gcd = s, v = d % s;
    while (v) { const int w = gcd % v; gcd = v; v = w; }
    t.kstep[a] = s / gcd; t.mstep[a] = d / gcd;
    for (int r = 0; r < kCdtMaxStride; ++r) {
      t.k0[a][r] = t.nk[a][r] = t.m0[a][r] = 0;
      if (r >= s) continue;
      int k0 = 0;
      while (k0 < t.kstep[a] && k0 < k && ((int64_t)k0 * d - r) % s) ++k0;
      if (k0 >= t.kstep[a] || k0 >= k) continue;      // (gcd(d, s) does not divide r, or the kernel ends before the first)
      t.k0[a][r] = k0; t.nk[a][r] = (k - 1 - k0) / t.kstep[a] + 1; t.m0[a][r] = (int)(((int64_t)k0 * d - r) / s);
    }
  }

  double best = -1.0;
  bool best_shared = false;
  // in units of a column's channels: one, or a cell of 8 (a ragged last cell counts whole)
  const int unit = h16 ? kH16Cell : 1, ncu = (int)cdiv(g.Cig, unit), maxsteps = h16 ? kTrH16MaxSteps : kCdMaxCols / 4;
  int cumax = std::min<int>(ncu, std::max(1, 4 * maxsteps / g.taps));
  while (cumax > 1 && tr_steps(t, cumax, nullptr) > maxsteps) --cumax;      // (one channel: at most 128 + 3 * 64 columns)
  const int sx = g.stride[2], rows = t.phases / sx;
  int last_cu = 0, tried = 0;
  for (int n = (int)cdiv(ncu, cumax); n <= ncu && tried < 8; ++n) {
    const int cu = (int)cdiv(ncu, n);
    if (cu == last_cu) continue;
    last_cu = cu; ++tried;
    const int cib = cu * unit, nib = (int)cdiv(g.Cig, cib), steps = tr_steps(t, cu, nullptr);
    for (int ph = 2; ph <= 16; ph *= 2) {
      if (ph < sx || (ph > 2 && ph / 2 >= sx && ph / 2 / sx >= rows)) continue;      // (no whole row; the slots of a smaller build)
      const int ppp = std::min(ph / sx, rows) * sx, npass = (int)cdiv(t.phases, ppp);
      for (int tz = 1; tz <= 8; tz *= 2)
        for (int ty = 1; ty <= 16; ty *= 2)
          for (int tx = 1; tx <= 64; tx *= 2) {
            const int q[3] = {std::min(tz, t.Q[0]), std::min(ty, t.Q[1]), std::min(tx, t.Q[2])};
            if ((tz > 1 && q[0] < tz && tz / 2 >= t.Q[0]) || (ty > 1 && q[1] < ty && ty / 2 >= t.Q[1]) ||
                (tx > 1 && q[2] < tx && tx / 2 >= t.Q[2]))
              continue;      // (the same clipped tile as a smaller candidate)
            const int P = q[0] * q[1] * q[2];
            int npt = 1;
            while (kCdWaves * npt * 16 < P) npt *= 2;
            if (ph * npt > kCdMaxPT) continue;
            int64_t hv = 1, ntiles = 1;
            for (int a = 0; a < 3; ++a) {
              hv *= (int64_t)q[a] + t.M[a];
              ntiles *= cdiv(t.Q[a], q[a]);
              if (hv > kLdsBudget) break;
            }
            if (hv > kLdsBudget) continue;
            const int64_t lds = h16 ? 16 * ((int64_t)steps * (kH16WPitch + 2) + cu * hv)      // wl, cbl and cwl (4 ints a step each), xl
                                    : 4 * ((int64_t)steps * (kCdWPitch + 8) + cib * hv);
            if (lds > kLdsBudget) continue;
            const bool shared = lds <= kLdsShared && ph * npt < kCdMaxPT;
            if (best_shared && !shared) continue;
            const double staged = nib > 1 ? (double)npass * cib * (double)hv : cib * (double)hv;      // (h16: a load per channel too)
            const double cost = (double)nib * (double)ntiles * (32.0 * steps * npt + 3000.0 * npass + 0.5 * (staged + 64.0 * steps));
            if (best < 0 || (shared && !best_shared) || cost < best) {
              best = cost; best_shared = shared;
              g.cib = cib; g.nib = nib; g.npt = npt; g.steps = steps; g.P = P; g.lds = lds;
              t.ph = ph; t.ppp = ppp; t.npass = npass;
              for (int a = 0; a < 3; ++a) { g.tile[a] = q[a]; g.ntile[a] = (int)cdiv(t.Q[a], q[a]); g.halo[a] = q[a] + t.M[a]; }
            }
          }
    }
  }
  if (best < 0)
    return fail(FC_ERR_UNSUPPORTED, "%s: the x samples that one base position reaches through every tap%s do not fit "
                "%lld bytes of LDS", who, h16 ? " (of a cell of 8 channels)" : "", (long long)kLdsBudget);
  tr_steps(t, g.cib / unit, t.soff);
  g.units = c.batch * g.ntile[0] * g.ntile[1] * g.ntile[2];
  if (g.units >= ((int64_t)1 << 31))
    return fail(FC_ERR_UNSUPPORTED, "%s: %lld (batch item, tile) units exceed 2^31", who, (long long)g.units);
  if (g.units * c.groups * g.nob > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "%s: %lld workgroups exceed the 2^31 of one launch", who, (long long)(g.units * c.groups * g.nob));
  return FC_OK;
}

int plan_tr_h16(const fc_desc& c, int cus, TrPlan& t) { return plan_tr(c, cus, t, true); }

// The kernel arguments of a plan()- or plan_h16()-planned launch (conv_direct_kernel and conv_direct_h16_kernel share the struct)
ConvDirectArgs direct_args(const fc_desc& c, const Geom& g, const void* x, const void* weight, const void* bias, void* y) {
  ConvDirectArgs a;
  std::memset(&a, 0, sizeof a);
  a.x = x; a.w = weight; a.bias = bias; a.y = y;
  for (int i = 0; i < 3; ++i) {
    a.map[i] = AxisMap{g.S[i], g.pad[i], c.padding_mode, 1};
    a.S[i] = g.S[i]; a.O[i] = g.O[i]; a.k[i] = g.k[i]; a.stride[i] = g.stride[i]; a.dil[i] = g.dil[i];
    a.tile[i] = g.tile[i]; a.ntile[i] = g.ntile[i]; a.halo[i] = g.halo[i];
  }
  a.fd_tx = make_fastdiv(g.tile[2]); a.fd_ty = make_fastdiv(g.tile[1]);
  a.fd_hx = make_fastdiv(g.halo[2]); a.fd_hy = make_fastdiv(g.halo[1]);
  a.Cin = (int)c.in_channels; a.Cout = (int)c.out_channels; a.Cig = g.Cig; a.Cog = g.Cog; a.G = (int)c.groups; a.taps = g.taps;
  a.cib = g.cib; a.nib = g.nib; a.nob = g.nob; a.P = g.P; a.steps = g.steps;
  a.io = c.dtype; a.transposed = c.transposed ? 1 : 0;
  return a;
}

// The kernel arguments of a plan_tr()- or plan_tr_h16()-planned launch (the two kernels share the struct)
ConvDirectTrArgs tr_args(const fc_desc& c, const TrPlan& t, const void* x, const void* weight, const void* bias, void* y) {
  const Geom& g = t.g;
  ConvDirectTrArgs a;
  std::memset(&a, 0, sizeof a);
  a.x = x; a.w = weight; a.bias = bias; a.y = y;
  for (int i = 0; i < 3; ++i) {
    a.S[i] = g.S[i]; a.O[i] = g.O[i]; a.k[i] = g.k[i]; a.up[i] = g.stride[i]; a.pad[i] = g.pad[i];
    a.qlo[i] = t.qlo[i]; a.Q[i] = t.Q[i]; a.M[i] = t.M[i];
    a.tile[i] = g.tile[i]; a.ntile[i] = g.ntile[i]; a.halo[i] = g.halo[i];
    a.kstep[i] = t.kstep[i]; a.mstep[i] = t.mstep[i];
  }
  std::memcpy(a.k0, t.k0, sizeof a.k0); std::memcpy(a.nk, t.nk, sizeof a.nk); std::memcpy(a.m0, t.m0, sizeof a.m0);
  std::memcpy(a.soff, t.soff, sizeof a.soff);
  a.fd_tx = make_fastdiv(g.tile[2]); a.fd_ty = make_fastdiv(g.tile[1]);
  a.fd_hx = make_fastdiv(g.halo[2]); a.fd_hy = make_fastdiv(g.halo[1]);
  a.Cin = (int)c.in_channels; a.Cout = (int)c.out_channels; a.Cig = g.Cig; a.Cog = g.Cog; a.G = (int)c.groups; a.taps = g.taps;
  a.cib = g.cib; a.nib = g.nib; a.nob = g.nob; a.P = g.P; a.steps = g.steps;
  a.phases = t.phases; a.ppp = t.ppp; a.npass = t.npass;
  a.io = c.dtype;
  return a;
}

}  // namespace

extern "C" int fc_conv_direct_geometry(const fc_desc* desc, int compute_units, int64_t info[8]) {
  if (!desc || !info) return fail(FC_ERR_INVALID, "null argument");
  Geom g;
  if (int st = plan(*desc, compute_units, g)) return st;
  for (int i = 0; i < 3; ++i) info[i] = i < desc->ndim ? g.tile[g.ax0 + i] : 0;
  info[3] = std::min(g.Cog, kCdRows); info[4] = g.cib; info[5] = g.nob; info[6] = g.nib; info[7] = g.lds;
  return FC_OK;
}

extern "C" int fc_conv_direct(const fc_desc* desc, const void* x, const void* weight, const void* bias, void* y, void* hip_stream) {
  if (!desc || !x || !weight || !y) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // (as fc_forward: a stale sticky error of an earlier call is not this call's)
  int cus = 0;
  if (!current_device_cus(&cus) || cus < 1) return fail(FC_ERR_HIP, "the CU count of the current device is not available");
  // the plan of the last call of this thread, while descriptor and CU count are what they were
  struct Last { fc_desc d; int cus; Geom g; bool set; };
  static thread_local Last last = {};
  if (!last.set || std::memcmp(&last.d, desc, sizeof(fc_desc)) || last.cus != cus) {
    last.set = false;
    if (int st = plan(*desc, cus, last.g)) return st;
    last.d = *desc; last.cus = cus; last.set = true;
  }
  const ConvDirectArgs a = direct_args(*desc, last.g, x, weight, bias, y);
  FC_HIP(conv_direct_launch(a, last.g.npt, last.g.units * desc->groups * last.g.nob, (size_t)last.g.lds,
                            static_cast<hipStream_t>(hip_stream)));
  return FC_OK;
}

extern "C" int fc_conv_direct_dw_geometry(const fc_desc* desc, int compute_units, int64_t info[8]) {
  if (!desc || !info) return fail(FC_ERR_INVALID, "null argument");
  Geom g;
  if (int st = plan_dw(*desc, compute_units, g)) return st;
  for (int i = 0; i < 3; ++i) info[i] = i < desc->ndim ? g.tile[g.ax0 + i] : 0;
  info[3] = g.kxb; info[4] = g.slots; info[5] = g.units * desc->groups; info[6] = g.lds; info[7] = g.nr;
  return FC_OK;
}

extern "C" int fc_conv_direct_dw(const fc_desc* desc, const void* x, const void* weight, const void* bias, void* y, void* hip_stream) {
  if (!desc || !x || !weight || !y) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // (as fc_forward: a stale sticky error of an earlier call is not this call's)
  int cus = 0;
  if (!current_device_cus(&cus) || cus < 1) return fail(FC_ERR_HIP, "the CU count of the current device is not available");
  // the plan of the last call of this thread, while descriptor and CU count are what they were
  struct Last { fc_desc d; int cus; Geom g; bool set; };
  static thread_local Last last = {};
  if (!last.set || std::memcmp(&last.d, desc, sizeof(fc_desc)) || last.cus != cus) {
    last.set = false;
    if (int st = plan_dw(*desc, cus, last.g)) return st;
    last.d = *desc; last.cus = cus; last.set = true;
  }
  const Geom& g = last.g;
  const fc_desc& c = *desc;
  ConvDirectDwArgs a;
  std::memset(&a, 0, sizeof a);
  a.x = x; a.w = weight; a.bias = bias; a.y = y;
  for (int i = 0; i < 3; ++i) {
    a.map[i] = AxisMap{g.S[i], g.pad[i], c.padding_mode, 1};
    a.S[i] = g.S[i]; a.O[i] = g.O[i]; a.k[i] = g.k[i]; a.stride[i] = g.stride[i]; a.dil[i] = g.dil[i];
    a.tile[i] = g.tile[i]; a.ntile[i] = g.ntile[i]; a.halo[i] = g.halo[i];
  }
  a.fd_hx = make_fastdiv(g.halo[2]); a.fd_hy = make_fastdiv(g.halo[1]);
  a.fd_rx = make_fastdiv((g.tile[2] + kDwR - 1) / kDwR); a.fd_ty = make_fastdiv(g.tile[1]);
  a.Cin = (int)c.in_channels; a.Cout = (int)c.out_channels; a.G = (int)c.groups; a.m = g.m; a.taps = g.taps;
  a.runs = g.runs; a.nbx = g.nbx; a.kxp = g.kxp; a.wp = g.wp; a.wl = g.wl;
  // a live run goes out as one access where every run of y starts on a multiple of 4 samples of a 16-byte aligned tensor
  a.vec = reinterpret_cast<uintptr_t>(y) % 16 == 0 && g.O[2] % kDwR == 0 && (g.tile[2] % kDwR == 0 || g.ntile[2] == 1);
  a.io = c.dtype;
  FC_HIP(conv_direct_dw_launch(a, g.kxb, c.transposed ? 1 : 0, g.units * c.groups, (size_t)g.lds, static_cast<hipStream_t>(hip_stream)));
  return FC_OK;
}

extern "C" int fc_conv_direct_h16_geometry(const fc_desc* desc, int compute_units, int64_t info[8]) {
  if (!desc || !info) return fail(FC_ERR_INVALID, "null argument");
  Geom g;
  if (int st = plan_h16(*desc, compute_units, g)) return st;
  for (int i = 0; i < 3; ++i) info[i] = i < desc->ndim ? g.tile[g.ax0 + i] : 0;
  info[3] = std::min(g.Cog, kCdRows); info[4] = std::min(g.cib, g.Cig); info[5] = g.nob; info[6] = g.nib; info[7] = g.lds;
  return FC_OK;
}

extern "C" int fc_conv_direct_h16(const fc_desc* desc, const void* x, const void* weight, const void* bias, void* y, void* hip_stream) {
  if (!desc || !x || !weight || !y) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // (as fc_forward: a stale sticky error of an earlier call is not this call's)
  int cus = 0;
  if (!current_device_cus(&cus) || cus < 1) return fail(FC_ERR_HIP, "the CU count of the current device is not available");
  // the plan of the last call of this thread, while descriptor and CU count are what they were
  struct Last { fc_desc d; int cus; Geom g; bool set; };
  static thread_local Last last = {};
  if (!last.set || std::memcmp(&last.d, desc, sizeof(fc_desc)) || last.cus != cus) {
    last.set = false;
    if (int st = plan_h16(*desc, cus, last.g)) return st;
    last.d = *desc; last.cus = cus; last.set = true;
  }
  const ConvDirectArgs a = direct_args(*desc, last.g, x, weight, bias, y);
  FC_HIP(conv_direct_h16_launch(a, last.g.npt, last.g.units * desc->groups * last.g.nob, (size_t)last.g.lds,
                                static_cast<hipStream_t>(hip_stream)));
  return FC_OK;
}

extern "C" int fc_conv_direct_tr_geometry(const fc_desc* desc, int compute_units, int64_t info[8]) {
  if (!desc || !info) return fail(FC_ERR_INVALID, "null argument");
  TrPlan t;
  if (int st = plan_tr(*desc, compute_units, t)) return st;
  for (int i = 0; i < 3; ++i) info[i] = i < desc->ndim ? t.g.tile[t.g.ax0 + i] : 0;
  info[3] = t.phases; info[4] = t.ppp; info[5] = t.g.cib; info[6] = t.g.nib; info[7] = t.g.lds;
  return FC_OK;
}

extern "C" int fc_conv_direct_tr(const fc_desc* desc, const void* x, const void* weight, const void* bias, void* y, void* hip_stream) {
  if (!desc || !x || !weight || !y) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // (as fc_forward: a stale sticky error of an earlier call is not this call's)
  int cus = 0;
  if (!current_device_cus(&cus) || cus < 1) return fail(FC_ERR_HIP, "the CU count of the current device is not available");
  // the plan of the last call of this thread, while descriptor and CU count are what they were
  struct Last { fc_desc d; int cus; TrPlan t; bool set; };
  static thread_local Last last = {};
  if (!last.set || std::memcmp(&last.d, desc, sizeof(fc_desc)) || last.cus != cus) {
    last.set = false;
    if (int st = plan_tr(*desc, cus, last.t)) return st;
    last.d = *desc; last.cus = cus; last.set = true;
  }
  const ConvDirectTrArgs a = tr_args(*desc, last.t, x, weight, bias, y);
  FC_HIP(conv_direct_tr_launch(a, last.t.ph, last.t.g.npt, last.t.g.units * desc->groups * last.t.g.nob, (size_t)last.t.g.lds,
                               static_cast<hipStream_t>(hip_stream)));
  return FC_OK;
}

extern "C" int fc_conv_direct_tr_h16_geometry(const fc_desc* desc, int compute_units, int64_t info[8]) {
  if (!desc || !info) return fail(FC_ERR_INVALID, "null argument");
  TrPlan t;
  if (int st = plan_tr_h16(*desc, compute_units, t)) return st;
  for (int i = 0; i < 3; ++i) info[i] = i < desc->ndim ? t.g.tile[t.g.ax0 + i] : 0;
  info[3] = t.phases; info[4] = t.ppp; info[5] = t.g.cib; info[6] = t.g.nib; info[7] = t.g.lds;
  return FC_OK;
}

extern "C" int fc_conv_direct_tr_h16(const fc_desc* desc, const void* x, const void* weight, const void* bias, void* y, void* hip_stream) {
  if (!desc || !x || !weight || !y) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // (as fc_forward: a stale sticky error of an earlier call is not this call's)
  int cus = 0;
  if (!current_device_cus(&cus) || cus < 1) return fail(FC_ERR_HIP, "the CU count of the current device is not available");
  // the plan of the last call of this thread, while descriptor and CU count are what they were
  struct Last { fc_desc d; int cus; TrPlan t; bool set; };
  static thread_local Last last = {};
  if (!last.set || std::memcmp(&last.d, desc, sizeof(fc_desc)) || last.cus != cus) {
    last.set = false;
    if (int st = plan_tr_h16(*desc, cus, last.t)) return st;
    last.d = *desc; last.cus = cus; last.set = true;
  }
  const ConvDirectTrArgs a = tr_args(*desc, last.t, x, weight, bias, y);
  FC_HIP(conv_direct_tr_h16_launch(a, last.t.ph, last.t.g.npt, last.t.g.units * desc->groups * last.t.g.nob, (size_t)last.t.g.lds,
                                   static_cast<hipStream_t>(hip_stream)));
  return FC_OK;
}
