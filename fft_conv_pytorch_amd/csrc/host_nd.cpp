// host_nd.cpp -- float32 2-D / 3-D plans (PlanKind::F32_ND): transforms of the rows and middle axes (full length or
// overlap-save tiles), the fused outermost-axis tile, the plane-major pipeline and the 2-D column pass (`planes`),
// workspace and spectrum sizes, kernels longer than a tile in segments of taps; the kernel transform and the forward of
// such a plan, the N-d weight gradient's image maps included (`swap`, fc_wgrad_nd).  A complex64 plan (PlanKind::C64_ND)
// is planned and launched here too: the same separable passes with the complex builds of the two row passes
// (nd_passes.hpp), Tx bin columns per x tile, 8-byte samples; no plane-major / row-major pipeline, no segments of taps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "fc_plan.h"

namespace fc {

static const fc::TileImpl* smallest_tile_at_least(int64_t n) {
  int ntl;
  auto tiles = all_tiles(&ntl);
  const fc::TileImpl* best = nullptr;
  for (int i = 0; i < ntl; ++i)
    if (tiles[i]->T >= n && (!best || tiles[i]->T < best->T)) best = tiles[i];
  return best;
}

// Transform of one axis of the row / middle-axis passes: the smallest FFT that holds the axis (`need` samples), else
// overlap-save tiles of T = 2048 or 4096 points.  `knob` (testing) forces tiles of that length where the kernel fits.
// A row just past a power of two ('same' padding on a power-of-two image: 518 samples -> a 1024-point transform, and
// twice the bin columns for every pass behind it) is cheaper in overlap-save tiles of a quarter of that length: the
// points per row decide (measured, scripts/experiments/sweep_same_xtile.py: B16 512^2 k7 'same' 499 us with one
// 1024-point transform, 281 us in 128-point tiles, 342 in 256-point ones; B8 1024^2 k5 1,209 / 537).  Taken when it
// saves at least 15 % of the points with at most max_tiles tiles; tiles keep at least half of themselves and are at
// least 64 long.
static int plan_axis_tiles(const fc_plan* p, int ax, const char* knob, int64_t max_tiles, const char* axis_name,
                           const fc::TileImpl** t_out, int* V_out, int* n_out) {
  *n_out = 1;
  *V_out = p->Lf[ax];
  *t_out = smallest_tile_at_least(p->need[ax]);
  const char* env = getenv(knob);
  const int64_t kd = p->kd[ax];
  int forced = env ? atoi(env) : 0;
  if (forced && (!find_tile(forced) || find_tile(forced)->T < kd)) forced = 0;
  if (!*t_out || forced) {
    const fc::TileImpl* t = forced ? find_tile(forced) : find_tile(kd <= 1025 ? 2048 : 4096);
    if (!t || t->T < kd)
      return fail(FC_ERR_UNSUPPORTED, "dilated kernel extent %lld along %s exceeds the largest FFT (4096)", (long long)kd, axis_name);
    *t_out = t;
    *V_out = (int)(t->T - kd + 1);
    *n_out = (int)((p->Lf[ax] + *V_out - 1) / *V_out);
  } else if (!env && !p->fnd.swap) {
    const int64_t single = (*t_out)->T;
    int64_t best_pts = single;
    const fc::TileImpl* best_t = nullptr;
    int ntl2;
    auto tl = all_tiles(&ntl2);
    for (int i = 0; i < ntl2; ++i) {
      const fc::TileImpl* t = tl[i];
      if (t->T < 64 || t->T >= single || t->T < 2 * kd) continue;
      const int64_t V = t->T - kd + 1, n = (p->Lf[ax] + V - 1) / V, pts = n * t->T;
      if (n <= max_tiles && pts * 100 <= single * 85 && pts < best_pts) { best_pts = pts; best_t = t; }
    }
    if (best_t) {
      *t_out = best_t;
      *V_out = (int)(best_t->T - kd + 1);
      *n_out = (int)((p->Lf[ax] + *V_out - 1) / *V_out);
    }
  }
  return FC_OK;
}

// Whether the fused (outermost-axis) pass can run tile t with this plan's channel chunk: the CB sequences (twice that with
// running sums over several input chunks) must fit 160 KiB of LDS.
static bool outer_tile_fits(const fc_plan* p, const fc::TileImpl* t, size_t* lds_out) {
  const size_t lds = (size_t)(p->accumulate ? 2 : 1) * p->CB * t->lseqp * sizeof(fc::f2);
  if (lds_out) *lds_out = lds;
  return p->CB <= t->fusedc_max_cib && lds <= 160 * 1024;
}

// Points-based cost of one pass over an axis of Lf stride-1 outputs against a dilated extent kd, with the padded axis
// (Lf + kd - 1) held whole: the row / middle-axis transforms (plan_axis_tiles without its sub-tile search) and the fused
// outer-axis tiles (the tile loop of plan_nd).  < 0 when no tile holds kd.
static double axis_cost(const fc_plan* p, int ax, int64_t kd, int64_t Lf) {
  const int64_t Sp = Lf + kd - 1;
  if (ax != 0) {
    const fc::TileImpl* t = smallest_tile_at_least(Sp);
    int64_t n = 1;
    if (!t) {
      t = find_tile(kd <= 1025 ? 2048 : 4096);
      if (!t || t->T < kd) return -1;
      n = (Lf + t->T - kd) / (t->T - kd + 1);
    }
    return (double)n * t->T * (2.0 * std::log2((double)t->T) + 4.0);
  }
  double best = -1;
  int ntl;
  auto tiles = all_tiles(&ntl);
  for (int i = 0; i < ntl; ++i) {
    const fc::TileImpl* t = tiles[i];
    size_t lds;
    if (t->T < kd || !outer_tile_fits(p, t, &lds)) continue;
    const int64_t nt = t->T >= Sp ? 1 : (Lf + t->T - kd) / (t->T - kd + 1);
    double cost = (double)nt * t->T * (2.0 * std::log2((double)t->T) + 4.0 + 2.0 * p->CB);
    if (lds > 80 * 1024) cost *= 1.25;
    if (best < 0 || cost < best) best = cost;
  }
  return best;
}

// Segments of taps.  An axis whose dilated extent no tile holds -- past 4096 along the rows / middle
// axes, past the largest tile the fused pass can run with this channel chunk along the outermost axis -- is cut into
// segments of C taps: segment j holds taps [j*C, min(k, (j+1)*C)), a convolution of dilated extent (C-1)*d + 1 with the
// same Lf stride-1 outputs that reads the padded axis from position j*C*d on (forward_nd adds the segments into y).  C
// minimises segments x (the axis' points-based cost over all rows of the problem + a fixed cost per segment): every
// segment runs the whole pipeline (4-6 launches of at least ~4 us each), and a small problem spent most of its time in
// them when only points counted (training step B2 3->4 16x8192 k3, dW: 33 segments of 256-point rows, 965 us per step;
// profiles/r05_nd_segments.txt).  The two constants are rough fits to those rows: ~2e6 cost units per us, 20 us per
// segment.  FFTCONV_NDSEG=<taps> (testing) forces segments of that many taps on every axis with more taps.  The plan's
// kd, Sp and need become those of one segment (no zero-wrap shortening).
static int plan_nd_segments(fc_plan* p) {
  const fc_desc& d = p->d;
  const char* env = getenv("FFTCONV_NDSEG");
  const int64_t forced = env ? atoll(env) : 0;
  long long total = 1;
  constexpr double kUnitsPerUs = 2e6, kSegmentUs = 20.0;
  for (int ax = 0; ax < p->nd; ++ax) {
    p->fnd.nseg[ax] = 1;
    p->fnd.seg_taps[ax] = (int)d.kernel[ax];
    int64_t limit = 4096;
    if (ax == 0) {
      limit = 0;
      int ntl;
      auto tiles = all_tiles(&ntl);
      for (int i = 0; i < ntl; ++i)
        if (outer_tile_fits(p, tiles[i], nullptr)) limit = std::max<int64_t>(limit, tiles[i]->T);
      if (!limit) continue;     // (refused by the tile loop)
    }
    const int64_t k = d.kernel[ax], dil = d.dilation[ax], Lf = p->Lf[ax];
    const int64_t cmax = (limit - 1) / dil + 1;       // most taps whose dilated extent fits
    int64_t C = 0;
    if (forced > 0 && k > forced && forced <= cmax) {
      C = forced;
    } else if (p->kd[ax] > limit) {
      // rows of the problem along this axis: images on both sides, padded extents of the other axes
      double rows = (double)d.batch * (double)(d.in_channels + d.out_channels);
      for (int b = 0; b < p->nd; ++b)
        if (b != ax) rows *= p->Sp[b];
      double best = 0;
      for (int64_t ns = (k + cmax - 1) / cmax; ns <= std::min<int64_t>(k, 64); ++ns) {
        const int64_t c = (k + ns - 1) / ns;
        if ((k + c - 1) / c != ns) continue;            // (the taps of a smaller count)
        const double cost = axis_cost(p, ax, (c - 1) * dil + 1, Lf);
        if (cost < 0) continue;
        const double us = (double)ns * (cost * rows / kUnitsPerUs + kSegmentUs);
        if (!C || us < best) { C = c; best = us; }
      }
      if (!C) C = cmax;                                 // (more than 64 segments: refused below)
    }
    if (!C) continue;
    p->fnd.nseg[ax] = (int)((k + C - 1) / C);
    p->fnd.seg_taps[ax] = (int)C;
    p->kd[ax] = (C - 1) * dil + 1;
    p->Sp[ax] = (int)(Lf + p->kd[ax] - 1);
    p->need[ax] = p->Sp[ax];
    total = std::min<long long>(total * p->fnd.nseg[ax], 1LL << 40);
  }
  if (total > 64)
    return fail(FC_ERR_UNSUPPORTED, "the kernel would run as %lld segments of taps (at most 64): kernel extents or "
                "dilations too large", total);
  p->fnd.nseg_total = (int)total;
  return FC_OK;
}

int plan_nd(fc_plan* p) {
  const fc_desc& d = p->d;
  const int nd = p->nd;
  const bool cplx = p->kind == PlanKind::C64_ND;
  int rc = plan_nd_segments(p);
  if (rc != FC_OK) return rc;
  const bool segmented = p->fnd.nseg_total > 1;
  if (cplx && segmented)
    return fail(FC_ERR_UNSUPPORTED, "a complex64 plan does not run its kernel in segments of taps (a dilated kernel extent past "
                "4096 on an axis, or FFTCONV_NDSEG): the accumulating store of the last pass is float32-only");
  // rows axis: one full-length transform when the padded row fits the largest FFT, overlap-save tiles otherwise
  // (the reference has no size limit: functional.py:66-70); middle axis (3-D): the same
  rc = plan_axis_tiles(p, nd - 1, "FFTCONV_XTILE", INT64_MAX, "the last axis", &p->fnd.tx, &p->fnd.Vx, &p->fnd.nxt);
  if (rc != FC_OK) return rc;
  // odd-frequency bins along the rows axis (nd_passes.hpp, rows_r2c); a complex row keeps all Tx bins (rows_c2c_fwd)
  p->fnd.Fx = cplx ? p->fnd.tx->T : p->fnd.tx->T / 2;
  p->fnd.Fxt = p->fnd.nxt * p->fnd.Fx;
  {
    // the row passes address one (bin column, row) block per workgroup with 32-bit byte offsets
    const int64_t rows = std::max<int64_t>(p->Sp[nd - 2], p->out_sp[nd - 2]);
    if ((int64_t)p->fnd.Fx * rows * 8 >= ((int64_t)1 << 31))
      return fail(FC_ERR_UNSUPPORTED, "%lld rows of %d-point transforms along the last axis exceed the 2 GiB a block of bin "
                  "columns may span (split the second-to-last axis)", (long long)rows, p->fnd.tx->T);
    // ... and the rows_c2r output stores a workgroup's (at most 32) output rows the same way (8-byte samples when complex)
    if (p->out_sp[nd - 1] * (cplx ? 8 : 4) * 32 >= ((int64_t)1 << 31))
      return fail(FC_ERR_UNSUPPORTED, "output rows of %lld samples exceed the 2 GiB a workgroup's block of rows may span "
                  "(2-D / 3-D plans; 1-D rows have no such limit)", (long long)p->out_sp[nd - 1]);
  }
  p->fnd.tm = nullptr;
  p->fnd.nyt = 1;
  p->fnd.Vy = nd == 3 ? p->Lf[1] : 0;
  if (nd == 3) {
    // (at most 8 tiles: one c2c launch per tile)
    rc = plan_axis_tiles(p, 1, "FFTCONV_YTILE", 8, "the middle axis", &p->fnd.tm, &p->fnd.Vy, &p->fnd.nyt);
    if (rc != FC_OK) return rc;
    if (p->fnd.nyt == 1) p->Sp[1] = std::min(p->Sp[1], p->fnd.tm->T);    // (rows past the transform are zero padding: not produced)
  }
  // 3-D planes larger than 64 x 64 after padding: cut into overlap-save tiles of 64 x 64 so that the plane-major pipeline
  // (below) still applies -- each tile is one workgroup of planes_fwd / planes_inv and one block of 2048 columns of colz.
  // Measured against the separable passes with the planner's own x / y tiles (profiles/r03_experiments.md block 12).
  if (nd == 3 && !getenv("FFTCONV_XTILE") && !getenv("FFTCONV_YTILE") && !p->fnd.swap && !d.tile_hint && !segmented && !cplx) {
    const char* pl = getenv("FFTCONV_PLANES");
    const fc::TileImpl* t64 = find_tile(64);
    const bool wide = p->fnd.tx->T > 64 || p->fnd.tm->T > 64 || p->fnd.nxt > 1 || p->fnd.nyt > 1;
    if ((!pl || atoi(pl) != 0) && t64 && t64->colz && wide && p->CB == 8 && !p->accumulate && p->kd[0] <= 33 && p->kd[1] <= 33 &&
        p->kd[2] <= 33) {
      const int64_t Vx = 64 - p->kd[2] + 1, Vy = 64 - p->kd[1] + 1;
      const int64_t nx = p->need[2] <= 64 ? 1 : (p->Lf[2] + Vx - 1) / Vx, ny = p->need[1] <= 64 ? 1 : (p->Lf[1] + Vy - 1) / Vy;
      // (taken while the tiles hold at most 1.5x the points of the separable plan's own transforms: at equal points the
      //  pipeline measured 1.3-2.0x faster -- 64^3 k3 'same' 663 -> 507 us, 128^3 k5 'same' 772 -> 455, 200^3 k5 1,571 -> 787 --
      //  at 2.25x, 128^3 k9 unpadded against single 128-point transforms, 14 % slower)
      const int64_t sep_pts = (int64_t)p->fnd.nxt * p->fnd.tx->T * p->fnd.nyt * p->fnd.tm->T;
      if (nx * ny <= 36 && nx * ny * 4096 * 2 <= sep_pts * 3) {
        p->fnd.tx = t64; p->fnd.tm = t64;
        p->fnd.nxt = (int)nx; p->fnd.Vx = nx == 1 ? p->Lf[2] : (int)Vx;
        p->fnd.nyt = (int)ny; p->fnd.Vy = ny == 1 ? p->Lf[1] : (int)Vy;
        p->fnd.Fx = 32; p->fnd.Fxt = p->fnd.nxt * p->fnd.Fx;
        if (p->fnd.nyt == 1) p->Sp[1] = std::min(p->Sp[1], 64);
      }
    }
  }
  // channel blocking of the fused (complex) pass: one sequence per channel
  p->fnd.cob = std::min(p->CB, p->Cog);
  p->fnd.Cog_pad = (int)round_up(p->Cog, p->fnd.cob);
  // Plane-major 3-D pipeline (planes3d.hpp): padded (y, x) planes within one 64 x 64 transform, 8-channel chunks with a
  // single input chunk, and a 64-point z tile (taken whenever the z kernel leaves at least half of it valid).
  // FFTCONV_PLANES=0 keeps the separable passes (A/B runs, tests).
  bool planes_ok = false;
  {
    const char* env = getenv("FFTCONV_PLANES");
    const fc::TileImpl* t64 = find_tile(64);
    planes_ok = (!env || atoi(env) != 0) && !p->fnd.swap && nd == 3 && t64 && t64->colz && p->fnd.tx->T == 64 && p->fnd.tm->T == 64 &&
                (int64_t)p->fnd.nxt * p->fnd.nyt <= 36 && (p->fnd.nxt == 1 || p->kd[2] <= 33) && (p->fnd.nyt == 1 || p->kd[1] <= 33) &&
                p->CB == 8 && !p->accumulate && p->kd[0] <= 33 && (!d.tile_hint || d.tile_hint == 64) &&
                (int64_t)2 * std::max(d.in_channels, d.out_channels) * std::max<int64_t>(p->Sp[0], p->out_sp[0]) * p->fnd.nxt * p->fnd.nyt < 65536;   // (32-bit offsets below 2 GiB per workgroup)
    // 2-D: the same column pass (one thread per 64-point sequence along y, lanes over neighbouring bin columns) between
    // row passes that keep the rows as they are -- taken under the same conditions on the y kernel and the channel blocks
    // Measured (scripts/experiments/time_rows2d.py, profiles/r03_experiments.md block 10): 5-13 % faster than the LDS column
    // pass on large images with y kernels up to ~25 taps (B16 512^2 k3..k23, B2 1024^2 k7), level at k31 (a 64-point tile then
    // keeps 34 samples), 8-10 % slower on small problems (B4 256^2) -- taken from 2^20 intermediate samples per channel and
    // 25 dilated taps down (33 where the LDS pass would need several tiles); FFTCONV_PLANES=2 takes it wherever it is possible (tests), 0 never.
    if (nd == 2) {
      const int knob = env ? atoi(env) : 1;
      // (26-33 taps: level with ONE 512-point tile of the LDS column pass -- cfgB -- but ahead of several of them:
      //  B16 512^2 k31 'same' 341 us against 439)
      const bool big = (int64_t)d.batch * p->Sp[0] * p->fnd.Fxt >= ((int64_t)1 << 20) && (p->kd[0] <= 25 || p->need[0] > 512);
      planes_ok = knob != 0 && (big || knob == 2) && !p->fnd.swap && t64 && t64->colz && p->CB == 8 && !p->accumulate &&
                  p->kd[0] <= 33 && (!d.tile_hint || d.tile_hint == 64) && p->fnd.Fx % 16 == 0 &&
                  (int64_t)4 * std::max(d.in_channels, d.out_channels) * std::max<int64_t>(p->Sp[0], p->out_sp[0]) * p->fnd.Fxt * 8 < ((int64_t)1 << 31);
    }
  }
  if (segmented || cplx) planes_ok = false;   // (segments and complex64 plans run the separable passes only)
  // overlap-save tiles along the outermost axis
  const int64_t Kd = p->kd[0], Lfull = p->Lf[0];
  const fc::TileImpl* best = nullptr;
  double best_cost = 0;
  int ntl;
  auto tiles = all_tiles(&ntl);
  for (int i = 0; i < ntl; ++i) {
    const fc::TileImpl* t = tiles[i];
    if (d.tile_hint && t->T != d.tile_hint) continue;
    if (planes_ok && t->T != 64) continue;
    size_t lds;
    if (t->T < Kd || !outer_tile_fits(p, t, &lds)) continue;
    const int64_t V = t->T - Kd + 1;
    const int64_t nt = t->T >= p->need[0] ? 1 : (Lfull + V - 1) / V;     // (one tile when the zero padding absorbs the wrap)
    double cost = (double)nt * t->T * (2.0 * std::log2((double)t->T) + 4.0 + 2.0 * p->CB);
    if (lds > 80 * 1024) cost *= 1.25;
    if (!best || cost < best_cost) { best = t; best_cost = cost; }
  }
  if (!best) {
    if (d.tile_hint) return fail(FC_ERR_INVALID, "tile_hint %d is not usable for this problem", d.tile_hint);
    return fail(FC_ERR_UNSUPPORTED, "no FFT tile fits the outermost axis (dilated kernel extent %lld, %d channels per chunk)",
                (long long)Kd, p->CB);
  }
  p->tile = best;
  if (best->T >= p->need[0]) {
    // the whole axis in one cyclic tile: every one of its Lfull outputs is kept, padded positions past the tile are zero
    p->V = (int)std::max<int64_t>(best->T - Kd + 1, Lfull);
    p->ntiles = 1;
    p->Sp[0] = std::min(p->Sp[0], best->T);
  } else {
    p->V = (int)(best->T - Kd + 1);
    p->ntiles = (int)((Lfull + p->V - 1) / p->V);
  }
  p->Lfull = (int)Lfull;

  const size_t B = (size_t)d.batch, Ci = (size_t)d.in_channels, Co = (size_t)d.out_channels;
  const size_t Fx = (size_t)p->fnd.Fx;          // bin columns of the kernel spectrum (one x tile)
  const size_t Fs = (size_t)p->fnd.Fxt;         // bin columns of the signal side (all x tiles)
  size_t ncol, a_sig, b_sig, a_w, b_w;
  if (nd == 2) {
    ncol = Fx;
    a_sig = B * Ci * Fs * p->Sp[0];                       // S1[(b,ci)][xt,fx][yp]
    b_sig = B * Co * Fs * (size_t)p->out_sp[0];           // O1[(b,co)][xt,fx][y_out]
    a_w = Co * p->Cig * Fx * (size_t)p->kd[0];            // S1w[(o,i)][fx][y<Kd]
    b_w = 0;
  } else {
    const size_t Ty = (size_t)p->fnd.tm->T, Tys = Ty * (size_t)p->fnd.nyt;  // kernel side / signal side (all middle-axis tiles)
    ncol = Fx * Ty;
    a_sig = std::max(B * Ci * p->Sp[0] * Fs * p->Sp[1],            // S1[(b,ci)][zp][xt,fx][yp]
                     B * Co * Fs * Tys * (size_t)p->out_sp[0]);     // O2[(b,co)][xt,fx][yt,fy][z_out]
    b_sig = std::max(B * Ci * Fs * Tys * p->Sp[0],                  // S2[(b,ci)][xt,fx][yt,fy][zp]
                     B * Co * (size_t)p->out_sp[0] * Fs * (size_t)p->out_sp[1]);   // O1[(b,co)][z_out][xt,fx][y_out]
    a_w = Co * p->Cig * (size_t)p->kd[0] * Fx * (size_t)p->kd[1];
    b_w = Co * p->Cig * Fx * Ty * (size_t)p->kd[0];
  }
  p->fnd.planes = (planes_ok && best->T == 64) ? (nd == 3 ? 1 : 2) : 0;
  if (p->fnd.planes == 1) {
    const size_t ntile = (size_t)p->fnd.nxt * p->fnd.nyt;
    a_sig = B * Ci * (size_t)p->Sp[0] * ntile * fc::kPlCols;              // S[(b,ci)][zp][tile][col]
    b_sig = B * Co * (size_t)p->out_sp[0] * ntile * fc::kPlCols;          // O[(b,co)][z_out][tile][col]
  }
  p->ws_a = std::max(a_sig, a_w);
  p->ws_b = std::max(b_sig, b_w);
  p->workspace_bytes = (p->ws_a + p->ws_b) * sizeof(fc::f2);
  p->fnd.seg_spectrum_bytes = (size_t)d.groups * p->fnd.Cog_pad * (p->Cig_pad / 2) * ncol * best->T * sizeof(fc::f4);
  p->spectrum_bytes = p->fnd.seg_spectrum_bytes * (size_t)p->fnd.nseg_total;   // (one spectrum per segment, in tensor order)
  rc = get_twiddles(best, &p->tw);
  if (rc == FC_OK) rc = get_twiddles(p->fnd.tx, &p->fnd.twx);
  if (rc == FC_OK && p->fnd.tm) rc = get_twiddles(p->fnd.tm, &p->fnd.twm);
  return rc;
}

// segment s of a segmented plan (tensor order) -> its index along every axis
static void segment_of(const fc_plan& p, int s, int j[3]) {
  j[0] = j[1] = j[2] = 0;
  for (int ax = p.nd - 1; ax >= 0; --ax) { j[ax] = s % p.fnd.nseg[ax]; s /= p.fnd.nseg[ax]; }
}

static int transform_kernel_nd_segment(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st,
                                       const int j[3]);

// kernel spectrum: the separable passes, fed from the dilated taps -- one spectrum per segment of taps
int transform_kernel_nd(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st) {
  // phantom channels (padding of the channel counts up to the chunk size) must read as zero; without any, every
  // entry of the spectrum is written by the passes below and the fill (6 us per call on a 2-D training step) is skipped
  if (p.Cig_pad != p.Cig || p.fnd.Cog_pad != p.Cog) FC_HIP(hipMemsetAsync(w_hat, 0, p.spectrum_bytes, st));
  for (int s = 0; s < p.fnd.nseg_total; ++s) {
    int j[3];
    segment_of(p, s, j);
    const int rc = transform_kernel_nd_segment(p, weight, (char*)w_hat + (size_t)s * p.fnd.seg_spectrum_bytes, workspace, st, j);
    if (rc != FC_OK) return rc;
  }
  return FC_OK;
}

static int transform_kernel_nd_segment(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st,
                                       const int j[3]) {
  fc::f2* wsA = (fc::f2*)workspace;
  fc::f2* wsB = wsA + p.ws_a;
  const int nd = p.nd;
  const int Co = (int)p.d.out_channels;
  fc::RowsR2CArgs r{};
  r.src = weight; r.dst = wsA; r.twA = p.fnd.twx.twA; r.twB = p.fnd.twx.twB; r.from_kernel = 1;
  r.kx = (int)p.d.kernel[nd - 1]; r.dx = (int)p.d.dilation[nd - 1];
  r.ky = (int)p.d.kernel[nd - 2]; r.dy = (int)p.d.dilation[nd - 2];
  r.kz = nd == 3 ? (int)p.d.kernel[0] : 1; r.dz = nd == 3 ? (int)p.d.dilation[0] : 1;
  r.NA = Co * p.Cig; r.NC = nd == 3 ? (int)p.kd[0] : 1; r.NY = (int)p.kd[nd - 2]; r.NYa = r.NY;
  r.SZ = r.kz; r.SY = r.ky; r.SX = r.kx; r.Fx = p.fnd.Fx;
  // segment j of an axis: taps [j*C, min(k, (j+1)*C)) (the source keeps its full extent SX / SY / SZ)
  const int zx = nd - 1, zy = nd - 2;
  auto seg_taps = [&](int ax) { return std::min(p.fnd.seg_taps[ax], (int)p.d.kernel[ax] - j[ax] * p.fnd.seg_taps[ax]); };
  if (!p.fnd.swap) {
    r.kx = seg_taps(zx); r.tox = j[zx] * p.fnd.seg_taps[zx];
    r.ky = seg_taps(zy); r.toy = j[zy] * p.fnd.seg_taps[zy];
    if (nd == 3) { r.kz = seg_taps(0); r.toz = j[0] * p.fnd.seg_taps[0]; }
  }
  r.nxt = 1; r.Vx = 0;                       // the kernel sits in the first x tile
  if (p.io == FC_C64) r.io = FC_C64;         // complex taps, conjugated as rows_c2c_fwd loads them
  r.transposed = p.d.transposed; r.Cig = p.Cig; r.Cog = p.Cog;
  if (p.fnd.swap) {   // "kernel" = the output gradient (B, g*Cog, *Lout), read as ((g, o), b): image o_all*B + b sits at b*(g*Cog) + o_all
    r.im.on = 1; r.im.n1 = 1; r.im.n2 = (int)p.fnd.sw_B; r.im.s0 = 1; r.im.s1 = 0; r.im.s2 = p.fnd.sw_g * p.fnd.sw_Cog;
    // a tensor as large as the signal: read it through the signal's index maps (taps spread by the dilation = a source
    // spread over a grid of that step, nothing in front), which have the unrolled zero-padding path the tap loop lacks
    r.from_kernel = 0;
    // (segment j of an axis: the taps [j*C, min(k, (j+1)*C)) moved to the front)
    auto tmap = [&](int ax, int64_t taps, int64_t dil) {
      const int C = ax >= 0 ? p.fnd.seg_taps[ax] : (int)taps, jj = ax >= 0 ? j[ax] : 0;
      fc::AxisMap m; m.size = (int)std::min<int64_t>(taps, (int64_t)(jj + 1) * C); m.pad = -(int)(jj * C * dil);
      m.mode = FC_PAD_CONSTANT; m.up = (int)dil; return m;
    };
    r.mx = tmap(zx, r.kx, r.dx); r.my = tmap(zy, r.ky, r.dy); r.mz = tmap(nd == 3 ? 0 : -1, r.kz, r.dz);
    r.io = p.io;                             // dY has the element type of x
    const unsigned long long bytes = (p.io == FC_F32 ? 4ull : 2ull) * (unsigned long long)r.NA * r.SZ * r.SY * r.SX;
    r.src_bytes = bytes < 0xFFFFFFFFull ? (unsigned)bytes : 0u;
  }
  FC_HIP(p.fnd.tx->rows_r2c(r, st));
  const float norm = 1.0f / ((float)p.fnd.tx->T * (float)p.tile->T * (nd == 3 ? (float)p.fnd.tm->T : 1.0f));
  fc::C2CArgs c{};
  c.Cig = p.Cig; c.Cog = p.Cog; c.Cig_pad = p.Cig_pad; c.Cog_pad = p.fnd.Cog_pad; c.scale = norm;
  c.NV = 0; c.stride = 1; c.noff = 0;
  if (nd == 2) {
    // S1w[(o,i)][fx][y<Kd] -> wspec[..][fx][fy]
    c.src = wsA; c.dst = (fc::f2*)w_hat; c.twA = p.tw.twA; c.twB = p.tw.twB;
    c.NA = Co * p.Cig; c.NC = 1; c.NB = p.fnd.Fx; c.NLEN = (int)p.kd[0];
    c.sa = (long long)p.fnd.Fx * r.NYa; c.sc = 0; c.sb = r.NYa; c.store_mode = 1;
    FC_HIP(p.tile->c2c_fwd(c, st));
  } else {
    const int Ty = p.fnd.tm->T, Kz = (int)p.kd[0];
    // S1w[(o,i)][z<Kdz][fx][y<Kdy] -> S2w[(o,i)][fx][fy][z<Kdz]
    c.src = wsA; c.dst = wsB; c.twA = p.fnd.twm.twA; c.twB = p.fnd.twm.twB;
    c.NA = Co * p.Cig; c.NC = p.fnd.Fx; c.NB = Kz; c.NLEN = (int)p.kd[1];
    c.sa = (long long)Kz * p.fnd.Fx * r.NYa; c.sb = (long long)p.fnd.Fx * r.NYa; c.sc = r.NYa;
    c.ta = (long long)p.fnd.Fx * Ty * Kz; c.tc = (long long)Ty * Kz; c.tf = Kz; c.store_mode = 0;
    FC_HIP(p.fnd.tm->c2c_fwd(c, st));
    // S2w[(o,i)][(fx,fy)][z<Kdz] -> wspec[..][(fx,fy)][fz]
    c.src = wsB; c.dst = (fc::f2*)w_hat; c.twA = p.tw.twA; c.twB = p.tw.twB;
    c.NC = 1; c.NB = p.fnd.Fx * Ty; c.NLEN = Kz;
    c.sa = (long long)p.fnd.Fx * Ty * Kz; c.sc = 0; c.sb = Kz; c.store_mode = 1;
    FC_HIP(p.tile->c2c_fwd(c, st));
  }
  return FC_OK;
}

// arguments of the thread-per-sequence column pass (planes3d.hpp colz): ncol signal-side bin columns per plane, hcol
// kernel-spectrum columns
static fc::ColZArgs colz_args(const fc_plan& p, const fc::f2* src, const void* w_hat, fc::f2* dst, int ncol, int hcol,
                              void* stamps) {
  fc::ColZArgs cz{};
  cz.src = src; cz.wspec = (const fc::f4*)w_hat; cz.dst = dst;
  cz.B = (int)p.d.batch; cz.Cin = (int)p.d.in_channels; cz.Cout = (int)p.d.out_channels; cz.G = (int)p.d.groups;
  cz.Cig = p.Cig; cz.Cog = p.Cog; cz.Cog_pad = p.fnd.Cog_pad;
  cz.cob = p.fnd.cob; cz.n_ochunks = p.fnd.Cog_pad / p.fnd.cob;
  cz.NZ = p.Sp[0]; cz.NZo = (int)p.out_sp[0];
  cz.V = p.V; cz.ntiles = p.ntiles; cz.Lfull = p.Lfull; cz.stride = p.ostride[0];
  cz.ncol = ncol; cz.hcol = hcol;
  cz.stamps = (unsigned long long*)stamps;        // profiling build of the column pass (scripts/phase_profile_nd.py)
  return cz;
}

// Channels-last tensors: the first and the last pass of a separable float32 / float16 / bfloat16 plan have
// builds that read the signal / write the output where element (b, ch, z, y, x) lies at ((((b*SZ + z)*SY + y)*SX + x)*C + ch).
// The layout never enters the plan: this only says whether this plan's launches can take it.
int plan_takes_layout_nd(const fc_plan& p, bool x_cl, bool y_cl) {
  if (!x_cl && !y_cl) return FC_OK;
  if (p.kind == PlanKind::C64_ND)
    return fail(FC_ERR_UNSUPPORTED, "a complex64 plan reads and writes contiguous (B, C, *spatial) tensors only: the complex row "
                "passes have no channels-last build");
  if (p.kind != PlanKind::F32_ND)
    return fail(FC_ERR_UNSUPPORTED, "channels-last tensors are taken by float32 / float16 / bfloat16 2-D and 3-D plans only "
                "(float64 plans and 1-D plans read and write contiguous tensors; 1-D rows: fc_long_forward_lay)");
  if (p.fnd.swap)
    return fail(FC_ERR_UNSUPPORTED, "a weight-gradient plan (fc_wgrad_nd_plan_create) reads x and dY and writes dW contiguous");
  if (p.fnd.nseg_total > 1)
    return fail(FC_ERR_UNSUPPORTED, "a plan that runs its kernel in %d segments of taps has no channels-last launch (the "
                "accumulating store of the last pass is contiguous-only)", p.fnd.nseg_total);
  if (p.fnd.planes == 1)
    return fail(FC_ERR_UNSUPPORTED, "the plane-major 3-D pipeline (planes_fwd / planes_inv) has no channels-last build");
  if (!p.fnd.tx->rows_cl_nch)
    return fail(FC_ERR_UNSUPPORTED, "the %d-point row transform has no channels-last build (its workgroups hold fewer than "
                "four sequences; 64 ... 1024 points have one)", p.fnd.tx->T);
  const int nd = p.nd;
  const int64_t es = p.io == FC_F32 ? 4 : 2;
  if (x_cl) {
    // rows_r2c_cl: byte offsets from the start of x (buffer loads over the whole tensor)
    int64_t bytes = es * p.d.batch * p.d.in_channels;
    for (int i = 0; i < nd; ++i) bytes *= p.d.spatial[i];
    if (bytes >= 0xFFFFFFFFLL)
      return fail(FC_ERR_UNSUPPORTED, "a channels-last signal of %lld bytes exceeds the 4 GiB its 32-bit offsets span", (long long)bytes);
  }
  if (y_cl) {
    // rows_c2r_cl: byte offsets from a workgroup's first output row over its (at most 16) rows, the x positions of an
    // overlap-save tile past the row's end included (they get bit 31 and must not wrap)
    const int64_t span = (16 * p.out_sp[nd - 1] + p.Lf[nd - 1] + 2 * 4096) * p.d.out_channels * es;
    if (span >= ((int64_t)1 << 31))
      return fail(FC_ERR_UNSUPPORTED, "channels-last output rows of %lld x %lld samples exceed the 2 GiB a workgroup's block of "
                  "rows may span", (long long)p.out_sp[nd - 1], (long long)p.d.out_channels);
  }
  return FC_OK;
}

int forward_nd(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
               hipStream_t st, void* stamps, bool x_cl, bool y_cl) {
  fc::f2* wsA = (fc::f2*)workspace;
  fc::f2* wsB = wsA + p.ws_a;
  const int nd = p.nd;
  const int B = (int)p.d.batch, Ci = (int)p.d.in_channels, Co = (int)p.d.out_channels;
  if (x_cl || y_cl) {
    const int rc = plan_takes_layout_nd(p, x_cl, y_cl);
    if (rc != FC_OK) return rc;
  }
  if (p.fnd.planes == 1) {
    // x (B,Ci,Z,Y,X) -> S[(b,ci)][zp][col] -> O[(b,co)][z_out][col] -> y; col = fx*64 + fy
    fc::PlaneFwdArgs f1{};
    f1.src = x; f1.dst = wsA; f1.twA = p.fnd.twx.twA; f1.twB = p.fnd.twx.twB; f1.io = p.io;
    f1.mx = axis_map(p, 2); f1.my = axis_map(p, 1); f1.mz = axis_map(p, 0);
    f1.SZ = (int)p.d.spatial[0]; f1.SY = (int)p.d.spatial[1]; f1.SX = (int)p.d.spatial[2]; f1.NZ = p.Sp[0];
    f1.nxt = p.fnd.nxt; f1.nyt = p.fnd.nyt; f1.Vx = p.fnd.Vx; f1.Vy = p.fnd.Vy;
    FC_HIP(p.tile->planes_fwd(f1, B * Ci, st));
    // (the tiles of a plane share the spectrum's 2048 columns)
    FC_HIP(p.tile->colz(colz_args(p, wsA, w_hat, wsB, fc::kPlCols * p.fnd.nxt * p.fnd.nyt, fc::kPlCols, stamps), st));
    fc::PlaneInvArgs f3{};
    f3.src = wsB; f3.dst = y; f3.bias = p.d.has_bias ? bias : nullptr; f3.twA = p.fnd.twx.twA; f3.twB = p.fnd.twx.twB; f3.io = p.io_y;
    f3.NZo = (int)p.out_sp[0]; f3.Cout = Co;
    f3.NVy = p.Lf[1]; f3.sy = p.ostride[1]; f3.Yo = (int)p.out_sp[1];
    f3.NVx = p.Lf[2]; f3.sx = p.ostride[2]; f3.Xo = (int)p.out_sp[2];
    f3.nxt = p.fnd.nxt; f3.nyt = p.fnd.nyt; f3.Vx = p.fnd.Vx; f3.Vy = p.fnd.Vy;
    FC_HIP(p.tile->planes_inv(f3, B * Co, st));
    return FC_OK;
  }
  fc::RowsR2CArgs r{};
  r.src = x; r.dst = wsA; r.twA = p.fnd.twx.twA; r.twB = p.fnd.twx.twB; r.from_kernel = 0; r.io = p.io;
  r.mx = axis_map(p, nd - 1); r.my = axis_map(p, nd - 2);
  // a one-plane padded z axis still goes through its map: a transposed plan can crop its only source plane away
  if (nd == 3) r.mz = axis_map(p, 0);
  else { r.mz.size = 1; r.mz.pad = 0; r.mz.mode = FC_PAD_CONSTANT; r.mz.up = 1; }
  r.kx = r.ky = r.kz = r.dx = r.dy = r.dz = 1; r.transposed = 0; r.Cig = p.Cig; r.Cog = p.Cog;
  r.NA = B * Ci; r.NC = nd == 3 ? p.Sp[0] : 1; r.NY = p.Sp[nd - 2]; r.NYa = r.NY;
  r.SZ = nd == 3 ? (int)p.d.spatial[0] : 1; r.SY = (int)p.d.spatial[nd - 2]; r.SX = (int)p.d.spatial[nd - 1]; r.Fx = p.fnd.Fx;
  r.nxt = p.fnd.nxt; r.Vx = p.fnd.Vx;
  const int Fs = p.fnd.Fxt;                       // signal-side bin columns per plane (all x tiles)
  {
    const unsigned long long es = p.io == FC_C64 ? 8ull : (p.io == FC_F32 ? 4ull : 2ull);
    const unsigned long long bytes = es * (unsigned long long)B * Ci * r.SZ * r.SY * r.SX;
    r.src_bytes = bytes < 0xFFFFFFFFull ? (unsigned)bytes : 0u;
  }
  r.rowmajor = p.fnd.planes == 2;
  if (x_cl) r.cl_C = Ci;
  const int64_t dil[3] = {p.d.dilation[0], p.d.dilation[1], p.d.dilation[2]};
  if (p.fnd.swap) {   // signal = x (B, g*Cig, *S) read as (i, (g, b)): image (i*g + gi)*B + b sits at b*(g*Cig) + gi*Cig + i
    r.im.on = 1; r.im.n1 = (int)p.fnd.sw_g; r.im.n2 = (int)p.fnd.sw_B; r.im.s0 = 1; r.im.s1 = p.fnd.sw_Cig; r.im.s2 = p.fnd.sw_g * p.fnd.sw_Cig;
  }
  fc::FusedCArgs f{};
  f.wspec = (const fc::f4*)w_hat; f.twA = p.tw.twA; f.twB = p.tw.twB;
  f.B = B; f.Cin = Ci; f.Cout = Co; f.G = (int)p.d.groups; f.Cig = p.Cig; f.Cog = p.Cog;
  f.Cig_pad = p.Cig_pad; f.Cog_pad = p.fnd.Cog_pad; f.cob = p.fnd.cob; f.n_ochunks = p.fnd.Cog_pad / p.fnd.cob;
  f.Kd = (int)p.kd[0]; f.V = p.V; f.ntiles = p.ntiles; f.Lfull = p.Lfull; f.NVo = (int)p.out_sp[0];
  f.stride = p.ostride[0]; f.accumulate = p.accumulate; f.NLEN = p.Sp[0];
  f.stamps = (unsigned long long*)stamps;

  fc::RowsC2RArgs o{};
  o.dst = y; o.bias = p.d.has_bias ? bias : nullptr; o.twA = p.fnd.twx.twA; o.twB = p.fnd.twx.twB; o.io = p.io_y;
  o.NA = B * Co; o.Fx = p.fnd.Fx; o.Cout = Co; o.nxt = p.fnd.nxt; o.Vx = p.fnd.Vx;
  f.wfx = p.fnd.Fx; f.wty = nd == 3 ? p.fnd.tm->T : 1; f.wrep = nd == 3 ? p.fnd.nyt : 1; f.wncol = f.wfx * f.wty;
  o.NV = p.Lf[nd - 1]; o.stride = p.ostride[nd - 1]; o.Xo = (int)p.out_sp[nd - 1];
  o.NY = (int)p.out_sp[nd - 2]; o.NYa = o.NY;
  if (y_cl) o.cl_C = Co;
  if (p.fnd.swap) {   // output (i, (g, o), *k) written as dW ((g, o), i, *k): image i*(g*Cog) + o_all goes to o_all*Cig + i
    o.im.on = 1; o.im.n1 = 1; o.im.n2 = (int)(p.fnd.sw_g * p.fnd.sw_Cog); o.im.s0 = 1; o.im.s1 = 0; o.im.s2 = p.fnd.sw_Cig;
  }

  // segments of taps: segment j of an axis reads the padded signal from j*C*dilation on, against its own spectrum; the
  // first stores y with the bias, the later ones add into it (an unsegmented plan runs this once, as segment 0)
  for (int s = 0; s < p.fnd.nseg_total; ++s) {
    int j[3];
    segment_of(p, s, j);
    auto shift = [&](int ax) { return (int)(j[ax] * p.fnd.seg_taps[ax] * dil[ax]); };
    r.shx = shift(nd - 1); r.shy = shift(nd - 2); r.shz = nd == 3 ? shift(0) : 0;
    f.wspec = (const fc::f4*)((const char*)w_hat + (size_t)s * p.fnd.seg_spectrum_bytes);
    o.accum = s > 0;
    if (s > 0) o.bias = nullptr;
    FC_HIP(p.fnd.tx->rows_r2c(r, st));

    if (nd == 2 && p.fnd.planes == 2) {
      // x (B,Ci,Y,X) -> S[(b,ci)][yp][fx] (rows_r2c above, rows as they are) -> O[(b,co)][y_out][fx] -> y
      // (all x tiles of the signal; they share the Tx/2 spectrum columns)
      FC_HIP(p.tile->colz(colz_args(p, wsA, w_hat, wsB, Fs, p.fnd.Fx, stamps), st));
      o.src = wsB; o.NC = 1; o.rowmajor = 1;
      FC_HIP(p.fnd.tx->rows_c2r(o, st));
    } else if (nd == 2) {
      f.src = wsA; f.dst = wsB; f.ncol = Fs;
      FC_HIP(p.tile->fusedc(p.CB, f, st));
      o.src = wsB; o.NC = 1;
      FC_HIP(p.fnd.tx->rows_c2r(o, st));
    } else {
      const int Ty = p.fnd.tm->T, Szp = p.Sp[0], Syp = p.Sp[1], Lzo = (int)p.out_sp[0], Lyo = (int)p.out_sp[1];
      fc::C2CArgs c{};
      c.scale = 1.f; c.store_mode = 0; c.twA = p.fnd.twm.twA; c.twB = p.fnd.twm.twB;
      // S1[(b,ci)][zp][fx][yp] -> S2[(b,ci)][fx][yt,fy][zp]   (one launch per middle-axis tile yt)
      const int nyt = p.fnd.nyt, Vy = p.fnd.Vy;
      const long long Tys = (long long)nyt * Ty;
      c.NA = B * Ci; c.NC = Fs; c.NB = Szp;
      c.sa = (long long)Szp * Fs * Syp; c.sb = (long long)Fs * Syp; c.sc = Syp;
      c.ta = (long long)Fs * Tys * Szp; c.tc = Tys * Szp; c.tf = Szp;
      c.NV = 0; c.stride = 1; c.noff = 0;
      for (int yt = 0; yt < nyt; ++yt) {
        c.src = wsA + (size_t)yt * Vy; c.dst = wsB + (size_t)yt * Ty * Szp;
        c.NLEN = std::min(Ty, Syp - yt * Vy);
        FC_HIP(p.fnd.tm->c2c_fwd(c, st));
      }
      f.src = wsB; f.dst = wsA; f.ncol = (int)(Fs * Tys);
      FC_HIP(p.tile->fusedc(p.CB, f, st));
      // O2[(b,co)][fx][yt,fy][z_out] -> O1[(b,co)][z_out][fx][y_out]
      c.NA = B * Co; c.NC = Fs; c.NB = Lzo;
      c.sa = (long long)Fs * Tys * Lzo; c.sc = Tys * Lzo; c.sb = Lzo;
      c.ta = (long long)Lzo * Fs * Lyo; c.tb = (long long)Fs * Lyo; c.tc = Lyo;
      c.stride = p.ostride[1];
      for (int yt = 0; yt < nyt; ++yt) {
        c.src = wsA + (size_t)yt * Ty * Lzo; c.dst = wsB;
        c.noff = yt * Vy; c.NV = std::min(Vy, p.Lf[1] - yt * Vy);
        FC_HIP(p.fnd.tm->c2c_inv(c, st));
      }
      o.src = wsB; o.NC = Lzo;
      FC_HIP(p.fnd.tx->rows_c2r(o, st));
    }
  }
  return FC_OK;
}

}  // namespace fc
