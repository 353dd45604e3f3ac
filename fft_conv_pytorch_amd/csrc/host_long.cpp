// host_long.cpp -- plans and launches the long-filter path (include/fftconv_amd.h "Long filters", kernels in
// long1d.hpp): descriptor checks, the factorisation N = N1 * N2, sizes, slabs, the two-table twiddles, the launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "fc_plan.h"
#include "long1d.hpp"

namespace {

using namespace fc;

constexpr int64_t kMaxN = (int64_t)1 << 24;        // 4096 x 4096
constexpr int64_t kDefaultBudgetMB = 8192;         // W1 + W2 of one slab

const LongImpl* find_long(int T) {
  static const LongImpl* impls[] = {get_long_P8_S1(),  get_long_P8_S2(),  get_long_P16_S1(), get_long_P16_S2(),
                                    get_long_P32_S1(), get_long_P32_S2(), get_long_P32_S4()};
  for (const LongImpl* l : impls)
    if (l->T == T) return l;
  return nullptr;
}

struct LongGeom {
  int64_t B, Cin, Cout, G, Cig, Cog, L, K;
  int64_t nout;                 // kept output samples
  int64_t padl;                 // row position p holds x[p - padl]
  int64_t tap0, tstep, keff;    // row position p < keff of a filter row holds taps[tap0 + tstep*p]
  int64_t need;                 // shortest cyclic length: out_step * (nout - 1) + tap_dil * (keff - 1) + 1
  int pad_mode;                 // PadMode of the signal row, and the positions it fills before / behind the data
  int64_t mpadl, mpadr;
  int64_t up, dil, step;        // src_up, tap_dil, out_step
  int N1, N2;
  int64_t N;
  int kind;                     // fc_long_kind bits: complex rows, conjugated reads
  int64_t npairs, slab_pairs, slabs;      // rows of the transform per channel: batch pairs, or batch items of a complex plan
  int ob;
  size_t spectrum_bytes, workspace_bytes;
  // a phases plan (phases_geometry below): Cout, Cog and nout above count the s phases of every filter
  int64_t ph_s, ph_cog, ph_off, ph_lout;      // stride (0: not a phases plan), filters per group, y index of sample 0 of phase 0, length of y
  // a decimation plan (decim_geometry below): Cin and Cig above count the s decimated rows of every input channel, L and K
  // are those of the tensors
  int64_t dc_s, dc_padl, dc_flip;             // stride (0: not a decimation plan), the phase origin (pad_left), the tap order
  // a blocks plan (blocks_geometry below): npairs counts pairs of units (batch item, block); N is the block's
  int64_t bk_V, bk_T, bk_U;                   // kept samples per block, blocks per row (0: not a blocks plan), units B * T
  int pad_only;                               // every kept output sees padding only: padl is a marker, not a place (long_row)
};

bool is_tile_len(long long v) { return v >= 64 && v <= 4096 && (v & (v - 1)) == 0; }

const fc_long_ext kDefaultExt = {0, 1, 1, 1};

// The row of a long plan: descriptor checks, the output length, the taps that are read and where the data lies (everything
// up to g.need, the points one cyclic transform of the whole row must hold)
int long_row(const fc_long_desc* desc, const fc_long_ext* ext, int kind, LongGeom* out) {
  if (!desc || !out) return fail(FC_ERR_INVALID, "null argument");
  if (kind & ~(FC_LONG_COMPLEX | FC_LONG_CONJ_SIGNAL | FC_LONG_CONJ_TAPS)) return fail(FC_ERR_INVALID, "unknown long-plan kind %d", kind);
  const bool cx = (kind & FC_LONG_COMPLEX) != 0;
  if (!cx && kind) return fail(FC_ERR_INVALID, "long-plan kind %d: conjugated reads go with complex rows (FC_LONG_COMPLEX) only", kind);
  const fc_long_desc& d = *desc;
  const fc_long_ext& e = ext ? *ext : kDefaultExt;
  if (d.batch < 1 || d.in_channels < 1 || d.out_channels < 1 || d.groups < 1)
    return fail(FC_ERR_INVALID, "batch, channels and groups must be positive");
  if (d.in_channels % d.groups || d.out_channels % d.groups)
    return fail(FC_ERR_INVALID, "in_channels (%lld) and out_channels (%lld) must be divisible by groups (%lld)",
                (long long)d.in_channels, (long long)d.out_channels, (long long)d.groups);
  if (d.length < 1 || d.kernel < 1) return fail(FC_ERR_INVALID, "length and kernel must be positive");
  if (d.pad_left < 0 || d.pad_right < 0 || d.out_keep < 0) return fail(FC_ERR_INVALID, "padding and out_keep must not be negative");
  if (d.flip != 0 && d.flip != 1) return fail(FC_ERR_INVALID, "flip must be 0 or 1");
  if (e.pad_mode < PAD_CONSTANT || e.pad_mode > PAD_CIRCULAR) return fail(FC_ERR_INVALID, "unknown pad_mode %d", e.pad_mode);
  if (e.src_up < 1 || e.tap_dil < 1 || e.out_step < 1)
    return fail(FC_ERR_INVALID, "src_up (%d), tap_dil (%d) and out_step (%d) must be >= 1", e.src_up, e.tap_dil, e.out_step);
  if (e.src_up > 1 && e.pad_mode != PAD_CONSTANT)
    return fail(FC_ERR_INVALID, "src_up (%d) spreads the row over zeros: it goes with pad_mode constant only", e.src_up);
  // (4-byte samples: a row lies behind one resource of at most 2^31 bytes, where the offset 2^31 still reads as zero)
  const int64_t lim = (int64_t)1 << 29;
  if (d.length > lim || d.kernel > lim || d.pad_left > lim || d.pad_right > lim || e.src_up > lim || e.tap_dil > lim ||
      e.out_step > lim)
    return fail(FC_ERR_UNSUPPORTED, "rows, filters and paddings of more than 2^29 samples are not addressed by the long-filter kernels");
  // (8-byte samples: the byte size of a row and every offset in use stay below the 2^31 that reads as zero)
  const int64_t clim = (int64_t)1 << 28;
  if (cx && (d.length >= clim || d.kernel >= clim || d.pad_left >= clim || d.pad_right >= clim))
    return fail(FC_ERR_UNSUPPORTED, "complex rows, filters and paddings of 2^28 samples or more are not addressed by the long-filter kernels");
  if (e.pad_mode == PAD_REFLECT && (d.pad_left >= d.length || d.pad_right >= d.length))
    return fail(FC_ERR_INVALID, "reflect padding (%lld, %lld) must be smaller than the input size (%lld)", (long long)d.pad_left,
                (long long)d.pad_right, (long long)d.length);
  if (e.pad_mode == PAD_CIRCULAR && (d.pad_left > d.length || d.pad_right > d.length))
    return fail(FC_ERR_INVALID, "circular padding (%lld, %lld) must not exceed the input size (%lld)", (long long)d.pad_left,
                (long long)d.pad_right, (long long)d.length);
  const int64_t up = e.src_up, dil = e.tap_dil, step = e.out_step;
  const int64_t span = up * (d.length - 1) + 1;          // positions from the first sample of the data to the last
  const int64_t Lp = span + d.pad_left + d.pad_right;
  const int64_t kext = dil * (d.kernel - 1) + 1;
  if (kext > Lp) {
    if (dil == 1)
      return fail(FC_ERR_INVALID, "kernel (%lld taps) is longer than the padded row (%lld samples)", (long long)d.kernel, (long long)Lp);
    return fail(FC_ERR_INVALID, "kernel (%lld taps, %lld samples at dilation %lld) is longer than the padded row (%lld samples)",
                (long long)d.kernel, (long long)kext, (long long)dil, (long long)Lp);
  }
  const int64_t full = (Lp - kext) / step + 1;
  if (d.out_keep > full)
    return fail(FC_ERR_INVALID, "out_keep (%lld) exceeds the output length %lld", (long long)d.out_keep, (long long)full);
  LongGeom g{};
  g.B = d.batch; g.Cin = d.in_channels; g.Cout = d.out_channels; g.G = d.groups;
  g.Cig = g.Cin / g.G; g.Cog = g.Cout / g.G; g.L = d.length; g.K = d.kernel;
  g.nout = d.out_keep ? d.out_keep : full;
  g.pad_mode = e.pad_mode; g.up = up; g.dil = dil; g.step = step;
  int64_t klo = 0, khi = d.kernel - 1;
  if (e.pad_mode == PAD_CONSTANT) {
    // tap k (of u) can meet the data for some kept output only if
    //   pad_left - step*(nout - 1) <= dil*k <= pad_left + span - 1
    // (with step = dil = up = 1 exactly the taps that do; otherwise a superset of them)
    const int64_t lo = d.pad_left - step * (g.nout - 1);
    klo = lo > 0 ? (lo + dil - 1) / dil : 0;
    khi = std::min<int64_t>(d.kernel - 1, (d.pad_left + span - 1) / dil);
  } else {
    g.mpadl = d.pad_left; g.mpadr = d.pad_right;     // every position of the padded row holds a sample: no tap is dropped
  }
  if (khi < klo) {               // every kept output sees padding only: one tap against a row that reads as zero, y = bias
    g.keff = 1; g.tap0 = 0; g.tstep = 1;
    g.padl = kMaxN + 1;          // the data lies past every position of the transform
    g.pad_only = 1;
  } else {
    g.keff = khi - klo + 1;
    g.padl = d.pad_left - dil * klo;
    g.tap0 = d.flip ? d.kernel - 1 - klo : klo;
    g.tstep = d.flip ? -1 : 1;
  }
  g.need = step * (g.nout - 1) + dil * (g.keff - 1) + 1;
  g.kind = kind;
  *out = g;
  return FC_OK;
}

// The transform of a plan whose row is known: N = N1 * N2 for g.need points, the slabs over `npairs` rows of the transform
// per channel, sizes and the grid check.  `exact`: g.need is the N of a blocks plan, which FFTCONV_LONG_N must factor
int long_factor(LongGeom& g, int64_t npairs, bool exact) {
  const bool cx = (g.kind & FC_LONG_COMPLEX) != 0;
  // smallest N = N1 * N2 >= need with both factors tile lengths; the most balanced split, N2 >= N1
  int lg = 12;
  while (((int64_t)1 << lg) < g.need) ++lg;
  int l1 = lg / 2, l2 = lg - l1;
  g.N1 = 1 << l1; g.N2 = 1 << l2;
  if (const char* env = getenv("FFTCONV_LONG_N")) {
    if (*env) {
      long long n1 = 0, n2 = 0;
      if (sscanf(env, "%lldx%lld", &n1, &n2) != 2 || !is_tile_len(n1) || !is_tile_len(n2))
        return fail(FC_ERR_INVALID, "FFTCONV_LONG_N=%s: expected <N1>x<N2>, both powers of two from 64 to 4096", env);
      if (n1 * n2 < g.need)
        return fail(FC_ERR_INVALID, "FFTCONV_LONG_N=%s holds %lld points but the row needs %lld", env, n1 * n2, (long long)g.need);
      if (exact && n1 * n2 != g.need)
        return fail(FC_ERR_INVALID, "FFTCONV_LONG_N=%s holds %lld points but the blocks of the plan have %lld", env, n1 * n2,
                    (long long)g.need);
      g.N1 = (int)n1; g.N2 = (int)n2;
    }
  }
  g.N = (int64_t)g.N1 * g.N2;
  const LongImpl* rows = find_long(g.N2);
  g.ob = rows ? rows->ob : 1;
  g.npairs = npairs;
  int64_t budget_mb = kDefaultBudgetMB;
  if (const char* env = getenv("FFTCONV_LONG_WS_MB"))
    if (*env && atoll(env) > 0) budget_mb = atoll(env);
  const int64_t pair_bytes = (g.Cin + g.Cout) * g.N * 8;
  g.slab_pairs = std::max<int64_t>(1, std::min<int64_t>(g.npairs, (budget_mb << 20) / pair_bytes));
  g.slabs = (g.npairs + g.slab_pairs - 1) / g.slab_pairs;
  g.workspace_bytes = (size_t)(g.slab_pairs * pair_bytes);
  g.spectrum_bytes = (size_t)(g.Cout * g.Cig * g.N * 8);
  // grids are 32-bit: (blocks per row) x rows
  const int64_t worst = std::max<int64_t>(g.N2 / 2, g.N1 / 2) * std::max<int64_t>(g.slab_pairs * std::max(g.Cin, g.Cout), 1);
  if (worst > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "a slab of %lld %s x %lld channels x %lld points exceeds the 2^31 workgroups of one "
                "launch: lower FFTCONV_LONG_WS_MB", (long long)g.slab_pairs, exact ? "unit pairs" : cx ? "batch items" : "batch pairs",
                (long long)std::max(g.Cin, g.Cout), (long long)g.N);
  return FC_OK;
}

int long_geometry(const fc_long_desc* desc, const fc_long_ext* ext, int kind, LongGeom* out) {
  LongGeom g;
  int st = long_row(desc, ext, kind, &g);
  if (st != FC_OK) return st;
  if (g.need > kMaxN)
    return fail(FC_ERR_UNSUPPORTED, "the row needs a transform of %lld points; the long-filter path stops at 2^24 = %lld "
                "(4096 x 4096)", (long long)g.need, (long long)kMaxN);
  if ((st = long_factor(g, (kind & FC_LONG_COMPLEX) ? g.B : (g.B + 1) / 2, false)) != FC_OK) return st;
  *out = g;
  return FC_OK;
}

// A row longer than the transform as overlap-save blocks (include/fftconv_amd.h "Rows in overlap-save blocks"): the row of
// the plain real plan with the default fc_long_ext, cut into T blocks of N points that start hop = N - keff + 1 samples
// apart; unit u = b*T + t, two units to a complex row.  Everything but the two tensor sides is the long plan of U / 2
// "batch pairs" at N points.
constexpr int64_t kMinBlock = 4096;

int blocks_points(int64_t keff, int64_t block_points, int64_t* N) {
  if (block_points == 0) {
    // the planner's choice: blocks keep 3/4 of their points, N1 = 512 still reads whole 128-byte segments
    int64_t n = (int64_t)1 << 18;
    while (n < 4 * keff && n < kMaxN) n <<= 1;
    *N = n;
    return FC_OK;
  }
  if (block_points < kMinBlock || block_points > kMaxN || (block_points & (block_points - 1)))
    return fail(FC_ERR_INVALID, "block_points (%lld) must be a power of two from 4096 to 2^24, or 0 for the planner's choice",
                (long long)block_points);
  *N = block_points;
  return FC_OK;
}

int blocks_row(const fc_long_desc* desc, int64_t block_points, LongGeom* out) {
  LongGeom g;
  int st = long_row(desc, nullptr, FC_LONG_REAL, &g);
  if (st != FC_OK) return st;
  int64_t N = 0;
  if ((st = blocks_points(g.keff, block_points, &N)) != FC_OK) return st;
  if (g.keff > N / 2)
    return fail(FC_ERR_UNSUPPORTED, "a filter of K = %lld taps (%lld of them read) against blocks of N = %lld points: a block must "
                "keep at least half of its points, so it takes at most N / 2 = %lld taps", (long long)g.K, (long long)g.keff,
                (long long)N, (long long)(N / 2));
  // (a row of y lies behind one buffer resource, as a row of x does)
  if (g.nout > (int64_t)1 << 29)
    return fail(FC_ERR_UNSUPPORTED, "an output row of %lld samples: rows of more than 2^29 samples are not addressed by the "
                "long-filter kernels", (long long)g.nout);
  g.bk_V = N - g.keff + 1;
  g.bk_T = (g.nout + g.bk_V - 1) / g.bk_V;
  if (g.B > 0x7ffffff0LL / g.bk_T)
    return fail(FC_ERR_UNSUPPORTED, "%lld batch items x %lld blocks exceed the 2^31 units of a blocks plan", (long long)g.B,
                (long long)g.bk_T);
  g.bk_U = g.B * g.bk_T;
  // (every kept output sees padding only: the data lies past every position t*V + q of every block, all below 2^31.  A
  // real padl is a place in the row, min(pad_left, nout - 1) <= 2^29, and stays what it is: t*V + q - padl fits an int)
  if (g.pad_only) g.padl = 0x7fffffff;
  g.need = N;
  *out = g;
  return FC_OK;
}

int blocks_geometry(const fc_long_blocks_desc* desc, LongGeom* out) {
  if (!desc || !out) return fail(FC_ERR_INVALID, "null argument");
  LongGeom g;
  int st = blocks_row(&desc->row, desc->block_points, &g);
  if (st != FC_OK) return st;
  if ((st = long_factor(g, (g.bk_U + 1) / 2, true)) != FC_OK) return st;
  *out = g;
  return FC_OK;
}

void fill_blocks(const LongGeom& g, int64_t blocks[4]) {
  blocks[0] = g.bk_V; blocks[1] = g.bk_T; blocks[2] = g.bk_U; blocks[3] = (g.bk_U + 1) / 2;
}

LongBlocks blocks_args(const LongGeom& g, int64_t win) {
  LongBlocks bk{};
  bk.d_T = make_fastdiv((unsigned)g.bk_T);
  bk.U = (int)g.bk_U; bk.hop = (int)g.bk_V; bk.win = (int)win;
  return bk;
}

// A transposed convolution of stride s and dilation 1 as s ordinary convolutions of the unspread row:
//   y[s*T + p - padding] = sum_j w[p + s*j] * x[T - j],   0 <= p < s,   Kp = ceil(K / s) taps per phase,
// the forward long plan with s*Cout output channels (o*s + p: phase p of filter o), Kp flipped taps per filter row, Kp - 1
// zeros in front of the row and the samples T0 <= T <= (Lout - 1 + padding) / s kept, T0 = min(padding / s, Kp - 1) (a
// padding wider than the filter leaves a few samples in front that the store drops).  Sample t of the plan is T = T0 + t.
int phases_geometry(const fc_long_phases_desc* desc, LongGeom* out) {
  if (!desc || !out) return fail(FC_ERR_INVALID, "null argument");
  const fc_long_phases_desc& d = *desc;
  if (d.batch < 1 || d.in_channels < 1 || d.out_channels < 1 || d.groups < 1)
    return fail(FC_ERR_INVALID, "batch, channels and groups must be positive");
  if (d.in_channels % d.groups || d.out_channels % d.groups)
    return fail(FC_ERR_INVALID, "in_channels (%lld) and out_channels (%lld) must be divisible by groups (%lld)",
                (long long)d.in_channels, (long long)d.out_channels, (long long)d.groups);
  if (d.length < 1 || d.kernel < 1) return fail(FC_ERR_INVALID, "length and kernel must be positive");
  if (d.stride < 1) return fail(FC_ERR_INVALID, "stride (%lld) must be >= 1", (long long)d.stride);
  if (d.padding < 0) return fail(FC_ERR_INVALID, "padding must not be negative");
  if (d.output_padding < 0 || d.output_padding >= d.stride)
    return fail(FC_ERR_INVALID, "output_padding (%lld) must lie in [0, stride = %lld)", (long long)d.output_padding, (long long)d.stride);
  const int64_t lim = (int64_t)1 << 29;      // (4-byte samples: a row of y and a row of the weight lie behind one resource)
  if (d.length >= lim || d.kernel >= lim || d.padding >= lim || d.stride > 4096 || d.out_channels > lim / d.stride)
    return fail(FC_ERR_UNSUPPORTED, "rows, filters and paddings of 2^29 samples or more and strides above 4096 are not addressed by "
                "the phases plan of the long-filter kernels");
  const int64_t s = d.stride, K = d.kernel, L = d.length;
  const int64_t lout = (L - 1) * s - 2 * d.padding + (K - 1) + d.output_padding + 1;
  if (lout < 1) return fail(FC_ERR_INVALID, "the output length (%lld) must be positive", (long long)lout);
  if (lout >= lim) return fail(FC_ERR_UNSUPPORTED, "an output row of %lld samples: the phases plan addresses rows below 2^29", (long long)lout);
  const int64_t Kp = (K + s - 1) / s;
  const int64_t t0 = std::min(d.padding / s, Kp - 1), t1 = (lout - 1 + d.padding) / s, nt = t1 - t0 + 1;
  fc_long_desc f{};
  f.batch = d.batch; f.in_channels = d.in_channels; f.out_channels = d.out_channels * s; f.groups = d.groups;
  f.length = L; f.kernel = Kp;
  f.pad_left = Kp - 1 - t0;
  f.pad_right = std::max<int64_t>(0, nt + Kp - 1 - f.pad_left - L);
  f.out_keep = nt; f.flip = 1; f.has_bias = d.has_bias;
  LongGeom g;
  const int st = long_geometry(&f, nullptr, FC_LONG_REAL, &g);
  if (st != FC_OK) return st;
  if (s * g.N > (int64_t)1 << 30)      // (s*t + p as a 32-bit index for every sample t of the transform)
    return fail(FC_ERR_UNSUPPORTED, "stride %lld x a transform of %lld points exceeds the 2^30 samples the phases plan indexes",
                (long long)s, (long long)g.N);
  // the grid of the inverse pass: up to (s + 3) / NC phase blocks of NC phases x N2 * NC / (columns per workgroup >= 2) column blocks
  // per filter and pair
  if (g.slab_pairs * d.out_channels * (g.N2 / 2) * (s + 3) > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "a slab of %lld batch pairs x %lld filters x %lld phases x %lld points exceeds the 2^31 workgroups of "
                "one launch: lower FFTCONV_LONG_WS_MB", (long long)g.slab_pairs, (long long)d.out_channels, (long long)s, (long long)g.N);
  g.K = K;      // (the filter rows are read from the weight's rows of K taps)
  g.ph_s = s; g.ph_cog = d.out_channels / d.groups; g.ph_off = s * t0 - d.padding; g.ph_lout = lout;
  *out = g;
  return FC_OK;
}

// A strided convolution of stride s and dilation 1 on the s decimated rows of the signal, the adjoint of the phases store
// (DESIGN 4.7): with k = s*m + p,
//   y[j] = sum_k u[k] * xrow[s*j + k] = sum_p sum_m u_p[m] * x_p[j + m],   x_p[t] = xrow[s*t + p],   u_p[m] = u[s*m + p],
// the plain long plan with s*Cin input channels (i*s + p: decimated row p of channel i), Kp = ceil(K / s) taps per filter
// row and rows of T = nout + Kp - 1 positions.  The descriptor goes to long_geometry in those units, so factorisation,
// slabs, FFTCONV_LONG_N and the limits are those of every long plan.
int decim_geometry(const fc_long_decim_desc* desc, LongGeom* out) {
  if (!desc || !out) return fail(FC_ERR_INVALID, "null argument");
  const fc_long_decim_desc& d = *desc;
  if (d.batch < 1 || d.in_channels < 1 || d.out_channels < 1 || d.groups < 1)
    return fail(FC_ERR_INVALID, "batch, channels and groups must be positive");
  if (d.in_channels % d.groups || d.out_channels % d.groups)
    return fail(FC_ERR_INVALID, "in_channels (%lld) and out_channels (%lld) must be divisible by groups (%lld)",
                (long long)d.in_channels, (long long)d.out_channels, (long long)d.groups);
  if (d.length < 1 || d.kernel < 1) return fail(FC_ERR_INVALID, "length and kernel must be positive");
  if (d.stride < 2 || d.stride > 64)
    return fail(FC_ERR_INVALID, "stride (%lld) of a decimation plan must lie in [2, 64]", (long long)d.stride);
  if (d.pad_left < 0 || d.pad_right < 0 || d.out_keep < 0) return fail(FC_ERR_INVALID, "padding and out_keep must not be negative");
  if (d.flip != 0 && d.flip != 1) return fail(FC_ERR_INVALID, "flip must be 0 or 1");
  const int64_t lim = (int64_t)1 << 29;      // (4-byte samples: a row of x and a row of the weight lie behind one resource)
  if (d.length >= lim || d.kernel >= lim || d.pad_left >= lim || d.pad_right >= lim)
    return fail(FC_ERR_UNSUPPORTED, "rows, filters and paddings of 2^29 samples or more are not addressed by the decimation plan of "
                "the long-filter kernels");
  const int64_t s = d.stride, K = d.kernel, L = d.length;
  const int64_t Lp = L + d.pad_left + d.pad_right;
  if (K > Lp)
    return fail(FC_ERR_INVALID, "kernel (%lld taps) is longer than the padded row (%lld samples)", (long long)K, (long long)Lp);
  const int64_t full = (Lp - K) / s + 1;
  if (d.out_keep > full)
    return fail(FC_ERR_INVALID, "out_keep (%lld) exceeds the output length %lld", (long long)d.out_keep, (long long)full);
  const int64_t nout = d.out_keep ? d.out_keep : full, Kp = (K + s - 1) / s;
  fc_long_desc f{};
  f.batch = d.batch; f.in_channels = d.in_channels * s; f.out_channels = d.out_channels; f.groups = d.groups;
  f.length = nout + Kp - 1; f.kernel = Kp;
  f.pad_left = 0; f.pad_right = 0; f.out_keep = nout; f.flip = 0; f.has_bias = d.has_bias;
  LongGeom g;
  const int st = long_geometry(&f, nullptr, FC_LONG_REAL, &g);
  if (st != FC_OK) return st;
  if (s * g.N > (int64_t)1 << 30)      // (s*t + p as a 32-bit index for every position t of the transform)
    return fail(FC_ERR_UNSUPPORTED, "stride %lld x a transform of %lld points exceeds the 2^30 samples the decimation plan indexes",
                (long long)s, (long long)g.N);
  // the grid of the forward column pass: up to (s + 3) / NC phase blocks of NC phases x N2 * NC / (columns per workgroup >= 2)
  // column blocks per channel and pair
  if (g.slab_pairs * d.in_channels * (g.N2 / 2) * (s + 3) > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "a slab of %lld batch pairs x %lld channels x %lld phases x %lld points exceeds the 2^31 workgroups of "
                "one launch: lower FFTCONV_LONG_WS_MB", (long long)g.slab_pairs, (long long)d.in_channels, (long long)s, (long long)g.N);
  g.L = L; g.K = K;      // (the rows are read from the tensors: x rows of L samples, weight rows of K taps)
  g.dc_s = s; g.dc_padl = d.pad_left; g.dc_flip = d.flip;
  *out = g;
  return FC_OK;
}

// The weight gradient of the layer a forward long plan runs: the forward plan's own geometry -- N1 x N2, the
// taps it reads (keff of them from tap0 in steps of tstep), padl -- with a workspace of its own: W1 of x and W1 of dY for
// the batch pairs of a slab, and W2 for all Cout * Cin/g rows of dW, which the slabs add into.
struct WgradGeom {
  LongGeom f;                   // the forward plan of the layer, out_keep = out_len
  int64_t rows;                 // Cout * Cin/g rows of dW
  int ob;                       // output channels per workgroup of the row pass
  int64_t slab_pairs, slabs;
  size_t workspace_bytes;
};

int wgrad_sizes(WgradGeom& w, WgradGeom* out);

int wgrad_geometry(const fc_long_wgrad_desc* desc, WgradGeom* out) {
  if (!desc || !out) return fail(FC_ERR_INVALID, "null argument");
  const fc_long_wgrad_desc& d = *desc;
  if (d.out_len < 1) return fail(FC_ERR_INVALID, "out_len (%lld) must be positive", (long long)d.out_len);
  if (d.stride < 1 || d.dilation < 1)
    return fail(FC_ERR_INVALID, "stride (%d) and dilation (%d) must be >= 1", d.stride, d.dilation);
  fc_long_desc f{};
  f.batch = d.batch; f.in_channels = d.in_channels; f.out_channels = d.out_channels; f.groups = d.groups;
  f.length = d.length; f.kernel = d.kernel; f.pad_left = d.pad_left; f.pad_right = d.pad_right;
  f.out_keep = d.out_len; f.flip = d.flip; f.has_bias = 0;
  const fc_long_ext e = {d.pad_mode, 1, d.dilation, d.stride};
  WgradGeom w{};
  const int st = long_geometry(&f, &e, FC_LONG_REAL, &w.f);
  if (st != FC_OK) return st;
  return wgrad_sizes(w, out);
}

// the blocks twin: the row of the plain layer in overlap-save blocks of block_points (blocks_row above); x is read through
// the N-point window of a block, dY through the window of the V samples the block keeps
int wgrad_blocks_geometry(const fc_long_wgrad_desc* desc, int64_t block_points, WgradGeom* out) {
  if (!desc || !out) return fail(FC_ERR_INVALID, "null argument");
  const fc_long_wgrad_desc& d = *desc;
  if (d.out_len < 1) return fail(FC_ERR_INVALID, "out_len (%lld) must be positive", (long long)d.out_len);
  if (d.stride != 1 || d.dilation != 1 || d.pad_mode != PAD_CONSTANT)
    return fail(FC_ERR_UNSUPPORTED, "the weight gradient by blocks takes stride 1, dilation 1 and pad_mode constant only (got "
                "stride %d, dilation %d, pad_mode %d): a block is a window of the zero-padded stride-1 row", d.stride, d.dilation,
                d.pad_mode);
  fc_long_desc f{};
  f.batch = d.batch; f.in_channels = d.in_channels; f.out_channels = d.out_channels; f.groups = d.groups;
  f.length = d.length; f.kernel = d.kernel; f.pad_left = d.pad_left; f.pad_right = d.pad_right;
  f.out_keep = d.out_len; f.flip = d.flip; f.has_bias = 0;
  WgradGeom w{};
  int st = blocks_row(&f, block_points, &w.f);
  if (st != FC_OK) return st;
  if ((st = long_factor(w.f, (w.f.bk_U + 1) / 2, true)) != FC_OK) return st;
  return wgrad_sizes(w, out);
}

// the workspace, slabs and grids of a weight-gradient plan whose forward geometry w.f is known
int wgrad_sizes(WgradGeom& w, WgradGeom* out) {
  const LongGeom& g = w.f;
  const LongImpl* rows = find_long(g.N2);
  w.ob = rows ? rows->wg_ob : 1;
  w.rows = g.Cout * g.Cig;
  int64_t budget_mb = kDefaultBudgetMB;
  if (const char* env = getenv("FFTCONV_LONG_WS_MB"))
    if (*env && atoll(env) > 0) budget_mb = atoll(env);
  const int64_t row_bytes = g.N * 8, budget = budget_mb << 20;
  if (w.rows > budget / row_bytes)
    return fail(FC_ERR_UNSUPPORTED, "the weight gradient keeps %lld x %lld rows of %lld points (%lld MiB) in its workspace, more than "
                "the budget of %lld MiB (FFTCONV_LONG_WS_MB)", (long long)g.Cout, (long long)g.Cig, (long long)g.N,
                (long long)((w.rows * row_bytes) >> 20), (long long)budget_mb);
  const int64_t pair_bytes = (g.Cin + g.Cout) * row_bytes;
  w.slab_pairs = std::max<int64_t>(1, std::min<int64_t>(g.npairs, (budget - w.rows * row_bytes) / pair_bytes));
  w.slabs = (g.npairs + w.slab_pairs - 1) / w.slab_pairs;
  w.workspace_bytes = (size_t)(w.slab_pairs * pair_bytes + w.rows * row_bytes);
  // grids are 32-bit: the column passes over x and dY (as the forward's), the row pass and the inverse pass over dW's rows
  const int64_t nob = (g.Cog + w.ob - 1) / w.ob;
  const int64_t worst = std::max<int64_t>(std::max<int64_t>(g.N2 / 2, g.N1 / 2) * std::max(w.slab_pairs * std::max(g.Cin, g.Cout), w.rows),
                                          (g.N1 / 2) * g.G * g.Cig * nob);
  if (worst > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "a weight gradient of %lld x %lld rows, %lld batch pairs per slab and %lld points exceeds the 2^31 "
                "workgroups of one launch", (long long)g.Cout, (long long)g.Cig, (long long)w.slab_pairs, (long long)g.N);
  *out = w;
  return FC_OK;
}

void fill_wgrad_info(const WgradGeom& w, int64_t info[8]) {
  info[0] = w.f.N1; info[1] = w.f.N2; info[2] = w.f.K; info[3] = w.f.keff;
  info[4] = (int64_t)w.workspace_bytes; info[5] = w.slabs; info[6] = w.ob; info[7] = w.slab_pairs;
}

void fill_info(const LongGeom& g, int64_t info[8]) {
  info[0] = g.N1; info[1] = g.N2; info[2] = g.ph_s ? g.ph_lout : g.nout; info[3] = (int64_t)g.spectrum_bytes;
  info[4] = (int64_t)g.workspace_bytes; info[5] = g.slabs; info[6] = g.ob; info[7] = g.slab_pairs;
}

// w_N^m = thi[m >> 12] * tlo[m & 4095], both tables rounded once from float64; shared per (device, N)
struct LongTables {
  f2* thi = nullptr;
  f2* tlo = nullptr;
};
std::mutex g_lt_mutex;
std::map<std::pair<int, int64_t>, LongTables> g_lt;

int get_long_tables(int64_t N, LongTables* out) {
  int dev = 0;
  FC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_lt_mutex);
  const auto key = std::make_pair(dev, N);
  auto it = g_lt.find(key);
  if (it != g_lt.end()) { *out = it->second; return FC_OK; }
  const int64_t nhi = N >> kLongLoBits, nlo = (int64_t)1 << kLongLoBits;
  std::vector<f2> hi((size_t)nhi), lo((size_t)nlo);
  const double tau = 6.283185307179586476925286766559;
  for (int64_t a = 0; a < nhi; ++a) {
    const double ang = -tau * (double)(a << kLongLoBits) / (double)N;
    hi[(size_t)a] = f2{(float)std::cos(ang), (float)std::sin(ang)};
  }
  for (int64_t b = 0; b < nlo; ++b) {
    const double ang = -tau * (double)b / (double)N;
    lo[(size_t)b] = f2{(float)std::cos(ang), (float)std::sin(ang)};
  }
  LongTables t;
  FC_HIP_SETUP(hipMalloc(&t.thi, hi.size() * sizeof(f2)));
  FC_HIP_SETUP(hipMalloc(&t.tlo, lo.size() * sizeof(f2)));
  FC_HIP_SETUP(hipMemcpy(t.thi, hi.data(), hi.size() * sizeof(f2), hipMemcpyHostToDevice));
  FC_HIP_SETUP(hipMemcpy(t.tlo, lo.data(), lo.size() * sizeof(f2), hipMemcpyHostToDevice));
  g_lt[key] = t;
  *out = t;
  return FC_OK;
}

}  // namespace

struct fc_long_plan {
  fc_long_desc d;
  LongGeom g;
  const fc::LongImpl* cols;    // N1-point geometry
  const fc::LongImpl* rows;    // N2-point geometry
  fc::Twiddles tw1, tw2;
  LongTables lt;
};

struct fc_long_wgrad_plan {
  WgradGeom w;
  std::unique_ptr<fc_long_plan> f;      // kernels and tables: those of the forward plan of the layer
};

namespace {

LongArgs base_args(const fc_long_plan& p) {
  const LongGeom& g = p.g;
  LongArgs a{};
  a.thi = p.lt.thi; a.tlo = p.lt.tlo;
  a.twA1 = p.tw1.twA; a.twB1 = p.tw1.twB; a.twA2 = p.tw2.twA; a.twB2 = p.tw2.twB;
  a.N1 = g.N1; a.N2 = g.N2;
  a.lgN2 = 0;
  while ((1 << a.lgN2) < g.N2) ++a.lgN2;
  a.B = (int)g.B; a.G = (int)g.G; a.Cig = (int)g.Cig; a.Cog = (int)g.Cog;
  a.ob = g.ob; a.nob = (int)((g.Cog + g.ob - 1) / g.ob);
  a.C = 1;
  a.L = (int)g.L; a.padl = (int)g.padl;
  a.tap0 = (int)g.tap0; a.tstep = (int)g.tstep; a.keff = (int)g.keff; a.K = (int)g.K;
  a.nout = (int)g.nout;
  a.scale = (float)(1.0 / (double)g.N);
  a.pad_mode = g.pad_mode; a.mpadl = (int)g.mpadl; a.mpadr = (int)g.mpadr;
  a.src_up = (int)g.up;
  a.kpos = (int)(g.dil * (g.keff - 1) + 1);
  a.d_up = make_fastdiv((unsigned)g.up); a.d_tdil = make_fastdiv((unsigned)g.dil); a.d_ostep = make_fastdiv((unsigned)g.step);
  a.conj_src = 0;
  a.ph_s = (int)g.ph_s; a.ph_cog = (int)g.ph_cog; a.ph_off = (int)g.ph_off;
  if (g.dc_s) {      // (a decimation plan lends the words of the phases builds, long1d.hpp LongArgs)
    a.ph_s = (int)g.dc_s; a.ph_cog = 0; a.ph_off = (int)g.dc_padl;
    a.tap0 = g.dc_flip ? (int)g.K - 1 : 0; a.tstep = g.dc_flip ? -1 : 1;
  }
  return a;
}

// fc_dtype of a tensor argument -> the element code of a launch (LongArgs src_io / y_io)
int io_code(int dtype, const char* what, int* code) {
  switch (dtype) {
    case FC_F32: *code = 0; return FC_OK;
    case FC_F16: *code = IO_CODE_F16; return FC_OK;
    case FC_BF16: *code = IO_CODE_BF16; return FC_OK;
    case FC_F64:
      return fail(FC_ERR_UNSUPPORTED, "%s is float64: the long-filter path takes float32, float16 and bfloat16 tensors", what);
    default:
      return fail(FC_ERR_INVALID, "%s has dtype code %d; expected FC_F32 (0), FC_F16 (2) or FC_BF16 (3), or FC_C64 (4) on a "
                  "complex plan", what, dtype);
  }
}

// the same for a tensor argument of `plan`: a complex plan takes FC_C64 and nothing else, a real plan no FC_C64
int plan_io_code(const fc_long_plan* plan, int dtype, const char* what, int* code) {
  const bool cx = (plan->g.kind & FC_LONG_COMPLEX) != 0;
  if (dtype == FC_C64) {
    if (!cx)
      return fail(FC_ERR_INVALID, "%s is complex64 (FC_C64) but the plan is a real plan: a complex plan comes from "
                  "fc_long_plan_create_kind with FC_LONG_COMPLEX", what);
    *code = IO_CODE_C64;
    return FC_OK;
  }
  if (int e = io_code(dtype, what, code)) return e;
  if (cx)
    return fail(FC_ERR_INVALID, "%s has the real dtype code %d but the plan is a complex plan: it takes FC_C64 (4) tensors only",
                what, dtype);
  return FC_OK;
}

// bytes per sample of an element code
int64_t io_bytes(int io) { return io == IO_CODE_C64 ? 8 : (io ? 2 : 4); }

// a layout code of fc_long_forward_lay, and the size a channels-last tensor may have: one batch item's (len, channels)
// block lies behind one buffer resource whose offsets from 2^31 on mean "outside"
int layout_check(int layout, const char* what, int64_t len, int64_t channels, int io) {
  if (layout == FC_LONG_NCL) return FC_OK;
  if (layout != FC_LONG_NLC)
    return fail(FC_ERR_INVALID, "%s has layout code %d; expected FC_LONG_NCL (0) or FC_LONG_NLC (1)", what, layout);
  const int64_t es = io_bytes(io);
  const int64_t bytes = len * channels * es;
  if (bytes >= (int64_t)1 << 31)
    return fail(FC_ERR_UNSUPPORTED, "%s in the channels-last layout: one batch item is %lld samples x %lld channels x %lld "
                "bytes = %lld bytes; the long-filter kernels address blocks below 2^31 bytes (pass a (B, C, L) copy)", what,
                (long long)len, (long long)channels, (long long)es, (long long)bytes);
  return FC_OK;
}

}  // namespace

extern "C" {

int fc_long_geometry(const fc_long_desc* desc, int64_t info[8]) { return fc_long_geometry_ext(desc, nullptr, info); }

int fc_long_geometry_ext(const fc_long_desc* desc, const fc_long_ext* ext, int64_t info[8]) {
  return fc_long_geometry_kind(desc, ext, FC_LONG_REAL, info);
}

int fc_long_geometry_kind(const fc_long_desc* desc, const fc_long_ext* ext, int kind, int64_t info[8]) {
  if (!info) return fail(FC_ERR_INVALID, "null argument");
  LongGeom g;
  const int st = long_geometry(desc, ext, kind, &g);
  if (st != FC_OK) return st;
  fill_info(g, info);
  return FC_OK;
}

int fc_long_plan_create(const fc_long_desc* desc, fc_long_plan** out_plan) {
  return fc_long_plan_create_ext(desc, nullptr, out_plan);
}

int fc_long_plan_create_ext(const fc_long_desc* desc, const fc_long_ext* ext, fc_long_plan** out_plan) {
  return fc_long_plan_create_kind(desc, ext, FC_LONG_REAL, out_plan);
}

int fc_long_plan_kind(const fc_long_plan* plan) { return plan ? plan->g.kind : -1; }

// the kernels and tables of a plan whose geometry is known
static int finish_long_plan(std::unique_ptr<fc_long_plan>& p, fc_long_plan** out_plan) {
  int st;
  p->cols = find_long(p->g.N1);
  p->rows = find_long(p->g.N2);
  const fc::TileImpl* t1 = find_tile(p->g.N1);
  const fc::TileImpl* t2 = find_tile(p->g.N2);
  if (!p->cols || !p->rows || !t1 || !t2)
    return fail(FC_ERR_UNSUPPORTED, "no kernels built for %d x %d points", p->g.N1, p->g.N2);
  if ((st = get_twiddles(t1, &p->tw1)) != FC_OK) return st;
  if ((st = get_twiddles(t2, &p->tw2)) != FC_OK) return st;
  if ((st = get_long_tables(p->g.N, &p->lt)) != FC_OK) return st;
  *out_plan = p.release();
  return FC_OK;
}

int fc_long_plan_create_kind(const fc_long_desc* desc, const fc_long_ext* ext, int kind, fc_long_plan** out_plan) {
  if (!desc || !out_plan) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();
  *out_plan = nullptr;
  std::unique_ptr<fc_long_plan> p(new fc_long_plan());
  p->d = *desc;
  const int st = long_geometry(desc, ext, kind, &p->g);
  if (st != FC_OK) return st;
  return finish_long_plan(p, out_plan);
}

int fc_long_phases_geometry(const fc_long_phases_desc* desc, int64_t info[8]) {
  if (!info) return fail(FC_ERR_INVALID, "null argument");
  LongGeom g;
  const int st = phases_geometry(desc, &g);
  if (st != FC_OK) return st;
  fill_info(g, info);
  return FC_OK;
}

int fc_long_phases_plan_create(const fc_long_phases_desc* desc, fc_long_plan** out_plan) {
  if (!desc || !out_plan) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();
  *out_plan = nullptr;
  std::unique_ptr<fc_long_plan> p(new fc_long_plan());
  const int st = phases_geometry(desc, &p->g);
  if (st != FC_OK) return st;
  p->d = fc_long_desc{};
  p->d.has_bias = desc->has_bias;      // (the one field of the descriptor that the launches read)
  return finish_long_plan(p, out_plan);
}

int fc_long_decim_geometry(const fc_long_decim_desc* desc, int64_t info[8]) {
  if (!info) return fail(FC_ERR_INVALID, "null argument");
  LongGeom g;
  const int st = decim_geometry(desc, &g);
  if (st != FC_OK) return st;
  fill_info(g, info);
  return FC_OK;
}

int fc_long_decim_plan_create(const fc_long_decim_desc* desc, fc_long_plan** out_plan) {
  if (!desc || !out_plan) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();
  *out_plan = nullptr;
  std::unique_ptr<fc_long_plan> p(new fc_long_plan());
  const int st = decim_geometry(desc, &p->g);
  if (st != FC_OK) return st;
  p->d = fc_long_desc{};
  p->d.has_bias = desc->has_bias;      // (the one field of the descriptor that the launches read)
  return finish_long_plan(p, out_plan);
}

int fc_long_blocks_geometry(const fc_long_blocks_desc* desc, int64_t info[8], int64_t blocks[4]) {
  if (!info || !blocks) return fail(FC_ERR_INVALID, "null argument");
  LongGeom g;
  const int st = blocks_geometry(desc, &g);
  if (st != FC_OK) return st;
  fill_info(g, info);
  fill_blocks(g, blocks);
  return FC_OK;
}

int fc_long_blocks_plan_create(const fc_long_blocks_desc* desc, fc_long_plan** out_plan) {
  if (!desc || !out_plan) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();
  *out_plan = nullptr;
  std::unique_ptr<fc_long_plan> p(new fc_long_plan());
  const int st = blocks_geometry(desc, &p->g);
  if (st != FC_OK) return st;
  p->d = desc->row;
  return finish_long_plan(p, out_plan);
}

void fc_long_plan_destroy(fc_long_plan* plan) { delete plan; }

int fc_long_plan_info(const fc_long_plan* plan, int64_t info[8]) {
  if (!plan || !info) return fail(FC_ERR_INVALID, "null argument");
  fill_info(plan->g, info);
  return FC_OK;
}

int fc_long_transform_kernel(const fc_long_plan* plan, const float* weight, void* spectrum, void* workspace,
                             void* hip_stream) {
  return fc_long_transform_kernel_io(plan, weight, FC_F32, spectrum, workspace, hip_stream);
}

int fc_long_transform_kernel_io(const fc_long_plan* plan, const void* weight, int weight_dtype, void* spectrum,
                                void* workspace, void* hip_stream) {
  if (!plan || !weight || !spectrum || !workspace) return fail(FC_ERR_INVALID, "null argument");
  int wio = 0;
  if (int e = plan_io_code(plan, weight_dtype, "weight", &wio)) return e;
  const LongGeom& g = plan->g;
  hipStream_t st = (hipStream_t)hip_stream;
  // the filter rows go through the workspace a chunk at a time (it holds at least Cin + Cout >= 2 rows of N points)
  const int64_t rows_total = g.Cout * g.Cig;
  const int64_t fit = std::max<int64_t>(1, (int64_t)(g.workspace_bytes / (size_t)(g.N * 8)));
  const int64_t grid_cap = 0x7fffffffLL / std::max<int64_t>(g.N1, g.N2);
  const int64_t chunk = std::min(fit, grid_cap);
  for (int64_t r0 = 0; r0 < rows_total; r0 += chunk) {
    const int64_t n = std::min(chunk, rows_total - r0);
    LongArgs a = base_args(*plan);
    a.from_kernel = 1;
    a.src_io = wio;
    a.conj_src = (g.kind & FC_LONG_CONJ_TAPS) != 0;
    // (a phases plan reads the (Cin, Cout/g, K) weight where it lies: the kernel maps spectrum row r0 + q to its weight row)
    a.ph_row0 = (int)r0;
    // (so does a decimation plan, from the (Cout, Cin/g, K) weight)
    a.src = g.ph_s || g.dc_s ? (const float*)weight : (const float*)((const char*)weight + (size_t)r0 * g.K * (size_t)io_bytes(wio));
    a.w1 = (f2*)workspace;
    FC_HIP(plan->cols->cols_fwd(a, g.dil > 1, false, n, st));      // (the mapped build only where the taps are spread)
    a.spec_mode = 1;
    a.spec_out = (f2*)spectrum + (size_t)r0 * g.N;
    FC_HIP(plan->rows->rows(a, n, st));
  }
  return FC_OK;
}

int fc_long_forward(const fc_long_plan* plan, const float* x, const void* spectrum, const float* bias, float* y,
                    void* workspace, void* hip_stream) {
  return fc_long_forward_io(plan, x, FC_F32, spectrum, bias, y, FC_F32, workspace, hip_stream);
}

int fc_long_forward_io(const fc_long_plan* plan, const void* x, int x_dtype, const void* spectrum, const float* bias,
                       void* y, int y_dtype, void* workspace, void* hip_stream) {
  return fc_long_forward_lay(plan, x, x_dtype, FC_LONG_NCL, spectrum, bias, y, y_dtype, FC_LONG_NCL, workspace, hip_stream);
}

int fc_long_forward_lay(const fc_long_plan* plan, const void* x, int x_dtype, int x_layout, const void* spectrum,
                        const float* bias, void* y, int y_dtype, int y_layout, void* workspace, void* hip_stream) {
  if (!plan || !x || !spectrum || !y || !workspace) return fail(FC_ERR_INVALID, "null argument");
  if (plan->d.has_bias && !bias) return fail(FC_ERR_INVALID, "the plan was made with a bias");
  int xio = 0, yio = 0;
  if (int e = plan_io_code(plan, x_dtype, "x", &xio)) return e;
  if (int e = plan_io_code(plan, y_dtype, "y", &yio)) return e;
  if (plan->g.ph_s && (x_layout != FC_LONG_NCL || y_layout != FC_LONG_NCL))
    return fail(FC_ERR_UNSUPPORTED, "a phases plan reads and writes (B, C, L) tensors only: its inverse pass gives the lanes that "
                "a channels-last store runs over the channels to the phases of one filter (run the zero-spread long plan, or "
                "pass contiguous tensors)");
  if (plan->g.dc_s && x_layout != FC_LONG_NCL)
    return fail(FC_ERR_UNSUPPORTED, "a decimation plan reads a (B, C, L) signal only: its forward column pass gives the lanes that "
                "a channels-last load runs over the channels to the decimated rows of one channel (run the plain long plan, or "
                "pass a contiguous signal)");
  if (plan->g.bk_T && (x_layout != FC_LONG_NCL || y_layout != FC_LONG_NCL))
    return fail(FC_ERR_UNSUPPORTED, "a blocks plan reads and writes (B, C, L) tensors only: no channels-last build of the blocks "
                "column kernels exists (pass contiguous tensors)");
  if (int e = layout_check(x_layout, "x", plan->g.L, plan->g.Cin, xio)) return e;
  if (int e = layout_check(y_layout, "y", plan->g.nout, plan->g.Cout, yio)) return e;
  const bool x_nlc = x_layout == FC_LONG_NLC, y_nlc = y_layout == FC_LONG_NLC;
  const LongGeom& g = plan->g;
  // (the mapped builds only where the row is read through a padding mode or spread, and where outputs are skipped)
  const bool map_in = g.pad_mode != PAD_CONSTANT || g.up > 1, map_out = g.step > 1;
  hipStream_t st = (hipStream_t)hip_stream;
  for (int64_t s = 0; s < g.slabs; ++s) {
    const int64_t pair0 = s * g.slab_pairs;
    const int64_t np = std::min(g.slab_pairs, g.npairs - pair0);
    LongArgs a = base_args(*plan);
    a.pair0 = (int)pair0;
    a.src = (const float*)x; a.bias = bias; a.y = (float*)y;
    a.src_io = xio; a.y_io = yio;
    a.conj_src = (g.kind & FC_LONG_CONJ_SIGNAL) != 0;
    a.spec = (const f2*)spectrum;
    a.w1 = (f2*)workspace;
    a.w2 = a.w1 + (size_t)(g.slab_pairs * g.Cin * g.N);
    a.C = (int)(g.dc_s ? g.Cin / g.dc_s : g.Cin);      // (the forward pass of a decimation plan counts the tensor's channels)
    if (g.bk_T) {      // (a blocks plan: np pairs of units, the two tensor sides through the block map)
      FC_HIP(plan->cols->cols_fwd_blocks(a, blocks_args(g, g.N), np, st));
      FC_HIP(plan->rows->rows(a, np * g.G * a.nob, st));
      a.C = (int)g.Cout;
      FC_HIP(plan->cols->cols_inv_blocks(a, blocks_args(g, g.N), np, st));
      continue;
    }
    FC_HIP(plan->cols->cols_fwd(a, map_in, x_nlc, np, st));
    FC_HIP(plan->rows->rows(a, np * g.G * a.nob, st));
    a.C = (int)g.Cout;
    if (g.ph_s) {      // (the inverse pass of a phases plan counts filters, and y in its own samples)
      a.C = (int)(g.Cout / g.ph_s);
      a.nout = (int)g.ph_lout;
    }
    FC_HIP(plan->cols->cols_inv(a, map_out, y_nlc, np, st));
  }
  return FC_OK;
}

// ---- gates fused into the column passes (include/fftconv_amd.h "Gated long forward")

int fc_long_forward_gated(const fc_long_plan* plan, const void* x, int x_dtype, const void* pregate, const void* spectrum,
                          const float* bias, void* y, const void* gate, void* y2, const void* gate2, int y_dtype,
                          int y2_dtype, void* workspace, void* hip_stream) {
  if (!plan || !x || !spectrum || !y || !workspace) return fail(FC_ERR_INVALID, "null argument");
  if (plan->d.has_bias && !bias) return fail(FC_ERR_INVALID, "the plan was made with a bias");
  const LongGeom& g = plan->g;
  if (g.kind & FC_LONG_COMPLEX)
    return fail(FC_ERR_UNSUPPORTED, "fc_long_forward_gated takes real plans only: the gated builds of the column kernels read two "
                "real rows per row of the transform (multiply complex tensors around fc_long_forward_io)");
  if (g.ph_s || g.dc_s)
    return fail(FC_ERR_UNSUPPORTED, "fc_long_forward_gated takes neither a phases plan nor a decimation plan: their column passes "
                "give the block layout to phases, and no gated build of those exists");
  if (g.bk_T)
    return fail(FC_ERR_UNSUPPORTED, "fc_long_forward_gated takes no blocks plan: no gated build of the blocks column kernels "
                "exists (multiply around fc_long_forward_io)");
  if (g.pad_mode != PAD_CONSTANT || g.up != 1 || g.dil != 1 || g.step != 1)
    return fail(FC_ERR_UNSUPPORTED, "fc_long_forward_gated takes plans with the default fc_long_ext only (pad_mode constant, "
                "src_up, tap_dil and out_step 1): the gated builds are builds of the unmapped column kernels");
  if (gate2 && !y2) return fail(FC_ERR_INVALID, "gate2 without y2: the second gate belongs to the second result");
  int xio = 0, yio = 0, y2io = 0;
  if (int e = plan_io_code(plan, x_dtype, "x", &xio)) return e;
  if (int e = plan_io_code(plan, y_dtype, "y", &yio)) return e;
  if (int e = plan_io_code(plan, y2 ? y2_dtype : y_dtype, "y2", &y2io)) return e;
  if (y2io != yio && !(y2io == 0 && !gate2))
    return fail(FC_ERR_INVALID, "y2 has dtype code %d and y %d: y2 shares y's element type, or is float32 with no gate2 (the "
                "unrounded c = z + bias of a 16-bit launch)", y2_dtype, y_dtype);
  const LongGates gt = {(const float*)pregate, (const float*)gate, (float*)y2, (const float*)gate2, y2 && y2io != yio};
  const bool gated_out = gate || y2;
  hipStream_t st = (hipStream_t)hip_stream;
  for (int64_t s = 0; s < g.slabs; ++s) {
    const int64_t pair0 = s * g.slab_pairs;
    const int64_t np = std::min(g.slab_pairs, g.npairs - pair0);
    LongArgs a = base_args(*plan);
    a.pair0 = (int)pair0;      // (the gates advance with pair0 as x and y do: the kernels index them by the batch item)
    a.src = (const float*)x; a.bias = bias; a.y = (float*)y;
    a.src_io = xio; a.y_io = yio;
    a.spec = (const f2*)spectrum;
    a.w1 = (f2*)workspace;
    a.w2 = a.w1 + (size_t)(g.slab_pairs * g.Cin * g.N);
    a.C = (int)g.Cin;
    if (pregate) FC_HIP(plan->cols->cols_fwd_gated(a, gt, np, st));
    else FC_HIP(plan->cols->cols_fwd(a, false, false, np, st));
    FC_HIP(plan->rows->rows(a, np * g.G * a.nob, st));
    a.C = (int)g.Cout;
    if (gated_out) FC_HIP(plan->cols->cols_inv_gated(a, gt, np, st));
    else FC_HIP(plan->cols->cols_inv(a, false, false, np, st));
  }
  return FC_OK;
}

// ---- the weight gradient (include/fftconv_amd.h "Weight gradient of a long plan")

int fc_long_wgrad_geometry(const fc_long_wgrad_desc* desc, int64_t info[8]) {
  if (!info) return fail(FC_ERR_INVALID, "null argument");
  WgradGeom w;
  const int st = wgrad_geometry(desc, &w);
  if (st != FC_OK) return st;
  fill_wgrad_info(w, info);
  return FC_OK;
}

int fc_long_wgrad_blocks_geometry(const fc_long_wgrad_desc* desc, int64_t block_points, int64_t info[8], int64_t blocks[4]) {
  if (!info || !blocks) return fail(FC_ERR_INVALID, "null argument");
  WgradGeom w;
  const int st = wgrad_blocks_geometry(desc, block_points, &w);
  if (st != FC_OK) return st;
  fill_wgrad_info(w, info);
  fill_blocks(w.f, blocks);
  return FC_OK;
}

// the element codes of a call and its layouts against the sizes of the plan's tensors
static int wgrad_io(const WgradGeom& w, int x_dtype, int x_layout, int dy_dtype, int dy_layout, int dw_dtype, int* xio,
                    int* dyio, int* dwio) {
  if (int e = io_code(x_dtype, "x", xio)) return e;
  if (int e = io_code(dy_dtype, "dy", dyio)) return e;
  if (int e = io_code(dw_dtype, "dw", dwio)) return e;
  if (int e = layout_check(x_layout, "x", w.f.L, w.f.Cin, *xio)) return e;
  return layout_check(dy_layout, "dy", w.f.nout, w.f.Cout, *dyio);
}

int fc_long_wgrad_check_io(const fc_long_wgrad_desc* desc, int x_dtype, int x_layout, int dy_dtype, int dy_layout,
                           int dw_dtype) {
  WgradGeom w;
  if (int e = wgrad_geometry(desc, &w)) return e;
  int xio = 0, dyio = 0, dwio = 0;
  return wgrad_io(w, x_dtype, x_layout, dy_dtype, dy_layout, dw_dtype, &xio, &dyio, &dwio);
}

// block_points < 0: the plan of the whole row; else by blocks (0: the planner's choice)
static int wgrad_plan_create(const fc_long_wgrad_desc* desc, int64_t block_points, fc_long_wgrad_plan** out_plan) {
  if (!desc || !out_plan) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();
  *out_plan = nullptr;
  std::unique_ptr<fc_long_wgrad_plan> p(new fc_long_wgrad_plan());
  int st = block_points < 0 ? wgrad_geometry(desc, &p->w) : wgrad_blocks_geometry(desc, block_points, &p->w);
  if (st != FC_OK) return st;
  // (the tables and kernels of the forward plan of the layer)
  std::unique_ptr<fc_long_plan> f(new fc_long_plan());
  f->g = p->w.f;
  fc_long_plan* fp = nullptr;
  if ((st = finish_long_plan(f, &fp)) != FC_OK) return st;
  p->f.reset(fp);
  *out_plan = p.release();
  return FC_OK;
}

int fc_long_wgrad_plan_create(const fc_long_wgrad_desc* desc, fc_long_wgrad_plan** out_plan) {
  return wgrad_plan_create(desc, -1, out_plan);
}

int fc_long_wgrad_blocks_plan_create(const fc_long_wgrad_desc* desc, int64_t block_points, fc_long_wgrad_plan** out_plan) {
  if (block_points < 0) return fail(FC_ERR_INVALID, "block_points (%lld) must not be negative", (long long)block_points);
  return wgrad_plan_create(desc, block_points, out_plan);
}

void fc_long_wgrad_plan_destroy(fc_long_wgrad_plan* plan) { delete plan; }

int fc_long_wgrad_plan_info(const fc_long_wgrad_plan* plan, int64_t info[8]) {
  if (!plan || !info) return fail(FC_ERR_INVALID, "null argument");
  fill_wgrad_info(plan->w, info);
  return FC_OK;
}

// fc_long_wgrad and fc_long_wgrad_gated: a side with a gate (NULL: none) runs the gated build of its column pass
static int wgrad_run(const fc_long_wgrad_plan* plan, const void* x, const void* pregate, int x_dtype, int x_layout,
                     const void* dy, const void* postgate, int dy_dtype, int dy_layout, void* dw, int dw_dtype,
                     void* workspace, void* hip_stream) {
  if (!plan || !x || !dy || !dw || !workspace) return fail(FC_ERR_INVALID, "null argument");
  const WgradGeom& w = plan->w;
  int xio = 0, dyio = 0, dwio = 0;
  if (int e = wgrad_io(w, x_dtype, x_layout, dy_dtype, dy_layout, dw_dtype, &xio, &dyio, &dwio)) return e;
  const LongGeom& g = w.f;
  // (the gated builds are builds of the unmapped (B, C, L) column kernel: what the plain call reads through a mapped or a
  // channels-last build takes no gate)
  if (pregate && g.pad_mode != PAD_CONSTANT)
    return fail(FC_ERR_UNSUPPORTED, "fc_long_wgrad_gated takes a pregate on plans with pad_mode constant only: pad_mode %d reads x "
                "through the mapped build of the column kernel, and no gated build of that exists", g.pad_mode);
  if (pregate && x_layout == FC_LONG_NLC)
    return fail(FC_ERR_UNSUPPORTED, "fc_long_wgrad_gated takes a pregate with a (B, C, L) x only: a channels-last x is read by the "
                "channels-last build of the column kernel, and no gated build of that exists");
  if (postgate && g.step > 1)
    return fail(FC_ERR_UNSUPPORTED, "fc_long_wgrad_gated takes a postgate on plans with stride 1 only: at stride %lld dY is read "
                "spread over the grid of the stride by the mapped build of the column kernel, and no gated build of that exists",
                (long long)g.step);
  if (postgate && dy_layout == FC_LONG_NLC)
    return fail(FC_ERR_UNSUPPORTED, "fc_long_wgrad_gated takes a postgate with a (B, C, L) dY only: a channels-last dY is read by "
                "the channels-last build of the column kernel, and no gated build of that exists");
  if (g.bk_T && (pregate || postgate))
    return fail(FC_ERR_UNSUPPORTED, "fc_long_wgrad_gated takes no gate on a blocks plan: no gated build of the blocks column "
                "kernel exists (multiply before fc_long_wgrad)");
  if (g.bk_T && (x_layout != FC_LONG_NCL || dy_layout != FC_LONG_NCL))
    return fail(FC_ERR_UNSUPPORTED, "a weight gradient by blocks reads (B, C, L) tensors only: no channels-last build of the "
                "blocks column kernel exists (pass contiguous tensors)");
  const fc_long_plan& fp = *plan->f;
  hipStream_t st = (hipStream_t)hip_stream;
  f2* const w1x = (f2*)workspace;
  f2* const w1dy = w1x + (size_t)(w.slab_pairs * g.Cin * g.N);
  f2* const w2 = w1dy + (size_t)(w.slab_pairs * g.Cout * g.N);
  const int64_t nob = (g.Cog + w.ob - 1) / w.ob;
  for (int64_t s = 0; s < w.slabs; ++s) {
    const int64_t pair0 = s * w.slab_pairs;
    const int64_t np = std::min(w.slab_pairs, g.npairs - pair0);
    // x: the rows the forward reads, its padding mode and paddings
    LongArgs a = base_args(fp);
    a.pair0 = (int)pair0;
    a.src = (const float*)x; a.src_io = xio;
    a.w1 = w1x;
    a.C = (int)g.Cin;
    if (g.bk_T) FC_HIP(fp.cols->cols_fwd_blocks(a, blocks_args(g, g.N), np, st));      // (the N-point window of each unit)
    else if (pregate) FC_HIP(fp.cols->cols_fwd_gated(a, LongGates{(const float*)pregate}, np, st));
    else FC_HIP(fp.cols->cols_fwd(a, g.pad_mode != PAD_CONSTANT, x_layout == FC_LONG_NLC, np, st));
    // dY: rows of nout samples spread over the grid of the stride, zero elsewhere
    LongArgs b = base_args(fp);
    b.pair0 = (int)pair0;
    b.src = (const float*)dy; b.src_io = dyio;
    b.w1 = w1dy;
    b.C = (int)g.Cout;
    b.L = (int)g.nout; b.padl = 0;
    b.pad_mode = PAD_CONSTANT; b.mpadl = 0; b.mpadr = 0;
    b.src_up = (int)g.step; b.d_up = make_fastdiv((unsigned)g.step);
    // (the gated build reads the words above -- L, padl, C -- and the gate, which lies as dY does, in LongGates::pregate)
    // (by blocks: the V samples each unit keeps, [t*V, t*V + V) of the row; the rest of the block reads zero)
    if (g.bk_T) FC_HIP(fp.cols->cols_fwd_blocks(b, blocks_args(g, g.bk_V), np, st));
    else if (postgate) FC_HIP(fp.cols->cols_fwd_gated(b, LongGates{(const float*)postgate}, np, st));
    else FC_HIP(fp.cols->cols_fwd(b, g.step > 1, dy_layout == FC_LONG_NLC, np, st));
    // the product summed over the pairs of the slab, transformed back into W2 (a later slab adds)
    LongArgs r = base_args(fp);
    r.w1 = w1x; r.spec = w1dy; r.w2 = w2;
    r.B = (int)np;
    r.spec_mode = s > 0;
    r.ob = w.ob; r.nob = (int)nob;
    r.C = 1;
    FC_HIP(fp.rows->wgrad_rows(r, g.G * g.Cig * nob, st));
  }
  // one item of Cout * Cin/g rows: lag dilation * q -> the element of tap q, the imaginary part dropped
  LongArgs c = base_args(fp);
  c.B = 1; c.pair0 = 0;
  c.w2 = w2;
  c.y = (float*)dw; c.y_io = dwio; c.bias = nullptr;
  c.C = (int)w.rows;
  c.d_ostep = make_fastdiv((unsigned)g.dil);
  FC_HIP(fp.cols->wgrad_inv(c, st));
  // the elements whose tap meets no data for any output: zero (two strided fills, in front of and behind the kept taps)
  const int64_t es = io_bytes(dwio);
  const int64_t first = g.tstep > 0 ? g.tap0 : g.tap0 - (g.keff - 1), behind = g.K - (first + g.keff);
  if (first > 0)
    FC_HIP(hipMemset2DAsync(dw, (size_t)(g.K * es), 0, (size_t)(first * es), (size_t)w.rows, st));
  if (behind > 0)
    FC_HIP(hipMemset2DAsync((char*)dw + (first + g.keff) * es, (size_t)(g.K * es), 0, (size_t)(behind * es), (size_t)w.rows, st));
  return FC_OK;
}

int fc_long_wgrad(const fc_long_wgrad_plan* plan, const void* x, int x_dtype, int x_layout, const void* dy, int dy_dtype,
                  int dy_layout, void* dw, int dw_dtype, void* workspace, void* hip_stream) {
  return wgrad_run(plan, x, nullptr, x_dtype, x_layout, dy, nullptr, dy_dtype, dy_layout, dw, dw_dtype, workspace, hip_stream);
}

int fc_long_wgrad_gated(const fc_long_wgrad_plan* plan, const void* x, const void* pregate, int x_dtype, int x_layout,
                        const void* dy, const void* postgate, int dy_dtype, int dy_layout, void* dw, int dw_dtype,
                        void* workspace, void* hip_stream) {
  return wgrad_run(plan, x, pregate, x_dtype, x_layout, dy, postgate, dy_dtype, dy_layout, dw, dw_dtype, workspace, hip_stream);
}

}  // extern "C"
