// host_f64.cpp -- float64 plans: the direct time-domain kernel (PlanKind::F64_DIRECT, direct_f64.hip), 1-D FFTs in
// tiles (F64_FFT_1D, fft_f64.hip) or as one long transform (F64_FFT_LONG, long_f64.hip) and 2-D / 3-D FFTs (F64_FFT_ND,
// nd_f64.hip): the choice between them, their tiles and sizes, kernel transforms and forwards.  Chosen from the descriptor alone, with no device query: float64 plans can be
// made anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "direct_f64.h"
#include "fft_f64.h"
#include "long_f64.h"
#include "nd_f64.h"
#include "fc_plan.h"

namespace fc {

// float64 2-D / 3-D plans (forward and transposed) leave the direct kernel from this many of its multiply-adds per
// output of the FFT path: Cin/g x prod(k), divided by prod(stride) for a forward plan (its FFT computes every
// stride-1 output and decimates).  MI355X sweep (profiles/r04_float64_nd.txt): the FFT path runs 0.36-1.0x as fast
// as the direct kernel at 4-72, 1.6-15x at 125-2744 (2-D B4 128^2 and 3-D B2 32^3, 1 and 8 input channels, k 2-7);
// stride-2 forward rows 0.52-0.95x at 18-50 and 1.65-2.6x at 98-196 (per stride-1 output); stride-2 transposed rows,
// whose direct kernel still walks every tap, 1.4-4.9x at 128-1024 undivided.
static const int64_t kF64MinMacs = 100;

// One axis of a float64 N-d plan: one transform of nextpow2(Sp) points while that is <= 2048, else overlap-save tiles
// of T >= 2 kd points (V = T - kd + 1 valid samples each) or of 2048 points (V >= 1024 for any kd <= 1025); the fewest
// transformed points n*T, the shorter tile on a tie (an axis just past a power of two takes several short tiles rather
// than one transform of twice its length).  Returns false if no tile fits (kd > 2048).
static bool f64_axis_plan(int64_t Sp, int64_t Lf, int64_t kd, int* T_out, int* V_out, int* nt_out) {
  int64_t best_cost = -1;
  int best_T = 0;
  auto consider = [&](int T) {
    const int64_t V = T - kd + 1;
    if (V < 1) return;
    const int64_t cost = (Lf + V - 1) / V * T;
    if (best_cost < 0 || cost < best_cost || (cost == best_cost && T < best_T)) { best_cost = cost; best_T = T; }
  };
  int Ts = 8;
  while (Ts < Sp) Ts *= 2;
  if (Ts <= 2048) consider(Ts);
  for (int T = 8; T <= 2048; T *= 2)
    if (T >= 2 * kd || T == 2048) consider(T);
  if (best_T == 0) return false;
  *T_out = best_T;
  *V_out = (int)(best_T - kd + 1);
  *nt_out = (int)((Lf + *V_out - 1) / *V_out);
  return true;
}

// float64 2-D / 3-D plan on the FFT path (nd_f64.hip): per-axis transforms, channel blocking of the fused pass,
// kernel-spectrum and workspace sizes.  Axis 0 = outermost (fused pass), nd-1 = rows, 1 = middle (3-D).  Returns false,
// with the plan untouched (the direct kernel's state), when an axis gets no transform or a launch would exceed what one
// dispatch can address (2^31 workgroups, 2^32 work-items).
static bool plan_nd_f64(fc_plan* p) {
  const fc_desc& d = p->d;
  const int nd = p->nd;
  int T[3] = {0, 0, 0}, V[3] = {0, 0, 0}, nt[3] = {0, 0, 0};
  for (int i = 0; i < nd; ++i)
    if (!f64_axis_plan(p->Sp[i], p->Lf[i], p->kd[i], &T[i], &V[i], &nt[i])) return false;
  const int Tx = T[nd - 1], Fx = Tx / 2 + 1;
  const size_t B = (size_t)d.batch, Ci = (size_t)d.in_channels, Co = (size_t)d.out_channels, NA = Co * p->Cig;
  const size_t Ncol = (size_t)nt[nd - 1] * Fx;
  const size_t t_outer = (size_t)T[0] * (nd == 3 ? (size_t)T[1] : 1);
  const size_t spectrum_bytes = (size_t)d.groups * p->Cog * p->Cig * t_outer * Fx * sizeof(double2);
  // fused pass: 8 accumulator slots per thread and bin, shared by nb batch items x cob output channels; spare slots
  // (few output channels) and a large kernel spectrum both make batch items share each read of it
  int cob = std::min(8, p->Cog), nb = 1;
  if (cob <= 2 && d.batch >= 3) nb = 4;
  else if (cob <= 4 && d.batch >= 2) nb = 2;
  else if (spectrum_bytes >= ((size_t)32 << 20) && d.batch >= 2) { nb = 2; cob = 4; }
  // every launch of the forward and of the kernel transform within one dispatch (grid and work-items as nd_f64.hip)
  bool fits = true;
  auto launch = [&](int t, size_t seqs) {        // seqs: sequences (column groups count NS sequences each)
    const size_t ns = (size_t)fc::nd_f64_nseq(t), grid = (seqs + ns - 1) / ns;
    fits = fits && grid < ((size_t)1 << 31) && grid * ns * (size_t)(t / 2) < ((size_t)1 << 32);
  };
  auto cols = [&](int t, size_t lines, size_t ncol) {
    const size_t ns = (size_t)fc::nd_f64_nseq(t);
    launch(t, lines * ((ncol + ns - 1) / ns) * ns);
  };
  size_t rows_in = B * Ci, rows_out = B * Co, krows = NA;
  for (int i = 0; i < nd - 1; ++i) { rows_in *= d.spatial[i]; rows_out *= p->out_sp[i]; krows *= d.kernel[i]; }
  launch(Tx, (rows_in + 1) / 2 * nt[nd - 1]);
  launch(Tx, (krows + 1) / 2);
  launch(Tx, (rows_out + 1) / 2 * nt[nd - 1]);
  size_t ncol_outer = Ncol, a, b;
  if (nd == 3) {
    const size_t Mcol = (size_t)nt[1] * T[1] * Ncol;
    cols(T[1], B * Ci * d.spatial[0] * nt[1], Ncol);                 // middle axis forward
    cols(T[1], B * Co * p->out_sp[0] * nt[1], Ncol);                 // and back
    cols(T[1], NA * d.kernel[0], Fx);                                // kernel: middle axis
    cols(T[0], NA, (size_t)T[1] * Fx);                               // kernel: outer axis
    ncol_outer = Mcol;
    a = std::max({B * Ci * d.spatial[0] * d.spatial[1] * Ncol, NA * d.kernel[0] * d.kernel[1] * Fx,   // rows
                  B * Co * p->out_sp[0] * Mcol});                                                     // fused pass out
    b = std::max({B * Ci * d.spatial[0] * Mcol, NA * d.kernel[0] * T[1] * Fx,                        // middle axis
                  B * Co * p->out_sp[0] * p->out_sp[1] * Ncol});                                      // middle axis back
  } else {
    cols(T[0], NA, Fx);                                              // kernel: outer axis
    a = std::max(B * Ci * d.spatial[0] * Ncol, NA * d.kernel[0] * Fx);          // rows of the signal / of the taps
    b = B * Co * p->out_sp[0] * Ncol;                                              // after the fused pass
  }
  cols(T[0], (B + nb - 1) / nb * d.groups * ((p->Cog + cob - 1) / cob) * nt[0], ncol_outer);   // fused pass
  if (!fits) return false;
  for (int i = 0; i < nd; ++i) { p->f64.t[i] = T[i]; p->f64.v[i] = V[i]; p->f64.nt[i] = nt[i]; }
  p->f64.T = Tx;
  p->spectrum_bytes = spectrum_bytes;
  p->ws_a = a;
  p->ws_b = b;
  p->workspace_bytes = (a + b) * sizeof(double2);
  p->f64.cob = cob;
  p->f64.nb = nb;
  return true;
}

// ---- 1-D plans whose dilated extent no 2048-point tile holds: one cyclic transform of N = N1 x N2 points (long_f64.hip)

// The long route's work follows N log2 N per row whatever the outputs kept; the direct kernel's is nout x Cin/g x K per
// (batch, output channel) row.  The long route is taken from kF64LongC multiply-adds of the direct kernel per
// transformed point and stage: nout * Cig * K >= kF64LongC * ntiles * N * log2(N).
// MI355X sweep (profiles/f64_long.jsonl, scripts/f64_long_bench.py --sweep): not measured yet.
static const double kF64LongC = 4.0;
static const int64_t kF64LongMaxN = (int64_t)1 << 22;      // 2048 x 2048: the 2048-point transform takes 80 KiB of LDS

static bool long_tile_len(long long v) { return v >= 64 && v <= 2048 && (v & (v - 1)) == 0; }

// Fills the plan and sets *taken when the plan runs the long route; leaves it untouched (the direct kernel's state)
// otherwise.  `force`: FFTCONV_F64_LONG=2, no crossover.  Fails on a bad FFTCONV_F64_LONG_N only.
static int plan_long_f64(fc_plan* p, bool force, bool* taken) {
  *taken = false;
  const fc_desc& d = p->d;
  const int64_t kd = p->kd[0], Lf = p->Lf[0], need = p->need[0];
  if ((int64_t)p->Sp[0] + kF64LongMaxN >= ((int64_t)1 << 31)) return FC_OK;     // (padded positions are 32-bit in the kernels)
  // smallest N = N1 * N2 >= need (zero padding absorbs the wrap, fc_api.cpp) with both factors 64 .. 2048; the most
  // balanced split, N2 >= N1
  int lg = 12;
  while (((int64_t)1 << lg) < need && lg < 22) ++lg;
  int64_t n1 = (int64_t)1 << (lg / 2), n2 = (int64_t)1 << (lg - lg / 2);
  bool forced_n = false;
  if (const char* env = getenv("FFTCONV_F64_LONG_N")) {
    if (*env) {
      long long a = 0, b = 0;
      char tail = 0;
      if (sscanf(env, "%lldx%lld%c", &a, &b, &tail) != 2 || !long_tile_len(a) || !long_tile_len(b))
        return fail(FC_ERR_INVALID, "FFTCONV_F64_LONG_N=%s: expected <N1>x<N2>, both powers of two from 64 to 2048", env);
      n1 = a; n2 = b; forced_n = true;
    }
  }
  const int64_t N = n1 * n2;
  // rows that need more than N points: overlap-save tiles of one transform each, V valid samples per tile
  int64_t V = Lf, ntiles = 1;
  if (N < need) {
    V = N - kd + 1;
    if (V < N / 2) {
      if (forced_n)
        return fail(FC_ERR_INVALID, "FFTCONV_F64_LONG_N=%s holds %lld points, of which a kernel extent of %lld leaves %lld "
                    "valid: fewer than half", getenv("FFTCONV_F64_LONG_N"), (long long)N, (long long)kd, (long long)(V > 0 ? V : 0));
      return FC_OK;
    }
    ntiles = (Lf + V - 1) / V;
  }
  int lgN = 0;
  while (((int64_t)1 << lgN) < N) ++lgN;
  if (!force && (double)p->out_sp[0] * p->Cig * (double)d.kernel[0] < kF64LongC * (double)ntiles * (double)N * lgN) return FC_OK;
  const int nc = fc::long_f64_nc((int)n1), nr = fc::long_f64_nr((int)n2);
  const int64_t npairs = (d.batch + 1) / 2;
  // output channels per workgroup of the row pass: the rule of the tiled 1-D plan (8, fewer while CUs would idle)
  int cob = 8;
  while (cob > 2 && npairs * d.groups * ((p->Cog + cob - 1) / cob) * (n1 / nr) < 256) cob /= 2;
  cob = std::min(cob, std::max(p->Cog, 1));
  const int64_t n_ochunks = (p->Cog + cob - 1) / cob;
  // batch pairs run in slabs under the workspace budget (W1 + W2 of one slab), every grid below 2^31 workgroups
  int64_t budget_mb = 8192;
  if (const char* env = getenv("FFTCONV_LONG_WS_MB"))
    if (*env && atoll(env) > 0) budget_mb = atoll(env);
  const int64_t pair_bytes = (d.in_channels + d.out_channels) * N * (int64_t)sizeof(double2);
  const int64_t pair_grid = std::max({d.in_channels * (n2 / nc), d.groups * n_ochunks * (n1 / nr), d.out_channels * (n2 / nc)});
  if (pair_grid > 0x7fffffffLL) return FC_OK;
  int64_t slab_pairs = std::max<int64_t>(1, std::min<int64_t>(npairs, (budget_mb << 20) / pair_bytes));
  slab_pairs = std::min<int64_t>(slab_pairs, 0x7fffffffLL / pair_grid);
  p->f64.N1 = (int)n1; p->f64.N2 = (int)n2; p->f64.T = (int)n2;
  p->f64.V = (int)V; p->f64.ntiles = (int)ntiles; p->f64.cob = cob;
  p->f64.npairs = npairs; p->f64.slab_pairs = slab_pairs;
  p->Lfull = (int)Lf;
  p->spectrum_bytes = (size_t)d.out_channels * p->Cig * (size_t)N * sizeof(double2);
  p->workspace_bytes = (size_t)(slab_pairs * pair_bytes);
  p->kind = PlanKind::F64_FFT_LONG;
  *taken = true;
  return FC_OK;
}

int plan_f64(fc_plan* p) {
  const fc_desc& d = p->d;
  // float64: direct time-domain kernel (direct_f64.hip); the "kernel spectrum" is the weight tensor itself
  p->kind = PlanKind::F64_DIRECT;
  size_t nw = (size_t)(d.transposed ? d.in_channels : d.out_channels) * (size_t)((d.transposed ? d.out_channels : d.in_channels) / d.groups);
  for (int i = 0; i < d.ndim; ++i) nw *= (size_t)d.kernel[i];
  p->spectrum_bytes = nw * sizeof(double);
  p->workspace_bytes = 0;
  p->tile = nullptr;
  // The FFT paths in double precision: 1-D plans, forward and transposed, with at least 16 taps (fft_f64.hip);
  // 2-D / 3-D plans, forward and transposed, from kF64MinMacs multiply-adds of the direct kernel per output of the FFT
  // path (nd_f64.hip).
  // A dilated extent past 1025 keeps the direct kernel on a 2-D / 3-D plan; a 1-D plan takes one long transform of
  // N1 x N2 points per row (long_f64.hip) from the crossover of plan_long_f64 on.  FFTCONV_F64_FFT=0 keeps the direct
  // kernel for everything (A/B runs, tests).  Chosen from the descriptor alone, with no device query: float64 plans can
  // be made anywhere.  FFTCONV_F64_FFT=2 (crossover sweeps) takes the 2-D / 3-D FFT path at any size.
  // FFTCONV_F64_LONG=0 keeps the direct kernel for the long 1-D plans, =2 takes the long transform for any 1-D plan of at
  // least 16 taps; FFTCONV_F64_LONG_N=<N1>x<N2> forces its factorisation.  Both are read here, at plan creation.
  const char* env = getenv("FFTCONV_F64_FFT");
  const bool fft_on = !env || atoi(env) != 0;
  const bool force_nd = env && atoi(env) == 2;
  int64_t macs = p->Cig, strides = 1;      // multiply-adds of the direct kernel per output (x strides: per FFT output)
  bool kd_ok = true;
  for (int i = 0; i < d.ndim; ++i) {
    macs *= d.kernel[i];
    if (!d.transposed) strides *= d.stride[i];
    kd_ok = kd_ok && p->kd[i] <= 1025;
  }
  const char* lenv = getenv("FFTCONV_F64_LONG");
  const int long_knob = lenv && *lenv ? atoi(lenv) : 1;
  if (fft_on && d.ndim == 1 && long_knob != 0 && (p->kd[0] > 1025 || (long_knob == 2 && d.kernel[0] >= 16))) {
    bool taken = false;
    if (int rc = plan_long_f64(p, long_knob == 2, &taken)) return rc;
    if (taken) return FC_OK;
  }
  if (fft_on && kd_ok && d.ndim == 1 && d.kernel[0] >= 16 &&
      (int64_t)d.batch * d.groups * ((p->out_sp[0] + 255) / 256) < 0x40000000) {
    int T = 256;
    while (T < 2 * p->kd[0] && T < 2048) T *= 2;
    // a longer tile wastes less of itself on the overlap; taken while the launch still has two workgroups per CU
    while (T < 2048) {
      const int64_t V2 = 2 * T - p->kd[0] + 1, tiles2 = (p->Lf[0] + V2 - 1) / V2;
      if (d.batch * d.groups * ((p->Cog + 7) / 8) * tiles2 < 512) break;
      T *= 2;
    }
    p->f64.T = T;
    p->f64.V = (int)(T - p->kd[0] + 1);
    p->f64.ntiles = (int)((p->Lf[0] + p->f64.V - 1) / p->f64.V);
    // output channels per workgroup: 8, fewer (even) while the launch would leave CUs idle -- a workgroup's life is its
    // transforms in a row (Cig/2 forward + cob/2 inverse), so small launches gain from more, shorter workgroups
    int cob = 8;
    while (cob > 2 && d.batch * d.groups * ((p->Cog + cob - 1) / cob) * p->f64.ntiles < 256) cob /= 2;   // (fewer workgroups than CUs)
    p->f64.cob = std::min(cob, std::max(p->Cog, 1));
    p->Lfull = p->Lf[0];
    p->spectrum_bytes = (size_t)d.out_channels * p->Cig * T * 2 * sizeof(double);
    p->kind = PlanKind::F64_FFT_1D;
  } else if (fft_on && kd_ok && d.ndim > 1 && (force_nd || macs >= kF64MinMacs * strides)) {
    if (plan_nd_f64(p)) p->kind = PlanKind::F64_FFT_ND;   // false: the direct kernel, as set up above
  }
  return FC_OK;
}

static void fill_f64_args(const fc_plan& p, fc::FftF64Args* a) {
  a->B = (int)p.d.batch; a->Cin = (int)p.d.in_channels; a->Cout = (int)p.d.out_channels; a->G = (int)p.d.groups;
  a->Cig = p.Cig; a->Cog = p.Cog;
  a->L = (int)p.d.spatial[0]; a->pad = p.padl[0]; a->pad_mode = p.d.padding_mode;
  a->K = (int)p.d.kernel[0]; a->dil = (int)p.d.dilation[0]; a->stride = p.ostride[0];
  a->up = p.up[0]; a->transposed = p.d.transposed;
  a->T = p.f64.T; a->V = p.f64.V; a->ntiles = p.f64.ntiles; a->Lfull = p.Lf[0]; a->Lout = (int)p.out_sp[0];
  a->cob = p.f64.cob; a->n_ochunks = (p.Cog + p.f64.cob - 1) / p.f64.cob;
}

// ---- direct kernel: the "kernel spectrum" is a copy of the weights
int transform_kernel_f64_direct(const fc_plan& p, const float* weight, void* w_hat, void*, hipStream_t st) {
  FC_HIP(hipMemcpyAsync(w_hat, weight, p.spectrum_bytes, hipMemcpyDeviceToDevice, st));
  return FC_OK;
}

int forward_f64_direct(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void*,
                       hipStream_t st, void* stamps) {
  if (stamps) return fail(FC_ERR_UNSUPPORTED, "no timestamp hook in the float64 kernel");
  fc::DirectF64Args a{};
  a.x = (const double*)x; a.w = (const double*)w_hat; a.bias = p.d.has_bias ? (const double*)bias : nullptr; a.y = (double*)y;
  a.B = (int)p.d.batch; a.Cin = (int)p.d.in_channels; a.Cout = (int)p.d.out_channels; a.G = (int)p.d.groups;
  a.pad_mode = p.d.padding_mode; a.transposed = p.d.transposed;
  for (int i = 0; i < 3; ++i) {          // axes right-aligned: leading axes of extent 1 for 1-D / 2-D
    const int ax = i - (3 - p.nd);
    const bool live = ax >= 0;
    a.S[i] = live ? (int)p.d.spatial[ax] : 1; a.K[i] = live ? (int)p.d.kernel[ax] : 1; a.O[i] = live ? (int)p.out_sp[ax] : 1;
    a.stride[i] = live ? (int)p.d.stride[ax] : 1; a.pad[i] = live ? (int)p.d.padding[ax] : 0; a.dil[i] = live ? (int)p.d.dilation[ax] : 1;
  }
  FC_HIP(fc::launch_direct_f64(a, st));
  return FC_OK;
}

// ---- 1-D FFTs (fft_f64.hip)
int transform_kernel_f64_1d(const fc_plan& p, const float* weight, void* w_hat, void*, hipStream_t st) {
  fc::FftF64Args a{};
  fill_f64_args(p, &a);
  a.w = (const double*)weight; a.wspec = (double2*)w_hat;
  FC_HIP(fc::launch_fft_f64(0, a, st));
  return FC_OK;
}

int forward_f64_1d(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void*,
                   hipStream_t st, void* stamps) {
  if (stamps) return fail(FC_ERR_UNSUPPORTED, "no timestamp hook in the float64 kernels");
  fc::FftF64Args a{};
  fill_f64_args(p, &a);
  a.x = (const double*)x; a.wspec = (double2*)const_cast<void*>(w_hat); a.bias = p.d.has_bias ? (const double*)bias : nullptr;
  a.y = (double*)y;
  FC_HIP(fc::launch_fft_f64(1, a, st));
  return FC_OK;
}

// ---- 1-D, one long transform per row (long_f64.hip)
static fc::LongF64Args long_f64_args(const fc_plan& p) {
  fc::LongF64Args a{};
  a.N1 = p.f64.N1; a.N2 = p.f64.N2;
  while ((1 << a.lgN2) < a.N2) ++a.lgN2;
  a.B = (int)p.d.batch; a.G = (int)p.d.groups; a.Cig = p.Cig; a.Cog = p.Cog;
  a.cob = p.f64.cob; a.n_ochunks = (p.Cog + p.f64.cob - 1) / p.f64.cob;
  a.L = (int)p.d.spatial[0]; a.pad = p.padl[0]; a.pad_mode = p.d.padding_mode; a.up = p.up[0];
  a.K = (int)p.d.kernel[0]; a.dil = (int)p.d.dilation[0]; a.transposed = p.d.transposed;
  a.stride = p.ostride[0]; a.Lout = (int)p.out_sp[0];
  a.scale = 1.0 / ((double)p.f64.N1 * (double)p.f64.N2);
  return a;
}

// kernel spectrum: the forward column pass on the dilated taps (flipped, channels exchanged for a transposed plan) and
// the row pass in its filter mode, which conjugates and scales by 1/N; the filter rows go through the workspace a chunk
// at a time (it holds at least Cin + Cout >= 2 rows of N points)
int transform_kernel_f64_long(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st) {
  const int64_t N = (int64_t)p.f64.N1 * p.f64.N2;
  const int64_t rows_total = p.d.out_channels * (int64_t)p.Cig;
  const int64_t fit = std::max<int64_t>(1, (int64_t)(p.workspace_bytes / ((size_t)N * sizeof(double2))));
  const int64_t grid_cap = 0x7fffffffLL / std::max(p.f64.N2 / fc::long_f64_nc(p.f64.N1), p.f64.N1 / fc::long_f64_nr(p.f64.N2));
  const int64_t chunk = std::min(fit, grid_cap);
  for (int64_t r0 = 0; r0 < rows_total; r0 += chunk) {
    const int64_t n = std::min(chunk, rows_total - r0);
    fc::LongF64Args a = long_f64_args(p);
    a.from_kernel = 1; a.row0 = (int)r0;
    a.src = (const double*)weight; a.w1 = (double2*)workspace;
    FC_HIP(fc::launch_long_f64_cols_fwd(a, n, st));
    a.spec_mode = 1;
    a.spec_out = (double2*)w_hat + (size_t)r0 * N;
    FC_HIP(fc::launch_long_f64_rows(a, n, st));
  }
  return FC_OK;
}

// forward: three launches per slab of batch pairs and tile
int forward_f64_long(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
                     hipStream_t st, void* stamps) {
  if (stamps) return fail(FC_ERR_UNSUPPORTED, "no timestamp hook in the float64 kernels");
  const int64_t N = (int64_t)p.f64.N1 * p.f64.N2;
  const int64_t Cin = p.d.in_channels, Cout = p.d.out_channels;
  for (int64_t pair0 = 0; pair0 < p.f64.npairs; pair0 += p.f64.slab_pairs) {
    const int64_t np = std::min(p.f64.slab_pairs, p.f64.npairs - pair0);
    for (int tile = 0; tile < p.f64.ntiles; ++tile) {
      fc::LongF64Args a = long_f64_args(p);
      a.pair0 = (int)pair0;
      a.src = (const double*)x; a.bias = p.d.has_bias ? (const double*)bias : nullptr; a.y = (double*)y;
      a.spec = (const double2*)w_hat;
      a.w1 = (double2*)workspace;
      a.w2 = a.w1 + (size_t)(p.f64.slab_pairs * Cin * N);
      a.p0 = a.t0 = tile * p.f64.V;                    // (one tile: V = Lf, the whole stride-1 result)
      a.limit = std::min(p.f64.V, p.Lf[0] - a.t0);
      a.C = (int)Cin;
      FC_HIP(fc::launch_long_f64_cols_fwd(a, np * Cin, st));
      FC_HIP(fc::launch_long_f64_rows(a, np * p.d.groups * a.n_ochunks, st));
      a.C = (int)Cout;
      FC_HIP(fc::launch_long_f64_cols_inv(a, np * Cout, st));
    }
  }
  return FC_OK;
}

// ---- 2-D / 3-D FFTs (nd_f64.hip).  Axis 0 = outermost, nd-1 = rows (x), 1 = middle (3-D); see nd_f64.h for layouts.
// kernel spectrum: the forward passes on the dilated taps (flipped, channels exchanged for a transposed plan), the
// last one conjugating and scaling by 1/prod(T); ndim launches
int transform_kernel_f64_nd(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st) {
  const double* w = (const double*)weight;
  double2* H = (double2*)w_hat;
  double2* ws = (double2*)workspace;
  const int nd = p.nd, X = nd - 1;
  const int Tx = p.f64.t[X], Fx = Tx / 2 + 1;
  const long long NA = p.d.out_channels * (long long)p.Cig;
  const int flip = p.d.transposed;
  double2* wsA = ws;
  double2* wsB = ws + p.ws_a;
  fc::RowsF64Args r{};
  r.src = w; r.dst = wsA;
  r.NR = nd == 3 ? (int)(p.d.kernel[0] * p.d.kernel[1]) : (int)p.d.kernel[0];
  r.R = NA * r.NR; r.Sx = (int)p.d.kernel[X];
  r.T = Tx; r.V = Tx; r.nt = 1; r.Fx = Fx;
  r.from_kernel = 1; r.K = (int)p.d.kernel[X]; r.dil = (int)p.d.dilation[X]; r.kd = (int)p.kd[X]; r.flip = flip;
  if (flip) { r.tw_Cig = p.Cig; r.tw_Cog = p.Cog; }
  FC_HIP(fc::launch_rows_r2c_f64(r, st));
  double scale = 1.0;
  for (int i = 0; i < nd; ++i) scale /= (double)p.f64.t[i];
  fc::ColF64Args c{};
  c.mode = 1; c.nt = 1; c.flip = flip;
  if (nd == 3) {
    // rows [img][kz][ky][Fx] -> [img][kz][Ty][Fx]
    const int Ty = p.f64.t[1];
    c.src = wsA; c.dst = wsB; c.nlines = NA * p.d.kernel[0]; c.ncol = Fx; c.T = Ty; c.V = Ty;
    c.src_line = p.d.kernel[1] * (long long)Fx; c.src_pt = Fx;
    c.dst_line = (long long)Ty * Fx; c.dst_pt = Fx; c.dst_tile = 0;
    c.K = (int)p.d.kernel[1]; c.dil = (int)p.d.dilation[1]; c.kd = (int)p.kd[1];
    FC_HIP(fc::launch_col_f64(c, st));
    // [img][kz][Ty*Fx] -> H[img][Tz][Ty*Fx]
    const int Tz = p.f64.t[0];
    c.src = wsB; c.dst = H; c.nlines = NA; c.ncol = Ty * Fx; c.T = Tz; c.V = Tz;
    c.src_line = p.d.kernel[0] * (long long)Ty * Fx; c.src_pt = (long long)Ty * Fx;
    c.dst_line = (long long)Tz * Ty * Fx; c.dst_pt = (long long)Ty * Fx;
    c.K = (int)p.d.kernel[0]; c.dil = (int)p.d.dilation[0]; c.kd = (int)p.kd[0];
  } else {
    // rows [img][ky][Fx] -> H[img][Ty][Fx]
    const int Ty = p.f64.t[0];
    c.src = wsA; c.dst = H; c.nlines = NA; c.ncol = Fx; c.T = Ty; c.V = Ty;
    c.src_line = p.d.kernel[0] * (long long)Fx; c.src_pt = Fx;
    c.dst_line = (long long)Ty * Fx; c.dst_pt = Fx;
    c.K = (int)p.d.kernel[0]; c.dil = (int)p.d.dilation[0]; c.kd = (int)p.kd[0];
  }
  c.conj_scale = 1; c.scale = scale;
  FC_HIP(fc::launch_col_f64(c, st));
  return FC_OK;
}

// forward: rows, (middle,) fused outer pass, (middle back,) rows back -- three launches in 2-D, five in 3-D
int forward_f64_nd(const fc_plan& p, const float* xf, const void* w_hat, const float* bias_f, float* yf, void* workspace,
                   hipStream_t st, void* stamps) {
  if (stamps) return fail(FC_ERR_UNSUPPORTED, "no timestamp hook in the float64 kernels");
  const double* x = (const double*)xf;
  const double2* H = (const double2*)w_hat;
  const double* bias = p.d.has_bias ? (const double*)bias_f : nullptr;
  double* y = (double*)yf;
  double2* ws = (double2*)workspace;
  const int nd = p.nd, X = nd - 1;
  const int Tx = p.f64.t[X], Fx = Tx / 2 + 1;
  const long long B = p.d.batch, Ci = p.d.in_channels, Co = p.d.out_channels;
  const long long Ncol = (long long)p.f64.nt[X] * Fx;
  double2* wsA = ws;
  double2* wsB = ws + p.ws_a;
  // rows of the signal: (b, ci, [z,] y) rows that exist in the input
  fc::RowsF64Args r{};
  r.src = x; r.dst = wsA;
  r.NR = 1;
  for (int i = 0; i < X; ++i) r.NR *= (int)p.d.spatial[i];
  r.R = B * Ci * r.NR; r.Sx = (int)p.d.spatial[X];
  r.T = Tx; r.V = p.f64.v[X]; r.nt = p.f64.nt[X]; r.Fx = Fx; r.mx = axis_map(p, X);
  FC_HIP(fc::launch_rows_r2c_f64(r, st));
  const double2* fsrc = wsA;
  long long ncol = Ncol, Tmid = 1;
  if (nd == 3) {
    // middle axis: [img*Sz][Sy][Ncol] -> [img*Sz][nty*Ty][Ncol]
    const int Ty = p.f64.t[1];
    fc::ColF64Args c{};
    c.mode = 0; c.src = wsA; c.dst = wsB; c.nlines = B * Ci * p.d.spatial[0]; c.ncol = (int)Ncol;
    c.T = Ty; c.V = p.f64.v[1]; c.nt = p.f64.nt[1]; c.m = axis_map(p, 1);
    c.src_line = p.d.spatial[1] * Ncol; c.src_pt = Ncol;
    c.dst_line = (long long)p.f64.nt[1] * Ty * Ncol; c.dst_tile = (long long)Ty * Ncol; c.dst_pt = Ncol;
    FC_HIP(fc::launch_col_f64(c, st));
    fsrc = wsB;
    ncol = c.dst_line;
    Tmid = Ty;
  }
  // outermost axis: [b*Cin + ci][S0][ncol] -> [b*Cout + co][O0][ncol]
  fc::FusedF64Args f{};
  f.src = fsrc; f.H = H; f.dst = nd == 3 ? wsA : wsB;
  f.ncol = (int)ncol; f.src_img = p.d.spatial[0] * ncol; f.src_pt = ncol;
  f.dst_img = p.out_sp[0] * ncol; f.dst_pt = ncol;
  f.T = p.f64.t[0]; f.V = p.f64.v[0]; f.nt = p.f64.nt[0]; f.m = axis_map(p, 0);
  f.B = (int)B; f.Cin = (int)Ci; f.Cout = (int)Co; f.G = (int)p.d.groups; f.Cig = p.Cig; f.Cog = p.Cog;
  f.cob = p.f64.cob; f.n_ochunks = (p.Cog + p.f64.cob - 1) / p.f64.cob; f.nb = p.f64.nb;
  f.Lf = p.Lf[0]; f.ostride = p.ostride[0];
  f.Ncol = (int)Ncol; f.Tmid = (int)Tmid; f.Fx = Fx; f.Hcols = (int)(Tmid * Fx);
  FC_HIP(fc::launch_fused_f64(f, st));
  const double2* rsrc = f.dst;
  if (nd == 3) {
    // middle axis back: [(b,co,zo)][nty*Ty][Ncol] -> [(b,co,zo)][Oy][Ncol]
    const int Ty = p.f64.t[1];
    fc::ColF64Args c{};
    c.mode = 2; c.src = wsA; c.dst = wsB; c.nlines = B * Co * p.out_sp[0]; c.ncol = (int)Ncol;
    c.T = Ty; c.V = p.f64.v[1]; c.nt = p.f64.nt[1];
    c.src_line = ncol; c.src_tile = (long long)Ty * Ncol; c.src_pt = Ncol;
    c.dst_line = p.out_sp[1] * Ncol; c.dst_pt = Ncol;
    c.Lf = p.Lf[1]; c.ostride = p.ostride[1];
    FC_HIP(fc::launch_col_f64(c, st));
    rsrc = wsB;
  }
  // rows back: [(b, co, [zo,] yo)][ntx][Fx] -> y
  fc::RowsC2RF64Args o{};
  o.src = rsrc; o.y = y; o.bias = bias;
  o.rows_per_co = 1;
  for (int i = 0; i < X; ++i) o.rows_per_co *= p.out_sp[i];
  o.R = B * Co * o.rows_per_co; o.Cout = (int)Co;
  o.T = Tx; o.V = p.f64.v[X]; o.nt = p.f64.nt[X]; o.Fx = Fx; o.Lf = p.Lf[X]; o.ostride = p.ostride[X];
  o.Ox = (int)p.out_sp[X];
  FC_HIP(fc::launch_rows_c2r_f64(o, st));
  return FC_OK;
}

}  // namespace fc
