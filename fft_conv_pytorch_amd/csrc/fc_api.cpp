// fc_api.cpp -- C ABI of libfftconv_amd.so (see include/fftconv_amd.h).
//
// Descriptor checks and the per-axis geometry of a plan, the choice of its path (fc::PlanKind), the queries, and the
// helpers the paths share (error text, tile registry, twiddle tables, CU count).  Each path plans and launches in its
// own file (fc_plan.h).  The arithmetic of the reference's functional.py:44-47,66,76-82 that runs on the host lives in
// these files; everything else is in the HIP kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fc_plan.h"

namespace {

thread_local std::string g_err;
std::mutex g_tw_mutex;
std::map<std::pair<int, int>, fc::Twiddles> g_tw;  // (device, T)

}  // namespace

namespace fc {

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

const fc::TileImpl* const* all_tiles(int* n) {
  static const fc::TileImpl* tiles[] = {fc::get_tile_P8_S1(),  fc::get_tile_P8_S2(),  fc::get_tile_P16_S1(), fc::get_tile_P16_S2(),
                                        fc::get_tile_P32_S1(), fc::get_tile_P32_S2(), fc::get_tile_P32_S4()};   // T = 64 .. 4096
  *n = (int)(sizeof tiles / sizeof tiles[0]);
  return tiles;
}

const fc::TileImpl* find_tile(int T) {
  int n;
  auto t = all_tiles(&n);
  for (int i = 0; i < n; ++i)
    if (t[i]->T == T) return t[i];
  return nullptr;
}

int get_twiddles(const fc::TileImpl* t, Twiddles* out) {
  int dev = 0;
  FC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_tw_mutex);
  auto key = std::make_pair(dev, t->T);
  auto it = g_tw.find(key);
  if (it != g_tw.end()) { *out = it->second; return FC_OK; }
  const int P = t->P, S = t->S, N2 = P * S, T = t->T;
  std::vector<fc::f2> a((size_t)P * N2), b((size_t)S * P);
  const double tau = 6.283185307179586476925286766559;
  for (int k1 = 0; k1 < P; ++k1)
    for (int n2 = 0; n2 < N2; ++n2) {
      const double ang = -tau * (double)((long long)k1 * n2 % T) / (double)T;
      a[(size_t)k1 * N2 + n2] = fc::f2{(float)std::cos(ang), (float)std::sin(ang)};
    }
  for (int r = 0; r < S; ++r)
    for (int k = 0; k < P; ++k) {
      const double ang = -tau * (double)(r * k) / (double)N2;
      b[(size_t)r * P + k] = fc::f2{(float)std::cos(ang), (float)std::sin(ang)};
    }
  Twiddles tw;
  FC_HIP_SETUP(hipMalloc(&tw.twA, a.size() * sizeof(fc::f2)));
  FC_HIP_SETUP(hipMalloc(&tw.twB, b.size() * sizeof(fc::f2)));
  FC_HIP_SETUP(hipMemcpy(tw.twA, a.data(), a.size() * sizeof(fc::f2), hipMemcpyHostToDevice));
  FC_HIP_SETUP(hipMemcpy(tw.twB, b.data(), b.size() * sizeof(fc::f2), hipMemcpyHostToDevice));
  g_tw[key] = tw;
  *out = tw;
  return FC_OK;
}

int find_twiddles(const fc::TileImpl* t, Twiddles* out) {
  int dev = 0;
  FC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_tw_mutex);
  auto it = g_tw.find(std::make_pair(dev, t->T));
  if (it == g_tw.end())
    return fail(FC_ERR_INVALID, "device tables for the %d-point tile are not prepared on device %d "
                "(call fc_wgrad1d_slices on this device first)", t->T, dev);
  *out = it->second;
  return FC_OK;
}

int current_device_cus(int* cus_out) {
  static std::mutex m;
  static std::map<int, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lock(m);
  auto it = cache.find(dev);
  if (it == cache.end()) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
    it = cache.emplace(dev, cus).first;
  }
  *cus_out = it->second;
  return 1;
}

int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

void set_channel_layout(fc_plan* p, int G, int Cig, int Cog) {
  p->G = G; p->Cig = Cig; p->Cog = Cog;
  const int cmax = std::max(Cig, Cog);
  p->CB = cmax <= 2 ? 2 : (cmax <= 4 ? 4 : 8);
  p->Cig_pad = (int)round_up(Cig, p->CB);
  p->cob = std::min(p->CB, (int)round_up(Cog, 2));
  p->Cog_pad = (int)round_up(Cog, p->cob);
  p->n_ochunks = p->Cog_pad / p->cob;
  p->accumulate = p->Cig_pad > p->CB;
}

AxisMap axis_map(const fc_plan& p, int axis) {
  AxisMap m;
  m.size = (int)p.d.spatial[axis]; m.pad = p.padl[axis]; m.mode = p.d.padding_mode; m.up = p.up[axis];
  return m;
}

}  // namespace fc

using namespace fc;

// the original convolution behind a weight-gradient plan: batch, channels per group, groups, taps to keep per axis
struct WgradSwap {
  int64_t B, Cig, Cog, g, keep[3];
};

extern "C" {

int fc_version(void) { return FC_ABI_VERSION; }

const char* fc_last_error(void) { return g_err.c_str(); }

static int plan_create_impl(const fc_desc* desc, const WgradSwap* sw, fc_plan** out_plan);

int fc_plan_create(const fc_desc* desc, fc_plan** out_plan) { return plan_create_impl(desc, nullptr, out_plan); }

static int plan_create_impl(const fc_desc* desc, const WgradSwap* sw, fc_plan** out_plan) {
  if (!desc || !out_plan) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // a stale sticky error of an earlier, unrelated call (e.g. an invalidated capture) is not this call's
  *out_plan = nullptr;
  const fc_desc& d = *desc;
  if (d.ndim < 1 || d.ndim > 3) return fail(FC_ERR_INVALID, "ndim must be 1, 2 or 3 (got %d)", d.ndim);
  if (d.dtype != FC_F32 && d.dtype != FC_F64 && d.dtype != FC_F16 && d.dtype != FC_BF16 && d.dtype != FC_C64)
    return fail(FC_ERR_UNSUPPORTED, "dtype must be FC_F32, FC_F64, FC_F16, FC_BF16 or (2-D / 3-D) FC_C64");
  if (sw && (d.dtype == FC_F64 || d.dtype == FC_C64))
    return fail(FC_ERR_UNSUPPORTED, "weight-gradient plans take float32, float16 or bfloat16 x and dY");
  if (d.dtype == FC_C64 && d.ndim == 1)
    return fail(FC_ERR_UNSUPPORTED, "a 1-D descriptor takes no FC_C64: complex rows run the long-filter calls "
                "(fc_long_plan_create_kind with FC_LONG_COMPLEX, fc_long_transform_kernel_io, fc_long_forward_io)");
  if (d.batch < 1 || d.in_channels < 1 || d.out_channels < 1 || d.groups < 1)
    return fail(FC_ERR_INVALID, "batch, channels and groups must be positive");
  if (d.in_channels % d.groups || d.out_channels % d.groups)
    return fail(FC_ERR_INVALID, "in_channels (%lld) and out_channels (%lld) must be divisible by groups (%lld)",
                (long long)d.in_channels, (long long)d.out_channels, (long long)d.groups);
  if (d.padding_mode < 0 || d.padding_mode > 3) return fail(FC_ERR_INVALID, "unknown padding_mode %d", d.padding_mode);

  std::unique_ptr<fc_plan> p(new fc_plan());
  std::memset(p.get(), 0, sizeof *p);
  p->d = d;
  p->nd = d.ndim;
  // 16-bit x / y: planned exactly as the float32 plan of the descriptor (same route, spectrum layout and sizes, so a
  // float32 plan's kernel spectrum serves it); only the launches' loads of x and stores of y take the element type
  p->io = d.dtype == FC_F64 ? FC_F32 : d.dtype;
  if (p->io != FC_F32 && p->io != FC_C64) p->d.dtype = FC_F32;   // (a complex64 plan is a kind of its own, below)
  // a weight-gradient plan reads 16-bit x and dY but writes a float32 dW (which segments of taps may add into)
  p->io_y = sw ? FC_F32 : p->io;
  if (sw) { p->fnd.swap = 1; p->fnd.sw_B = sw->B; p->fnd.sw_Cig = sw->Cig; p->fnd.sw_Cog = sw->Cog; p->fnd.sw_g = sw->g; }
  if (d.transposed && d.padding_mode != FC_PAD_CONSTANT) {
    return fail(FC_ERR_INVALID, "a transposed plan supports zero padding only");
  }
  // A cyclic transform of length T >= Sp holds the whole padded axis.  With ZERO padding a shorter one does: output n reads
  // the padded positions n .. n+kd-1; those past T wrap to the head of the tile, and the result is unchanged when both the
  // true sample (position >= T) and the one wrapped in (position - T) are zero -- all data inside the tile (T >= padl + size)
  // and the wrapped range inside the left padding (T >= size + padr).  The input gradient of an unpadded convolution is the
  // case that matters: its padded axis is size + 2(kd-1) = out + kd - 1 long, just past the power of two the image has, and
  // out itself is enough (cfgB dX: 512 instead of 1024-point rows and one 512-point column tile instead of several).
  const char* zw_env = getenv("FFTCONV_ZEROWRAP");
  const bool zero_wrap = !zw_env || atoi(zw_env) != 0;
  auto set_need = [&](int i) {
    int64_t need = p->Sp[i];
    const int64_t size_eff = (d.spatial[i] - 1) * p->up[i] + 1;
    const int64_t padr = p->Sp[i] - p->padl[i] - size_eff;
    if (zero_wrap && d.padding_mode == FC_PAD_CONSTANT && p->padl[i] >= 0 && padr >= 0)
      need = std::min<int64_t>(need, std::max<int64_t>(std::max<int64_t>(p->Lf[i], p->kd[i]), std::max<int64_t>(p->padl[i] + size_eff, size_eff + padr)));
    p->need[i] = (int)need;
  };
  for (int i = 0; i < d.ndim; ++i) {
    if (d.spatial[i] < 1 || d.kernel[i] < 1 || d.stride[i] < 1 || d.dilation[i] < 1 || d.padding[i] < 0 ||
        (d.transposed && d.output_padding[i] < 0)) {
        return fail(FC_ERR_INVALID, "axis %d: spatial/kernel/stride/dilation must be >= 1 and padding >= 0", i);
    }
    p->kd[i] = (d.kernel[i] - 1) * d.dilation[i] + 1;
    {
      // padded extent and stride-1 output count of an axis are held as int here and in every kernel's arguments
      const int64_t ext = d.transposed ? (d.spatial[i] - 1) * d.stride[i] + 2 * (p->kd[i] - 1) + d.output_padding[i] + 1
                                       : d.spatial[i] + 2 * d.padding[i];
      if (ext >= ((int64_t)1 << 31))
        return fail(FC_ERR_UNSUPPORTED, "axis %d: padded extent %lld exceeds 32-bit positions (must be < 2^31 samples)", i,
                    (long long)ext);
    }
    if (d.transposed) {
      // functional.py:126-154: spread by the stride, full correlation, keep out samples from `padding`
      const int64_t out = (d.spatial[i] - 1) * d.stride[i] - 2 * d.padding[i] + p->kd[i] - 1 + d.output_padding[i] + 1;
      if (out < 1) {
            return fail(FC_ERR_INVALID, "axis %d: transposed output extent %lld is not positive", i, (long long)out);
      }
      p->out_sp[i] = out;
      p->padl[i] = (int)(p->kd[i] - 1 - d.padding[i]);
      p->up[i] = (int)d.stride[i];
      p->ostride[i] = 1;
      p->Sp[i] = (int)(out + p->kd[i] - 1);
      p->Lf[i] = (int)out;
      set_need(i);
      continue;
    }
    const int64_t span = d.spatial[i] + 2 * d.padding[i] - p->kd[i];
    if (span < 0) {
        return fail(FC_ERR_INVALID, "axis %d: dilated kernel extent %lld is larger than the padded input %lld", i,
                  (long long)p->kd[i], (long long)(d.spatial[i] + 2 * d.padding[i]));
    }
    p->out_sp[i] = span / d.stride[i] + 1;
    p->padl[i] = (int)d.padding[i];
    p->up[i] = 1;
    p->ostride[i] = (int)d.stride[i];
    p->Sp[i] = (int)(d.spatial[i] + 2 * d.padding[i]);
    p->Lf[i] = (int)(span + 1);
    if (sw && p->out_sp[i] > sw->keep[i]) {
      // weight gradient: only the first k lags are taps of dW (the input samples a strided convolution never reached
      // would give more); the passes then read no further than those lags need
      p->out_sp[i] = sw->keep[i];
      p->Lf[i] = (int)((sw->keep[i] - 1) * d.stride[i] + 1);
      p->Sp[i] = (int)(p->Lf[i] + p->kd[i] - 1);
    }
    set_need(i);
    if (d.padding_mode == FC_PAD_REFLECT && d.padding[i] >= d.spatial[i]) {
        return fail(FC_ERR_INVALID, "axis %d: reflect padding (%lld) must be smaller than the input size (%lld)", i,
                  (long long)d.padding[i], (long long)d.spatial[i]);
    }
    if (d.padding_mode == FC_PAD_CIRCULAR && d.padding[i] > d.spatial[i]) {
        return fail(FC_ERR_INVALID, "axis %d: circular padding (%lld) must not exceed the input size (%lld)", i,
                  (long long)d.padding[i], (long long)d.spatial[i]);
    }
  }
  set_channel_layout(p.get(), (int)d.groups, (int)(d.in_channels / d.groups), (int)(d.out_channels / d.groups));

  int rc;
  if (d.dtype == FC_F64) rc = plan_f64(p.get());                 // picks one of the four float64 kinds
  else if (d.dtype == FC_C64) { p->kind = PlanKind::C64_ND; rc = plan_nd(p.get()); }   // (2-D / 3-D: checked above)
  else if (d.ndim == 1) { p->kind = PlanKind::F32_1D; rc = plan_1d(p.get()); }
  else { p->kind = PlanKind::F32_ND; rc = plan_nd(p.get()); }
  if (rc != FC_OK) return rc;
  if (p->io_y != FC_F32) {
    // routes that read y back between launches would round a 16-bit output between them: not offered (the caller computes
    // such shapes in float32 and rounds once)
    const char* route = nullptr;
    if (p->kind == PlanKind::F32_1D && p->f1d.chunk_launches) route = "1-D chunk launches (chunk_launches)";
    else if (p->kind == PlanKind::F32_1D && p->f1d.nseg > 1) route = "1-D segments of taps (nseg > 1)";
    else if (p->kind == PlanKind::F32_ND && p->fnd.nseg_total > 1) route = "2-D / 3-D segments of taps (nseg0*nseg1*nseg2 > 1)";
    if (route) {
      fc_plan_destroy(p.release());
      return fail(FC_ERR_UNSUPPORTED, "float16 / bfloat16 I/O: the route %s accumulates into y across launches; "
                  "run this shape in float32", route);
    }
  }
  *out_plan = p.release();
  return FC_OK;
}

void fc_plan_destroy(fc_plan* plan) {
  if (!plan) return;
  if (plan->f1d.d_items) (void)hipFree(plan->f1d.d_items);
  delete plan;
}

int fc_output_shape(const fc_plan* plan, int64_t out_spatial[3]) {
  if (!plan || !out_spatial) return fail(FC_ERR_INVALID, "null argument");
  for (int i = 0; i < 3; ++i) out_spatial[i] = i < plan->nd ? plan->out_sp[i] : 1;
  return FC_OK;
}

size_t fc_kernel_spectrum_bytes(const fc_plan* plan) { return plan ? plan->spectrum_bytes : 0; }
size_t fc_workspace_bytes(const fc_plan* plan) { return plan ? plan->workspace_bytes : 0; }
int fc_plan_tile(const fc_plan* plan) {
  if (!plan) return 0;
  switch (plan->kind) {
    case PlanKind::F32_1D:
    case PlanKind::F32_ND:
    case PlanKind::C64_ND: return plan->tile->T;
    case PlanKind::F64_DIRECT: return 0;
    case PlanKind::F64_FFT_1D:
    case PlanKind::F64_FFT_ND: return plan->f64.T;
    case PlanKind::F64_FFT_LONG: return plan->f64.N2;
  }
  return 0;
}

int fc_plan_layout(const fc_plan* plan, int32_t layout[8]) {
  if (!plan || !layout) return fail(FC_ERR_INVALID, "null argument");
  const fc_plan& p = *plan;
  for (int i = 0; i < 8; ++i) layout[i] = 0;
  switch (p.kind) {
    case PlanKind::F32_1D:
      layout[0] = p.tile->T;
      layout[1] = p.f1d.ph; layout[2] = p.f1d.nseg; layout[3] = p.f1d.seg_taps;
      layout[4] = p.f1d.diag; layout[5] = p.f1d.bd_gs; layout[6] = p.f1d.dense ? 2 : p.f1d.wide; layout[7] = p.f1d.pers_nb;
      break;
    case PlanKind::F32_ND:   // the spectrum is laid out over the row / middle-axis transform lengths and the segments too
    case PlanKind::C64_ND:   // (Tx bin columns where the real plan has Tx/2: the spectrum bytes differ, the words do not)
      layout[0] = p.tile->T;
      layout[1] = p.fnd.tx->T; layout[2] = p.fnd.tm ? p.fnd.tm->T : 0; layout[3] = p.fnd.cob;   // (x tiles share one kernel spectrum)
      for (int a = 0; a < p.nd; ++a) layout[4 + a] = p.fnd.nseg[a] > 1 ? p.fnd.seg_taps[a] : 0;   // taps per segment (0: whole axis)
      layout[7] = p.fnd.planes;      // 1 / 2: the thread-per-sequence column pass (3-D plane-major / 2-D); same spectrum bytes either way
      break;
    case PlanKind::F64_FFT_ND:   // [outermost T, Tx, middle T (3-D)]
      layout[0] = p.f64.t[0]; layout[1] = p.f64.t[p.nd - 1]; layout[2] = p.nd == 3 ? p.f64.t[1] : 0;
      break;
    case PlanKind::F64_FFT_LONG:   // the factorisation orders the bins of the spectrum
      layout[0] = p.f64.N1; layout[1] = p.f64.N2;
      break;
    case PlanKind::F64_DIRECT:
    case PlanKind::F64_FFT_1D:
      break;
  }
  return FC_OK;
}

long long fc_debug_grid(const fc_plan* plan) {
  if (!plan) return 0;
  const fc_plan& p = *plan;
  switch (p.kind) {
    case PlanKind::F32_1D:
      if (p.f1d.pers_nb) return (long long)p.f1d.pers_items * 16;   // one record per wave (up to 16) of every work item
      return (long long)p.d.batch * p.ntiles * p.n_ochunks * p.G;
    case PlanKind::F32_ND:
    case PlanKind::C64_ND:
      if (p.fnd.planes) {   // upper bound of colz's grid (one batch item per workgroup)
        const long long ncol = p.fnd.planes == 1 ? (long long)fc::kPlCols * p.fnd.nxt * p.fnd.nyt : p.fnd.Fxt;
        return (long long)p.d.batch * p.ntiles * (p.fnd.Cog_pad / p.fnd.cob) * p.d.groups * ((ncol / 16 + 7) / 8) * 8;
      } else {   // upper bound of the fused column pass's grid (one batch item per workgroup)
        const long long ncol = p.nd == 2 ? p.fnd.Fxt : (long long)p.fnd.Fxt * p.fnd.tm->T * p.fnd.nyt;
        return (long long)p.d.batch * p.ntiles * (p.fnd.Cog_pad / p.fnd.cob) * p.d.groups * ((ncol + 7) / 8) * 8;
      }
    default:
      return 0;
  }
}

int fc_debug_route(const fc_plan* plan, int32_t route[16]) {
  if (!plan || !route) return fail(FC_ERR_INVALID, "null argument");
  const fc_plan& p = *plan;
  for (int i = 0; i < 16; ++i) route[i] = 0;
  route[0] = (int32_t)p.kind;
  switch (p.kind) {
    case PlanKind::F32_1D: {
      const int32_t w[] = {p.tile->T, p.ntiles, p.f1d.pers_nb, p.f1d.ph, p.f1d.ph2, p.f1d.slot_tiles, p.f1d.nseg,
                           p.f1d.diag, p.f1d.bd_gs, p.f1d.wide, p.f1d.dense, p.f1d.chunk_launches, p.accumulate,
                           p.n_ochunks, p.f1d.pers_items};
      for (int i = 0; i < 15; ++i) route[1 + i] = w[i];
      break;
    }
    case PlanKind::F32_ND:
    case PlanKind::C64_ND: {   // (word 0 tells the complex plan apart; the words behind it mean what they mean for F32_ND)
      const int32_t w[] = {p.tile->T, p.ntiles, p.fnd.tx->T, p.fnd.nxt, p.fnd.tm ? p.fnd.tm->T : 0, p.fnd.nyt,
                           p.fnd.planes, p.fnd.cob, p.accumulate};
      for (int i = 0; i < 9; ++i) route[1 + i] = w[i];
      for (int a = 0; a < p.nd; ++a) { route[10 + a] = p.fnd.nseg[a]; route[13 + a] = p.fnd.seg_taps[a]; }   // (tensor order)
      break;
    }
    case PlanKind::F64_DIRECT:
      break;
    case PlanKind::F64_FFT_1D:
      route[1] = p.f64.T; route[2] = p.f64.ntiles; route[3] = p.f64.cob;
      break;
    case PlanKind::F64_FFT_ND:
      for (int i = 0; i < 3; ++i) { route[1 + i] = p.f64.t[i]; route[4 + i] = p.f64.nt[i]; }
      route[7] = p.f64.nb; route[8] = p.f64.cob;
      break;
    case PlanKind::F64_FFT_LONG:
      route[1] = p.f64.N1; route[2] = p.f64.N2; route[3] = p.f64.ntiles; route[4] = p.f64.cob;
      break;
  }
  return FC_OK;
}

int fc_transform_kernel(const fc_plan* plan, const float* weight, void* w_hat, void* workspace, void* hip_stream) {
  if (!plan || !weight || !w_hat) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // a stale sticky error of an earlier, unrelated call (e.g. an invalidated capture) is not this call's
  hipStream_t st = (hipStream_t)hip_stream;
  const fc_plan& p = *plan;
  if (p.workspace_bytes && !workspace) return fail(FC_ERR_INVALID, "workspace is NULL but %zu bytes are required", p.workspace_bytes);
  switch (p.kind) {
    case PlanKind::F32_1D: return transform_kernel_1d(p, weight, w_hat, workspace, st);
    case PlanKind::F32_ND:
    case PlanKind::C64_ND: return transform_kernel_nd(p, weight, w_hat, workspace, st);
    case PlanKind::F64_DIRECT: return transform_kernel_f64_direct(p, weight, w_hat, workspace, st);
    case PlanKind::F64_FFT_1D: return transform_kernel_f64_1d(p, weight, w_hat, workspace, st);
    case PlanKind::F64_FFT_ND: return transform_kernel_f64_nd(p, weight, w_hat, workspace, st);
    case PlanKind::F64_FFT_LONG: return transform_kernel_f64_long(p, weight, w_hat, workspace, st);
  }
  return fail(FC_ERR_INVALID, "internal: unknown plan kind");
}

int fc_forward(const fc_plan* plan, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
               void* hip_stream) {
  return fc_forward_stamped(plan, x, w_hat, bias, y, workspace, hip_stream, nullptr);
}

int fc_forward_stamped(const fc_plan* plan, const float* x, const void* w_hat, const float* bias, float* y,
                       void* workspace, void* hip_stream, void* stamps) {
  if (!plan || !x || !w_hat || !y) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // a stale sticky error of an earlier, unrelated call (e.g. an invalidated capture) is not this call's
  hipStream_t st = (hipStream_t)hip_stream;
  const fc_plan& p = *plan;
  if (p.d.has_bias && !bias) return fail(FC_ERR_INVALID, "plan was created with has_bias=1 but bias is NULL");
  if (p.workspace_bytes && !workspace) return fail(FC_ERR_INVALID, "workspace is NULL but %zu bytes are required", p.workspace_bytes);
  if (stamps && p.io != FC_F32) return fail(FC_ERR_UNSUPPORTED, "a float16 / bfloat16 / complex64 plan has no stamped forward");
  if (stamps && p.kind == PlanKind::F32_ND && p.fnd.nseg_total > 1)
    return fail(FC_ERR_UNSUPPORTED, "a plan that runs its kernel in %d segments of taps has no stamped forward", p.fnd.nseg_total);
  switch (p.kind) {
    case PlanKind::F32_1D: return forward_1d(p, x, w_hat, bias, y, workspace, st, stamps);
    case PlanKind::F32_ND:
    case PlanKind::C64_ND: return forward_nd(p, x, w_hat, bias, y, workspace, st, stamps);
    case PlanKind::F64_DIRECT: return forward_f64_direct(p, x, w_hat, bias, y, workspace, st, stamps);
    case PlanKind::F64_FFT_1D: return forward_f64_1d(p, x, w_hat, bias, y, workspace, st, stamps);
    case PlanKind::F64_FFT_ND: return forward_f64_nd(p, x, w_hat, bias, y, workspace, st, stamps);
    case PlanKind::F64_FFT_LONG: return forward_f64_long(p, x, w_hat, bias, y, workspace, st, stamps);
  }
  return fail(FC_ERR_INVALID, "internal: unknown plan kind");
}

// ---- channels-last tensors of the 2-D / 3-D plans (host_nd.cpp, plan_takes_layout_nd)
static int check_layouts(const fc_plan* plan, int x_layout, int y_layout) {
  if (!plan) return fail(FC_ERR_INVALID, "null argument");
  for (int lay : {x_layout, y_layout})
    if (lay != FC_ND_PLANAR && lay != FC_ND_CHANNELS_LAST)
      return fail(FC_ERR_INVALID, "unknown layout code %d (fc_nd_layout: 0 planar, 1 channels-last)", lay);
  if (x_layout == FC_ND_PLANAR && y_layout == FC_ND_PLANAR) return FC_OK;
  switch (plan->kind) {
    case PlanKind::F32_ND:
    case PlanKind::C64_ND: return plan_takes_layout_nd(*plan, x_layout == FC_ND_CHANNELS_LAST, y_layout == FC_ND_CHANNELS_LAST);
    case PlanKind::F32_1D:
    case PlanKind::F64_FFT_1D:
    case PlanKind::F64_FFT_LONG:
      return fail(FC_ERR_UNSUPPORTED, "a 1-D plan reads and writes contiguous (B, C, L) tensors only (channels-last rows: "
                  "fc_long_forward_lay)");
    case PlanKind::F64_DIRECT:
    case PlanKind::F64_FFT_ND:
      return fail(FC_ERR_UNSUPPORTED, "a float64 plan reads and writes contiguous (B, C, *spatial) tensors only");
  }
  return fail(FC_ERR_INVALID, "internal: unknown plan kind");
}

int fc_plan_takes_layout(const fc_plan* plan, int x_layout, int y_layout) { return check_layouts(plan, x_layout, y_layout); }

int fc_forward_lay(const fc_plan* plan, const float* x, int x_layout, const void* w_hat, const float* bias, float* y,
                   int y_layout, void* workspace, void* hip_stream) {
  const int rc = check_layouts(plan, x_layout, y_layout);
  if (rc != FC_OK) return rc;
  if (x_layout == FC_ND_PLANAR && y_layout == FC_ND_PLANAR) return fc_forward(plan, x, w_hat, bias, y, workspace, hip_stream);
  if (!x || !w_hat || !y) return fail(FC_ERR_INVALID, "null argument");
  (void)hipGetLastError();   // (as fc_forward_stamped)
  const fc_plan& p = *plan;
  if (p.d.has_bias && !bias) return fail(FC_ERR_INVALID, "plan was created with has_bias=1 but bias is NULL");
  if (p.workspace_bytes && !workspace) return fail(FC_ERR_INVALID, "workspace is NULL but %zu bytes are required", p.workspace_bytes);
  return forward_nd(p, x, w_hat, bias, y, workspace, (hipStream_t)hip_stream, nullptr, x_layout == FC_ND_CHANNELS_LAST,
                    y_layout == FC_ND_CHANNELS_LAST);
}

// ---- N-d weight gradient (the reference's dW comes from autograd through its
// rfftn / einsum / irfftn graph, tests/test_functional.py:111-117): dW[(g,o)][i][k] = sum_b sum_t dY[b][(g,o)][t] *
// Xp[b][(g,i)][t*s + k*d] is the convolution of signal' = X with batch and channels exchanged against kernel' = dY,
// stride' = dilation, dilation' = stride, of which the first k lags per axis are kept.  The plan is that convolution;
// both tensors are read, and dW written, in the caller's layout (ImgMap) -- no transposed copies, no crop afterwards.
int fc_wgrad_nd_plan_create(const fc_desc* conv, fc_plan** out_plan) {
  if (!conv || !out_plan) return fail(FC_ERR_INVALID, "null argument");
  *out_plan = nullptr;
  const fc_desc& c = *conv;
  if (c.ndim < 2 || c.ndim > 3) return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_nd covers 2-D and 3-D convolutions (1-D: fc_wgrad1d)");
  if (c.dtype == FC_C64)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_nd takes no complex64 tensors: run the exchanged forward plan (FC_C64 fc_plan_create) "
                "on conj(x) and dY");
  if ((c.dtype != FC_F32 && c.dtype != FC_F16 && c.dtype != FC_BF16) || c.transposed)
    return fail(FC_ERR_UNSUPPORTED, "fc_wgrad_nd: float32, float16 or bfloat16 x and dY, not transposed");
  if (c.batch < 1 || c.in_channels < 1 || c.out_channels < 1 || c.groups < 1 || c.in_channels % c.groups || c.out_channels % c.groups)
    return fail(FC_ERR_INVALID, "batch, channels and groups must be positive and the channels divisible by groups");
  WgradSwap sw;
  sw.B = c.batch; sw.g = c.groups; sw.Cig = c.in_channels / c.groups; sw.Cog = c.out_channels / c.groups;
  fc_desc d = c;
  d.batch = sw.Cig; d.in_channels = sw.g * sw.B; d.out_channels = sw.g * sw.Cog; d.groups = sw.g;
  d.has_bias = 0; d.tile_hint = 0;
  for (int i = 0; i < 3; ++i) sw.keep[i] = 1;
  for (int i = 0; i < c.ndim; ++i) {
    if (c.spatial[i] < 1 || c.kernel[i] < 1 || c.stride[i] < 1 || c.dilation[i] < 1 || c.padding[i] < 0)
      return fail(FC_ERR_INVALID, "axis %d: spatial/kernel/stride/dilation must be >= 1 and padding >= 0", i);
    const int64_t kd = (c.kernel[i] - 1) * c.dilation[i] + 1;
    const int64_t span = c.spatial[i] + 2 * c.padding[i] - kd;
    if (span < 0) return fail(FC_ERR_INVALID, "axis %d: dilated kernel extent %lld is larger than the padded input", i, (long long)kd);
    d.kernel[i] = span / c.stride[i] + 1;          // taps of kernel' = output extent of the convolution
    d.stride[i] = c.dilation[i];
    d.dilation[i] = c.stride[i];
    sw.keep[i] = c.kernel[i];
  }
  return plan_create_impl(&d, &sw, out_plan);
}

int fc_wgrad_nd(const fc_plan* plan, const float* x, const float* dy, float* dw, void* spectrum, void* workspace, void* hip_stream) {
  if (!plan || !x || !dy || !dw || !spectrum) return fail(FC_ERR_INVALID, "null argument");
  if (!plan->fnd.swap) return fail(FC_ERR_INVALID, "not a weight-gradient plan (fc_wgrad_nd_plan_create)");
  int rc = fc_transform_kernel(plan, dy, spectrum, workspace, hip_stream);
  if (rc != FC_OK) return rc;
  return fc_forward(plan, x, spectrum, nullptr, dw, workspace, hip_stream);
}

}  // extern "C"
