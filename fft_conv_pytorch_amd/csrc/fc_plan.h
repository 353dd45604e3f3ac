// fc_plan.h -- the plan behind the C ABI (include/fftconv_amd.h) and the host helpers its paths share.
//
// A plan runs one of seven paths (fc::PlanKind), chosen once when it is created (fc_api.cpp).  Each path plans and
// launches in a file of its own: host_1d.cpp (float32 1-D), host_nd.cpp (float32 and complex64 2-D / 3-D), host_f64.cpp
// (float64).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "fc_internal.h"
#include "fftconv_amd.h"

namespace fc {

int fail(int code, const char* fmt, ...);   // sets the text of fc_last_error, returns code

#define FC_HIP(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return ::fc::fail(FC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Plan creation allocates and uploads device tables (twiddles, work lists) with synchronous calls: it must run OUTSIDE
// stream capture -- run the call once before capturing; every later call of the same shape only launches kernels on the
// caller's stream and is capture-safe (tests/test_gpu_round3.py).  A capture error gets that hint instead of a bare code.
#define FC_HIP_SETUP(expr)                                                               \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      const char* name_ = hipGetErrorName(e_);                                           \
      (void)hipGetLastError();                                                           \
      if (name_ && std::strstr(name_, "Capture"))                                        \
        return ::fc::fail(FC_ERR_HIP, "%s: %s -- plans cannot be created while a stream is being captured: run this call " \
                          "once before the capture (plan creation allocates device tables; later calls only launch kernels)", \
                          #expr, hipGetErrorString(e_));                                 \
      return ::fc::fail(FC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));             \
    }                                                                                    \
  } while (0)

const TileImpl* const* all_tiles(int* n);   // T = 64 .. 4096
const TileImpl* find_tile(int T);

// Device twiddle tables, shared by every plan of the same tile geometry and device.
struct Twiddles {
  f2* twA = nullptr;  // [P][N2]  exp(-2 pi i n2 k1 / T)
  f2* twB = nullptr;  // [S][P]   exp(-2 pi i r k / N2)
};
int get_twiddles(const TileImpl* t, Twiddles* out);    // builds them on first use
int find_twiddles(const TileImpl* t, Twiddles* out);   // never allocates (hot-call side of get_twiddles)

int current_device_cus(int* cus_out);   // CU count of the current device, queried once per device; 0 on failure
int64_t round_up(int64_t v, int64_t m);

enum class PlanKind {
  F32_1D,       // host_1d.cpp: fused / batch-sharing / wide / dense kernels, segments, phases
  F32_ND,       // host_nd.cpp: separable passes, plane-major pipeline, 2-D column pass, segments of taps
  F64_DIRECT,   // host_f64.cpp: direct time-domain kernel (any ndim)
  F64_FFT_1D,   // host_f64.cpp: fft_f64.hip
  F64_FFT_ND,   // host_f64.cpp: nd_f64.hip
  F64_FFT_LONG, // host_f64.cpp: long_f64.hip (1-D, dilated extent past 1025: one transform of N1 x N2 points per row)
  C64_ND,       // host_nd.cpp: complex64 2-D / 3-D on the separable passes (one row per sequence, Fx = Tx bin columns; the
                // state of F32_ND in `fnd`, planes = 0, no segments of taps)
};

}  // namespace fc

struct fc_plan {
  fc_desc d;                  // (a float16 / bfloat16 plan holds its descriptor with dtype FC_F32: it is planned as float32)
  fc::PlanKind kind;
  int nd;
  int io;                     // fc_dtype of x (and of the kernel' dY of a weight-gradient plan): FC_F32, FC_F16 or FC_BF16 on
                              // the float32 kinds (Io<> in fft_engine.hpp); FC_C64 on C64_ND (x, weight, bias and y)
  int io_y;                   // fc_dtype of y: io, but FC_F32 for a weight-gradient plan (dW is float32 whatever x and dY are)
  // ---- axis geometry (axis 0 = fused (outermost), axis nd-1 = rows (x), middle axis only in 3-D)
  int64_t out_sp[3];
  int64_t kd[3];              // dilated kernel extent per axis
  int Sp[3], Lf[3];           // padded extent / stride-1 output extent per axis
  int need[3];                // shortest cyclic length that yields all Lf outputs exactly (<= Sp: zero padding absorbs the wrap)
  int padl[3], up[3], ostride[3];   // left pad in grid coordinates, source spread step, output decimation
  // ---- channel blocking
  int Cig, Cog, CB, cob, Cig_pad, Cog_pad, n_ochunks, accumulate;
  int G;                      // channel groups as the 1-D kernels see them (C/8 blocks for a depthwise plan)
  // ---- fused-axis tiling (float32 plans; float64 1-D FFT plans use Lfull)
  const fc::TileImpl* tile;
  fc::Twiddles tw;
  int V, ntiles, Lfull;
  size_t spectrum_bytes, workspace_bytes;
  size_t ws_a, ws_b;          // element counts of the two workspace regions (F32_ND: fc::f2, F64_FFT_ND: double2)

  struct F1d {                // ---- F32_1D
    size_t lds_conv, lds_spec;
    int pers_nb;                // batch items per workgroup of the batch-sharing kernel (0 = not used)
    int pers_grid, pers_items;
    int chunk_launches;         // general kernel launched once per input chunk, later chunks add into y (host_1d.cpp decide_route)
    int wide;                   // > 8 input channels per group on the batch-sharing work list (conv1d_wide.hpp)
    int dense;                  // >= 16 channels per group on both sides: spectra through HBM + MFMA contraction (dense1d.hpp)
    int dense_mslab;            // rows (batch x tiles) per slab of that pipeline's workspace
    int dense_cus;              // CUs of the plan's device (grid of its persistent GEMM)
    int nseg, seg_taps;         // the kernel runs in nseg segments of seg_taps taps (1 = whole kernel)
    size_t seg_spectrum_bytes;  // kernel-spectrum bytes of one segment
    int diag;                   // depthwise (groups == Cin == Cout, multiple of 8): 8-channel blocks, per-channel mix
    int bd_gs;                  // groups of 2 or 4 channels regrouped into block-diagonal 8 x 8 blocks (0 = off)
    int slot_tiles;             // work-item slots = consecutive tiles of one batch item (else consecutive batch items)
    int ph;                     // dilation run as this many phases of a virtual batch (batch-sharing kernel), else 1
    int ph2;                    // the phases run in pairs (conv1d_pers.hpp PH2)
    fc::WorkItem* d_items;
  } f1d;

  struct {                    // ---- F32_ND
    const fc::TileImpl* tx;     // rows (last axis)
    const fc::TileImpl* tm;     // middle axis (3-D)
    fc::Twiddles twx, twm;
    int Fx;                     // Tx/2 (C64_ND: Tx)
    int nxt, Vx, Fxt;           // overlap-save tiles along the rows axis (nxt = 1: one full-length transform), valid
                                // stride-1 samples per tile, bin columns per plane = nxt * Fx
    int nyt, Vy;                // the same for the middle axis of a 3-D problem (one c2c launch per tile)
    int cob, Cog_pad;           // channel blocking of the fused (complex) pass: one sequence per channel
    int planes;                 // 1: 3-D plane-major three-launch pipeline (planes3d.hpp) instead of the five separable passes;
                                // 2: 2-D with the same thread-per-sequence column pass between row passes that keep the rows as they are
    // weight-gradient plan of an N-d convolution (fc_wgrad_nd): the convolution with batch and channels exchanged;
    // the tensors keep the caller's layout (ImgMap in the row passes)
    int swap;
    int64_t sw_B, sw_Cig, sw_Cog, sw_g;      // of the ORIGINAL convolution
    // segments of taps (host_nd.cpp plan_nd_segments): axis a runs as nseg[a] convolutions of seg_taps[a] taps each
    // (kd, Sp and need of the plan are those of one segment); nseg_total = their product, one kernel spectrum of
    // seg_spectrum_bytes each, in tensor order.  nseg[a] = 1, seg_taps[a] = kernel[a] on an axis that is not cut.
    int nseg[3], seg_taps[3], nseg_total;
    size_t seg_spectrum_bytes;
  } fnd;

  struct {                    // ---- F64_FFT_1D / F64_FFT_ND / F64_FFT_LONG
    int T, V, ntiles, cob;      // 1-D (fft_f64.hip): tile, valid samples, tiles per row, out-chunk (N-d: T = the last axis' transform length)
    int t[3], v[3], nt[3];      // N-d (nd_f64.hip): transform length, valid samples, tiles per axis
    int nb;                     // N-d: batch items per workgroup of its fused pass (cob output channels each)
    // F64_FFT_LONG (long_f64.hip): N = N1 x N2 points per transform (T = N2); V, ntiles and cob as above (one tile: V = Lf);
    // batch pairs, and how many of them share the workspace at a time
    int N1, N2;
    int64_t npairs, slab_pairs;
  } f64;
};

namespace fc {

void set_channel_layout(fc_plan* p, int G, int Cig, int Cog);
AxisMap axis_map(const fc_plan& p, int axis);   // index map of one padded signal axis

// ---- the paths.  plan_*: fill the path's state, spectrum and workspace sizes (plan_f64 also picks the float64 kind).
// transform_kernel_* / forward_*: fc_transform_kernel / fc_forward_stamped of a plan of that kind (arguments checked).
int plan_1d(fc_plan* p);
int plan_nd(fc_plan* p);
int plan_f64(fc_plan* p);

int transform_kernel_1d(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st);
int transform_kernel_nd(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st);
int transform_kernel_f64_direct(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st);
int transform_kernel_f64_1d(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st);
int transform_kernel_f64_nd(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st);
int transform_kernel_f64_long(const fc_plan& p, const float* weight, void* w_hat, void* workspace, hipStream_t st);

int forward_1d(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
               hipStream_t st, void* stamps);
// (x_cl / y_cl: the signal / the output lies channels-last -- only where plan_takes_layout_nd says so)
int forward_nd(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
               hipStream_t st, void* stamps, bool x_cl = false, bool y_cl = false);
// FC_OK when the kernels of an N-d plan read x (x_cl) / write y (y_cl) channels-last, else FC_ERR_UNSUPPORTED with text
int plan_takes_layout_nd(const fc_plan& p, bool x_cl, bool y_cl);
int forward_f64_direct(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
                       hipStream_t st, void* stamps);
int forward_f64_1d(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
                   hipStream_t st, void* stamps);
int forward_f64_nd(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
                   hipStream_t st, void* stamps);
int forward_f64_long(const fc_plan& p, const float* x, const void* w_hat, const float* bias, float* y, void* workspace,
                     hipStream_t st, void* stamps);

}  // namespace fc
