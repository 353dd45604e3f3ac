/* fftconv_amd.h -- C ABI of libfftconv_amd.so (MI355X / gfx950 FFT convolution).
 *
 * The reference (klae01/fft-conv-pytorch) has no FFI: its boundary is the Python
 * signature fft_conv(signal, kernel, bias, stride, padding, dilation, groups,
 * padding_mode) at fft_conv_pytorch/functional.py:19-28.  This ABI is what a
 * native backend for that function binds to; each entry point cites the piece
 * of the reference it replaces.  Plain pointers and sizes only -- no torch
 * types.  All device buffers are owned by the caller; the library owns only the
 * plan (device twiddle tables + launch geometry).  Every launch is asynchronous
 * on the caller's stream; no entry point on the hot path allocates or
 * synchronises.  Status: 0 = OK, non-zero = error, text via fc_last_error().
 */
#ifndef FFTCONV_AMD_H
#define FFTCONV_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FC_ABI_VERSION 7

enum fc_status {
  FC_OK = 0,
  FC_ERR_INVALID = 1,      /* bad argument / shape (ValueError on the Python side) */
  FC_ERR_UNSUPPORTED = 2,  /* valid but outside what this build handles */
  FC_ERR_HIP = 3           /* a HIP runtime call failed */
};

enum fc_pad_mode { FC_PAD_CONSTANT = 0, FC_PAD_REFLECT = 1, FC_PAD_REPLICATE = 2, FC_PAD_CIRCULAR = 3 };
enum fc_dtype {
  FC_F32 = 0,  /* the FFT kernels; every float* below is float */
  FC_F64 = 1,  /* float64 tensors: x, weight, w_hat, bias and y are double (pass them through the float* / void*
                  parameters); double-precision FFT kernels compute the same function (the reference is dtype-agnostic):
                  1-D plans with >= 16 taps, 2-D / 3-D plans from 100 multiply-adds per output (Cin/groups x
                  prod(kernel), over prod(stride) when forward), forward and transposed; a direct time-domain kernel the rest.  A 1-D
                  plan whose dilated kernel extent exceeds 1025 runs one transform of N1 x N2 points per row (three launches,
                  the scheme of the long filters below in double precision) from its crossover with the direct kernel on.
                  N-d plans and those long 1-D plans need fc_workspace_bytes of workspace.  fc_wgrad1d, fc_wgrad_nd and the profiling hook take no float64 */
  FC_F16 = 2,
  FC_BF16 = 3, /* float16 / bfloat16 signal and output (ABI 7): x and y are 16-bit (pass them through the float* parameters);
                  weight, w_hat and bias stay float32 (the caller widens the weight and the bias).  The kernels widen x exactly as
                  they load it, compute in float32 and round y once as they store it (to nearest even; bfloat16 NaN -> 0x7FC0), so
                  the result has the bits of: widen to float32, run the float32 plan, round.  The plan is the float32 plan of the
                  descriptor under the same knobs: equal fc_debug_route, fc_plan_layout, fc_kernel_spectrum_bytes and
                  fc_workspace_bytes, so a float32 plan's spectrum serves it.  Routes that add into y across launches are refused
                  with FC_ERR_UNSUPPORTED, the text naming the route: 1-D chunk launches, 1-D segments of taps, 2-D / 3-D
                  segments of taps.  fc_forward_stamped takes no 16-bit plan.
                  Weight gradients (ABI 7 extension): fc_wgrad1d_slices, fc_wgrad1d, fc_wgrad1d_db, fc_wgrad1d_db_supported
                  and fc_wgrad_nd_plan_create accept a 16-bit descriptor.  x and dy are then 16-bit; partial, db_partial,
                  dw, the spectrum and the workspace stay float32.  Sizes, slices and the route equal those of the float32
                  descriptor, and the loads widen exactly, so every partial and dW has the float32 call's bits on the widened
                  tensors; segments of taps add into the float32 dW as they do there.  A library that predates this answers
                  such a descriptor with 0 slices or FC_ERR_UNSUPPORTED: a caller widens x and dy for that gradient. */
  FC_C64 = 4   /* complex64 tensors, (re, im) float32 pairs (ABI 7 extension).  Two homes:
                  1-D rows: the long-filter calls fc_long_transform_kernel_io and fc_long_forward_io on a complex plan
                  (fc_long_plan_create_kind); a 1-D fc_desc with this dtype answers FC_ERR_UNSUPPORTED naming them.
                  2-D / 3-D: an fc_desc with this dtype, forward or transposed (fc_plan_create): x, weight, bias and y are
                  complex64 and travel through the float* parameters as float64 tensors do (bias: Cout (re, im) pairs); w_hat
                  and the workspace stay float32 pairs, sized by fc_kernel_spectrum_bytes / fc_workspace_bytes.  The product
                  is plain bilinear, y[t] = sum w[k] * x[t + k], nothing conjugated (torch.nn.functional.conv2d on complex
                  tensors).  The plan runs the separable passes with one row per transform of the last axis and all of its
                  bins kept (twice the bin columns of the float32 plan of the same shape); fc_debug_route reports word 0 = 6
                  and behind it the words of a float32 2-D / 3-D plan (planes is always 0).  Not offered, each
                  FC_ERR_UNSUPPORTED with text: segments of taps (a dilated kernel extent past 4096 on an axis, or
                  FFTCONV_NDSEG), fc_wgrad_nd_plan_create, fc_forward_stamped with stamps.  Rows of the output are addressed
                  with 32-bit byte offsets of 8-byte samples: the guards of the float32 plans hold at half the samples. */
};

/* Problem descriptor: the arguments of functional.py:19-28 after to_ntuple
 * (utils.py:4-20) has been applied on the host side.  Axis order is the tensor
 * order: spatial[0] is the slowest spatial axis. */
typedef struct fc_desc {
  int32_t ndim;          /* 1, 2 or 3 spatial axes */
  int32_t dtype;         /* fc_dtype */
  int64_t batch;
  int64_t in_channels;
  int64_t out_channels;
  int64_t groups;
  int64_t spatial[3];    /* input extent per axis (unpadded) */
  int64_t kernel[3];     /* kernel taps per axis */
  int64_t stride[3];
  int64_t padding[3];
  int64_t dilation[3];
  int32_t padding_mode;  /* fc_pad_mode; "zeros" of nn.Conv == constant (nn.py:12) */
  int32_t has_bias;
  int32_t tile_hint;     /* 0 = auto; otherwise force the 1-D FFT tile length */
  int32_t transposed;    /* 0: fft_conv (functional.py:19-89); 1: fft_conv_transpose (functional.py:92-176):
                            kernel is (Cin, Cout/groups, *k), stride spreads the input, padding crops the
                            output, output_padding extends it; padding_mode must be constant */
  int64_t output_padding[3];   /* transposed only */
} fc_desc;

typedef struct fc_plan fc_plan;

/* ABI version of the loaded library (FC_ABI_VERSION). */
int fc_version(void);

/* Thread-local text of the last error returned on this thread. */
const char* fc_last_error(void);

/* Validate the descriptor, choose tiles and build device twiddle tables.
 * Host-side arithmetic of functional.py:44-47,66 (a1, a4). May allocate. */
int fc_plan_create(const fc_desc* desc, fc_plan** out_plan);
void fc_plan_destroy(fc_plan* plan);

/* Output extent per spatial axis: floor((S + 2p - d(k-1) - 1)/stride) + 1,
 * the slice arithmetic of functional.py:76-82 (a9); for a transposed plan
 * (S-1)*stride - 2p + d(k-1) + output_padding + 1 (functional.py:144-154). */
int fc_output_shape(const fc_plan* plan, int64_t out_spatial[3]);

/* Bytes the caller must provide for the transformed kernel / the scratch area (N-d plans and the many-channel
 * 1-D pipeline use a scratch area, in fc_transform_kernel AND fc_forward; 0 for the fused 1-D kernels). */
size_t fc_kernel_spectrum_bytes(const fc_plan* plan);
size_t fc_workspace_bytes(const fc_plan* plan);

/* FFT tile length chosen for the last (fused) axis, for reporting. */
int fc_plan_tile(const fc_plan* plan);

/* Everything the byte layout of the kernel spectrum depends on besides the descriptor itself:
 * float32 1-D {tile, dilation phases, kernel segments, taps per segment, depthwise blocks, regrouped small groups,
 * wide-input kernel (2 = the many-channel pipeline: bin-major complex matrices for its per-bin GEMM), batch items
 * per workgroup}; float32 2-D / 3-D {outer tile, x tile, middle tile (0 in 2-D), channel block, taps per segment of
 * kernel axis 0, 1, 2 in tensor order (0 on an axis not cut into segments; the segments' spectra follow one another),
 * column-pass variant}.  Two plans of equal descriptor (up to the batch size),
 * equal fc_kernel_spectrum_bytes() and equal layout words accept each other's fc_transform_kernel()
 * output -- what a multi-GPU caller checks before broadcasting one rank's spectrum (the planner looks at
 * the local batch size).  No counterpart in the reference (it re-transforms the kernel on every call,
 * functional.py:71). */
int fc_plan_layout(const fc_plan* plan, int32_t layout[8]);

/* Kernel transform: dilation scatter + zero pad + real FFT + conjugate
 * (functional.py:49-57 and :71; rows a2, a6).  weight is (Cout, Cin/groups, *k)
 * contiguous fp32 on the device; w_hat receives fc_kernel_spectrum_bytes(). */
int fc_transform_kernel(const fc_plan* plan, const float* weight, void* w_hat, void* workspace,
                        void* hip_stream);

/* Forward convolution (functional.py:60-87; rows a3, a5, a7-a10): padding,
 * forward real FFT, per-bin grouped channel contraction, inverse FFT, valid
 * window, stride, bias -- x is (B, Cin, *spatial), y is (B, Cout, *out) fp32
 * contiguous on the device.  bias may be NULL. */
int fc_forward(const fc_plan* plan, const float* x, const void* w_hat, const float* bias, float* y,
               void* workspace, void* hip_stream);

/* Weight gradient of the 1-D convolution described by `desc` (the FORWARD descriptor):
 *   dW[o][i][k] = sum_b sum_t dY[b][o][t] * pad(x)[b][i][t + k*dilation]
 * i.e. what autograd derives from functional.py:60-87 for `kernel` (pinned by the reference's
 * tests/test_functional.py:111-117).  Covered: ndim 1, stride 1, <= 64 channels per group on both
 * sides, any kernel length and padding mode (long kernels run in segments of taps; depthwise shapes
 * with a multiple of 8 channels take a per-channel variant).  Cross-spectra are accumulated over the batch
 * and the row on chip; the result comes in `slices` partial tensors that the caller sums:
 *   partial is (slices, Cout, Cin/groups, K) fp32, fully written by the call.
 * fc_wgrad1d_slices returns the slice count for the current device, 0 when the shape is not covered
 * (the caller then differentiates through fc_forward plans instead); it also builds the device tables
 * the launch needs, so fc_wgrad1d itself never allocates or copies (call fc_wgrad1d_slices first, on the
 * same device -- the caller needs its answer to size `partial` anyway). */
/* desc->dtype may be FC_F16 / FC_BF16: x and dy are then 16-bit, partial and db_partial float32 (see fc_dtype). */
int fc_wgrad1d_slices(const fc_desc* desc);
int fc_wgrad1d(const fc_desc* desc, const float* x, const float* dy, float* partial, int slices, void* hip_stream);
/* The same launch with the bias gradient folded in (ABI 5): db[o] = sum over batch and row of dY[b][o][t] is bin 0 of the
 * gradient spectra the kernel forms anyway, so the separate reduction over dY (tests/test_functional.py:114-117 pins db)
 * costs nothing.  Slice s of the result starts at partial + s*slice_stride floats (0 = densely packed) and at
 * db_partial + s*slice_stride: one buffer of `slices` rows [dW | db] with db_partial = partial + Cout*Cin/groups*K is
 * summed by ONE reduction.  db_partial may be NULL.  Not available for depthwise plans (fc_wgrad1d_db_supported = 0). */
int fc_wgrad1d_db_supported(const fc_desc* desc);
int fc_wgrad1d_db(const fc_desc* desc, const float* x, const float* dy, float* partial, float* db_partial,
                  long long slice_stride, int slices, void* hip_stream);

/* Weight gradient of a 2-D / 3-D convolution (ABI 6; row N1: the reference's dW comes out of autograd through its
 * rfftn / einsum / irfftn graph, tests/test_functional.py:62-117 pin it for ndim 1-3, stride 1-2, groups 1-3):
 *   dW[(g,o)][i][k] = sum_b sum_t dY[b][(g,o)][t] * Xpad[b][(g,i)][t*stride + k*dilation]
 * is the convolution of x with batch and channels exchanged against dY (stride and dilation exchanged too), of which
 * the first kernel[i] lags per axis are kept.  fc_wgrad_nd_plan_create takes the descriptor OF THE CONVOLUTION and
 * returns the plan of that gradient (destroy with fc_plan_destroy; fc_kernel_spectrum_bytes / fc_workspace_bytes size the
 * two scratch buffers).  fc_wgrad_nd transforms dY (B, Cout, *Lout), runs x (B, Cin, *S) against it and writes
 * dw (Cout, Cin/groups, *k) completely -- both tensors are read and dW is written in these layouts, no transposed
 * copies, no partial results.  Asynchronous on hip_stream; allocates nothing. */
/* conv_desc->dtype may be FC_F16 / FC_BF16: x and dy are then 16-bit, dw, spectrum and workspace float32 (see fc_dtype). */
int fc_wgrad_nd_plan_create(const fc_desc* conv_desc, fc_plan** out_plan);
int fc_wgrad_nd(const fc_plan* plan, const float* x, const float* dy, float* dw, void* spectrum, void* workspace,
                void* hip_stream);

/* Profiling variant of fc_forward (not part of the drop-in surface; the plan stays immutable; a float32 2-D / 3-D plan
 * that runs its kernel in segments of taps has no stamped forward: FC_ERR_UNSUPPORTED when stamps is not NULL):
 * `stamps` is a device buffer of 16 * fc_debug_grid(plan) uint64 in which lane 0 of the waves of the
 * fused kernels stores the 100 MHz wall clock at its phase boundaries (batch-sharing 1-D kernel: one
 * record of 16 stamps per wave, 16 wave slots per work item).  The stamped launch drains its loads at
 * two extra points: read shares, not totals. */
int fc_forward_stamped(const fc_plan* plan, const float* x, const void* w_hat, const float* bias, float* y,
                       void* workspace, void* hip_stream, void* stamps);
long long fc_debug_grid(const fc_plan* plan);

/* Which kernel build a plan runs, for tests (read-only: no device call, nothing a launch reads changes).
 * route[0] = plan kind (0 float32 1-D, 1 float32 N-d, 2 float64 direct, 3 float64 1-D FFT, 4 float64 N-d FFT,
 *             5 float64 1-D long transform); then
 *   float32 1-D:  tile, tiles, batch items per workgroup (0 = general kernel), phases, phase pairs (1) / quads (2),
 *                 slots are tiles, segments, depthwise blocks, block-diagonal group size, wide, dense, launches per
 *                 input chunk, running sums, out-chunks, work items
 *   float32 N-d:  outer tile, outer tiles, x tile, x tiles, middle tile (0 in 2-D), middle tiles, planes, channel
 *                 block, running sums, segments of taps per kernel axis (3, tensor order: 1 on an axis not cut),
 *                 taps per segment per kernel axis (3, tensor order: the kernel extent on an axis not cut); words of
 *                 the third axis are 0 in 2-D
 *   float64 1-D:  tile, tiles, channel block
 *   float64 N-d:  tile per axis (3), tiles per axis (3), batch items per workgroup, channel block
 *   float64 long: N1, N2, overlap-save tiles of N1 x N2 points per row, channel block (fc_plan_tile reports N2)
 * Unused words are 0.  NULL plan or array: FC_ERR_INVALID. */
int fc_debug_route(const fc_plan* plan, int32_t route[16]);

/* ---- Long filters (ABI 7 extension: new entry points only, nothing that existed changes): a 1-D filter as long as the row, functional.py:66-75 with one transform over the whole
 * padded row instead of overlap-save tiles.  float32 (float16 / bfloat16 tensors: the _io calls below); stride, dilation and the padding modes: the _ext calls below.  The plan computes
 *   y[b][(g,o)][t] = bias[(g,o)] + sum_i sum_k u[(g,o)][i][k] * xpad[b][(g,i)][t + k],   0 <= t < out_keep,
 * xpad = x with pad_left zeros in front and pad_right behind, u[k] = w[k] (flip 0, cross-correlation) or w[K-1-k]
 * (flip 1).  The causal long convolution y[t] = sum_s h[s] x[t-s] is pad_left = K-1, pad_right = 0, flip = 1,
 * out_keep = L; its gradients are the same call with other paddings.  Taps that meet only padding for every
 * kept output are not read.  One cyclic transform of N = N1 * N2 >= out_keep + (taps that are read) - 1 points per row, N1
 * and N2 tile lengths (64 .. 4096), as two on-chip transforms with a trip through the workspace between them. */
typedef struct fc_long_desc {
  int64_t batch, in_channels, out_channels, groups;
  int64_t length;        /* L: samples per signal row */
  int64_t kernel;        /* K: taps per filter row; weight is (Cout, Cin/groups, K) */
  int64_t pad_left, pad_right;
  int64_t out_keep;      /* leading output samples kept; 0 = all of them, L + pad_left + pad_right - K + 1 */
  int32_t flip;          /* tap order, see above */
  int32_t has_bias;
} fc_long_desc;

typedef struct fc_long_plan fc_long_plan;

/* info words of a long plan: N1, N2, output length, kernel-spectrum bytes, workspace bytes, slabs (the batch pairs
 * run in this many rounds of three launches so that the workspace stays inside the budget), output channels per
 * workgroup of the row pass, batch pairs per slab (a complex plan, below: batch items where this says pairs). */
enum { FC_LONG_INFO_WORDS = 8 };

/* The info words from the descriptor alone: validates it, touches no device.  FFTCONV_LONG_N=<N1>x<N2> forces the
 * factorisation (tests), FFTCONV_LONG_WS_MB the workspace budget.  A row that needs more than 2^24 points:
 * FC_ERR_UNSUPPORTED, the text naming the length. */
int fc_long_geometry(const fc_long_desc* desc, int64_t info[8]);

/* Plan of the CURRENT device (allocates the twiddle tables: not capturable; everything after it is). */
int fc_long_plan_create(const fc_long_desc* desc, fc_long_plan** out_plan);
void fc_long_plan_destroy(fc_long_plan* plan);
int fc_long_plan_info(const fc_long_plan* plan, int64_t info[8]);

/* weight (Cout, Cin/groups, K) float32 -> spectrum (info[3] bytes); workspace: info[4] bytes. */
int fc_long_transform_kernel(const fc_long_plan* plan, const float* weight, void* spectrum, void* workspace,
                              void* hip_stream);
/* x (B, Cin, L) -> y (B, Cout, info[2]) float32, every sample written; bias may be NULL.  Three launches per slab on
 * hip_stream, nothing allocated or synchronised. */
int fc_long_forward(const fc_long_plan* plan, const float* x, const void* spectrum, const float* bias, float* y,
                     void* workspace, void* hip_stream);

/* The two calls above with the element types of their tensors named (ABI 7 extension: new entry points only; the calls
 * above are these with FC_F32).  A long plan is independent of the element types -- the same N1 x N2, tables, spectrum,
 * workspace and slabs serve every combination -- so the types are arguments of the call, not fields of fc_long_desc.
 * weight_dtype, x_dtype and y_dtype are fc_dtype codes: FC_F32, FC_F16 or FC_BF16, each on its own (16-bit x and dy with
 * a float32 y is how a weight gradient is taken); FC_F64 answers FC_ERR_UNSUPPORTED and any other value FC_ERR_INVALID,
 * both with text.  A 16-bit weight (Cout, Cin/groups, K) and a 16-bit x (B, Cin, L) are read where they lie and widened
 * exactly as they are loaded; no float32 copy is made.  spectrum, workspace and bias are float32 whatever the types, and
 * the spectrum of a 16-bit weight has the bytes of the spectrum of the widened weight.  The arithmetic is float32; a
 * 16-bit y receives the float32 result with the float32 bias added, rounded once as it is stored (to nearest even;
 * float16 overflows to inf, a bfloat16 NaN stays a NaN), every sample of the kept window written.  The result therefore
 * has the bits of: widen the tensors to float32, run fc_long_transform_kernel / fc_long_forward, round y. */
int fc_long_transform_kernel_io(const fc_long_plan* plan, const void* weight, int weight_dtype, void* spectrum,
                                 void* workspace, void* hip_stream);
int fc_long_forward_io(const fc_long_plan* plan, const void* x, int x_dtype, const void* spectrum, const float* bias,
                        void* y, int y_dtype, void* workspace, void* hip_stream);

/* Stride, dilation and padding modes (ABI 7 extension: new entry points only; fc_long_desc keeps its 80 bytes and the two
 * calls above that take it are these with ext = NULL, which is {0, 1, 1, 1}).  With the extension the plan computes
 *   y[b][(g,o)][j] = bias[(g,o)] + sum_i sum_k u[(g,o)][i][k] * xrow[b][(g,i)][out_step*j + tap_dil*k],   0 <= j < nout,
 * nout = out_keep, or floor((Lp - tap_dil*(K-1) - 1) / out_step) + 1 when out_keep is 0, Lp the length of xrow:
 *   pad_mode   fc PadMode code (0 constant, 1 reflect, 2 replicate, 3 circular): position p of xrow inside
 *              [0, pad_left + L + pad_right) holds x[map(p - pad_left)], map the reflect / replicate / circular map of the
 *              mode, and zero where the mode is constant and the difference lies outside [0, L).  reflect: both paddings
 *              < L; circular: both <= L.
 *   src_up     u >= 1: position p holds x[(p - pad_left) / u] where the difference is a non-negative multiple of u with a
 *              quotient < L, zero elsewhere; Lp = pad_left + u*(L-1) + 1 + pad_right.  With pad_mode constant only
 *              (FC_ERR_INVALID otherwise).  This is the row the gradient of a strided convolution reads.
 *   tap_dil    d >= 1: the taps lie d positions apart, the filter covers d*(K-1) + 1 positions.
 *   out_step   s >= 1: kept output j is sample s*j of the stride-1 result; y is compact, (B, Cout, nout), every sample
 *              written.
 * The cyclic length is out_step*(nout-1) + tap_dil*(taps that are read - 1) + 1; with pad_mode constant, taps that cannot
 * meet the data for any kept output are not read (exactly those when u = d = s = 1, as before), with another mode all are.
 * fc_long_plan_info, the transform and forward calls, the slabs and the workspace rules are those of any long plan. */
typedef struct fc_long_ext {
  int32_t pad_mode;
  int32_t src_up, tap_dil, out_step;
} fc_long_ext;

int fc_long_geometry_ext(const fc_long_desc* desc, const fc_long_ext* ext, int64_t info[8]);
int fc_long_plan_create_ext(const fc_long_desc* desc, const fc_long_ext* ext, fc_long_plan** out_plan);

/* complex64 tensors (ABI 7 extension: new entry points only; fc_long_desc, fc_long_ext and every call above keep their
 * signatures, and the two calls above are these with kind = FC_LONG_REAL).  The transform underneath is complex: a real
 * plan packs two batch items into one row of it, a complex plan (FC_LONG_COMPLEX) gives every batch item a row of its own.
 * It computes the formula above with complex x, weight, bias and y and a plain bilinear product -- nothing is conjugated,
 * as torch.nn.functional.conv1d on complex tensors.  Its info words count rows where a real plan counts pairs: slabs are
 * rounds of batch ITEMS, info[7] items per slab, the workspace info[7] * (Cin + Cout) * N * 8 bytes; the spectrum has the
 * size of the real plan's (N complex bins per filter row either way).  length, kernel and both paddings must stay below
 * 2^28 (FC_ERR_UNSUPPORTED): a sample has 8 bytes and buffer offsets 32 bits.
 *   fc_long_transform_kernel_io / fc_long_forward_io on a complex plan take FC_C64 for weight, x and y (complex64 tensors,
 *   read and written where they lie); bias then points to Cout (re, im) pairs.  Arithmetic, spectrum and workspace are
 *   float32 as ever.  FC_C64 on a real plan and a real code on a complex plan: FC_ERR_INVALID, the text naming the
 *   mismatch; FC_F64 and unknown codes answer as on a real plan.  The calls without _io are FC_F32 calls: real plans only.
 *   FC_LONG_CONJ_SIGNAL  the plan reads x conjugated: y = sum u * conj(xrow) (+ bias)
 *   FC_LONG_CONJ_TAPS    the plan reads the weight conjugated: u = conj(w) in tap order / flipped
 * Both are sign flips as a sample is loaded; they exist for the gradients (PyTorch's convention: dX runs dY against
 * conj(w), dW runs conj(x) against dY as the filter) and go with FC_LONG_COMPLEX only (FC_ERR_INVALID otherwise). */
enum fc_long_kind { FC_LONG_REAL = 0, FC_LONG_COMPLEX = 1, FC_LONG_CONJ_SIGNAL = 2, FC_LONG_CONJ_TAPS = 4 };

int fc_long_geometry_kind(const fc_long_desc* desc, const fc_long_ext* ext, int kind, int64_t info[8]);
int fc_long_plan_create_kind(const fc_long_desc* desc, const fc_long_ext* ext, int kind, fc_long_plan** out_plan);
/* The kind bits a plan was made with (-1: NULL plan). */
int fc_long_plan_kind(const fc_long_plan* plan);

/* Channels-last tensors (ABI 7 extension: a new entry point only; every call above keeps its signature and meaning, and
 * fc_long_forward_io is this call with both layouts FC_LONG_NCL).  The layout of x and of y is an argument of the call,
 * like their element types: the plan, its tables, spectrum, workspace, slabs and launch count do not depend on it.
 *   FC_LONG_NCL  x (B, Cin, L), y (B, Cout, nout) contiguous, as everywhere above
 *   FC_LONG_NLC  element (b, c, t) of x lies at ((b*L + t)*Cin + c) samples from x, element (b, o, j) of y at
 *                ((b*nout + j)*Cout + o) samples from y: contiguous (B, L, Cin) / (B, nout, Cout) tensors
 * The two layouts are independent of each other and of the dtypes; any channel count is taken.  The tensors are read and
 * written where they lie -- no transposed copy is made -- and the result has the bits of the FC_LONG_NCL call on
 * transposed copies.  Every sample of the kept window of y is written and no other byte.  One batch item's block lies
 * behind one 32-bit buffer resource, so L * Cin * (bytes per sample of x) and nout * Cout * (bytes per sample of y) must
 * stay below 2^31 for a channels-last tensor: beyond that FC_ERR_UNSUPPORTED, the text naming the size (pass a (B, C, L)
 * copy).  Any other layout code: FC_ERR_INVALID with text.  weight and bias are what they were. */
enum fc_long_layout { FC_LONG_NCL = 0, FC_LONG_NLC = 1 };
int fc_long_forward_lay(const fc_long_plan* plan, const void* x, int x_dtype, int x_layout, const void* spectrum,
                         const float* bias, void* y, int y_dtype, int y_layout, void* workspace, void* hip_stream);

/* Transposed convolution by phases (ABI 7 extension: new entry points only; every struct, enum value and call above keeps
 * its layout, value and meaning).  A transposed 1-D convolution of stride s and dilation 1,
 *   y[b][(g,o)][n] = bias[(g,o)] + sum_i sum_k w[(g,i)][o][k] * x[b][(g,i)][t],   n = s*t + k - padding,   0 <= n < Lout,
 *   Lout = (L - 1)*s - 2*padding + K + output_padding,   weight (Cin, Cout/groups, K) as torch.nn.ConvTranspose1d holds it,
 * is s ordinary convolutions of the row with the phase filters w_p[j] = w[p + s*j], interleaved:
 *   y[s*T + p - padding] = sum_j w[p + s*j] * x[T - j].
 * A phases plan is the long plan of those: s * Cout output channels (o*s + p carries phase p of filter o) on the UNSPREAD
 * row, ceil(K / s) taps per filter row, one cyclic transform of N = N1 * N2 >= (kept samples T) + ceil(K / s) - 1 points
 * per row where the zero-spread long plan (src_up = s) needs about s times as many.  The input side is transformed once and
 * shared by the phases; the spectrum holds s * Cout * Cin/groups rows of N bins, in the order [(g*Cog + o)*s + p][i].
 * The filter rows are read from the weight where it lies -- phase, flip and the exchange of in and out channels are index
 * arithmetic of the load, no copy is made, a tap past K - 1 reads as zero (shorter phases; phases p >= K have no tap) --
 * and the inverse pass stores sample T of phase p at y[s*T + p - padding]: every sample of y is written exactly once, the
 * output_padding tail and the samples of tap-less phases (bias alone) included, and no other byte.
 *   The geometry call validates the descriptor and touches no device; info words as fc_long_plan_info, info[2] = Lout.
 *   The plan is an fc_long_plan: fc_long_plan_info, fc_long_transform_kernel_io (weight (Cin, Cout/groups, K), FC_F32 /
 *   FC_F16 / FC_BF16), fc_long_forward_io (x (B, Cin, L) -> y (B, Cout, Lout), bias Cout float32 values or NULL) and
 *   fc_long_plan_destroy take it; fc_long_plan_kind answers FC_LONG_REAL.  Slabs, workspace and dtype rules are those of
 *   any real long plan.  fc_long_forward_lay with FC_LONG_NLC for x or y answers FC_ERR_UNSUPPORTED with text.
 * stride >= 1, padding >= 0, 0 <= output_padding < stride, Lout >= 1 (FC_ERR_INVALID otherwise); L, K, padding and Lout
 * below 2^29, stride <= 4096 and stride * N <= 2^30 (FC_ERR_UNSUPPORTED); a row that needs more than 2^24 points answers as
 * fc_long_geometry does. */
typedef struct fc_long_phases_desc {
  int64_t batch, in_channels, out_channels, groups;
  int64_t length;        /* L: samples per signal row */
  int64_t kernel;        /* K: taps per filter row; weight is (Cin, Cout/groups, K) */
  int64_t stride, padding, output_padding;
  int32_t has_bias;
  int32_t reserved;      /* 0 */
} fc_long_phases_desc;

int fc_long_phases_geometry(const fc_long_phases_desc* desc, int64_t info[8]);
int fc_long_phases_plan_create(const fc_long_phases_desc* desc, fc_long_plan** out_plan);

/* Strided convolution by decimation (ABI 7 extension: new entry points only; every struct, enum value and call above keeps
 * its layout, value and meaning).  The strided long primitive of dilation 1 on a zero-padded row,
 *   y[b][(g,o)][j] = bias[(g,o)] + sum_i sum_k u[(g,o)][i][k] * xrow[b][(g,i)][s*j + k],   0 <= j < nout,
 * xrow = x with pad_left zeros in front and pad_right behind, u = w in tensor order (flip 0) or flipped (flip 1), nout =
 * out_keep or floor((L + pad_left + pad_right - K) / s) + 1, is the sum of s ordinary convolutions of decimated rows, the
 * adjoint of the phases plan above: with k = s*m + p,
 *   y[j] = sum_p sum_m u_p[m] * x_p[j + m],   x_p[t] = xrow[s*t + p],   u_p[m] = u[s*m + p].
 * A decimation plan is the long plan of those: s * Cin input channels (i*s + p carries decimated row p of channel i),
 * ceil(K / s) taps per filter row, one cyclic transform of N = N1 * N2 >= nout + ceil(K / s) - 1 points per row where the
 * plain plan with out_step = s needs s*(nout - 1) + K.  The input side transforms the same samples in s shorter rows; the
 * inverse side, W2 and the 2^24-point limit shrink s-fold.  The spectrum holds Cout * s * Cin/groups rows of N bins in the
 * order [(g*Cog + o)][i*s + p].  Nothing is copied: the forward column pass reads position t of phase p from
 * x[s*t + p - pad_left] where that lies in the row (zero elsewhere), and the filter rows are read from the (Cout,
 * Cin/groups, K) weight where it lies, in either tap order; a tap past K - 1 ends a shorter phase, a phase p >= K has none.
 *   The geometry call validates the descriptor and touches no device; info words as fc_long_plan_info.
 *   The plan is an fc_long_plan: fc_long_plan_info, fc_long_transform_kernel_io (FC_F32 / FC_F16 / FC_BF16),
 *   fc_long_forward_io (x (B, Cin, L) -> y (B, Cout, nout)) and fc_long_plan_destroy take it; fc_long_plan_kind answers
 *   FC_LONG_REAL; slabs, workspace, FFTCONV_LONG_N and dtype rules are those of any real long plan.  fc_long_forward_lay
 *   takes FC_LONG_NLC for y (the last pass is that of every long plan) and answers FC_ERR_UNSUPPORTED with text for a
 *   channels-last x.
 * 2 <= stride <= 64, paddings and out_keep >= 0, K <= L + pad_left + pad_right, out_keep <= the output length
 * (FC_ERR_INVALID otherwise); L, K and the paddings below 2^29, stride * N <= 2^30 and the forward grid of a slab inside 2^31
 * workgroups (FC_ERR_UNSUPPORTED); a decimated row that needs more than 2^24 points answers as fc_long_geometry does. */
typedef struct fc_long_decim_desc {
  int64_t batch, in_channels, out_channels, groups;
  int64_t length;        /* L: samples per signal row */
  int64_t kernel;        /* K: taps per filter row; weight is (Cout, Cin/groups, K) */
  int64_t stride;
  int64_t pad_left, pad_right;
  int64_t out_keep;      /* leading output samples kept; 0 = all of them */
  int32_t flip;          /* tap order, as in fc_long_desc */
  int32_t has_bias;
} fc_long_decim_desc;

int fc_long_decim_geometry(const fc_long_decim_desc* desc, int64_t info[8]);
int fc_long_decim_plan_create(const fc_long_decim_desc* desc, fc_long_plan** out_plan);

/* Weight gradient of a long plan (ABI 7 extension: new entry points only; every struct, enum value and call above keeps
 * its layout, value and meaning).  For the layer whose forward is the long primitive with out_step = stride and tap_dil =
 * dilation on x (B, Cin, L) and a (Cout, Cin/groups, K) weight, the call computes from x and dY (B, Cout, out_len)
 *   dW[(g,o)][i][k] = sum_b sum_j dY[b][(g,o)][j] * xrow[b][(g,i)][stride*j + dilation*k'],   k' = k (flip 0) or K-1-k (flip 1),
 * xrow = x read through pad_left / pad_right in pad_mode exactly as the forward plan reads it.  Both operands are read
 * where they lie: x and dY are signal-shaped, so the forward column pass transforms both, two batch items to a complex
 * row (z = x[2p] + i*x[2p+1], w = dY[2p] + i*dY[2p+1], dY spread over the grid of the stride), and
 *   IFFT( FFT(z) * conj(FFT(w)) )[m] = sum_t conj(w[t]) * z[t + m]
 * has the pair's contribution to the lag m in its real part.  The row pass sums the product over the batch pairs in
 * registers and transforms back once per (o, i); the last pass keeps the real part of every dilation-th lag and stores it
 * at the place of its tap, in the weight's own order for either flip.  No transposed copy and no spectrum buffer exists.
 *   Geometry: N1 x N2 is that of the forward plan of the same layer (out_keep = out_len), FFTCONV_LONG_N and the 2^24-point
 *   refusal included.  With pad_mode constant the lags of taps that can meet no data for any output are not transformed;
 *   they are written as zero.  Every element of dW is written exactly once and no other byte.
 *   info words: N1, N2, K, lags transformed, workspace bytes, slabs, output channels per workgroup of the row pass, batch
 *   pairs per slab.  The workspace holds W1 of x and of dY for the pairs of a slab and W2 for all of dW:
 *   (info[7] * (Cin + Cout) + Cout * Cin/groups) * N * 8 bytes, under FFTCONV_LONG_WS_MB.  The sum over the pairs crosses
 *   slabs: every slab after the first ADDS its transformed sum into W2, so the bits of dW depend on the slab count (not on
 *   anything else).  W2 alone above the budget, or a grid above 2^31 workgroups: FC_ERR_UNSUPPORTED with text.
 *   x_dtype, dy_dtype and dw_dtype are FC_F32 / FC_F16 / FC_BF16, x_layout and dy_layout FC_LONG_NCL / FC_LONG_NLC, each
 *   on its own; dW is (Cout, Cin/groups, K) contiguous, float32 arithmetic rounded once at the store.  A channels-last block
 *   of 2^31 bytes or more answers FC_ERR_UNSUPPORTED as in fc_long_forward_lay; fc_long_wgrad_check_io answers for a call
 *   from the descriptor alone (no device).  Three launches per slab, one more and up to two strided fills on hip_stream;
 *   after plan creation nothing is allocated or synchronised. */
typedef struct fc_long_wgrad_desc {
  int64_t batch, in_channels, out_channels, groups;
  int64_t length;              /* L: samples per row of x */
  int64_t kernel;              /* K: dW is (Cout, Cin/groups, K) */
  int64_t pad_left, pad_right; /* of the forward's row */
  int64_t out_len;             /* nout: samples per row of dY */
  int32_t flip;                /* the forward's tap order */
  int32_t pad_mode;            /* the forward's PadMode code */
  int32_t stride, dilation;    /* the forward's out_step and tap_dil */
} fc_long_wgrad_desc;

typedef struct fc_long_wgrad_plan fc_long_wgrad_plan;

int fc_long_wgrad_geometry(const fc_long_wgrad_desc* desc, int64_t info[8]);
int fc_long_wgrad_check_io(const fc_long_wgrad_desc* desc, int x_dtype, int x_layout, int dy_dtype, int dy_layout,
                            int dw_dtype);
int fc_long_wgrad_plan_create(const fc_long_wgrad_desc* desc, fc_long_wgrad_plan** out_plan);
void fc_long_wgrad_plan_destroy(fc_long_wgrad_plan* plan);
int fc_long_wgrad_plan_info(const fc_long_wgrad_plan* plan, int64_t info[8]);
int fc_long_wgrad(const fc_long_wgrad_plan* plan, const void* x, int x_dtype, int x_layout, const void* dy, int dy_dtype,
                  int dy_layout, void* dw, int dw_dtype, void* workspace, void* hip_stream);

/* fc_long_wgrad with elementwise gates inside its two column reads (ABI 7 extension: one new entry point; the plan, its
 * geometry, its info words and its workspace are those of fc_long_wgrad): dW of the plan's layer for the signal rows
 * pregate * x and the output gradient postgate * dY, neither of which exists as a tensor.
 *   pregate   like x:  (B, Cin, L) contiguous, x_dtype;  NULL: all ones
 *   postgate  like dY: (B, Cout, out_len) contiguous, dy_dtype; NULL: all ones
 * Each product is one float32 multiply of the widened operands as the sample is loaded -- of two 16-bit values: exact -- so
 * dW has the bits of fc_long_wgrad on the float32 products.  A gate is read at the offset of its sample, through a buffer
 * resource of that tensor's row; the gates advance with the slabs as x and dY do.  No byte outside the five tensors and the
 * workspace is read or written.
 *   Launches: those of fc_long_wgrad per slab; a side with a gate runs the gated build of the forward column pass (the one
 *   fc_long_forward_gated runs for a pregate), a side without runs the build it runs in fc_long_wgrad.  With both gates
 *   NULL the call is fc_long_wgrad.
 *   The gated builds are builds of the unmapped (B, C, L) column kernel, so these answer FC_ERR_UNSUPPORTED with text and
 *   launch nothing: a pregate on a plan whose pad_mode is not constant, a pregate with x_layout FC_LONG_NLC, a postgate on
 *   a plan with stride > 1 (dY is then read spread over the grid of the stride), a postgate with dy_layout FC_LONG_NLC.
 *   The dilation is free: it only chooses the lags the last pass keeps. */
int fc_long_wgrad_gated(const fc_long_wgrad_plan* plan, const void* x, const void* pregate, int x_dtype, int x_layout,
                        const void* dy, const void* postgate, int dy_dtype, int dy_layout, void* dw, int dw_dtype,
                        void* workspace, void* hip_stream);

/* Rows in overlap-save blocks (ABI 7 extension: new entry points only; every struct, enum value and call above keeps its
 * layout, value and meaning, and every kernel that existed its code).  The plain real primitive -- fc_long_desc with the
 * default fc_long_ext: zero padding, stride 1, dilation 1 -- on a row that is longer than the transform: the padded row is
 * cut into blocks of N = block_points points that overlap by (taps read) - 1, each block is one cyclic transform against
 * ONE filter spectrum of N bins, and the block index is treated like the batch index.
 *   nout, the taps read (keff of them; taps that meet only padding are not read) and the place of the data are those of
 *   fc_long_geometry for the row.  V = N - keff + 1 samples of a block are kept, T = ceil(nout / V) blocks make a row, the
 *   units (b, t) = u = b*T + t number U = B*T, and pair p carries units 2p and 2p+1 in one complex row (a last odd unit has
 *   no partner).  Position q in [0, N) of unit (b, t) of channel c holds xrow[b][c][t*V + q]; sample j in [0, V) of the
 *   unit's result is y[b][o][t*V + j] where t*V + j < nout, everything else is dropped.  Every sample of y is written
 *   exactly once and no other byte.
 *   The spectrum is Cout * Cin/groups rows of N bins whatever T is; the workspace holds (pairs per slab) * (Cin + Cout) * N
 *   * 8 bytes under FFTCONV_LONG_WS_MB, the slabs run over unit pairs; FFTCONV_LONG_N must factor N itself.
 *   info words as fc_long_plan_info (info[2] = nout); blocks[4] = V, T, U, unit pairs.
 *   block_points: a power of two 4096 ... 2^24 (FC_ERR_INVALID otherwise), or 0 for the planner's choice: the smallest power
 *   of two >= 4 * keff, not below 2^18, not above 2^24.
 *   The plan is an fc_long_plan: fc_long_plan_info, fc_long_transform_kernel_io, fc_long_forward_io (FC_F32 / FC_F16 /
 *   FC_BF16, each on its own) and fc_long_plan_destroy take it, fc_long_plan_kind answers FC_LONG_REAL.
 *   fc_long_forward_lay with FC_LONG_NLC on either side and fc_long_forward_gated answer FC_ERR_UNSUPPORTED with text and
 *   launch nothing.
 *   FC_ERR_UNSUPPORTED with text: keff > N / 2 (a block keeps at least half of its points, so K <= 2^23), grids past 2^31
 *   workgroups, B * T past 2^31, and rows of x, of the weight or of y past 2^29 samples (a row lies behind one buffer
 *   resource). */
typedef struct fc_long_blocks_desc {
  fc_long_desc row;        /* the primitive of fc_long_desc with the default fc_long_ext */
  int64_t block_points;    /* N of one block, a power of two 4096 .. 2^24; 0 = the planner's choice */
} fc_long_blocks_desc;

int fc_long_blocks_geometry(const fc_long_blocks_desc* desc, int64_t info[8], int64_t blocks[4]);
int fc_long_blocks_plan_create(const fc_long_blocks_desc* desc, fc_long_plan** out_plan);

/* The weight gradient of a layer that runs by blocks: fc_long_wgrad_desc with stride 1, dilation 1 and pad_mode constant
 * (FC_ERR_UNSUPPORTED otherwise) and the block_points of the forward.  The plan is an fc_long_wgrad_plan and fc_long_wgrad
 * runs it on (B, C, L) tensors: x is read through the N-point window of each unit, dY through the window of the V samples
 * the unit keeps, [t*V, t*V + V) of the row (the rest of its block reads zero), the row pass sums FFT(x) * conj(FFT(dY))
 * over the unit pairs exactly as it sums batch pairs, and the last pass stores lags 0 ... keff - 1 in the weight's order.
 * info words as fc_long_wgrad_plan_info, blocks[4] as above.  fc_long_wgrad_gated with a gate and channels-last operands
 * on such a plan answer FC_ERR_UNSUPPORTED with text. */
int fc_long_wgrad_blocks_geometry(const fc_long_wgrad_desc* desc, int64_t block_points, int64_t info[8], int64_t blocks[4]);
int fc_long_wgrad_blocks_plan_create(const fc_long_wgrad_desc* desc, int64_t block_points, fc_long_wgrad_plan** out_plan);

/* ---- Channels-last tensors of the 2-D / 3-D plans (ABI 7 extension: new entry points only; fc_desc keeps its size, every
 * call above keeps its signature and meaning, and the route words of fc_debug_route are what they were).  The layout of x
 * and of y is an argument of the call: plan creation, the plan's route, its spectrum and its workspace do not depend on it.
 *   FC_ND_PLANAR         x (B, Cin, *spatial), y (B, Cout, *out) contiguous, as fc_forward takes them
 *   FC_ND_CHANNELS_LAST  the channel index runs fastest: element (b, ch, z, y, x) of a tensor with C channels and spatial
 *                        extents (SZ, SY, SX) -- SZ = 1 for a 2-D plan -- lies at ((((b*SZ + z)*SY + y)*SX + x)*C + ch)
 *                        samples from the pointer; a contiguous (B, Y, X, C) / (B, Z, Y, X, C) tensor, what torch calls
 *                        torch.channels_last / torch.channels_last_3d.  For y: C = Cout and the extents of fc_output_shape.
 * The two layouts are independent of each other.  The tensors are read and written where they lie -- no copy is made -- by
 * channels-last builds of the first and the last pass; the passes between them and the workspace are those of fc_forward.
 * Every value has the bits of fc_forward on contiguous copies; every sample of y is written and no other byte.
 * fc_forward_lay with both layouts FC_ND_PLANAR is fc_forward.
 *
 * fc_plan_takes_layout tells, without touching a device, whether a plan's launches take the two layouts: FC_OK, or
 * FC_ERR_UNSUPPORTED with text (fc_forward_lay answers the same and launches nothing; the caller then passes contiguous
 * copies).  Taken: a float32 / float16 / bfloat16 2-D or 3-D plan of fc_plan_create, forward or transposed, that is
 * unsegmented, runs the separable passes or the 2-D row-major pipeline (route word `planes` 0 or 2), transforms its rows
 * with 64 ... 1024 points (route word `x tile`), and whose tensors fit 32-bit addressing: a channels-last x below 2^32 - 1
 * bytes, and for a channels-last y (16 * Xo + Lx + 8192) * Cout * (bytes per sample) below 2^31 (Xo: the output's last
 * extent, Lx: its stride-1 extent).  Not taken: the plane-major 3-D pipeline (`planes` 1), a kernel that runs in segments of
 * taps, 2048- and 4096-point row transforms, complex64 and float64 plans, weight-gradient plans, 1-D plans (rows:
 * fc_long_forward_lay).  Any other layout code: FC_ERR_INVALID with text. */
enum fc_nd_layout { FC_ND_PLANAR = 0, FC_ND_CHANNELS_LAST = 1 };
int fc_plan_takes_layout(const fc_plan* plan, int x_layout, int y_layout);
int fc_forward_lay(const fc_plan* plan, const float* x, int x_layout, const void* w_hat, const float* bias, float* y,
                   int y_layout, void* workspace, void* hip_stream);

/* ---- Gated long forward (ABI 7 extension: one new entry point; every struct and call above keeps its layout, signature
 * and meaning, and every kernel that existed its arguments).  fc_long_forward_io with elementwise gates fused into the two
 * column passes, which touch every sample of x and of y once anyway:
 *   row  = pregate * x                      (pregate: like x, (B, Cin, L) contiguous, x_dtype; NULL: all ones)
 *   c    = the plan's convolution of the rows + bias
 *   y    = gate  * c                        (gate:  like y, (B, Cout, out_len) contiguous, y_dtype; NULL: all ones)
 *   y2   = gate2 * c                        (y2: a second result like y, NULL: not stored; gate2: like gate, NULL: all ones)
 * Every product is one float32 multiply of the widened operands -- of two 16-bit values: exact -- and y, y2 are rounded once,
 * at the store; the product with c is never fused with the bias add.  So the results have the bits of widening the
 * tensors, multiplying in float32 around fc_long_forward_io on float32 tensors, and rounding.  y2_dtype is y_dtype, or
 * FC_F32 with gate2 NULL on a 16-bit launch: y2 then holds c unrounded (what the gradient of `gate` needs).  gate2 without
 * y2: FC_ERR_INVALID.  A gate is read at the offset of the store it scales, the pregate at the offset of its sample of x,
 * both through buffer resources of that tensor's row: no byte outside the tensors named is read or written.
 *   Slabs are those of fc_long_forward_io; the gates and y2 are indexed by the batch item as x and y are.  Launches: three
 *   per slab as ever, the gated build of a column pass where that pass has a gate (or a y2), the plain one where not;
 *   with every optional pointer NULL the call is fc_long_forward_io.
 *   Taken: real plans of fc_long_plan_create / _ext / _kind whose fc_long_ext words are the defaults (zero padding, no
 *   spread, dilation 1, every output kept), (B, C, L) tensors.  Complex plans, a non-default fc_long_ext, phases plans and
 *   decimation plans answer FC_ERR_UNSUPPORTED with text and launch nothing (multiply around the call instead); a
 *   weight-gradient plan is another type. */
int fc_long_forward_gated(const fc_long_plan* plan, const void* x, int x_dtype, const void* pregate, const void* spectrum,
                          const float* bias, void* y, const void* gate, void* y2, const void* gate2, int y_dtype,
                          int y2_dtype, void* workspace, void* hip_stream);

/* ---- Token-by-token decoding of a causal long filter (ABI 7 extension: one new struct and three new entry points; every
 * struct and call above keeps its layout, signature and meaning, and every kernel that existed its arguments).
 * A causal convolution y[t] = bias + sum_k kernel[k] * z[t - k] whose input arrives one sample at a time can be cut into
 * power-of-two blocks of history against segments of the taps; the caller runs those blocks with the calls above as they
 * fall due and adds them to a float32 accumulator `acc` at the positions they reach.  What is left for position t are the
 * first `head` taps, and fc_long_step is that remainder, ONE launch:
 *   z[b][c]     = pregate[b][c] * x_t[b][c]                (pregate: like x_t; NULL: all ones); stored to hist[b][c][t]
 *   y_t[b][o]   = postgate[b][o] * (bias[o] + acc[b][o][t]
 *                 + sum over the group's input channels c and the taps k < head with t - k >= first of
 *                   head_taps[o][c][k] * (k == 0 ? z[b][c] : hist[b][c][t - k]))
 * x_t, pregate (B, Cin) and y_t, postgate (B, Cout) are contiguous tensors of the descriptor's dtype (FC_F32, FC_F16 or
 * FC_BF16); hist (B, Cin, max_len), acc (B, Cout, max_len), head_taps (Cout, Cin/groups, head; zero past `kernel` taps)
 * and bias (Cout, or NULL) are float32.  The arithmetic is float32: 16-bit values are widened as they are loaded, each
 * product with a gate is one float32 multiply, y_t is rounded once as it is stored.  Column t of hist is the only place
 * of hist that is written, acc is only read, and y_t is written in full and no other byte.  `first` is the position at
 * which stepping began (history below it belongs to blocks the caller has already run): such positions read as zero.
 *   The call is stateless -- no plan, no allocation, no synchronisation -- and the position is an argument, so a step
 *   captured into a HIP graph replays the position it was captured at.
 *   One workgroup per (batch item, group); a group's history lies behind one buffer resource.
 *   FC_ERR_INVALID with text: a null tensor, a non-positive count, channels not divisible by groups, another dtype,
 *   t outside [0, max_len), first outside [0, t].  FC_ERR_UNSUPPORTED with text: head outside 8 ... 1024 or not a power of
 *   two, a group's history of 2^29 samples or more (Cin/groups * max_len), 2^20 channels per group or more, B * groups past
 *   2^31 workgroups.  Either launches nothing. */
typedef struct fc_long_step_desc {
  int64_t batch, in_channels, out_channels, groups;
  int64_t kernel;       /* K taps of the filter (head_taps rows are zero from tap K on) */
  int64_t head;         /* taps the step itself applies: a power of two 8 .. 1024 */
  int64_t max_len;      /* positions of hist and acc */
  int32_t dtype;        /* fc_dtype of x_t, the gates and y_t */
  int32_t reserved;     /* 0 */
} fc_long_step_desc;

int fc_long_step(const fc_long_step_desc* desc, const void* x_t, const void* pregate, const void* postgate,
                 const float* head_taps, const float* bias, float* hist, const float* acc, void* y_t, int64_t t,
                 int64_t first, void* hip_stream);

/* `count` consecutive steps in ONE launch: the columns t = t0 ... t0 + count - 1 that `count` calls of fc_long_step would
 * have produced, for a chunk of tokens that is known at once (a further chunk of a prompt, speculative tokens to verify).
 * The chunk tensors are indexed by j = t - t0:
 *   z[b][c][t]  = pregate[b][c][j] * x[b][c][j]            (one float32 multiply of the widened samples); stored to hist[b][c][t]
 *   y[b][o][j]  = postgate[b][o][j] * (bias[o] + acc[b][o][t]
 *                 + sum over the group's input channels c and the taps k < head with t - k >= first of
 *                   head_taps[o][c][k] * z[b][c][t - k])
 * x, pregate (B, Cin, count) and y, postgate (B, Cout, count) are contiguous tensors of the descriptor's dtype; the other
 * arguments are those of fc_long_step.  A sample t - k >= t0 is taken from the chunk (the product is formed again), never
 * from hist; one below t0 is read from hist, one below `first` is zero.  The columns [t0, t0 + count) of hist are the only
 * place of hist that is written, acc is only read -- that it is complete for these columns is the caller's affair: the
 * call has no alignment rule of its own -- and y is written in full and no other byte.  Each output is one chain of
 * float32 fused multiply-adds over c ascending, then k ascending, so the bits of a column do not depend on how a row is
 * cut into calls (they are not those of fc_long_step, whose lanes share the sum differently).
 *   One workgroup per (batch item, group, tile of 64 columns); stateless like the step.
 *   FC_ERR_INVALID with text: a null tensor, the descriptor errors of fc_long_step, count < 1, t0 < 0,
 *   t0 + count > max_len, first outside [0, t0].  FC_ERR_UNSUPPORTED with text: as for the step, and
 *   B * groups * ceil(count / 64) past 2^31 workgroups.  Either launches nothing. */
int fc_long_push(const fc_long_step_desc* desc, const void* x, const void* pregate, const void* postgate,
                 const float* head_taps, const float* bias, float* hist, const float* acc, void* y,
                 int64_t t0, int64_t count, int64_t first, void* hip_stream);

/* Up to `head` DRAFT tokens verified in ONE launch that leaves the accumulator alone: the columns t = t0 ... t0 + count - 1
 * that fc_long_push would return if the caller had first run the blocks that fall due inside the chunk -- which the
 * caller has NOT done, so that tokens the verifier rejects leave no trace in acc.  (A new entry point; ABI 7 as before.)
 * With M = (t0 / head + 1) * head, the only multiple of head that can lie inside (t0, t0 + count):
 *   z[b][c][t]  = pregate[b][c][j] * x[b][c][j]            stored to hist[b][c][t], as the push stores it
 *   y[b][o][j]  = postgate[b][o][j] * (acc[b][o][t] + bias[o]
 *                 + sum over c and the taps k < head with t - k >= first of head_taps[o][c][k] * z[b][c][t - k]
 *                 + late[b][o][t])
 *   late[b][o][t] = 0 for t < M, and whenever M >= t0 + count or M >= max_len; otherwise the sum over c, over the levels
 *                 n = head, 2 head, 4 head, ... < kernel that divide M, and over the samples s = M - n ... t - n with
 *                 s >= first and t - s < min(2n, kernel), of filter[o][c][t - s] * hist[b][c][s]
 * -- what the blocks due at M would have added to acc[b][o][t].  Every such s lies below t0: an old sample of hist.
 * filter_flipped (Cout, Cin/groups, kernel) is the whole float32 filter with tap k of (o, c) at index kernel - 1 - k; the
 * other arguments are those of fc_long_push, and count <= head.  The columns [t0, t0 + count) of hist are the only place
 * of hist that is written (a caller that rejects draft tokens simply does not advance: columns at or past the position
 * are never read), acc is only read, y is written in full and no other byte.
 * Bits: the head sum is the push kernel's chain and is added as there, so a column t < M has the bits fc_long_push gives
 * it.  late is ONE chain of float32 fused multiply-adds of its own -- c ascending, then n ascending, then s ascending,
 * pairs outside the conditions skipped -- added after the head sum; no atomics: the same call on the same state returns
 * the same bits.  A column t >= M need not have the bits of a push that ran the blocks (their sums are formed otherwise).
 *   One workgroup per (batch item, group, tile of 64 columns); stateless like the step.
 *   FC_ERR_INVALID with text: a null tensor (filter_flipped included), the descriptor errors of fc_long_step, count < 1,
 *   count > head, t0 < 0, t0 + count > max_len, first outside [0, t0].  FC_ERR_UNSUPPORTED with text: as for the push.
 *   Either launches nothing. */
int fc_long_spec(const fc_long_step_desc* desc, const void* x, const void* pregate, const void* postgate,
                 const float* head_taps, const float* filter_flipped, const float* bias, float* hist, const float* acc,
                 void* y, int64_t t0, int64_t count, int64_t first, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FFTCONV_AMD_H */
