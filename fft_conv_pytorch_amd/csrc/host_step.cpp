// host_step.cpp -- fc_long_step, fc_long_push and fc_long_spec (include/fftconv_amd.h "Token-by-token decoding"):
// descriptor checks and the one launch of long_step_kernel (long_step.hpp), long_push_kernel (long_push.hpp) or
// long_spec_kernel (long_spec.hpp).  The push and the draft are one chunk to the host as to the kernels (LongChunk): one
// set of checks and one argument fill; the draft adds its count limit, M and the levels.  Stateless: no plan, no
// allocation, nothing but the launch on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fc_plan.h"
#include "long_push.hpp"
#include "long_spec.hpp"
#include "long_step.hpp"

using namespace fc;

// the descriptor's counts and dtype (FC_ERR_INVALID), checked before the position of a call ...
static int step_desc_counts(const fc_long_step_desc& d) {
  if (d.batch < 1 || d.in_channels < 1 || d.out_channels < 1 || d.groups < 1 || d.kernel < 1 || d.max_len < 1)
    return fail(FC_ERR_INVALID, "batch, channels, groups, kernel and max_len must be positive");
  if (d.in_channels % d.groups || d.out_channels % d.groups)
    return fail(FC_ERR_INVALID, "in_channels (%lld) and out_channels (%lld) must be divisible by groups (%lld)",
                (long long)d.in_channels, (long long)d.out_channels, (long long)d.groups);
  if (d.dtype != FC_F32 && d.dtype != FC_F16 && d.dtype != FC_BF16)
    return fail(FC_ERR_INVALID, "dtype %d: a step reads and writes FC_F32, FC_F16 or FC_BF16 tensors", d.dtype);
  return FC_OK;
}

// ... and what the kernels address (FC_ERR_UNSUPPORTED), checked after it
static int step_desc_limits(const fc_long_step_desc& d) {
  if (d.head < 8 || d.head > 1024 || (d.head & (d.head - 1)))
    return fail(FC_ERR_UNSUPPORTED, "head (%lld) must be a power of two from 8 to 1024", (long long)d.head);
  const int64_t cig = d.in_channels / d.groups;
  if (d.max_len >= ((int64_t)1 << 29) || cig >= ((int64_t)1 << 20) || cig * d.max_len >= ((int64_t)1 << 29))
    return fail(FC_ERR_UNSUPPORTED, "a group's history of %lld channels x %lld positions: the step kernel addresses fewer "
                "than 2^29 samples behind one buffer resource and fewer than 2^20 channels per group",(long long)cig, (long long)d.max_len);
  if (d.batch * d.groups > 0x7fffffffLL || d.out_channels > 0x7fffffffLL)
    return fail(FC_ERR_UNSUPPORTED, "%lld batch items x %lld groups exceed the 2^31 workgroups of one launch",
                (long long)d.batch, (long long)d.groups);
  return FC_OK;
}

// the pointers and the shape that the three argument structs name alike
template <class Args>
static void fill_state(Args& a, const fc_long_step_desc& d, const void* x, const void* pregate, const void* postgate,
                       const float* head_taps, const float* bias, float* hist, const float* acc, void* y) {
  a.x = x; a.pregate = pregate; a.postgate = postgate; a.taps = head_taps; a.bias = bias;
  a.hist = hist; a.acc = acc; a.y = y;
  a.max_len = d.max_len;
  a.Cin = (int)d.in_channels; a.Cout = (int)d.out_channels; a.groups = (int)d.groups;
  a.ulog = __builtin_ctzll((unsigned long long)d.head);
  a.io = d.dtype;
}

extern "C" int fc_long_step(const fc_long_step_desc* desc, const void* x_t, const void* pregate, const void* postgate,
                            const float* head_taps, const float* bias, float* hist, const float* acc, void* y_t, int64_t t,
                            int64_t first, void* hip_stream) {
  if (!desc || !x_t || !head_taps || !hist || !acc || !y_t) return fail(FC_ERR_INVALID, "null argument");
  const fc_long_step_desc& d = *desc;
  if (int st = step_desc_counts(d)) return st;
  if (t < 0 || t >= d.max_len)
    return fail(FC_ERR_INVALID, "position %lld lies outside the stream's max_len = %lld", (long long)t, (long long)d.max_len);
  if (first < 0 || first > t)
    return fail(FC_ERR_INVALID, "first (%lld) must lie in [0, t = %lld]", (long long)first, (long long)t);
  if (int st = step_desc_limits(d)) return st;
  LongStepArgs a;
  fill_state(a, d, x_t, pregate, postgate, head_taps, bias, hist, acc, y_t);
  a.t = t;
  a.reach = (int)std::min<int64_t>(d.head - 1, t - first);
  const int waves = (int)std::min<int64_t>(d.out_channels / d.groups, kLongStepWaves);
  FC_HIP(long_step_launch(a, d.batch * d.groups, waves, static_cast<hipStream_t>(hip_stream)));
  return FC_OK;
}

// A chunk of `count` columns from t0 on, for the push and the draft alike: the refusals of the call's position, then
// what the kernels address ...
static int chunk_checks(const fc_long_step_desc& d, int64_t t0, int64_t count, int64_t first) {
  if (count < 1) return fail(FC_ERR_INVALID, "count (%lld) must be positive", (long long)count);
  if (t0 < 0 || t0 > d.max_len - count)
    return fail(FC_ERR_INVALID, "the columns [%lld, %lld + %lld) lie outside the stream's max_len = %lld", (long long)t0,
                (long long)t0, (long long)count, (long long)d.max_len);
  if (first < 0 || first > t0)
    return fail(FC_ERR_INVALID, "first (%lld) must lie in [0, t0 = %lld]", (long long)first, (long long)t0);
  return step_desc_limits(d);
}

struct ChunkLaunch { long long grid; int waves; size_t lds; };      // workgroups, waves of each, bytes of dynamic LDS

// ... and last (the draft's own limit comes before it) the workgroups of the launch; then what fill_state leaves open
static int fill_chunk(LongPushArgs& a, ChunkLaunch& l, const fc_long_step_desc& d, int64_t t0, int64_t count, int64_t first) {
  const int64_t tiles = (count + 63) / 64;      // (count <= max_len < 2^29)
  if (d.batch * d.groups > 0x7fffffffLL / tiles)
    return fail(FC_ERR_UNSUPPORTED, "%lld batch items x %lld groups x %lld tiles of 64 columns exceed the 2^31 workgroups of "
                "one launch", (long long)d.batch, (long long)d.groups, (long long)tiles);
  a.t0 = t0; a.count = count; a.first = first;
  a.tiles = (int)tiles;
  const int64_t window = (64 + d.head - 1) * 4;      // bytes of one channel's staged samples: at most 4348
  a.cblock = (int)std::min<int64_t>(d.in_channels / d.groups, kLongPushLds / window);
  l = {d.batch * d.groups * tiles, (int)std::min<int64_t>(d.out_channels / d.groups, kLongPushWaves),
       (size_t)(a.cblock * window)};
  return FC_OK;
}

extern "C" int fc_long_push(const fc_long_step_desc* desc, const void* x, const void* pregate, const void* postgate,
                            const float* head_taps, const float* bias, float* hist, const float* acc, void* y, int64_t t0,
                            int64_t count, int64_t first, void* hip_stream) {
  if (!desc || !x || !head_taps || !hist || !acc || !y) return fail(FC_ERR_INVALID, "null argument");
  const fc_long_step_desc& d = *desc;
  if (int st = step_desc_counts(d)) return st;
  if (int st = chunk_checks(d, t0, count, first)) return st;
  LongPushArgs a;
  ChunkLaunch l;
  if (int st = fill_chunk(a, l, d, t0, count, first)) return st;
  fill_state(a, d, x, pregate, postgate, head_taps, bias, hist, acc, y);
  FC_HIP(long_push_launch(a, l.grid, l.waves, l.lds, static_cast<hipStream_t>(hip_stream)));
  return FC_OK;
}

extern "C" int fc_long_spec(const fc_long_step_desc* desc, const void* x, const void* pregate, const void* postgate,
                            const float* head_taps, const float* filter_flipped, const float* bias, float* hist,
                            const float* acc, void* y, int64_t t0, int64_t count, int64_t first, void* hip_stream) {
  if (!desc || !x || !head_taps || !filter_flipped || !hist || !acc || !y) return fail(FC_ERR_INVALID, "null argument");
  const fc_long_step_desc& d = *desc;
  if (int st = step_desc_counts(d)) return st;
  if (int st = chunk_checks(d, t0, count, first)) return st;
  if (count > d.head)
    return fail(FC_ERR_INVALID, "count (%lld) exceeds head = %lld: a draft is verified against the head taps and the blocks "
                "due at one multiple of head", (long long)count, (long long)d.head);
  LongSpecArgs s;
  ChunkLaunch l;
  if (int st = fill_chunk(s.p, l, d, t0, count, first)) return st;
  fill_state(s.p, d, x, pregate, postgate, head_taps, bias, hist, acc, y);
  // the one multiple of head that can lie inside (t0, t0 + count); its blocks are due only if it does and below max_len
  const int64_t m = (t0 / d.head + 1) * d.head;
  s.flipped = filter_flipped; s.K = d.kernel; s.M = t0 + count; s.levels = 0;      // (M = the end: no column at or past it)
  if (m < t0 + count && m < d.max_len) {
    s.M = m;
    for (int64_t n = d.head; n < d.kernel && m % n == 0; n *= 2) ++s.levels;      // (n <= m < 2^29: at most 26 levels)
  }
  FC_HIP(long_spec_launch(s, l.grid, l.waves, l.lds, static_cast<hipStream_t>(hip_stream)));
  return FC_OK;
}
