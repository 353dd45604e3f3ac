// long_step.hip -- the builds of long_step_kernel (long_step.hpp), long_push_kernel (long_push.hpp) and long_spec_kernel
// (long_spec.hpp) and their launches: an object of its own.
#include "long_step.hpp"

#include "launch.hpp"
#include "long_push.hpp"
#include "long_spec.hpp"

namespace fc {

// the float32 or the 16-bit build of a kernel by the fc_dtype code `io` of its arguments
template <auto F32, auto H16, class Args>
static hipError_t launch_by_io(int io, long long grid, int waves, size_t lds, hipStream_t st, const Args& a) {
  if (io == 0) return launch_kernel<F32>(grid, 64u * waves, lds, st, a);
  if (io_is_h16(io)) return launch_kernel<H16>(grid, 64u * waves, lds, st, a);
  return hipErrorInvalidValue;
}

hipError_t long_step_launch(const LongStepArgs& a, long long grid, int waves, hipStream_t st) {
  if (waves < 1 || waves > kLongStepWaves) return hipErrorInvalidValue;
  return launch_by_io<long_step_kernel<IO_F32>, long_step_kernel<IO_H16>>(a.io, grid, waves, 0, st, a);
}

hipError_t long_push_launch(const LongPushArgs& a, long long grid, int waves, size_t lds, hipStream_t st) {
  if (waves < 1 || waves > kLongPushWaves || lds > (size_t)kLongPushLds) return hipErrorInvalidValue;
  return launch_by_io<long_push_kernel<IO_F32>, long_push_kernel<IO_H16>>(a.io, grid, waves, lds, st, a);
}

hipError_t long_spec_launch(const LongSpecArgs& s, long long grid, int waves, size_t lds, hipStream_t st) {
  if (waves < 1 || waves > kLongPushWaves || lds > (size_t)kLongPushLds) return hipErrorInvalidValue;
  return launch_by_io<long_spec_kernel<IO_F32>, long_spec_kernel<IO_H16>>(s.p.io, grid, waves, lds, st, s);
}

}  // namespace fc
