// long_step.hip -- the builds of long_step_kernel (long_step.hpp), long_push_kernel (long_push.hpp) and long_spec_kernel
// (long_spec.hpp) and their launches: an object of its own.
#include "long_step.hpp"

#include "launch.hpp"
#include "long_push.hpp"
#include "long_spec.hpp"

namespace fc {

hipError_t long_step_launch(const LongStepArgs& a, long long grid, int waves, hipStream_t st) {
  if (waves < 1 || waves > kLongStepWaves) return hipErrorInvalidValue;
  if (a.io == 0) return launch_kernel<long_step_kernel<IO_F32>>(grid, 64u * waves, 0, st, a);
  if (io_is_h16(a.io)) return launch_kernel<long_step_kernel<IO_H16>>(grid, 64u * waves, 0, st, a);
  return hipErrorInvalidValue;
}

hipError_t long_push_launch(const LongPushArgs& a, long long grid, int waves, size_t lds, hipStream_t st) {
  if (waves < 1 || waves > kLongPushWaves || lds > (size_t)kLongPushLds) return hipErrorInvalidValue;
  if (a.io == 0) return launch_kernel<long_push_kernel<IO_F32>>(grid, 64u * waves, lds, st, a);
  if (io_is_h16(a.io)) return launch_kernel<long_push_kernel<IO_H16>>(grid, 64u * waves, lds, st, a);
  return hipErrorInvalidValue;
}

hipError_t long_spec_launch(const LongSpecArgs& s, long long grid, int waves, size_t lds, hipStream_t st) {
  if (waves < 1 || waves > kLongPushWaves || lds > (size_t)kLongPushLds) return hipErrorInvalidValue;
  if (s.p.io == 0) return launch_kernel<long_spec_kernel<IO_F32>>(grid, 64u * waves, lds, st, s);
  if (io_is_h16(s.p.io)) return launch_kernel<long_spec_kernel<IO_H16>>(grid, 64u * waves, lds, st, s);
  return hipErrorInvalidValue;
}

}  // namespace fc
