// axis_map.hpp -- index maps of one padded axis, shared by the fp32 N-d passes (nd_passes.hpp, planes3d.hpp) and the
// float64 FFT kernels (fft_f64.hip, nd_f64.hip): padded coordinate -> unpadded source index or -1 (a zero).
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

enum PadMode : int { PAD_CONSTANT = 0, PAD_REFLECT = 1, PAD_REPLICATE = 2, PAD_CIRCULAR = 3 };

// Index map of one padded axis: position p in [0, n_padded) -> source index or -1 (zero).
struct AxisMap {
  int size;       // unpadded extent
  int pad;        // left padding (may be negative for a transposed plan)
  int mode;       // PadMode
  int up;         // transposed plan: source spread over a grid of this step
};
__device__ __forceinline__ int axis_src(const AxisMap& m, int p) {   // p: padded coordinate
  const int pos = p - m.pad;
  if (m.up > 1) {
    const int q = pos / m.up;
    return (pos >= 0 && q * m.up == pos && q < m.size) ? q : -1;
  }
  if ((unsigned)pos < (unsigned)m.size) return pos;
  if (pos < -m.pad || pos >= m.size + m.pad || m.mode == PAD_CONSTANT) return -1;
  if (m.mode == PAD_REFLECT) return pos < 0 ? -pos : 2 * (m.size - 1) - pos;
  if (m.mode == PAD_REPLICATE) return pos < 0 ? 0 : m.size - 1;
  return pos < 0 ? pos + m.size : pos - m.size;
}
// Kernel taps: position p -> tap index p/dil if p is a multiple of dil and in range.
__device__ __forceinline__ int tap_src(int p, int dil, int k) {
  const int t = p / dil;
  return (t * dil == p && t < k) ? t : -1;
}

}  // namespace fc
