// zero_loss.h -- the zero-interference losses of the side branches, L(v, 0) per element and its slope, as ATen's L1Loss and
// SmoothL1Loss (beta = 1) compute them in fp32: the sign and the SmoothL1 pair.  Everything here is internal linkage.
//
// What this pins: sgn(NaN) = 0, as ATen's sign -- both comparisons fail -- so a NaN activation sends a zero, not a -1, down
// the L1 slope and the SmoothL1 slope's outer part.
#ifndef ZIRA_ZERO_LOSS_H_
#define ZIRA_ZERO_LOSS_H_

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// (L1 is fabsf(v) with slope sign_of(v), L2 is v * v with slope 2 v: cet.hip's switch spells them in place)
__device__ __forceinline__ float smooth_l1_zero(float v)
{
    const float a = fabsf(v);
    return a < 1.f ? 0.5f * v * v : a - 0.5f;
}
__device__ __forceinline__ float smooth_l1_zero_slope(float v) { return fabsf(v) < 1.f ? v : sign_of(v); }

}  // namespace

#endif  // ZIRA_ZERO_LOSS_H_
