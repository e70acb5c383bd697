// What the chart units (chart_loss.hip, chart_align.hip) share on the device: the sign with sign(0) = 0 that autograd's abs
// takes and the clamped coordinate of replicate padding.
#pragma once

namespace g4s {

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float signf(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }  // sign(0) = 0

}  // namespace g4s
