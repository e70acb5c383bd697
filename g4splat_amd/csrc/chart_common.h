// What the chart units (chart_loss.hip, chart_match.hip, chart_align.hip, chart_deform.hip, chart_points.hip) share that
// is about charts:
//   - the sign with sign(0) = 0 that autograd's abs takes and the clamped coordinate of replicate padding;
//   - the per-view block count of the units that give 256 consecutive pixels of ONE view to a block.
// Their deterministic sums are in fixed_sums.h; the host-side checks and workspace layouts they use (null_pointer,
// check_workspace, WorkspaceCursor, workspace_at, blocks256) are in g4s_internal.h.
#pragma once
#include "g4s_internal.h"

namespace g4s {

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float signf(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }  // sign(0) = 0

// blocks of 256 consecutive pixels that cover ONE view of height x width (chart_match, chart_align)
inline unsigned chart_view_blocks(int height, int width) { return blocks256((long long)height * width); }

}  // namespace g4s
