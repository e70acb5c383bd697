// The core of the chart units (chart_loss.hip, chart_match.hip, chart_align.hip, chart_deform.hip, chart_points.hip):
//   - the sign with sign(0) = 0 that autograd's abs takes and the clamped coordinate of replicate padding;
//   - the deterministic sums over a 256-thread block, one function per order of summation that a unit's contract states;
//   - the one-workgroup fold of per-block partials that ends every loss value;
//   - the per-view block count of the units that give 256 consecutive pixels of ONE view to a block.
// The host-side checks and workspace layouts these units use (null_pointer, check_workspace, WorkspaceCursor,
// workspace_at, blocks256) are in g4s_internal.h.
#pragma once
#include "g4s_device.h"

namespace g4s {

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float signf(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }  // sign(0) = 0

// ---- sums over a 256-thread block in a fixed order.  Every thread of the block has to call them; s4 holds four values of
// this sum's own; the result is valid in every thread (the callers store it from thread 0).

// float32 (chart_loss, chart_match): the DPP ladder of wave_sum_to_lane63, lane 63 of each wave stores, (s0 + s1) + (s2 + s3)
__device__ __forceinline__ float chart_block_sum(float v, float* s4) {
    v = wave_sum_to_lane63(v);
    if ((threadIdx.x & 63) == 63) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// float64: wave_fold's tree (lane 0 ends with ((((v0 + v32) + (v16 + v48)) + ...): at every step a lane adds the partner's
// value to its own), lane 0 of each wave stores.  The two orders differ in how the four wave sums are added.
__device__ __forceinline__ void chart_wave_sums(double v, double* s4) {
    v = wave_fold(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
}
// chart_align: (s0 + s1) + (s2 + s3)
__device__ __forceinline__ double chart_block_sum_pairs(double v, double* s4) {
    chart_wave_sums(v, s4);
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}
// chart_points (the order of the depth cues' alignment): ((s0 + s1) + s2) + s3
__device__ __forceinline__ double chart_block_sum_chain(double v, double* s4) {
    chart_wave_sums(v, s4);
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// ---- the fold of `count` rows of K per-block partials by ONE workgroup of 1024 threads: thread t adds rows t, t + 1024, ...
// in ascending order in double, then an LDS tree (512, 256, ..., 1) adds the 1024 sums; the K totals are left in s_v[k][0],
// readable by every thread.  Fixed association => bit-reproducible.
template <int K, class T>
__device__ __forceinline__ void chart_fold_partials(const T* partials, int count, double (&s_v)[K][1024]) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = 0;
    for (int i = (int)threadIdx.x; i < count; i += 1024) {
#pragma unroll
        for (int k = 0; k < K; k++) v[k] += (double)partials[K * (size_t)i + k];
    }
#pragma unroll
    for (int k = 0; k < K; k++) s_v[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < K; k++) s_v[k][threadIdx.x] += s_v[k][threadIdx.x + o];
        }
        __syncthreads();
    }
}

// blocks of 256 consecutive pixels that cover ONE view of height x width (chart_match, chart_align)
inline unsigned chart_view_blocks(int height, int width) { return blocks256((long long)height * width); }

}  // namespace g4s
