// The sums whose ORDER is part of a contract: everything that returns a loss, a fitted scale and shift, a plane or a
// k-means centre gives the same bits in every run because it adds in the order stated here.  One definition of each
// building block, on top of the wave sums of g4s_device.h (wave_sum_to_lane63, wave_fold); DESIGN.md "Fixed-order sums"
// lists which unit uses which.
#pragma once
#include "g4s_device.h"

namespace g4s {

// ---- one value over a 256-thread block.  Every thread of the block has to call these; s4 holds four values of this
// sum's own; the result is valid in every thread (the callers store it from thread 0).

// float32: the DPP ladder of wave_sum_to_lane63, lane 63 of each wave stores, (s0 + s1) + (s2 + s3)
__device__ __forceinline__ float block_sum(float v, float* s4) {
    v = wave_sum_to_lane63(v);
    if ((threadIdx.x & 63) == 63) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// float64: wave_fold's tree (lane 0 ends with ((((v0 + v32) + (v16 + v48)) + ...): at every step a lane adds the partner's
// value to its own), lane 0 of each wave stores.  The two orders differ in how the four wave sums are added.
__device__ __forceinline__ void block_wave_sums(double v, double* s4) {
    v = wave_fold(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
}
// pairs: (s0 + s1) + (s2 + s3)
__device__ __forceinline__ double block_sum_pairs(double v, double* s4) {
    block_wave_sums(v, s4);
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}
// chain: ((s0 + s1) + s2) + s3
__device__ __forceinline__ double block_sum_chain(double v, double* s4) {
    block_wave_sums(v, s4);
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// ---- a row of float64 moments of a 256-thread block, in the chain order, behind ONE barrier: moment_fold once per term
// (every thread), then moment_store once (every thread); thread c < terms stores ((w0 + w1) + w2) + w3 of term c.
template <int STRIDE>
__device__ __forceinline__ void moment_fold(double s, double (*waves)[STRIDE], int term) {
    const double w = wave_fold(s);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6][term] = w;
}
template <int STRIDE>
__device__ __forceinline__ void moment_store(const double (*waves)[STRIDE], int terms, double* __restrict__ row) {
    __syncthreads();
    if ((int)threadIdx.x < terms) {
        const int c = (int)threadIdx.x;
        row[c] = ((waves[0][c] + waves[1][c]) + waves[2][c]) + waves[3][c];
    }
}

// ---- K columns of a run of `count` moment rows (`stride` doubles apart), by ONE wave of 64 threads: thread t adds rows
// t, t + 64, ... in ascending order, then wave_fold; the totals are valid in lane 0.
template <int K>
__device__ __forceinline__ void column_fold(const double* __restrict__ rows, uint32_t count, int stride, double (&s)[K]) {
#pragma unroll
    for (int c = 0; c < K; c++) s[c] = 0.0;
    for (uint32_t b = threadIdx.x; b < count; b += 64u) {
        const double* p = rows + (size_t)b * stride;
#pragma unroll
        for (int c = 0; c < K; c++) s[c] += p[c];
    }
#pragma unroll
    for (int c = 0; c < K; c++) s[c] = wave_fold(s[c]);
}

// ---- `count` rows of K per-block partials by ONE workgroup of 1024 threads: thread t adds rows t, t + 1024, ... in
// ascending order in double, then an LDS tree (512, 256, ..., 1) adds the 1024 sums; the K totals are left in s_v[k][0],
// readable by every thread.  Four independent row loads are in flight per thread (a serial loop of dependent round trips
// over the 22 500 block partials of a 1600x1200 frame took 24 us).  A row is K values of T at a multiple of its own size.
template <int K, class T>
struct alignas(((K & (K - 1)) == 0 ? K : 1) * sizeof(T)) PartialRow {
    T v[K];
};
template <int K, class T>
__device__ __forceinline__ void fold_partials(const T* partials, int count, double (&s_v)[K][1024]) {
    const PartialRow<K, T>* rows = reinterpret_cast<const PartialRow<K, T>*>(partials);
    double v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = 0;
    for (int i0 = (int)threadIdx.x; i0 < count; i0 += 4096) {
        PartialRow<K, T> r[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = i0 + 1024 * j;
            r[j] = rows[i < count ? i : 0];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i0 + 1024 * j < count) {
#pragma unroll
                for (int k = 0; k < K; k++) v[k] += (double)r[j].v[k];
            }
        }
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

// ---- the scale and shift of a least-squares line t ~ alpha + beta d from its five moments (n, sum t, sum d, sum t d,
// sum d d): what the depth cues' alignment and the chart points' disparity fit end with, one thread
__device__ __forceinline__ void scale_shift_solve(const double (&s)[5], float* __restrict__ coeffs2, int* __restrict__ count) {
    const double n = s[0], St = s[1], Sd = s[2], Std = s[3], Sdd = s[4];
    const double beta = (Std - St * Sd / n) / (Sdd - Sd * Sd / n);
    const double alpha = (St - beta * Sd) / n;
    coeffs2[0] = (float)alpha;
    coeffs2[1] = (float)beta;
    *count = (int)n;
}

}  // namespace g4s
