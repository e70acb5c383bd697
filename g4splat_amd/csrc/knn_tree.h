// The 64-ary box tree over a Z-curve order that knn.hip (distCUDA2) and tsdf/mesh_eval.hip (nearest neighbour between two
// clouds) both build and walk: the boxes, the extent / curve / leaves / parents kernels, the two gap bounds and the
// wave-level helpers of the walk.  knn.hip's header describes the tree; each unit keeps its own search kernel.
#pragma once
#include <float.h>

#include "g4s_internal.h"
#include "g4s_device.h"

namespace g4s {

constexpr int KNN_LEAF = 64;  // points per leaf = lanes per wave
constexpr int KNN_FAN = 64;   // children per inner node = lanes per wave

struct KnnLayout {
    size_t keys_a, keys_b, vals_a, vals_b, hist, bin_total, sorted, nodes, partial, extent, bytes;
    int n0, n1, n2, nparts;  // leaves, level-1 nodes, level-2 (top) nodes
};
inline KnnLayout knn_layout(size_t P) {
    KnnLayout L{};
    WorkspaceCursor c;
    L.n0 = (int)((P + KNN_LEAF - 1) / KNN_LEAF);
    L.n1 = (L.n0 + KNN_FAN - 1) / KNN_FAN;
    L.n2 = (L.n1 + KNN_FAN - 1) / KNN_FAN;
    L.nparts = (int)((P + 1023) / 1024);
    L.keys_a = c.take(P * 4); L.keys_b = c.take(P * 4); L.vals_a = c.take(P * 4); L.vals_b = c.take(P * 4);
    L.hist = c.take((size_t)256 * (sort_blocks(P, SORT_ITEMS_U32) + 1) * 4);
    L.bin_total = c.take(256 * 4);
    L.sorted = c.take((size_t)(L.n0 ? L.n0 : 1) * KNN_LEAF * 16);
    L.nodes = c.take((size_t)(L.n0 + L.n1 + L.n2 + 1) * 32);
    L.partial = c.take((size_t)(L.nparts ? L.nparts : 1) * 32);
    L.extent = c.take(32);
    L.bytes = c.off + 256;
    return L;
}

// axis-aligned box, 32 bytes (two quads): lo.xyz, hi.xyz
struct Box {
    float lx, ly, lz, hx, hy, hz, pad0, pad1;
};
__device__ __forceinline__ Box box_empty() { return Box{FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX, 0, 0}; }
__device__ __forceinline__ void box_join(Box& a, const Box& b) {
    a.lx = fminf(a.lx, b.lx); a.ly = fminf(a.ly, b.ly); a.lz = fminf(a.lz, b.lz);
    a.hx = fmaxf(a.hx, b.hx); a.hy = fmaxf(a.hy, b.hy); a.hz = fmaxf(a.hz, b.hz);
}
// union over the 64 lanes, valid in every lane
__device__ __forceinline__ Box box_wave_join(Box m) {
    for (int off = 32; off >= 1; off >>= 1) {
        Box o;
        o.lx = __shfl_xor(m.lx, off, 64); o.ly = __shfl_xor(m.ly, off, 64); o.lz = __shfl_xor(m.lz, off, 64);
        o.hx = __shfl_xor(m.hx, off, 64); o.hy = __shfl_xor(m.hy, off, 64); o.hz = __shfl_xor(m.hz, off, 64);
        box_join(m, o);
    }
    return m;
}
// union over a 1024-thread block; result valid in thread 0
__device__ __forceinline__ Box box_block_join(Box m, Box* sm16) {
    m = box_wave_join(m);
    const int w = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) sm16[w] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < 16; i++) box_join(m, sm16[i]);
    return m;
}

// ---- extent of the cloud (stays on the device) ------------------------------------------------------------------
static __global__ void __launch_bounds__(1024) knn_extent_partial_kernel(int P, const float* __restrict__ pts, Box* __restrict__ partial) {
    __shared__ Box sm[16];
    const int i = (int)(blockIdx.x * 1024 + threadIdx.x);
    Box m = box_empty();
    if (i < P) {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        m = Box{x, y, z, x, y, z, 0, 0};
    }
    m = box_block_join(m, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}
static __global__ void __launch_bounds__(1024) knn_extent_final_kernel(int nparts, const Box* __restrict__ partial, Box* __restrict__ extent) {
    __shared__ Box sm[16];
    Box m = box_empty();
    for (int i = (int)threadIdx.x; i < nparts; i += 1024) box_join(m, partial[i]);
    m = box_block_join(m, sm);
    if (threadIdx.x == 0) *extent = m;
}

// ---- position on the Z-curve ---------------------------------------------------------------------------------------
// bit i of a 10-bit value -> bit 3 i.  Each step doubles the gaps by adding a shifted copy (a multiplication by
// 2^k + 1: the copies never overlap, so the sum is an OR) and masking.
__device__ __forceinline__ uint32_t spread_by_3(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
// Lattice of 1024^3 CUBIC cells anchored at the cloud's lower corner, edge = longest extent / 1023.  (The order only
// has to be spatially coherent -- the result does not depend on it --, so NaN / inf coordinates simply land in cell 0.)
static __global__ void __launch_bounds__(256) knn_curve_kernel(int P, const float* __restrict__ pts, const Box* __restrict__ extent,
                                                        uint32_t* __restrict__ codes, uint32_t* __restrict__ idx) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P) return;
    const Box b = *extent;
    const float edge = fmaxf(fmaxf(b.hx - b.lx, b.hy - b.ly), b.hz - b.lz);
    const float cells = edge > 0.0f ? 1023.0f / edge : 0.0f;
    auto cell = [&](float v, float lo) {
        const float c = fminf(fmaxf((v - lo) * cells, 0.0f), 1023.0f);  // NaN -> 0
        return (uint32_t)c;
    };
    const uint32_t cx = cell(pts[3 * (size_t)i], b.lx), cy = cell(pts[3 * (size_t)i + 1], b.ly), cz = cell(pts[3 * (size_t)i + 2], b.lz);
    codes[i] = spread_by_3(cx) | (spread_by_3(cy) << 1) | (spread_by_3(cz) << 2);
    idx[i] = (uint32_t)i;
}

// ---- the tree ------------------------------------------------------------------------------------------------------
// A wave per leaf: gathers its 64 points in curve order (padding slots: NaN coordinates, which no comparison ever
// accepts) and stores the leaf's box.
static __global__ void __launch_bounds__(256) knn_leaves_kernel(int P, int n0, const float* __restrict__ pts, const uint32_t* __restrict__ order,
                                                         float4* __restrict__ sorted, Box* __restrict__ leaves) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);  // a wave per leaf, four per workgroup
    if ((i >> 6) >= n0) return;
    Box m = box_empty();
    float4 rec = make_float4(__uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u),
                             __uint_as_float(0xFFFFFFFFu));
    if (i < P) {
        const uint32_t src = order[i];
        const float x = pts[3 * (size_t)src], y = pts[3 * (size_t)src + 1], z = pts[3 * (size_t)src + 2];
        rec = make_float4(x, y, z, __uint_as_float(src));
        m = Box{x, y, z, x, y, z, 0, 0};
    }
    sorted[i] = rec;
    m = box_wave_join(m);
    if ((threadIdx.x & 63) == 0) leaves[i >> 6] = m;
}
// A wave per parent: the union of its (up to) 64 children.
static __global__ void __launch_bounds__(256) knn_parents_kernel(int n_child, const Box* __restrict__ child, int n_parent, Box* __restrict__ parent) {
    const int w = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= n_parent) return;
    const int c = w * KNN_FAN + (int)(threadIdx.x & 63);
    Box m = c < n_child ? child[c] : box_empty();
    m = box_wave_join(m);
    if ((threadIdx.x & 63) == 0) parent[w] = m;
}

// ---- the search ----------------------------------------------------------------------------------------------------
// Squared gap between two boxes / between a point and a box, with the operations of the distance itself in its own
// order (gap per axis by subtraction, three squares, (x^2 + y^2) + z^2): a lower bound, in floating point, of the
// distance computed for any candidate inside the box (see the header).  An empty box gives +inf (or NaN: not < r2).
__device__ __forceinline__ float gap2_box_box(const Box& a, const Box& q) {
    const float gx = fmaxf(fmaxf(a.lx - q.hx, q.lx - a.hx), 0.0f);
    const float gy = fmaxf(fmaxf(a.ly - q.hy, q.ly - a.hy), 0.0f);
    const float gz = fmaxf(fmaxf(a.lz - q.hz, q.lz - a.hz), 0.0f);
    return gx * gx + gy * gy + gz * gz;
}
__device__ __forceinline__ float gap2_box_point(float lx, float ly, float lz, float hx, float hy, float hz, float x, float y, float z) {
    const float gx = fmaxf(fmaxf(lx - x, x - hx), 0.0f);
    const float gy = fmaxf(fmaxf(ly - y, y - hy), 0.0f);
    const float gz = fmaxf(fmaxf(lz - z, z - hz), 0.0f);
    return gx * gx + gy * gy + gz * gz;
}
// lane j's value of v as a wave-uniform (scalar) value; j is uniform
__device__ __forceinline__ float lane_value(float v, int j) {
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), j));
}
__device__ __forceinline__ float wave_max_nonneg(float v) {  // v >= 0: the bit patterns order like the values
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(__float_as_uint(v))));
}

// Parks a leaf in the wave's 1-KB stage: one coalesced fetch, then broadcast reads.  LDS traffic of one wave is ordered
// by the hardware; the fences only keep the compiler from moving the broadcast reads above the store that feeds them
// (or the next store above the last reads).
__device__ __forceinline__ void stage_leaf(const float4* __restrict__ sorted, int leaf, int lane, float4* stage) {
    const float4 c = sorted[(size_t)leaf * KNN_LEAF + lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    stage[lane] = c;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Queues the tree of `points` into the workspace carved by knn_layout(P): extent, curve codes, sort, leaves, two levels
// of parents (10 launches, 8 of them the sort's).  Returns which key buffer holds the sorted codes (0 = keys_a).
inline int knn_build_tree(const KnnLayout& L, int P, const float* points, char* w, hipStream_t s) {
    uint32_t* keys_a = (uint32_t*)(w + L.keys_a);
    uint32_t* keys_b = (uint32_t*)(w + L.keys_b);
    uint32_t* vals_a = (uint32_t*)(w + L.vals_a);
    uint32_t* vals_b = (uint32_t*)(w + L.vals_b);
    Box* partial = (Box*)(w + L.partial);
    Box* extent = (Box*)(w + L.extent);
    Box* leaves = (Box*)(w + L.nodes);
    Box* mids = leaves + L.n0;
    Box* tops = mids + L.n1;
    float4* sorted = (float4*)(w + L.sorted);
    hipLaunchKernelGGL(knn_extent_partial_kernel, dim3(L.nparts), dim3(1024), 0, s, P, points, partial);
    hipLaunchKernelGGL(knn_extent_final_kernel, dim3(1), dim3(1024), 0, s, L.nparts, partial, extent);
    hipLaunchKernelGGL(knn_curve_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, points, extent, keys_a, vals_a);
    const int cur = radix_sort_u32_pairs(keys_a, keys_b, vals_a, vals_b, P, (uint32_t*)(w + L.hist),
                                         (uint32_t*)(w + L.bin_total), s);
    const uint32_t* order = cur ? vals_b : vals_a;
    const int leaf_blocks = (L.n0 + 3) / 4;  // four leaves (waves) per workgroup
    hipLaunchKernelGGL(knn_leaves_kernel, dim3(leaf_blocks), dim3(256), 0, s, P, L.n0, points, order, sorted, leaves);
    hipLaunchKernelGGL(knn_parents_kernel, dim3((L.n1 + 3) / 4), dim3(256), 0, s, L.n0, leaves, L.n1, mids);
    hipLaunchKernelGGL(knn_parents_kernel, dim3((L.n2 + 3) / 4), dim3(256), 0, s, L.n1, mids, L.n2, tops);
    return cur;
}

}  // namespace g4s
