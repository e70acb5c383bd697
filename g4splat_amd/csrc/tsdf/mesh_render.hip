// Mesh rasteriser and dilated depth (include/g4s_render_maps.h, "Mesh rasteriser and dilated depth"; the semantics stated
// there are the contract, tests/mesh_render_ref.py restates them in numpy).
//
// One primitive, a nearest-face-per-pixel z-buffer, in two passes over a [H*W] buffer of 64-bit keys
// float_bits(zpix) << 32 | face that starts as all-ones:
// Pass 1, coverage and depth.  One thread per face: indices checked, vertices projected and snapped to 1/256 pixel, the
//   clamped pixel box formed.  A box of at most MR_SMALL_BOX samples is walked by its thread.  Any other face is appended to
//   a list (one atomic add per wave: ballot, the leader adds the wave's count, every lane writes at its rank), and a
//   second launch rasterises the list with one wave per (face, slice), 64 samples of the box per step, so that no thread
//   ever walks a box longer than MR_SMALL_BOX and a screen-filling triangle is spread over MR_LARGE_SLICES waves.  The list's
//   length stays on the device: the second launch has a fixed grid that strides over it, so nothing is read back and the
//   whole call can be captured.  A sample's key goes in by an unsigned 64-bit atomic min after a plain read (planes.hip's
//   idiom: the cell only ever decreases, so a value read is an upper bound of the final one).  Integer min is
//   order-independent: two runs give the same bits, whatever the order of the list.
// Pass 2, resolve.  One thread per pixel reads its key once and recomputes the winner's weights with the same device
//   function that pass 1 used, so the depth in the key and the weights written belong to one evaluation.
// Dilate.  One launch forms the dilated view-space vertices of every view of the stack (12 B per pixel in the workspace,
//   the view table through view_stack.h); the raster runs over (view, cell) with the two faces of a cell generated from its
//   index -- no face list exists --, and the resolve falls back to the input maps where nothing won.
#include <math.h>

#include <algorithm>
#include <vector>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "view_stack.h"

namespace g4s {

constexpr int MR_SMALL_BOX = 64;     // samples: the box one wave of the large path covers in a single step
constexpr int MR_LARGE_SLICES = 8;   // waves that share a listed face; slice s takes the 64-sample chunks s, s + 8, ...
constexpr int MR_LARGE_BLOCKS = 512; // workgroups (of four waves) of the list launch per slice, at most
constexpr int MR_MAX_CHANNELS = G4S_MESH_RASTER_MAX_CHANNELS;
constexpr unsigned long long MR_EMPTY = ~0ull;
#define MR_INF __builtin_inff()

// A projection is any record with pm[16], off, znear, W, H and -- iff HAS_WV -- wv[16]; without, the positions are in view
// space already.  The mesh kernels hand in their argument block itself, read by constant indices, so it stays in scalar
// registers (a pointer into it would send the whole block through scratch); the dilation hands in this view of a table row.
struct MrViewSpace {
    static constexpr bool HAS_WV = false;
    const float* wv;  // unused
    const float* pm;
    float off, znear;
    int W, H;
};

enum MrStatus { MR_OK = 0, MR_SKIP = 1, MR_BEHIND = 2, MR_GUARD_BAND = 3 };

struct MrFace {
    int X[3], Y[3];  // snapped, 1/256 pixel
    float sx[3], sy[3], z[3];
    int s;           // +1 / -1: the orientation that makes the area positive
    int x0, x1, y0, y1;  // clamped pixel box; empty: x0 > x1 or y0 > y1
};

template <class Proj>
__device__ __forceinline__ bool mr_project(const Proj& c, const float (&p)[3], float& sx, float& sy, float& z) {
    float v0 = p[0], v1 = p[1], v2 = p[2];
    if (Proj::HAS_WV) {
        const auto& M = c.wv;
        v0 = ((p[0] * M[0] + p[1] * M[4]) + p[2] * M[8]) + M[12];
        v1 = ((p[0] * M[1] + p[1] * M[5]) + p[2] * M[9]) + M[13];
        v2 = ((p[0] * M[2] + p[1] * M[6]) + p[2] * M[10]) + M[14];
    }
    const auto& P = c.pm;
    const float q0 = ((v0 * P[0] + v1 * P[4]) + v2 * P[8]) + P[12];
    const float q1 = ((v0 * P[1] + v1 * P[5]) + v2 * P[9]) + P[13];
    const float q3 = ((v0 * P[3] + v1 * P[7]) + v2 * P[11]) + P[15];
    z = v2;
    sx = ((1.0f + q0 / q3) * (float)c.W) / 2.0f - c.off;
    sy = ((1.0f + q1 / q3) * (float)c.H) / 2.0f - c.off;
    return v2 > c.znear && v2 < MR_INF && fabsf(sx) < MR_INF && fabsf(sy) < MR_INF;  // a NaN fails
}

__device__ __forceinline__ int mr_floor256(int v) { return v >> 8; }  // arithmetic shift: floor for negatives too

// p: the three positions.  MR_OK leaves a complete face behind.
template <class Proj>
__device__ __forceinline__ int mr_setup(const Proj& c, const float (&p)[3][3], MrFace& f) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) ok = mr_project(c, p[k], f.sx[k], f.sy[k], f.z[k]) && ok;
    if (!ok) return MR_BEHIND;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (fabsf(f.sx[k]) > 32768.0f || fabsf(f.sy[k]) > 32768.0f) return MR_GUARD_BAND;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        f.X[k] = (int)rintf(f.sx[k] * 256.0f);  // exact: |sx * 256| <= 2^23
        f.Y[k] = (int)rintf(f.sy[k] * 256.0f);
    }
    const long long area = (long long)(f.X[1] - f.X[0]) * (f.Y[2] - f.Y[0]) - (long long)(f.Y[1] - f.Y[0]) * (f.X[2] - f.X[0]);
    if (area == 0) return MR_SKIP;
    f.s = area > 0 ? 1 : -1;
    const int xl = imin_(f.X[0], imin_(f.X[1], f.X[2])), xh = imax_(f.X[0], imax_(f.X[1], f.X[2]));
    const int yl = imin_(f.Y[0], imin_(f.Y[1], f.Y[2])), yh = imax_(f.Y[0], imax_(f.Y[1], f.Y[2]));
    f.x0 = imax_(mr_floor256(xl + 255), 0);
    f.x1 = imin_(mr_floor256(xh), c.W - 1);
    f.y0 = imax_(mr_floor256(yl + 255), 0);
    f.y1 = imin_(mr_floor256(yh), c.H - 1);
    return MR_OK;
}

// Sample (i, j) = row, column.  false: not covered.  Otherwise zpix and the perspective-correct weights.
__device__ __forceinline__ bool mr_sample(const MrFace& f, int i, int j, float& zpix, float (&w)[3]) {
    const long long PX = (long long)j * 256, PY = (long long)i * 256;
    const float px = (float)j, py = (float)i, sf = (float)f.s;
    long long E[3];
    float b[3];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, e = (k + 2) % 3;
        const long long dx = (long long)f.s * (f.X[e] - f.X[a]), dy = (long long)f.s * (f.Y[e] - f.Y[a]);
        E[k] = dx * (PY - f.Y[a]) - dy * (PX - f.X[a]);
        const bool owns = dy < 0 || (dy == 0 && dx > 0);  // a left edge, or a top edge (y grows downwards)
        in = in && (E[k] > 0 || (E[k] == 0 && owns));
        const float t = sf * ((f.sx[e] - f.sx[a]) * (py - f.sy[a]) - (f.sy[e] - f.sy[a]) * (px - f.sx[a]));
        b[k] = t > 0.0f ? t : 0.0f;
    }
    if (!in) return false;
    float sum = (b[0] + b[1]) + b[2];
    if (sum == 0.0f) {
#pragma unroll
        for (int k = 0; k < 3; k++) b[k] = (float)E[k];
        sum = (b[0] + b[1]) + b[2];
    }
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) r[k] = (b[k] / sum) / f.z[k];
    const float t = (r[0] + r[1]) + r[2];
    zpix = 1.0f / t;
#pragma unroll
    for (int k = 0; k < 3; k++) w[k] = r[k] / t;
    return true;
}

__device__ __forceinline__ void mr_put(unsigned long long* __restrict__ keys, size_t pix, float zpix, uint32_t face) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(zpix) << 32) | face;
    unsigned long long* cell = keys + pix;
    // the cell only ever decreases: a value read here is an upper bound of the final one, so skipping is safe
    if (key < *(volatile unsigned long long*)cell) atomicMin(cell, key);
}

__device__ __forceinline__ long long mr_box_samples(const MrFace& f) {
    if (f.x0 > f.x1 || f.y0 > f.y1) return 0;
    return (long long)(f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1);
}

// a box of at most MR_SMALL_BOX samples, by one thread
__device__ __forceinline__ void mr_walk(const MrFace& f, int W, unsigned long long* __restrict__ keys, uint32_t face) {
    for (int i = f.y0; i <= f.y1; i++) {
        for (int j = f.x0; j <= f.x1; j++) {
            float zpix, w[3];
            if (mr_sample(f, i, j, zpix, w)) mr_put(keys, (size_t)i * W + j, zpix, face);
        }
    }
}

// chunks `slice`, slice + MR_LARGE_SLICES, ... of a listed face's box, 64 samples per step, by one wave
__device__ __forceinline__ void mr_walk_wave(const MrFace& f, int W, unsigned long long* __restrict__ keys, uint32_t face,
                                             int slice) {
    const uint32_t n = (uint32_t)mr_box_samples(f);  // the box lies inside an image of fewer than 2^31 pixels
    const uint32_t bw = (uint32_t)(f.x1 - f.x0 + 1);
    for (uint32_t c = (uint32_t)slice; c * 64u < n; c += MR_LARGE_SLICES) {
        const uint32_t s = c * 64u + (uint32_t)lane_id();
        if (s >= n) continue;
        const uint32_t row = s / bw;
        const int i = f.y0 + (int)row, j = f.x0 + (int)(s - row * bw);
        float zpix, w[3];
        if (mr_sample(f, i, j, zpix, w)) mr_put(keys, (size_t)i * W + j, zpix, face);
    }
}

// Appends `item` of the lanes with `large` set to list[*count ...]: one atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void mr_append(bool large, uint32_t item, uint32_t* __restrict__ count, uint32_t* __restrict__ list,
                                          uint32_t capacity) {
    const unsigned long long mask = __ballot(large);
    if (mask == 0ull) return;  // wave-uniform
    const int leader = __builtin_ctzll(mask);
    uint32_t base = 0;
    if (lane_id() == leader) base = atomicAdd(count, (uint32_t)__builtin_popcountll(mask));
    base = (uint32_t)__shfl((int)base, leader);
    const uint32_t at = base + (uint32_t)__builtin_popcountll(mask & lanes_below_mask());
    if (large && at < capacity) list[at] = item;
}

// ---------------------------------------------------------------------------------------------------------------------
// a mesh from a camera

struct MrMeshArgs {
    static constexpr bool HAS_WV = true;
    float wv[16], pm[16], centre[3], background[MR_MAX_CHANNELS];
    float off, znear;
    int W, H, V, F, C, flags;
    const float* vertices;
    const int* faces;
    const float* attributes;
    unsigned long long* keys;
    uint32_t* count;
    uint32_t* list;
    int* stats;
    int* pix_to_face;
    float* zbuf;
    float* bary;
    float* attr_out;
    float* normal;
    unsigned char* seen;
};

// The face's indices and positions; false (and nothing read through an index) for an index outside [0, V).
__device__ __forceinline__ bool mr_mesh_face(const MrMeshArgs& a, uint32_t face, int (&idx)[3], float (&p)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) idx[k] = a.faces[3 * (size_t)face + k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (idx[k] < 0 || idx[k] >= a.V) return false;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int c = 0; c < 3; c++) p[k][c] = a.vertices[3 * (size_t)idx[k] + c];
    }
    return true;
}

__global__ void __launch_bounds__(256) mr_mesh_raster_kernel(MrMeshArgs a) {
    const uint32_t face = blockIdx.x * 256u + threadIdx.x;
    bool large = false;
    if (face < (uint32_t)a.F) {
        int idx[3];
        float p[3][3];
        if (mr_mesh_face(a, face, idx, p)) {
            MrFace f;
            const int st = mr_setup(a, p, f);
            if (a.stats != nullptr && st == MR_BEHIND) atomicAdd(a.stats + 0, 1);
            if (a.stats != nullptr && st == MR_GUARD_BAND) atomicAdd(a.stats + 1, 1);
            if (st == MR_OK) {
                const long long n = mr_box_samples(f);
                if (n > MR_SMALL_BOX) large = true;
                else if (n > 0) mr_walk(f, a.W, a.keys, face);
            }
        }
    }
    mr_append(large, face, a.count, a.list, (uint32_t)a.F);
}

__global__ void __launch_bounds__(256) mr_mesh_large_kernel(MrMeshArgs a) {
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, n_waves = gridDim.x * 4u;
    const uint32_t count = min(*a.count, (uint32_t)a.F);
    for (uint32_t e = wave; e < count; e += n_waves) {  // wave-uniform
        const uint32_t face = a.list[e];
        int idx[3];
        float p[3][3];
        if (face >= (uint32_t)a.F || !mr_mesh_face(a, face, idx, p)) continue;
        MrFace f;
        if (mr_setup(a, p, f) != MR_OK) continue;
        mr_walk_wave(f, a.W, a.keys, face, (int)blockIdx.y);
    }
}

__global__ void __launch_bounds__(256) mr_mesh_resolve_kernel(MrMeshArgs a) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (size_t)a.W * a.H) return;
    const unsigned long long key = a.keys[pix];
    const uint32_t face = (uint32_t)key;
    int idx[3];
    float p[3][3], w[3] = {0.0f, 0.0f, 0.0f}, zpix = 0.0f;
    bool won = key != MR_EMPTY && face < (uint32_t)a.F && mr_mesh_face(a, face, idx, p);
    if (won) {
        MrFace f;
        won = mr_setup(a, p, f) == MR_OK;
        const uint32_t row = (uint32_t)pix / (uint32_t)a.W;  // W H < 2^31
        if (won) mr_sample(f, (int)row, (int)((uint32_t)pix - row * (uint32_t)a.W), zpix, w);
    }
    if (a.pix_to_face != nullptr) a.pix_to_face[pix] = won ? (int)face : -1;
    if (a.zbuf != nullptr) a.zbuf[pix] = won ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
    if (a.bary != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.bary[3 * pix + k] = won ? w[k] : 0.0f;
    }
    if (a.attr_out != nullptr) {
        for (int c = 0; c < a.C; c++) {
            float v = 0.0f;
#pragma unroll  // constant indices into the argument block: a run-time one would copy the block to scratch
            for (int k = 0; k < MR_MAX_CHANNELS; k++) v = k == c ? a.background[k] : v;
            if (won) {
                const float a0 = a.attributes[(size_t)idx[0] * a.C + c], a1 = a.attributes[(size_t)idx[1] * a.C + c],
                            a2 = a.attributes[(size_t)idx[2] * a.C + c];
                v = (w[0] * a0 + w[1] * a1) + w[2] * a2;
            }
            a.attr_out[pix * a.C + c] = v;
        }
    }
    if (a.normal != nullptr) {
        float n[3] = {0.0f, 0.0f, 0.0f};
        if (won) {
            const float u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const float v[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            float g[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
            const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
            if (len > 0.0f) {
#pragma unroll
                for (int c = 0; c < 3; c++) g[c] = g[c] / len;
                if (a.flags & G4S_MESH_RASTER_FLIP_NORMALS) {
                    float d[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) d[c] = a.centre[c] - ((p[0][c] + p[1][c]) + p[2][c]) / 3.0f;
                    if ((d[0] * g[0] + d[1] * g[1]) + d[2] * g[2] < 0.0f) {
#pragma unroll
                        for (int c = 0; c < 3; c++) g[c] = -g[c];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; c++) n[c] = (g[0] * a.wv[c] + g[1] * a.wv[4 + c]) + g[2] * a.wv[8 + c];
                if (a.flags & G4S_MESH_RASTER_SURFELS_CONVENTION) {
                    n[0] = -n[0];
                    n[1] = -n[1];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) a.normal[3 * pix + c] = n[c];
    }
    if (a.seen != nullptr && won) a.seen[face] = 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// dilated depth

// One view of the stack as the kernels read it (the table is an array of these in the workspace).
struct DilateView {
    float pm[16];
    ViewMaps maps;
    float* depth_out;  // [H,W]
    float* rgb_out;    // [3,H,W] or NULL
    long long first;   // the view's first pixel in the stack's vertex and key ranges
};

struct DilateArgs {
    const DilateView* views;
    int n_views;
    float dilation_pixels, max_dilation, znear;
    float* verts;  // [total,3]: the dilated view-space vertices, NaN for an invalid depth
    unsigned long long* keys;  // [total]
    uint32_t* count;
    uint32_t* list;  // global face ids 2 * (first + a) + kind
    uint32_t capacity;
};

__device__ __forceinline__ bool dl_valid(float d) { return d > 0.0f && d < MR_INF; }

// the view-space point of pixel (i, j); false for an invalid depth
__device__ __forceinline__ bool dl_point(const DilateView& v, int i, int j, float (&p)[3]) {
    const int W = v.maps.W, H = v.maps.H;
    const float d = v.maps.depth[(size_t)i * W + j];
    const float nx = (2.0f * (float)j) / (float)W - 1.0f, ny = (2.0f * (float)i) / (float)H - 1.0f;
    p[0] = ((nx - v.pm[8]) * d) / v.pm[0];
    p[1] = ((ny - v.pm[9]) * d) / v.pm[5];
    p[2] = d;
    return dl_valid(d);
}

// n += cross(p_b - p_a, p_c - p_a) of the face (a, b, c) given as (row, column) pairs, unless a vertex is invalid
__device__ __forceinline__ void dl_add_face(const DilateView& v, int ia, int ja, int ib, int jb, int ic, int jc, float (&n)[3]) {
    float a[3], b[3], c[3];
    const bool ok_a = dl_point(v, ia, ja, a), ok_b = dl_point(v, ib, jb, b), ok_c = dl_point(v, ic, jc, c);
    if (!(ok_a && ok_b && ok_c)) return;
    const float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    n[0] = n[0] + (u[1] * w[2] - u[2] * w[1]);
    n[1] = n[1] + (u[2] * w[0] - u[0] * w[2]);
    n[2] = n[2] + (u[0] * w[1] - u[1] * w[0]);
}

__global__ void __launch_bounds__(256) dl_vertex_kernel(DilateArgs a) {
    const DilateView& v = a.views[blockIdx.y];
    const int W = v.maps.W, H = v.maps.H;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)W * H) return;
    const int i = (int)(pix / W), j = (int)(pix % W);
    float* out = a.verts + 3 * (size_t)(v.first + pix);
    float p[3];
    if (!dl_point(v, i, j, p)) {
        out[0] = out[1] = out[2] = __int_as_float(0x7FC00000);
        return;
    }
    const bool up = i >= 1, down = i < H - 1, left = j >= 1, right = j < W - 1;
    float n[3] = {0.0f, 0.0f, 0.0f};
    // the incident faces in ascending face index: first kind (a, a+W, a+1) of the cells (i-1,j), (i,j-1), (i,j), then
    // second kind (a+W+1, a+1, a+W) of the cells (i-1,j-1), (i-1,j), (i,j-1)
    if (up && right) dl_add_face(v, i - 1, j, i, j, i - 1, j + 1, n);
    if (down && left) dl_add_face(v, i, j - 1, i + 1, j - 1, i, j, n);
    if (down && right) dl_add_face(v, i, j, i + 1, j, i, j + 1, n);
    if (up && left) dl_add_face(v, i, j, i - 1, j, i, j - 1, n);
    if (up && right) dl_add_face(v, i, j + 1, i - 1, j + 1, i, j, n);
    if (down && left) dl_add_face(v, i + 1, j, i, j, i + 1, j - 1, n);
    const float len = fmaxf(sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]), 1e-6f);
    const float focal = ((v.pm[0] * (float)W) / 2.0f + (v.pm[5] * (float)H) / 2.0f) / 2.0f;
    const float delta = fminf((a.dilation_pixels / focal) * p[2], a.max_dilation);
#pragma unroll
    for (int c = 0; c < 3; c++) out[c] = p[c] + delta * (n[c] / len);
}

__device__ __forceinline__ MrViewSpace dl_proj(const DilateArgs& a, const DilateView& v) {
    return MrViewSpace{nullptr, v.pm, 0.0f, a.znear, v.maps.W, v.maps.H};
}

// The face `kind` of the cell whose corner is pixel (i, j), i < H - 1 and j < W - 1: its reference index and the pixels
// (as offsets in the view) of its three vertices.
__device__ __forceinline__ uint32_t dl_face(int W, int H, int i, int j, int kind, long long (&vert)[3]) {
    const long long a = (long long)i * W + j;
    if (kind == 0) {
        vert[0] = a, vert[1] = a + W, vert[2] = a + 1;
    } else {
        vert[0] = a + W + 1, vert[1] = a + 1, vert[2] = a + W;
    }
    const uint32_t cell = (uint32_t)i * (uint32_t)(W - 1) + (uint32_t)j;
    return kind == 0 ? cell : (uint32_t)(H - 1) * (uint32_t)(W - 1) + cell;
}

__device__ __forceinline__ int dl_setup(const DilateArgs& a, const DilateView& v, const long long (&vert)[3], MrFace& f) {
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int c = 0; c < 3; c++) p[k][c] = a.verts[3 * (size_t)(v.first + vert[k]) + c];
    }
    return mr_setup(dl_proj(a, v), p, f);
}

__global__ void __launch_bounds__(256) dl_raster_kernel(DilateArgs a) {
    const DilateView& v = a.views[blockIdx.y];
    const int W = v.maps.W, H = v.maps.H;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = pix < (long long)W * H;
    const int i = live ? (int)(pix / W) : 0, j = live ? (int)(pix % W) : 0;
    const bool cell = live && i < H - 1 && j < W - 1;
    for (int kind = 0; kind < 2; kind++) {
        bool large = false;
        if (cell) {
            long long vert[3];
            const uint32_t face = dl_face(W, H, i, j, kind, vert);
            MrFace f;
            if (dl_setup(a, v, vert, f) == MR_OK) {
                const long long n = mr_box_samples(f);
                if (n > MR_SMALL_BOX) large = true;
                else if (n > 0) mr_walk(f, W, a.keys + v.first, face);
            }
        }
        mr_append(large, (uint32_t)(2 * (v.first + pix) + kind), a.count, a.list, a.capacity);
    }
}

__global__ void __launch_bounds__(256) dl_large_kernel(DilateArgs a) {
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, n_waves = gridDim.x * 4u;
    const uint32_t count = min(*a.count, a.capacity);
    for (uint32_t e = wave; e < count; e += n_waves) {  // wave-uniform
        const uint32_t g = a.list[e];
        const long long gp = (long long)(g >> 1);
        int lo = 0, hi = a.n_views - 1;  // the last view that starts at or before gp
        while (lo < hi) {
            const int mid = lo + ((hi - lo + 1) >> 1);
            if (a.views[mid].first <= gp) lo = mid;
            else hi = mid - 1;
        }
        const DilateView& v = a.views[lo];
        const int W = v.maps.W, H = v.maps.H;
        const long long pix = gp - v.first;
        if (pix < 0 || pix >= (long long)W * H) continue;
        const int i = (int)(pix / W), j = (int)(pix % W);
        if (i >= H - 1 || j >= W - 1) continue;
        long long vert[3];
        const uint32_t face = dl_face(W, H, i, j, (int)(g & 1u), vert);
        MrFace f;
        if (dl_setup(a, v, vert, f) != MR_OK) continue;
        mr_walk_wave(f, W, a.keys + v.first, face, (int)blockIdx.y);
    }
}

__device__ __forceinline__ float dl_clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

__global__ void __launch_bounds__(256) dl_resolve_kernel(DilateArgs a) {
    const DilateView& v = a.views[blockIdx.y];
    const int W = v.maps.W, H = v.maps.H;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const size_t plane = (size_t)W * H;
    if (pix >= (long long)plane) return;
    const unsigned long long key = a.keys[v.first + pix];
    const uint32_t face = (uint32_t)key, cells = (uint32_t)(H - 1) * (uint32_t)(W - 1);
    bool won = key != MR_EMPTY && face < 2u * cells;
    float w[3] = {0.0f, 0.0f, 0.0f}, zpix = 0.0f;
    long long vert[3] = {0, 0, 0};
    if (won) {
        const int kind = face >= cells ? 1 : 0;
        const uint32_t cell = face - (kind ? cells : 0u);
        dl_face(W, H, (int)(cell / (uint32_t)(W - 1)), (int)(cell % (uint32_t)(W - 1)), kind, vert);
        MrFace f;
        won = dl_setup(a, v, vert, f) == MR_OK;
        if (won) mr_sample(f, (int)(pix / W), (int)(pix % W), zpix, w);
    }
    v.depth_out[pix] = won ? __uint_as_float((uint32_t)(key >> 32)) : v.maps.depth[pix];
    if (v.rgb_out != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float* ch = v.maps.rgb + c * plane;
            float out = ch[pix];
            if (won) out = (w[0] * dl_clamp01(ch[vert[0]]) + w[1] * dl_clamp01(ch[vert[1]])) + w[2] * dl_clamp01(ch[vert[2]]);
            v.rgb_out[c * plane + pix] = out;
        }
    }
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

struct MeshRasterLayout {
    size_t keys, count, list, bytes;
};

MeshRasterLayout mesh_raster_layout(long long n_faces, long long pixels) {
    MeshRasterLayout L{};
    WorkspaceCursor c;
    L.keys = c.take((size_t)(pixels > 0 ? pixels : 1) * 8);
    L.count = c.take(256);
    L.list = c.take((size_t)(n_faces > 0 ? n_faces : 1) * 4);
    L.bytes = c.off;
    return L;
}

bool raster_size_ok(int n_faces, int width, int height) {
    return n_faces >= 0 && width > 0 && height > 0 && (long long)width * height < (1ll << 31);
}

struct DilateLayout {
    size_t verts, keys, count, list, bytes;
};

DilateLayout dilate_layout(int n_views, long long total) {
    DilateLayout L{};
    const size_t t = (size_t)(total > 0 ? total : 1);
    WorkspaceCursor c;
    take_view_table<DilateView>(c, n_views);
    L.verts = c.take(t * 12);
    L.keys = c.take(t * 8);
    L.count = c.take(256);
    L.list = c.take(t * 8);  // two faces per pixel, four bytes each
    L.bytes = c.off;
    return L;
}

// Some output map of the stack shares bytes with an input map or with another output map: every map as an address range,
// sorted by its start, one sweep.  (The resolve of a pixel reads rgb at other pixels while other threads write rgb_out.)
bool outputs_overlap(int n_views, const int* sizes, const float* const* depth, const float* const* rgb,
                     float* const* depth_out, float* const* rgb_out) {
    struct Range {
        uintptr_t lo, hi;
        bool output;
    };
    std::vector<Range> r;
    for (int v = 0; v < n_views; v++) {
        const size_t plane = (size_t)sizes[2 * v] * sizes[2 * v + 1] * sizeof(float);
        r.push_back({(uintptr_t)depth[v], (uintptr_t)depth[v] + plane, false});
        r.push_back({(uintptr_t)depth_out[v], (uintptr_t)depth_out[v] + plane, true});
        if (rgb) r.push_back({(uintptr_t)rgb[v], (uintptr_t)rgb[v] + 3 * plane, false});
        if (rgb_out) r.push_back({(uintptr_t)rgb_out[v], (uintptr_t)rgb_out[v] + 3 * plane, true});
    }
    std::sort(r.begin(), r.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    uintptr_t in_hi = 0, out_hi = 0;  // the furthest end of the inputs and of the outputs seen so far
    for (const Range& x : r) {
        if (x.lo < out_hi || (x.output && x.lo < in_hi)) return true;
        if (x.output) out_hi = x.hi > out_hi ? x.hi : out_hi;
        else in_hi = x.hi > in_hi ? x.hi : in_hi;
    }
    return false;
}

unsigned large_blocks(long long faces) {
    const long long b = (faces + 3) / 4;
    return (unsigned)(b < MR_LARGE_BLOCKS ? (b > 0 ? b : 1) : MR_LARGE_BLOCKS);
}

}  // namespace

extern "C" size_t g4s_mesh_raster_workspace(int n_faces, int width, int height) {
    if (!raster_size_ok(n_faces, width, height)) return 0;
    return mesh_raster_layout(n_faces, (long long)width * height).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_mesh_raster(int n_vertices, const float* vertices, int n_faces, const int* faces, const float* world_view,
                               const float* projection, const float* camera_center, int width, int height, float pixel_offset,
                               float znear, int n_channels, const float* attributes, const float* background, int flags,
                               int* pix_to_face, float* zbuf, float* bary, float* attr_out, float* normal,
                               unsigned char* seen, int* stats, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_vertices < 0 || n_faces < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_vertices, n_faces must not be negative");
    if (width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive");
    if ((long long)width * height >= (1ll << 31)) return fail(G4S_ERR_INVALID_ARGUMENT, "width * height must be below 2^31");
    if (!(pixel_offset == 0.0f || pixel_offset == 0.5f)) return fail(G4S_ERR_INVALID_ARGUMENT, "pixel_offset must be 0 or 0.5");
    if (!finite_pos(znear)) return fail(G4S_ERR_INVALID_ARGUMENT, "znear must be positive");
    if (n_channels < 0 || n_channels > MR_MAX_CHANNELS)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_channels must be in 0 .. %d", MR_MAX_CHANNELS);
    if (flags & ~(G4S_MESH_RASTER_FLIP_NORMALS | G4S_MESH_RASTER_SURFELS_CONVENTION))
        return fail(G4S_ERR_INVALID_ARGUMENT, "unknown flag");
    if (!pix_to_face && !zbuf && !bary && !attr_out && !normal && !seen)
        return fail(G4S_ERR_INVALID_ARGUMENT, "no output: one of pix_to_face, zbuf, bary, attr_out, normal, seen is required");
    if (!world_view || !projection || (n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return null_pointer();
    if (attr_out && (n_channels == 0 || !attributes || !background))
        return fail(G4S_ERR_INVALID_ARGUMENT, "attr_out needs n_channels > 0, attributes and background");
    if (normal && (flags & G4S_MESH_RASTER_FLIP_NORMALS) && !camera_center)
        return fail(G4S_ERR_INVALID_ARGUMENT, "flipped normals need camera_center");
    if (check_workspace(workspace, workspace_bytes, g4s_mesh_raster_workspace(n_faces, width, height)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const long long pixels = (long long)width * height;
    const MeshRasterLayout L = mesh_raster_layout(n_faces, pixels);
    MrMeshArgs a{};
    for (int i = 0; i < 16; i++) {
        a.wv[i] = world_view[i];
        a.pm[i] = projection[i];
    }
    for (int i = 0; i < 3; i++) a.centre[i] = camera_center ? camera_center[i] : 0.0f;
    for (int i = 0; i < n_channels; i++) a.background[i] = background ? background[i] : 0.0f;
    a.off = pixel_offset, a.znear = znear;
    a.W = width, a.H = height, a.V = n_vertices, a.F = n_faces, a.C = n_channels, a.flags = flags;
    a.vertices = vertices, a.faces = faces, a.attributes = attributes;
    a.keys = workspace_at<unsigned long long>(workspace, L.keys);
    a.count = workspace_at<uint32_t>(workspace, L.count);
    a.list = workspace_at<uint32_t>(workspace, L.list);
    a.stats = stats, a.pix_to_face = pix_to_face, a.zbuf = zbuf, a.bary = bary, a.attr_out = attr_out, a.normal = normal;
    a.seen = seen;
    hipError_t e = hipMemsetAsync(a.keys, 0xFF, (size_t)pixels * 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.count, 0, 4, stream);
    if (e == hipSuccess && stats) e = hipMemsetAsync(stats, 0, 8, stream);
    if (e != hipSuccess) return finish(e, "mesh raster");
    if (n_faces > 0) {
        hipLaunchKernelGGL(mr_mesh_raster_kernel, dim3(blocks256(n_faces)), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(mr_mesh_large_kernel, dim3(large_blocks(n_faces), MR_LARGE_SLICES), dim3(256), 0, stream, a);
    }
    hipLaunchKernelGGL(mr_mesh_resolve_kernel, dim3(blocks256(pixels)), dim3(256), 0, stream, a);
    return finish(hipSuccess, "mesh raster");
}

extern "C" size_t g4s_depth_dilate_workspace(int n_views, const int* sizes) {
    long long largest, total;
    if (!grid_views_ok(n_views) || !view_sizes_ok(n_views, sizes, &largest, &total) || total >= (1ll << 31)) return 0;
    return dilate_layout(n_views, total).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_depth_dilate(int n_views, const float* projection, const int* sizes, const float* const* depth,
                                const float* const* rgb, float dilation_pixels, float max_dilation, float znear,
                                float* const* depth_out, float* const* rgb_out, char* workspace, size_t workspace_bytes,
                                void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (total >= (1ll << 31)) return fail(G4S_ERR_INVALID_ARGUMENT, "the views must have fewer than 2^31 pixels together");
    if (!(dilation_pixels >= 0.0f) || !finite(dilation_pixels)) return fail(G4S_ERR_INVALID_ARGUMENT, "dilation_pixels must be finite and not negative");
    if (!(max_dilation >= 0.0f)) return fail(G4S_ERR_INVALID_ARGUMENT, "max_dilation must not be negative");
    if (!finite_pos(znear)) return fail(G4S_ERR_INVALID_ARGUMENT, "znear must be positive");
    if (n_views == 0) return G4S_OK;
    if (!projection || !depth || !depth_out) return null_pointer();
    if ((rgb == nullptr) != (rgb_out == nullptr)) return fail(G4S_ERR_INVALID_ARGUMENT, "rgb and rgb_out come together");
    if (check_pointers("depth_out", depth_out, n_views) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (rgb_out && check_pointers("rgb_out", rgb_out, n_views) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    for (int v = 0; v < n_views; v++) {
        const float fx = projection[16 * (size_t)v], fy = projection[16 * (size_t)v + 5];
        if (!finite_pos(fx) || !finite_pos(fy))
            return fail(G4S_ERR_INVALID_ARGUMENT, "view %d: projection[0][0] and [1][1] must be positive", v);
    }
    if (check_pointers("depth", depth, n_views) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (rgb && check_pointers("rgb", rgb, n_views) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (outputs_overlap(n_views, sizes, depth, rgb, depth_out, rgb_out))
        return fail(G4S_ERR_INVALID_ARGUMENT, "an output map overlaps an input map or another output map");
    if (check_workspace(workspace, workspace_bytes, g4s_depth_dilate_workspace(n_views, sizes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const DilateLayout L = dilate_layout(n_views, total);
    const DilateView* table;
    long long first = 0;
    const int rc = stage_views("depth dilate", n_views, true, sizes, depth, rgb, rgb != nullptr, workspace, workspace_bytes,
                               stream, &table, [&](DilateView& u, int v) {
                                   for (int i = 0; i < 16; i++) u.pm[i] = projection[16 * (size_t)v + i];
                                   u.depth_out = depth_out[v];
                                   u.rgb_out = rgb_out ? rgb_out[v] : nullptr;
                                   u.first = first;
                                   first += (long long)sizes[2 * v] * sizes[2 * v + 1];
                               });
    if (rc != G4S_OK) return rc;
    DilateArgs a{};
    a.views = table, a.n_views = n_views;
    a.dilation_pixels = dilation_pixels, a.max_dilation = max_dilation, a.znear = znear;
    a.verts = workspace_at<float>(workspace, L.verts);
    a.keys = workspace_at<unsigned long long>(workspace, L.keys);
    a.count = workspace_at<uint32_t>(workspace, L.count);
    a.list = workspace_at<uint32_t>(workspace, L.list);
    a.capacity = (uint32_t)(2 * total);
    hipError_t e = hipMemsetAsync(a.keys, 0xFF, (size_t)total * 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.count, 0, 4, stream);
    if (e != hipSuccess) return finish(e, "depth dilate");
    const dim3 grid(blocks256(largest), (unsigned)n_views);
    hipLaunchKernelGGL(dl_vertex_kernel, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(dl_raster_kernel, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(dl_large_kernel, dim3(large_blocks(2 * total), MR_LARGE_SLICES), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(dl_resolve_kernel, grid, dim3(256), 0, stream, a);
    return finish(hipSuccess, "depth dilate");
}
