// Unbounded mesh extraction (include/g4s_render_maps.h, "Unbounded TSDF and dense marching cubes"; the semantics stated
// there are the contract, tests/unbounded_ref.py restates them in numpy).
//
// Fusion:  one thread per point, the whole view stack in one loop with the running mean (tsdf, w) in registers; the
// lattice is generated in the kernel and written exactly once.  A wave64 owns a 4x4x4 micro-brick of lattice points, so
// its 256 bilinear taps per view fall into a footprint of a few pixels; the view records (matrix, size, map pointers)
// sit in a device table indexed by the loop counter alone, which makes every read of them wave-uniform.  The explicit
// point kernel (vertex colours, probes) runs the same __device__ functions on points read from memory.  The record's
// tail, the bilinear tap, the staging of the table and the point kernel are view_stack.h's, shared with tetra.hip.
// Dense cubes:  one thread per lattice point in storage order (x fastest), 256 consecutive points per workgroup: count
// (owned-edge mask and in-workgroup vertex prefix per point, vertex / triangle totals per workgroup) -> fixed-order
// exclusive scans of the per-workgroup totals (scan.h) -> [host: sizes] -> emit.  No atomics: every output position is a
// scan result, so two runs are bit-identical.
#include <math.h>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "scan.h"
#include "tsdf_mc_table.h"
#include "view_stack.h"

namespace g4s {

// One view of the stack as the kernels read it (88 bytes; the table is an array of these in the workspace).
struct UtsdfView {
    float m[16];  // full_proj_transform, row-major, used as row-vector @ M
    ViewMaps maps;
};
static_assert(sizeof(UtsdfView) == 88, "g4s_utsdf_workspace is stated in records of 88 bytes");

struct UtsdfFrame {      // contracted space -> world
    float cx, cy, cz, radius, voxel_size;
};

struct UtsdfPoint {
    float p[3];          // world position
    float T;             // truncation
    float tsdf, w;
    float col[3];
};

// State of a point before the first view.  contracted: (y0, y1, y2) is a point of the contracted, normalised space;
// otherwise it is the world point itself.
__device__ __forceinline__ void utsdf_init(UtsdfPoint& s, bool contracted, float y0, float y1, float y2, const UtsdfFrame& f) {
    float T = 5.0f * f.voxel_size;
    if (contracted) {
        const float m = sqrtf((y0 * y0 + y1 * y1) + y2 * y2);
        float u0 = y0, u1 = y1, u2 = y2;
        if (!(m < 1.0f)) {
            const float sc = 1.0f / (2.0f - m);
            u0 = sc * (y0 / m);
            u1 = sc * (y1 / m);
            u2 = sc * (y2 / m);
        }
        s.p[0] = u0 * f.radius + f.cx;
        s.p[1] = u1 * f.radius + f.cy;
        s.p[2] = u2 * f.radius + f.cz;
        if (m > 1.0f) T = T * (1.0f / (2.0f - fminf(m, 1.9f)));
    } else {
        s.p[0] = y0;
        s.p[1] = y1;
        s.p[2] = y2;
    }
    s.T = T;
    s.tsdf = 1.0f;
    s.w = 1.0f;
    s.col[0] = s.col[1] = s.col[2] = 0.0f;
}

// The per-view update.  RGB = false leaves the colour alone (the lattice needs only tsdf); tsdf and w are the same.
template <bool RGB>
__device__ __forceinline__ void utsdf_view(UtsdfPoint& s, const UtsdfView& v) {
    const float* M = v.m;
    const float h0 = ((s.p[0] * M[0] + s.p[1] * M[4]) + s.p[2] * M[8]) + M[12];
    const float h1 = ((s.p[0] * M[1] + s.p[1] * M[5]) + s.p[2] * M[9]) + M[13];
    const float z = ((s.p[0] * M[3] + s.p[1] * M[7]) + s.p[2] * M[11]) + M[15];
    const float px = h0 / z, py = h1 / z;
    if (!(px > -1.0f && px < 1.0f && py > -1.0f && py < 1.0f && z > 0.0f)) return;
    const int W = v.maps.W, H = v.maps.H;
    // 0 <= ix <= W-1 follows from -1 < px < 1
    const ViewTap tap(((px + 1.0f) / 2.0f) * (float)(W - 1), ((py + 1.0f) / 2.0f) * (float)(H - 1), W, H);
    const float d = tap.blend(v.maps.depth);
    const float sdf = d - z;
    if (!(sdf > -s.T)) return;
    const float t = fminf(1.0f, fmaxf(-1.0f, sdf / s.T));
    const float w1 = s.w + 1.0f;
    s.tsdf = (s.tsdf * s.w + t) / w1;
    if (RGB) {
        const size_t plane = (size_t)W * H;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float sc = tap.blend(v.maps.rgb + c * plane);
            s.col[c] = (s.col[c] * s.w + sc) / w1;
        }
    }
    s.w = w1;
}

__device__ __forceinline__ float lattice_coord(int i, float R, float h) { return -R + (float)i * h; }

// ---------------------------------------------------------------------------------------------------------------------
// fusion

// grid (ceil(N/16), ceil(N/4), ceil(N/4)), 256 threads: wave w owns the 4x4x4 micro-brick at x = 16 bx + 4 w
__global__ void __launch_bounds__(256) utsdf_grid_kernel(int N, float R, float h, UtsdfFrame f,
                                                         const UtsdfView* __restrict__ views, int n_views,
                                                         float* __restrict__ tsdf) {
    const int l = lane_id(), wv = (int)(threadIdx.x >> 6);
    const int i = (int)blockIdx.x * 16 + wv * 4 + (l & 3), j = (int)blockIdx.y * 4 + ((l >> 2) & 3),
              k = (int)blockIdx.z * 4 + (l >> 4);
    if (i >= N || j >= N || k >= N) return;
    UtsdfPoint s;
    utsdf_init(s, true, lattice_coord(i, R, h), lattice_coord(j, R, h), lattice_coord(k, R, h), f);
    for (int v = 0; v < n_views; v++) utsdf_view<false>(s, views[v]);
    tsdf[(size_t)i + (size_t)N * ((size_t)j + (size_t)N * (size_t)k)] = s.tsdf;
}

// the field as view_stack.h's point kernel takes it
struct UtsdfField {
    using View = UtsdfView;
    using Point = UtsdfPoint;
    struct Params { UtsdfFrame f; int contracted; };
    static __device__ __forceinline__ void init(Point& s, float y0, float y1, float y2, const Params& a) {
        utsdf_init(s, a.contracted != 0, y0, y1, y2, a.f);
    }
    template <bool RGB>
    static __device__ __forceinline__ void view(Point& s, const View& v, const Params&) { utsdf_view<RGB>(s, v); }
};

// ---------------------------------------------------------------------------------------------------------------------
// dense marching cubes

constexpr int DMC_GROUP = 256;  // lattice points per workgroup, consecutive in storage order

struct DmcLayout {  // byte offsets into the workspace
    size_t vpre, nv, nt, vbase, tbase, chunks, words, bytes;
    int groups;
};

DmcLayout dmc_layout(int N) {
    DmcLayout L{};
    const size_t total = (size_t)N * N * N;
    L.groups = (int)((total + DMC_GROUP - 1) / DMC_GROUP);
    const size_t g = (size_t)L.groups;
    WorkspaceCursor c;
    L.vpre = c.take(g * DMC_GROUP * 2);  // per point: in-workgroup exclusive vertex prefix << 3 | owned-edge mask (<= 765 << 3 | 7)
    L.nv = c.take(g * 4);
    L.nt = c.take(g * 4);
    L.vbase = c.take(g * 4);
    L.tbase = c.take(g * 4);
    L.chunks = c.take((size_t)scan_chunks((long)g) * 4 + 4);
    L.words = c.take(64);
    L.bytes = c.off;
    return L;
}

struct DmcPoint {
    int i, j, k;
    uint32_t mask;  // bit a: the point owns a vertex on its +a edge
    uint32_t ntri;  // triangles of the cube whose lower corner it is
    uint32_t cfg;
};

// idx < N^3
__device__ __forceinline__ DmcPoint dmc_point(const float* __restrict__ tsdf, int N, size_t idx) {
    DmcPoint p;
    const size_t NN = (size_t)N * N;
    p.k = (int)(idx / NN);
    const size_t r = idx - (size_t)p.k * NN;
    p.j = (int)(r / N);
    p.i = (int)(r - (size_t)p.j * N);
    const bool ix = p.i < N - 1, jy = p.j < N - 1, kz = p.k < N - 1;
    const bool n0 = tsdf[idx] < 0.0f;
    p.mask = 0;
    if (ix && (tsdf[idx + 1] < 0.0f) != n0) p.mask |= 1u;
    if (jy && (tsdf[idx + N] < 0.0f) != n0) p.mask |= 2u;
    if (kz && (tsdf[idx + NN] < 0.0f) != n0) p.mask |= 4u;
    p.cfg = 0;
    p.ntri = 0;
    if (ix && jy && kz) {
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const float fv = tsdf[idx + (size_t)(c & 1) + (size_t)((c >> 1) & 1) * N + (size_t)(c >> 2) * NN];
            p.cfg |= (fv < 0.0f ? 1u : 0u) << c;
        }
        p.ntri = g4s_mc_ntris[p.cfg];
    }
    return p;
}

__global__ void __launch_bounds__(DMC_GROUP) dmc_count_kernel(const float* __restrict__ tsdf, int N, size_t total,
                                                              uint16_t* __restrict__ vpre, uint32_t* __restrict__ nv,
                                                              uint32_t* __restrict__ nt) {
    __shared__ uint32_t sm4[4];
    const size_t idx = (size_t)blockIdx.x * DMC_GROUP + threadIdx.x;
    uint32_t mask = 0, ntri = 0;
    if (idx < total) {
        const DmcPoint p = dmc_point(tsdf, N, idx);
        mask = p.mask;
        ntri = p.ntri;
    }
    uint32_t tv, tt;
    const uint32_t ex = block256_excl_scan_u32((uint32_t)__builtin_popcount(mask), sm4, &tv);
    vpre[idx] = (uint16_t)(ex << 3 | mask);  // the array is padded to whole workgroups
    (void)block256_excl_scan_u32(ntri, sm4, &tt);
    if (threadIdx.x == 0) {
        nv[blockIdx.x] = tv;
        nt[blockIdx.x] = tt;
    }
}

// index of the vertex on the +a edge of lattice point idx
__device__ __forceinline__ uint32_t dmc_vertex_id(const uint16_t* __restrict__ vpre, const uint32_t* __restrict__ vbase,
                                                  size_t idx, int a) {
    const uint32_t w = vpre[idx];
    return vbase[idx / DMC_GROUP] + mc_vertex_rank(w, a);
}

__global__ void __launch_bounds__(DMC_GROUP) dmc_emit_kernel(const float* __restrict__ tsdf, int N, size_t total, float R,
                                                             float h, UtsdfFrame f, float max_range,
                                                             const uint16_t* __restrict__ vpre,
                                                             const uint32_t* __restrict__ vbase,
                                                             const uint32_t* __restrict__ tbase, float* __restrict__ verts,
                                                             int* __restrict__ tris, uint32_t vcap, uint32_t tcap) {
    __shared__ uint32_t sm4[4];
    const size_t idx = (size_t)blockIdx.x * DMC_GROUP + threadIdx.x;
    const size_t NN = (size_t)N * N;
    uint32_t ntri = 0, cfg = 0;
    int i = 0, j = 0, k = 0;
    if (idx < total) {
        const DmcPoint p = dmc_point(tsdf, N, idx);
        ntri = p.ntri;
        cfg = p.cfg;
        i = p.i;
        j = p.j;
        k = p.k;
        uint32_t vi = vbase[blockIdx.x] + ((uint32_t)vpre[idx] >> 3);
        const float f0 = tsdf[idx];
        const float c[3] = {lattice_coord(i, R, h), lattice_coord(j, R, h), lattice_coord(k, R, h)};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!(p.mask >> a & 1u) || vi >= vcap) continue;
            const float f1 = tsdf[idx + (a == 0 ? (size_t)1 : (a == 1 ? (size_t)N : NN))];
            const float e = f0 / (f0 - f1);
            float y[3] = {c[0], c[1], c[2]};
            y[a] = c[a] + e * h;
            UtsdfPoint s;
            utsdf_init(s, true, y[0], y[1], y[2], f);
#pragma unroll
            for (int d = 0; d < 3; d++) verts[3 * (size_t)vi + d] = fminf(fmaxf(s.p[d], -max_range), max_range);
            vi++;
        }
    }
    uint32_t tt;
    uint32_t ti = tbase[blockIdx.x] + block256_excl_scan_u32(ntri, sm4, &tt);
    const signed char* row = g4s_mc_tris[cfg];
    for (uint32_t q = 0; q < 3 * ntri && ti + q / 3 < tcap; q++) {
        const McEdge e = mc_edge(row[q], i, j, k);
        tris[3 * (size_t)ti + q] = (int)dmc_vertex_id(vpre, vbase, (size_t)e.x + (size_t)N * ((size_t)e.y + (size_t)N * (size_t)e.z), e.a);
    }
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

int check_frame(const float* center, float radius, float voxel_size, bool need_frame, UtsdfFrame* f) {
    if (!finite_pos(voxel_size)) return fail(G4S_ERR_INVALID_ARGUMENT, "voxel_size must be positive");
    *f = UtsdfFrame{0.0f, 0.0f, 0.0f, 1.0f, voxel_size};
    if (!need_frame) return G4S_OK;
    if (!center) return null_pointer();
    if (!finite_pos(radius) || !finite(center[0]) || !finite(center[1]) || !finite(center[2]))
        return fail(G4S_ERR_INVALID_ARGUMENT, "radius must be positive and center finite");
    f->cx = center[0];
    f->cy = center[1];
    f->cz = center[2];
    f->radius = radius;
    return G4S_OK;
}

// the view table of this field in the workspace (view_stack.h)
int utsdf_table(int n_views, const float* full_proj, const int* sizes, const float* const* depth, const float* const* rgb,
                bool need_rgb, char* workspace, size_t workspace_bytes, hipStream_t stream, const UtsdfView** table) {
    return stage_views("utsdf", n_views, full_proj != nullptr, sizes, depth, rgb, need_rgb, workspace, workspace_bytes, stream,
                       table, [=](UtsdfView& u, int v) {
                           for (int i = 0; i < 16; i++) u.m[i] = full_proj[16 * (size_t)v + i];
                       });
}

}  // namespace

extern "C" size_t g4s_utsdf_workspace(int n_views) {
    return view_table_bytes<UtsdfView>(n_views);
}

extern "C" int g4s_utsdf_grid(int n, float half_extent, const float* center, float radius, float voxel_size, int n_views,
                              const float* full_proj, const int* sizes, const float* const* depth, float* tsdf,
                              char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_lattice(n) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!finite_pos(half_extent)) return fail(G4S_ERR_INVALID_ARGUMENT, "half_extent must be positive");
    UtsdfFrame f;
    if (check_frame(center, radius, voxel_size, true, &f) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!tsdf) return null_pointer();
    const UtsdfView* table;
    const int rc = utsdf_table(n_views, full_proj, sizes, depth, nullptr, false, workspace, workspace_bytes, stream, &table);
    if (rc != G4S_OK) return rc;
    const float h = (2.0f * half_extent) / (float)(n - 1);
    hipLaunchKernelGGL(utsdf_grid_kernel, dim3((n + 15) / 16, (n + 3) / 4, (n + 3) / 4), dim3(256), 0, stream, n, half_extent, h,
                       f, table, n_views, tsdf);
    return finish(hipSuccess, "utsdf grid");
}

extern "C" int g4s_utsdf_sample(int n_points, const float* points, int contracted, const float* center, float radius,
                                float voxel_size, int n_views, const float* full_proj, const int* sizes,
                                const float* const* depth, const float* const* rgb, float* tsdf, float* colour,
                                char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_points < 0 || n_points > (1 << 30)) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must be in 0 .. 2^30");
    UtsdfFrame f;
    if (check_frame(center, radius, voxel_size, contracted != 0, &f) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_points > 0 && (!points || (!tsdf && !colour))) return null_pointer();
    const UtsdfView* table;
    const int rc = utsdf_table(n_views, full_proj, sizes, depth, rgb, colour != nullptr, workspace, workspace_bytes, stream,
                               &table);
    if (rc != G4S_OK) return rc;
    if (n_points == 0) return G4S_OK;
    launch_point_sample<UtsdfField>(n_points, points, table, n_views, UtsdfField::Params{f, contracted}, tsdf, colour, stream);
    return finish(hipSuccess, "utsdf sample");
}

extern "C" size_t g4s_dense_mc_workspace(int n) { return lattice_ok(n) ? dmc_layout(n).bytes + 256 : 0; }

extern "C" int g4s_dense_mc_count(int n, const float* tsdf, int* totals, char* workspace, size_t workspace_bytes,
                                  void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_lattice(n) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!tsdf || !totals) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_dense_mc_workspace(n)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const DmcLayout L = dmc_layout(n);
    char* ws = align_ptr(workspace);
    uint32_t* nv = (uint32_t*)(ws + L.nv);
    uint32_t* nt = (uint32_t*)(ws + L.nt);
    uint32_t* chunks = (uint32_t*)(ws + L.chunks);
    uint32_t* words = (uint32_t*)(ws + L.words);
    hipLaunchKernelGGL(dmc_count_kernel, dim3(L.groups), dim3(DMC_GROUP), 0, stream, tsdf, n, (size_t)n * n * n,
                       (uint16_t*)(ws + L.vpre), nv, nt);
    scan_u32(nv, (uint32_t*)(ws + L.vbase), L.groups, chunks, words + 0, stream);
    scan_u32(nt, (uint32_t*)(ws + L.tbase), L.groups, chunks, words + 1, stream);
    int t[2];
    const hipError_t e = read_totals(words, t, stream);
    if (e != hipSuccess) return finish(e, "dense_mc count");
    if ((uint32_t)t[0] > 0x7FFFFFFFu / 3 || (uint32_t)t[1] > 0x7FFFFFFFu / 3)
        return fail(G4S_ERR_INVALID_ARGUMENT, "mesh exceeds 2^31 / 3 vertices or triangles");
    totals[0] = t[0];
    totals[1] = t[1];
    return G4S_OK;
}

extern "C" int g4s_dense_mc_emit(int n, const float* tsdf, float half_extent, const float* center, float radius,
                                 float max_range, float* vertices, int* triangles, int n_vertices, int n_triangles,
                                 char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_lattice(n) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_vertices < 0 || n_triangles < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "counts must not be negative");
    if (!finite_pos(half_extent) || !finite_pos(max_range))
        return fail(G4S_ERR_INVALID_ARGUMENT, "half_extent, max_range must be positive");
    UtsdfFrame f;
    if (check_frame(center, radius, 1.0f, true, &f) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!tsdf || (n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles))
        return null_pointer();
    if (n_vertices == 0) return G4S_OK;  // no crossing: nothing to write
    if (check_workspace(workspace, workspace_bytes, g4s_dense_mc_workspace(n)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const DmcLayout L = dmc_layout(n);
    char* ws = align_ptr(workspace);
    const float h = (2.0f * half_extent) / (float)(n - 1);
    hipLaunchKernelGGL(dmc_emit_kernel, dim3(L.groups), dim3(DMC_GROUP), 0, stream, tsdf, n, (size_t)n * n * n, half_extent, h,
                       f, max_range, (const uint16_t*)(ws + L.vpre), (const uint32_t*)(ws + L.vbase),
                       (const uint32_t*)(ws + L.tbase), vertices, triangles, (uint32_t)n_vertices, (uint32_t)n_triangles);
    return finish(hipSuccess, "dense_mc emit");
}
