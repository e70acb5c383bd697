// Tetrahedral mesh extraction (include/g4s_render_maps.h, "Adaptive TSDF at points and marching tetrahedra"; the semantics
// stated there are the contract, tests/tetra_ref.py restates them in numpy).
//
// Point TSDF:  one thread per point, the whole view stack in one loop with the running mean (tsdf, w, colour) in
// registers; the view records (two matrices, size, map pointers) sit in a device table indexed by the loop counter alone,
// which makes every read of them wave-uniform.  The record's tail, the bilinear tap, the staging of the table and the
// point kernel are view_stack.h's, shared with unbounded.hip; the update is the reference's AdaptiveTSDF.
// Bisection:  one thread per crossing edge runs all steps; every step is the same __device__ view loop at the midpoint, so
// one launch stands for the reference's eight render-and-integrate passes over the view stack.
// Marching tetrahedra:  per tet the numbers of crossing edges and triangles -> fixed-order exclusive scans (scan.h) ->
// [host: keys, faces] -> edge keys lo << 32 | hi written at the scanned positions -> radix_sort_u64_keys over the bits
// n_points needs -> unique flags, scan, compaction -> [host: edges]; emit: the unique keys are the vertices, and every tet
// looks its triangles' vertices up in them by binary search.  No atomics: every output position is a scan result, so two
// runs are bit-identical.
#include <math.h>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "scan.h"
#include "tsdf_mtet_table.h"
#include "view_stack.h"

namespace g4s {

// One view of the stack as the kernels read it (152 bytes; the table is an array of these in the workspace).
struct AtsdfView {
    float wv[16];  // world_view_transform, row-major, used as row-vector @ M
    float pm[16];  // projection_matrix, likewise
    ViewMaps maps;
};
static_assert(sizeof(AtsdfView) == 152, "g4s_atsdf_workspace is stated in records of 152 bytes");

struct AtsdfParams {
    float trunc, znear, zfar;
};

struct AtsdfPoint {
    float p[3];
    float tsdf, w;
    float col[3];
};

__device__ __forceinline__ void atsdf_init(AtsdfPoint& s, float x, float y, float z) {
    s.p[0] = x;
    s.p[1] = y;
    s.p[2] = z;
    s.tsdf = -1.0f;  // the reference's quirk: a point no view accepts counts as inside
    s.w = 0.0f;
    s.col[0] = s.col[1] = s.col[2] = 0.0f;
}

// The per-view update.  RGB = false leaves the colour alone; tsdf and w are the same.
template <bool RGB>
__device__ __forceinline__ void atsdf_view(AtsdfPoint& s, const AtsdfView& v, const AtsdfParams& a) {
    const float* M = v.wv;
    const float v0 = ((s.p[0] * M[0] + s.p[1] * M[4]) + s.p[2] * M[8]) + M[12];
    const float v1 = ((s.p[0] * M[1] + s.p[1] * M[5]) + s.p[2] * M[9]) + M[13];
    const float z = ((s.p[0] * M[2] + s.p[1] * M[6]) + s.p[2] * M[10]) + M[14];
    const float* P = v.pm;
    const float q0 = ((v0 * P[0] + v1 * P[4]) + z * P[8]) + P[12];
    const float q1 = ((v0 * P[1] + v1 * P[5]) + z * P[9]) + P[13];
    const float q3 = ((v0 * P[3] + v1 * P[7]) + z * P[11]) + P[15];
    const float qw = q3 > a.znear ? q3 : a.znear;  // clamp_min; a NaN q3 becomes znear, and the view is still rejected: ix, iy or z is NaN then
    const int W = v.maps.W, H = v.maps.H;
    const float ix = ((1.0f + q0 / qw) * (float)W) / 2.0f, iy = ((1.0f + q1 / qw) * (float)H) / 2.0f;
    if (!(ix >= 0.0f && ix <= (float)(W - 1) && iy >= 0.0f && iy <= (float)(H - 1) && z > a.znear && z < a.zfar)) return;
    const ViewTap tap(ix, iy, W, H);
    const float d = tap.blend(v.maps.depth);
    const float diff = d - z;
    if (!(d > 0.0f && diff >= -a.trunc)) return;
    const float dist = fminf(diff / a.trunc, 1.0f);
    const float w1 = s.w + 1.0f;
    s.tsdf = (s.tsdf * s.w + dist) / w1;
    if (RGB) {
        const size_t plane = (size_t)W * H;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float sc = tap.blend(v.maps.rgb + c * plane);
            s.col[c] = fminf(fmaxf((s.col[c] * s.w + sc) / w1, 0.0f), 1.0f);
        }
    }
    s.w = w1;
}

// the tsdf of the whole stack at one point
__device__ __forceinline__ float atsdf_at(float x, float y, float z, const AtsdfView* __restrict__ views, int n_views,
                                          const AtsdfParams& a) {
    AtsdfPoint s;
    atsdf_init(s, x, y, z);
    for (int v = 0; v < n_views; v++) atsdf_view<false>(s, views[v], a);
    return s.tsdf;
}

// the field as view_stack.h's point kernel takes it
struct AtsdfField {
    using View = AtsdfView;
    using Point = AtsdfPoint;
    using Params = AtsdfParams;
    static __device__ __forceinline__ void init(Point& s, float x, float y, float z, const Params&) { atsdf_init(s, x, y, z); }
    template <bool RGB>
    static __device__ __forceinline__ void view(Point& s, const View& v, const Params& a) { atsdf_view<RGB>(s, v, a); }
};

__global__ void __launch_bounds__(256) atsdf_bisect_kernel(int n_edges, const int* __restrict__ edges, int n_points,
                                                           const float* __restrict__ points, const float* __restrict__ sdf,
                                                           const AtsdfView* __restrict__ views, int n_views, AtsdfParams a,
                                                           int steps, float* __restrict__ vertices) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n_edges) return;
    const int lo = edges[2 * (size_t)i], hi = edges[2 * (size_t)i + 1];
    float* out = vertices + 3 * (size_t)i;
    if (lo < 0 || lo >= n_points || hi < 0 || hi >= n_points) {  // never used as an address
        out[0] = out[1] = out[2] = __int_as_float(0x7FC00000);
        return;
    }
    float l[3], r[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        l[c] = points[3 * (size_t)lo + c];
        r[c] = points[3 * (size_t)hi + c];
    }
    float ls = sdf[lo];
    for (int s = 0; s < steps; s++) {
        const float m[3] = {(l[0] + r[0]) / 2.0f, (l[1] + r[1]) / 2.0f, (l[2] + r[2]) / 2.0f};
        const float ms = atsdf_at(m[0], m[1], m[2], views, n_views, a);
        const bool low = (ms < 0.0f && ls < 0.0f) || (ms > 0.0f && ls > 0.0f);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            l[c] = low ? m[c] : l[c];
            r[c] = low ? r[c] : m[c];
        }
        ls = low ? ms : ls;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out[c] = (l[c] + r[c]) / 2.0f;
}

// ---------------------------------------------------------------------------------------------------------------------
// marching tetrahedra

struct MtetLayout {  // byte offsets into the workspace
    size_t ne, nt, eoff, toff, keys_a, keys_b, hist, bin_total, flag, pos, chunks, words, bytes;
};

constexpr int MTET_MAX_TETS = 0x7FFFFFFF / 4;  // four keys per tet at most, 4 T < 2^31

MtetLayout mtet_layout(int T) {
    MtetLayout L{};
    const size_t t = (size_t)(T > 0 ? T : 1), k = 4 * t;
    WorkspaceCursor c;
    L.ne = c.take(t * 4);
    L.nt = c.take(t * 4);
    L.eoff = c.take(t * 4);
    L.toff = c.take(t * 4);
    L.keys_a = c.take(k * 8);
    L.keys_b = c.take(k * 8);
    L.hist = c.take((size_t)256 * (sort_blocks(k, SORT_ITEMS_U64) + 1) * 4);
    L.bin_total = c.take(512 * 4);
    L.flag = c.take(k * 4);
    L.pos = c.take(k * 4);
    L.chunks = c.take((size_t)scan_chunks((long)k) * 4 + 4);
    L.words = c.take(64);  // [0] edge keys, [1] triangles, [2] unique keys
    L.bytes = c.off;
    return L;
}

struct MtetCorners {
    int v[4];
    uint32_t cs;  // case: bit c set iff sdf(corner c) > 0; 0 for a tet that names a point outside [0, n_points)
};

__device__ __forceinline__ MtetCorners mtet_corners(const int* __restrict__ tets, size_t t, const float* __restrict__ sdf,
                                                    int n_points) {
    MtetCorners m;
    const int4 q = *(const int4*)(tets + 4 * t);  // rows of four int32: 16-byte aligned with the array
    m.v[0] = q.x;
    m.v[1] = q.y;
    m.v[2] = q.z;
    m.v[3] = q.w;
    m.cs = 0;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 4; c++) ok = ok && m.v[c] >= 0 && m.v[c] < n_points;
    if (ok) {
#pragma unroll
        for (int c = 0; c < 4; c++) m.cs |= (sdf[m.v[c]] > 0.0f ? 1u : 0u) << c;
    }
    return m;
}

// key of edge e (0..5 = 01, 02, 03, 12, 13, 23) of the tet
__device__ __forceinline__ uint64_t mtet_key(const MtetCorners& m, int e) {
    const int a = e < 3 ? 0 : (e < 5 ? 1 : 2), b = e < 3 ? e + 1 : (e < 5 ? e - 1 : 3);
    const uint32_t p = (uint32_t)m.v[a], q = (uint32_t)m.v[b];
    return p < q ? ((uint64_t)p << 32 | q) : ((uint64_t)q << 32 | p);
}

__global__ void __launch_bounds__(256) mtet_count_kernel(int T, const int* __restrict__ tets, const float* __restrict__ sdf,
                                                         int n_points, uint32_t* __restrict__ ne, uint32_t* __restrict__ nt) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= T) return;
    const MtetCorners m = mtet_corners(tets, (size_t)t, sdf, n_points);
    ne[t] = (uint32_t)__builtin_popcount(g4s_mtet_edges[m.cs]);
    nt[t] = g4s_mtet_ntris[m.cs];
}

__global__ void __launch_bounds__(256) mtet_keys_kernel(int T, const int* __restrict__ tets, const float* __restrict__ sdf,
                                                        int n_points, const uint32_t* __restrict__ eoff,
                                                        uint64_t* __restrict__ keys, uint32_t n_keys) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= T) return;
    const MtetCorners m = mtet_corners(tets, (size_t)t, sdf, n_points);
    const uint32_t mask = g4s_mtet_edges[m.cs];
    uint32_t k = eoff[t];
#pragma unroll
    for (int e = 0; e < 6; e++) {
        if (!(mask >> e & 1u) || k >= n_keys) continue;
        keys[k++] = mtet_key(m, e);
    }
}

__global__ void __launch_bounds__(256) mtet_unique_flags_kernel(const uint64_t* __restrict__ keys, int n,
                                                                uint32_t* __restrict__ flag) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) mtet_compact_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag,
                                                           const uint32_t* __restrict__ pos, int n, uint64_t* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < n && flag[i]) out[pos[i]] = keys[i];
}

__global__ void __launch_bounds__(256) mtet_edges_kernel(const uint64_t* __restrict__ uniq, int n, int* __restrict__ edges) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const uint64_t k = uniq[i];
    *(int2*)(edges + 2 * (size_t)i) = make_int2((int)(uint32_t)(k >> 32), (int)(uint32_t)k);
}

// position of `key` in the ascending uniq[0, n), or -1
__device__ __forceinline__ int mtet_find(const uint64_t* __restrict__ uniq, int n, uint64_t key) {
    int lo = 0, hi = n;  // first position with uniq >= key
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (uniq[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && uniq[lo] == key ? lo : -1;
}

__global__ void __launch_bounds__(256) mtet_faces_kernel(int T, const int* __restrict__ tets, const float* __restrict__ sdf,
                                                         int n_points, const uint32_t* __restrict__ toff,
                                                         const uint64_t* __restrict__ uniq, int n_edges,
                                                         int* __restrict__ faces, uint32_t n_faces) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= T) return;
    const MtetCorners m = mtet_corners(tets, (size_t)t, sdf, n_points);
    const uint32_t ntri = g4s_mtet_ntris[m.cs];
    if (ntri == 0) return;
    const uint32_t f = toff[t];
    const signed char* row = g4s_mtet_tris[m.cs];
    for (uint32_t q = 0; q < 3 * ntri && f + q / 3 < n_faces; q++)
        faces[3 * (size_t)f + q] = mtet_find(uniq, n_edges, mtet_key(m, row[q]));
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

int check_params(float trunc, float znear, float zfar, AtsdfParams* a) {
    if (!finite_pos(trunc)) return fail(G4S_ERR_INVALID_ARGUMENT, "trunc_margin must be positive");
    if (!finite_pos(znear) || !finite_pos(zfar) || !(zfar > znear))
        return fail(G4S_ERR_INVALID_ARGUMENT, "znear must be positive and zfar greater than znear");
    *a = AtsdfParams{trunc, znear, zfar};
    return G4S_OK;
}

// the view table of this field in the workspace (view_stack.h)
int atsdf_table(int n_views, const float* world_view, const float* projection, const int* sizes, const float* const* depth,
                const float* const* rgb, bool need_rgb, char* workspace, size_t workspace_bytes, hipStream_t stream,
                const AtsdfView** table) {
    return stage_views("atsdf", n_views, world_view && projection, sizes, depth, rgb, need_rgb, workspace, workspace_bytes,
                       stream, table, [=](AtsdfView& u, int v) {
                           for (int i = 0; i < 16; i++) {
                               u.wv[i] = world_view[16 * (size_t)v + i];
                               u.pm[i] = projection[16 * (size_t)v + i];
                           }
                       });
}

int check_mtet(int n_points, int n_tets, const int* tets) {
    if (n_points < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must not be negative");
    if (n_tets < 0 || n_tets > MTET_MAX_TETS) return fail(G4S_ERR_INVALID_ARGUMENT, "n_tets must be in 0 .. 2^29 - 1");
    if (((uintptr_t)tets & 15) != 0) return fail(G4S_ERR_INVALID_ARGUMENT, "tets must be 16-byte aligned");  // int4 rows
    return G4S_OK;
}

int key_bits(int n_points) {  // bits of the largest point index
    int b = 1;
    while (b < 31 && ((uint32_t)1 << b) < (uint32_t)n_points) b++;
    return b;
}

}  // namespace

extern "C" size_t g4s_atsdf_workspace(int n_views) {
    return view_table_bytes<AtsdfView>(n_views);
}

extern "C" int g4s_atsdf_sample(int n_points, const float* points, float trunc_margin, float znear, float zfar, int n_views,
                                const float* world_view, const float* projection, const int* sizes,
                                const float* const* depth, const float* const* rgb, float* tsdf, float* colour,
                                char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_points < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must not be negative");
    AtsdfParams a;
    if (check_params(trunc_margin, znear, zfar, &a) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_points > 0 && (!points || (!tsdf && !colour))) return null_pointer();
    const AtsdfView* table;
    const int rc = atsdf_table(n_views, world_view, projection, sizes, depth, rgb, colour != nullptr, workspace,
                               workspace_bytes, stream, &table);
    if (rc != G4S_OK) return rc;
    if (n_points == 0) return G4S_OK;
    launch_point_sample<AtsdfField>(n_points, points, table, n_views, a, tsdf, colour, stream);
    return finish(hipSuccess, "atsdf sample");
}

extern "C" int g4s_atsdf_bisect(int n_edges, const int* edges, int n_points, const float* points, const float* sdf,
                                int steps, float trunc_margin, float znear, float zfar, int n_views, const float* world_view,
                                const float* projection, const int* sizes, const float* const* depth, float* vertices,
                                char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_edges < 0 || n_points < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_edges, n_points must not be negative");
    if (steps < 0 || steps > 64) return fail(G4S_ERR_INVALID_ARGUMENT, "steps must be in 0 .. 64");
    AtsdfParams a;
    if (check_params(trunc_margin, znear, zfar, &a) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_edges > 0 && (!edges || !vertices || (n_points > 0 && (!points || !sdf)))) return null_pointer();
    const AtsdfView* table;
    const int rc = atsdf_table(n_views, world_view, projection, sizes, depth, nullptr, false, workspace, workspace_bytes,
                               stream, &table);
    if (rc != G4S_OK) return rc;
    if (n_edges == 0) return G4S_OK;
    hipLaunchKernelGGL(atsdf_bisect_kernel, dim3(((unsigned)n_edges + 255u) / 256u), dim3(256), 0, stream, n_edges, edges,
                       n_points, points, sdf, table, n_views, a, steps, vertices);
    return finish(hipSuccess, "atsdf bisect");
}

extern "C" size_t g4s_mtet_workspace(int n_tets) {
    return n_tets >= 0 && n_tets <= MTET_MAX_TETS ? mtet_layout(n_tets).bytes + 256 : 0;
}

extern "C" int g4s_mtet_count(int n_points, int n_tets, const int* tets, const float* sdf, int* totals, char* workspace,
                              size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_mtet(n_points, n_tets, tets) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!totals || (n_tets > 0 && (!tets || (n_points > 0 && !sdf)))) return null_pointer();
    totals[0] = totals[1] = 0;
    if (n_tets == 0 || n_points == 0) return G4S_OK;
    if (check_workspace(workspace, workspace_bytes, g4s_mtet_workspace(n_tets)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const MtetLayout L = mtet_layout(n_tets);
    char* ws = align_ptr(workspace);
    uint32_t* ne = (uint32_t*)(ws + L.ne);
    uint32_t* nt = (uint32_t*)(ws + L.nt);
    uint32_t* eoff = (uint32_t*)(ws + L.eoff);
    uint32_t* chunks = (uint32_t*)(ws + L.chunks);
    uint32_t* words = (uint32_t*)(ws + L.words);
    uint64_t* ka = (uint64_t*)(ws + L.keys_a);
    uint64_t* kb = (uint64_t*)(ws + L.keys_b);
    const dim3 tet_grid(((unsigned)n_tets + 255u) / 256u);
    hipLaunchKernelGGL(mtet_count_kernel, tet_grid, dim3(256), 0, stream, n_tets, tets, sdf, n_points, ne, nt);
    scan_u32(ne, eoff, n_tets, chunks, words + 0, stream);
    scan_u32(nt, (uint32_t*)(ws + L.toff), n_tets, chunks, words + 1, stream);
    int kf[2];
    hipError_t e = read_totals(words, kf, stream);  // crossing-edge keys (with repeats), triangles
    if (e != hipSuccess) return finish(e, "mtet count");
    const int K = kf[0], F = kf[1];
    if ((uint32_t)F > 0x7FFFFFFFu / 3) return fail(G4S_ERR_INVALID_ARGUMENT, "mesh exceeds 2^31 / 3 triangles");
    if (K == 0) return G4S_OK;  // no tet crosses
    hipLaunchKernelGGL(mtet_keys_kernel, tet_grid, dim3(256), 0, stream, n_tets, tets, sdf, n_points, eoff, ka, (uint32_t)K);
    // hi field first, then lo: ascending (lo, hi); only the bits a point index can have
    const int bits = key_bits(n_points);
    uint32_t* hist = (uint32_t*)(ws + L.hist);
    uint32_t* bin_total = (uint32_t*)(ws + L.bin_total);
    // Both fields are `bits` wide and take the same number of passes, so the two sorts end where they began: the
    // sorted keys are in ka, and the unique ones are compacted into kb.
    const int half = radix_sort_u64_keys(ka, kb, K, 0, bits, hist, bin_total, stream);
    if (half == 0)
        radix_sort_u64_keys(ka, kb, K, 32, 32 + bits, hist, bin_total, stream);
    else
        radix_sort_u64_keys(kb, ka, K, 32, 32 + bits, hist, bin_total, stream);
    const uint64_t* sorted = ka;
    uint64_t* uniq = kb;
    uint32_t* flag = (uint32_t*)(ws + L.flag);
    uint32_t* pos = (uint32_t*)(ws + L.pos);
    const dim3 key_grid(((unsigned)K + 255u) / 256u);
    hipLaunchKernelGGL(mtet_unique_flags_kernel, key_grid, dim3(256), 0, stream, sorted, K, flag);
    scan_u32(flag, pos, K, chunks, words + 2, stream);
    hipLaunchKernelGGL(mtet_compact_kernel, key_grid, dim3(256), 0, stream, sorted, flag, pos, K, uniq);
    int fe[2];
    e = read_totals(words + 1, fe, stream);  // triangles again, unique keys
    if (e != hipSuccess) return finish(e, "mtet count");
    const int E = fe[1];
    if ((uint32_t)E > 0x7FFFFFFFu / 3) return fail(G4S_ERR_INVALID_ARGUMENT, "mesh exceeds 2^31 / 3 vertices");
    // g4s_mtet_emit finds the unique keys at the head of the first key buffer
    e = hipMemcpyAsync(ka, uniq, (size_t)E * 8, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return finish(e, "mtet count");
    totals[0] = E;
    totals[1] = F;
    return finish(hipSuccess, "mtet count");
}

extern "C" int g4s_mtet_emit(int n_points, int n_tets, const int* tets, const float* sdf, int* edges, int* faces,
                             int n_edges, int n_faces, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_mtet(n_points, n_tets, tets) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_edges < 0 || n_faces < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "counts must not be negative");
    if ((n_edges > 0 && (!edges || !tets || !sdf)) || (n_faces > 0 && !faces)) return null_pointer();
    if (n_edges == 0) return G4S_OK;  // no crossing: nothing to write
    if ((long long)n_edges > 4ll * n_tets) return fail(G4S_ERR_INVALID_ARGUMENT, "n_edges exceeds four per tet");
    if (check_workspace(workspace, workspace_bytes, g4s_mtet_workspace(n_tets)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const MtetLayout L = mtet_layout(n_tets);
    char* ws = align_ptr(workspace);
    const uint64_t* uniq = (const uint64_t*)(ws + L.keys_a);
    hipLaunchKernelGGL(mtet_edges_kernel, dim3(((unsigned)n_edges + 255u) / 256u), dim3(256), 0, stream, uniq, n_edges, edges);
    if (n_faces > 0)
        hipLaunchKernelGGL(mtet_faces_kernel, dim3(((unsigned)n_tets + 255u) / 256u), dim3(256), 0, stream, n_tets, tets, sdf,
                           n_points, (const uint32_t*)(ws + L.toff), uniq, n_edges, faces, (uint32_t)n_faces);
    return finish(hipSuccess, "mtet emit");
}
