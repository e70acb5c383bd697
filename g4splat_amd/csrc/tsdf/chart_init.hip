// Gaussian initialisation from depth charts (include/g4s_render_maps.h, "Chart surfels"; the semantics stated there are
// the contract, tests/chart_init_ref.py restates them in numpy): the triangulated pixel grid of every view, the elongated-
// face test, and one surfel per surviving face, in the reference's face order.
//
// Shape.  All views have one size.  A view has C = (H-1)(W-1) cells, G = ceil(C / 256) workgroups; one thread owns a cell
// and both of its faces.  The output order is segmented by (view, half): all face_1 of view 0, all face_2 of view 0, view 1,
// ...  So the per-workgroup counts are laid out segment-major, counts[(2 v + half) G + g], and ONE scan_u32 over the 2 V G
// counts gives every (view, half, workgroup) its first output row; its total is the number of faces.
//   [mask_any: is the mask true anywhere]  ->  count: keep bits -> __ballot -> one 64-bit word per (segment, workgroup,
//   wave) and the popcounts per (segment, workgroup)  ->  scan_u32  ->  [host: n_faces]  ->  emit: re-reads the ballot
//   words, row = segment/workgroup base + the waves before + the kept lanes below, and writes the surfel.
// The emit kernel re-READS the keep bits (16 bytes per wave) instead of re-deriving them: the rows cannot disagree with
// the count whatever the compiler does to the two instantiations.  Lanes of consecutive rank write consecutive rows.
// Vertices: the four corners of a cell are read straight from global memory.  Lanes of a wave read consecutive addresses of
// rows r and r + 1; the second row comes again for the cells below it, from L2 or the vector cache.  There is no LDS tile:
// a workgroup's 256 cells are a run of the row-major cell order, mostly one or two rows of a 1-cell-high strip, so a tile
// would stage 2 x 257 vertices to save one of the two row reads at best.  (Not measured against a staged version.)
// No atomics; every output is a function of the inputs alone.
#include "../../../include/g4s_render_maps.h"
#include "scan.h"
#include "vis_view.h"

namespace g4s {

struct ChartView {
    VisRay ray;                 // depth form only
    const unsigned char* mask;  // [H,W] or NULL
    ViewMaps maps;              // depth = the point map [H,W,3] or the depth map [H,W]; rgb = the image [H,W,3]
};

struct ChartLayout {
    size_t table, ballots, counts, offs, chunks, words, bytes;
    long long cells, groups, entries;  // per view, per view, 2 V G
};

static ChartLayout chart_layout(long long V, long long H, long long W) {
    ChartLayout L{};
    L.cells = (H - 1) * (W - 1);
    L.groups = blocks256(L.cells);
    L.entries = 2 * V * L.groups;
    const size_t e = L.entries > 0 ? (size_t)L.entries : 1;
    WorkspaceCursor c;
    L.table = c.take((size_t)(V > 0 ? V : 1) * sizeof(ChartView));
    L.ballots = c.take(e * 4 * 8);
    L.counts = c.take(e * 4);
    L.offs = c.take(e * 4);
    L.chunks = c.take((size_t)scan_chunks((long)e) * 4 + 4);
    L.words = c.take(64);  // [0] faces, [1] unused, [2] mask-any flag
    L.bytes = c.off;
    return L;
}

constexpr float CHART_EPS = 1e-12f;

__device__ __forceinline__ float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ float len3(const float (&a)[3]) { return sqrtf(dot3(a, a)); }
__device__ __forceinline__ float floor_eps(float x) { return x > CHART_EPS ? x : CHART_EPS; }  // a NaN gives the floor

template <bool DEPTH>
__device__ __forceinline__ void chart_vertex(const ChartView& v, int i, float (&p)[3]) {
    if (DEPTH) {
        pixel_point(v.ray, v.maps.W, i, v.maps.depth[i], p);
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) p[c] = v.maps.depth[3 * (size_t)i + c];
    }
}

// The keep test of the contract for the face (A, B, C).
__device__ __forceinline__ bool chart_keep(const float (&A)[3], const float (&B)[3], const float (&C)[3], float ratio_th) {
    float s[3][3], n[3][3], l[3];
#pragma unroll
    for (int k = 0; k < 3; k++) s[0][k] = C[k] - A[k], s[1][k] = A[k] - B[k], s[2][k] = B[k] - C[k];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float d = floor_eps(len3(s[i]));
#pragma unroll
        for (int k = 0; k < 3; k++) n[i][k] = s[i][k] / d;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3;
        const float t = dot3(s[i], n[j]);
        float a[3];
#pragma unroll
        for (int k = 0; k < 3; k++) a[k] = s[i][k] - t * n[i][k];
        l[i] = len3(a);
    }
    if (l[0] != l[0] || l[1] != l[1] || l[2] != l[2]) return false;
    const float mx = fmaxf(fmaxf(l[0], l[1]), l[2]), mn = fminf(fminf(l[0], l[1]), l[2]);
    return mx / mn < ratio_th;  // 0 / 0 is a NaN: dropped
}

__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }  // a NaN stays
__device__ __forceinline__ float sqrt_pos(float x) { return x > 0.0f ? sqrtf(x) : 0.0f; }              // a NaN gives 0

// The surfel of the contract for the kept face (A, B, C) with vertex pixels ia, ib, ic, written to row `row`.
__device__ __forceinline__ void chart_surfel(const float (&A)[3], const float (&B)[3], const float (&C)[3],
                                             const float* __restrict__ img, int ia, int ib, int ic, float normalized_scales,
                                             float normal_scale, size_t row, float* __restrict__ means,
                                             float* __restrict__ scales, float* __restrict__ quats, float* __restrict__ colors) {
    const float b0 = __uint_as_float(0x3eaaaaabu), b1 = __uint_as_float(0x3eaaaaabu), b2 = __uint_as_float(0x3eaaaaaau);
    const float e00 = __uint_as_float(0xbf3504f3u), e01 = __uint_as_float(0x3f3504f3u), e02 = 0.0f;
    const float e10 = __uint_as_float(0xbed105ecu), e11 = __uint_as_float(0xbed105ecu), e12 = __uint_as_float(0x3f5105ecu);
    float t[2][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        means[3 * row + k] = (b0 * A[k] + b1 * B[k]) + b2 * C[k];
        colors[3 * row + k] = (b0 * clamp01(img[3 * (size_t)ia + k]) + b1 * clamp01(img[3 * (size_t)ib + k])) +
                              b2 * clamp01(img[3 * (size_t)ic + k]);
        t[0][k] = (e00 * A[k] + e01 * B[k]) + e02 * C[k];
        t[1][k] = (e10 * A[k] + e11 * B[k]) + e12 * C[k];
    }
    const bool first0 = len3(t[0]) >= len3(t[1]);
    float u[3], w[3], o[2][3];
#pragma unroll
    for (int k = 0; k < 3; k++) u[k] = first0 ? t[0][k] : t[1][k], w[k] = first0 ? t[1][k] : t[0][k];
    const float wu = dot3(w, u), uu = dot3(u, u);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float w2 = w[k] - (wu * u[k]) / uu;
        o[0][k] = first0 ? u[k] : w2;
        o[1][k] = first0 ? w2 : u[k];
    }
    float x[2][3];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const float sv[3] = {o[j][0] * normalized_scales, o[j][1] * normalized_scales, o[j][2] * normalized_scales};
        scales[3 * row + j] = len3(sv);
        const float d = floor_eps(len3(o[j]));
#pragma unroll
        for (int k = 0; k < 3; k++) x[j][k] = o[j][k] / d;
    }
    scales[3 * row + 2] = normal_scale;
    const float nrm[3] = {x[0][1] * x[1][2] - x[0][2] * x[1][1], x[0][2] * x[1][0] - x[0][0] * x[1][2],
                          x[0][0] * x[1][1] - x[0][1] * x[1][0]};
    // R = columns (x0, x1, n): m_ij = column j, component i
    const float m00 = x[0][0], m01 = x[1][0], m02 = nrm[0];
    const float m10 = x[0][1], m11 = x[1][1], m12 = nrm[1];
    const float m20 = x[0][2], m21 = x[1][2], m22 = nrm[2];
    const float qa[4] = {sqrt_pos(((1.0f + m00) + m11) + m22), sqrt_pos(((1.0f + m00) - m11) - m22),
                         sqrt_pos(((1.0f - m00) + m11) - m22), sqrt_pos(((1.0f - m00) - m11) + m22)};
    int best = 0;
#pragma unroll
    for (int i = 1; i < 4; i++) best = qa[i] > qa[best] ? i : best;
    const float a = m21 - m12, b = m02 - m20, c = m10 - m01, d = m10 + m01, e = m02 + m20, f = m12 + m21;
    float q[4];
    if (best == 0) q[0] = qa[0] * qa[0], q[1] = a, q[2] = b, q[3] = c;
    else if (best == 1) q[0] = a, q[1] = qa[1] * qa[1], q[2] = d, q[3] = e;
    else if (best == 2) q[0] = b, q[1] = d, q[2] = qa[2] * qa[2], q[3] = f;
    else q[0] = c, q[1] = e, q[2] = f, q[3] = qa[3] * qa[3];
    const float qb = qa[best];
    const float den = 2.0f * (qb > 0.1f ? qb : 0.1f);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = q[k] / den;
    const bool flip = q[0] < 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) quats[4 * row + k] = flip ? -q[k] : q[k];
}

// flag[0] = 1 iff some mask byte of some view is set.  Every writer stores the same word: no atomic needed.
__global__ void __launch_bounds__(256) chart_mask_any_kernel(const ChartView* __restrict__ views, int pixels, int blocks_per_view,
                                                             uint32_t* __restrict__ flag) {
    const int v = (int)(blockIdx.x / (unsigned)blocks_per_view), b = (int)(blockIdx.x % (unsigned)blocks_per_view);
    const int i = b * 256 + (int)threadIdx.x;
    const bool set = i < pixels && views[v].mask[i] != 0;
    if (__ballot(set) != 0ull && lane_id() == 0) flag[0] = 1u;
}

struct ChartCell {
    int i00, i10, i01, i11;  // pixels (r, c), (r + 1, c), (r, c + 1), (r + 1, c + 1)
};
__device__ __forceinline__ ChartCell chart_cell(int t, int W) {
    const int r = t / (W - 1), c = t % (W - 1);
    const int i = r * W + c;
    return ChartCell{i, i + W, i + 1, i + W + 1};
}

template <bool DEPTH>
__global__ void __launch_bounds__(256) chart_count_kernel(const ChartView* __restrict__ views, int groups, int cells,
                                                          float ratio_th, const uint32_t* __restrict__ mask_any,
                                                          unsigned long long* __restrict__ ballots, uint32_t* __restrict__ counts) {
    __shared__ uint32_t sm[8];
    const int v = (int)(blockIdx.x / (unsigned)groups), g = (int)(blockIdx.x % (unsigned)groups);
    const int t = g * 256 + (int)threadIdx.x;
    const ChartView& view = views[v];
    bool k1 = false, k2 = false;
    if (t < cells) {
        const ChartCell q = chart_cell(t, view.maps.W);
        float p00[3], p10[3], p01[3], p11[3];
        chart_vertex<DEPTH>(view, q.i00, p00);
        chart_vertex<DEPTH>(view, q.i10, p10);
        chart_vertex<DEPTH>(view, q.i01, p01);
        chart_vertex<DEPTH>(view, q.i11, p11);
        k1 = chart_keep(p00, p10, p01, ratio_th);
        k2 = chart_keep(p11, p01, p10, ratio_th);
        if (view.mask != nullptr && mask_any[0] != 0u) {
            const bool m10 = view.mask[q.i10] != 0, m01 = view.mask[q.i01] != 0;
            k1 = k1 && (view.mask[q.i00] != 0 || m10 || m01);
            k2 = k2 && (view.mask[q.i11] != 0 || m01 || m10);
        }
    }
    const unsigned long long w1 = __ballot(k1), w2 = __ballot(k2);
    const int wave = (int)threadIdx.x >> 6;
    const size_t e1 = (size_t)(2 * (long long)v) * groups + g, e2 = e1 + groups;
    if (lane_id() == 0) {
        ballots[4 * e1 + wave] = w1;
        ballots[4 * e2 + wave] = w2;
        sm[wave] = (uint32_t)__builtin_popcountll(w1);
        sm[4 + wave] = (uint32_t)__builtin_popcountll(w2);
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[e1] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    if (threadIdx.x == 64) counts[e2] = (sm[4] + sm[5]) + (sm[6] + sm[7]);
}

template <bool DEPTH>
__global__ void __launch_bounds__(256) chart_emit_kernel(const ChartView* __restrict__ views, int groups, int cells,
                                                         const unsigned long long* __restrict__ ballots,
                                                         const uint32_t* __restrict__ offs, float normalized_scales,
                                                         float normal_scale, uint32_t n_faces, float* __restrict__ means,
                                                         float* __restrict__ scales, float* __restrict__ quats,
                                                         float* __restrict__ colors) {
    const int v = (int)(blockIdx.x / (unsigned)groups), g = (int)(blockIdx.x % (unsigned)groups);
    const int t = g * 256 + (int)threadIdx.x;
    if (t >= cells) return;  // nothing below is a wave or workgroup collective
    const ChartView& view = views[v];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const size_t e1 = (size_t)(2 * (long long)v) * groups + g;
    bool keep[2];
    uint32_t row[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const size_t e = e1 + (size_t)h * groups;
        uint32_t before = offs[e];
        for (int w = 0; w < wave; w++) before += (uint32_t)__builtin_popcountll(ballots[4 * e + w]);
        const unsigned long long mine = ballots[4 * e + wave];
        keep[h] = ((mine >> lane) & 1ull) != 0ull;
        row[h] = before + (uint32_t)__builtin_popcountll(mine & below);
    }
    if (!keep[0] && !keep[1]) return;
    const ChartCell q = chart_cell(t, view.maps.W);
    float p00[3], p10[3], p01[3], p11[3];
    chart_vertex<DEPTH>(view, q.i00, p00);
    chart_vertex<DEPTH>(view, q.i10, p10);
    chart_vertex<DEPTH>(view, q.i01, p01);
    chart_vertex<DEPTH>(view, q.i11, p11);
    if (keep[0] && row[0] < n_faces)  // the caller's capacity
        chart_surfel(p00, p10, p01, view.maps.rgb, q.i00, q.i10, q.i01, normalized_scales, normal_scale, row[0], means, scales,
                     quats, colors);
    if (keep[1] && row[1] < n_faces)
        chart_surfel(p11, p01, p10, view.maps.rgb, q.i11, q.i01, q.i10, normalized_scales, normal_scale, row[1], means, scales,
                     quats, colors);
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

// 0 <= V, 0 < H, W, and 2 V (H-1)(W-1) < 2^31 (so is V H W: the per-view pixel index and every table index fit an int)
bool chart_dims_ok(int V, int H, int W) {
    if (V < 0 || H <= 0 || W <= 0) return false;
    return (long long)H * W < (1ll << 31) && 2ll * V * ((long long)(H - 1) * (W - 1)) < (1ll << 31);
}

int check_chart_dims(int V, int H, int W) {
    if (V < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_views must not be negative");
    if (H <= 0 || W <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "height, width must be positive");
    if (!chart_dims_ok(V, H, W))
        return fail(G4S_ERR_INVALID_ARGUMENT, "2 * n_views * (height - 1) * (width - 1) must be below 2^31");
    return G4S_OK;
}

// the view table of both phases: maps, rays (depth form), images (emit) and masks (count)
int chart_table(const char* name, int V, int H, int W, const float* const* maps, const float* rays, const float* const* images,
                const unsigned char* const* masks, char* workspace, size_t workspace_bytes, hipStream_t stream,
                const ChartView** table) {
    std::vector<int> sizes((size_t)V * 2);
    for (int v = 0; v < V; v++) sizes[2 * (size_t)v] = W, sizes[2 * (size_t)v + 1] = H;
    return stage_views(name, V, true, sizes.data(), maps, images, images != nullptr, workspace, workspace_bytes, stream, table,
                       [&](ChartView& u, int v) {
                           u.ray = rays ? ray_record(rays + 12 * (size_t)v) : VisRay{};
                           u.mask = masks ? masks[v] : nullptr;
                       });
}

}  // namespace

extern "C" size_t g4s_chart_surfels_workspace(int n_views, int height, int width) {
    if (!chart_dims_ok(n_views, height, width)) return 0;
    return chart_layout(n_views, height, width).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_chart_surfels_count(int n_views, int height, int width, int depth_form, const float* const* maps,
                                       const float* rays, const unsigned char* const* masks, float ratio_th, int* n_faces,
                                       char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (check_chart_dims(n_views, height, width) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!n_faces) return null_pointer();
    *n_faces = 0;
    const ChartLayout L = chart_layout(n_views, height, width);
    if (L.entries == 0) return G4S_OK;  // no view, or a view one pixel high or wide: no face
    if (check_pointers("maps", maps, n_views) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (depth_form && !rays) return null_pointer();
    if (masks && check_pointers("masks", masks, n_views) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (check_workspace(workspace, workspace_bytes, g4s_chart_surfels_workspace(n_views, height, width)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    char* ws = align_ptr(workspace);
    uint32_t* words = (uint32_t*)(ws + L.words);
    uint32_t* counts = (uint32_t*)(ws + L.counts);
    hipError_t e = hipMemsetAsync(words, 0, 64, s);
    if (e != hipSuccess) return finish(e, "chart surfels count");
    const ChartView* table;
    const int rc = chart_table("chart surfels count", n_views, height, width, maps, depth_form ? rays : nullptr, nullptr, masks,
                               workspace, workspace_bytes, s, &table);
    if (rc != G4S_OK) return rc;
    if (masks) {
        const int pixels = height * width, per_view = (int)blocks256(pixels);
        hipLaunchKernelGGL(chart_mask_any_kernel, dim3((unsigned)((long long)n_views * per_view)), dim3(256), 0, s, table, pixels,
                           per_view, words + 2);
    }
    const auto kernel = depth_form ? chart_count_kernel<true> : chart_count_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_views * L.groups)), dim3(256), 0, s, table, (int)L.groups, (int)L.cells, ratio_th,
                       (const uint32_t*)(words + 2), (unsigned long long*)(ws + L.ballots), counts);
    scan_u32(counts, (uint32_t*)(ws + L.offs), (int)L.entries, (uint32_t*)(ws + L.chunks), words + 0, s);
    int t[2];
    e = read_totals(words, t, s);
    if (e != hipSuccess) return finish(e, "chart surfels count");
    *n_faces = t[0];
    return finish(hipSuccess, "chart surfels count");
}

extern "C" int g4s_chart_surfels_emit(int n_views, int height, int width, int depth_form, const float* const* maps,
                                      const float* rays, const float* const* images, float normalized_scales,
                                      float normal_scale, int n_faces, float* means, float* scales, float* quaternions,
                                      float* colors, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (check_chart_dims(n_views, height, width) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const ChartLayout L = chart_layout(n_views, height, width);
    if (n_faces < 0 || n_faces > n_views * L.cells * 2)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_faces must lie in 0 .. 2 * n_views * (height - 1) * (width - 1)");
    if (n_faces == 0) return G4S_OK;
    if (check_pointers("maps", maps, n_views) != G4S_OK || check_pointers("images", images, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if ((depth_form && !rays) || !means || !scales || !quaternions || !colors) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_chart_surfels_workspace(n_views, height, width)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    char* ws = align_ptr(workspace);
    const ChartView* table;
    const int rc = chart_table("chart surfels emit", n_views, height, width, maps, depth_form ? rays : nullptr, images, nullptr,
                               workspace, workspace_bytes, s, &table);
    if (rc != G4S_OK) return rc;
    const auto kernel = depth_form ? chart_emit_kernel<true> : chart_emit_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_views * L.groups)), dim3(256), 0, s, table, (int)L.groups, (int)L.cells,
                       (const unsigned long long*)(ws + L.ballots), (const uint32_t*)(ws + L.offs), normalized_scales,
                       normal_scale, (uint32_t)n_faces, means, scales, quaternions, colors);
    return finish(hipSuccess, "chart surfels emit");
}
