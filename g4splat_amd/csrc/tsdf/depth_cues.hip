// Depth cues of the inpainted views (include/g4s_render_maps.h, "Depth cues"; the semantics stated there are the contract,
// tests/depth_cues_ref.py restates them in numpy): the masked scale-and-shift alignment of a mono disparity, the maps that
// follow from it, the depths of the fitted global planes and the refill of what neither a plane nor a confident pixel covers.
//
//   sums    grid = (spans of ALIGN_SPAN pixels of the largest view, views).  A thread adds its ALIGN_ITEMS pixels in ascending
//           order in float64, a wave folds its lanes by a fixed shuffle tree, lane 0 of wave 0 adds the four wave sums in
//           wave order and stores the workgroup's five partials.  No atomics.
//   coeffs  one wave per view: lane l adds partials l, l + 64, ... in ascending order, the same shuffle tree folds the lanes,
//           lane 0 forms beta and alpha in float64 and rounds them to float32.  Two runs give the same bits.
//   apply, cues, planes, refill   one thread per pixel of every view, grid = (blocks of 256 pixels of the largest view, views).
//           The plane kernel finds the pixel's (view, id) entry by binary search in the view's sorted ids and counts what it
//           replaced and zeroed per view with one integer atomic per wave (wave_count.h).
// Every launch count is independent of the number of views and planes.
#include <math.h>

#include "../g4s_internal.h"
#include "../fixed_sums.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "vis_view.h"
#include "wave_count.h"

namespace g4s {

constexpr int ALIGN_ITEMS = 16;                // pixels per thread of the sums kernel
constexpr int ALIGN_SPAN = 256 * ALIGN_ITEMS;  // pixels one workgroup reduces (tests/test_gpu_depth_cues.py mirrors it)
constexpr int ALIGN_TERMS = 5;                 // n, sum t, sum d, sum t d, sum d d
static_assert(ALIGN_SPAN == G4S_DEPTH_ALIGN_SPAN, "the header states the span the workspace is sized by");

enum { ALIGN_DISPARITY = 0, ALIGN_DEPTH = 1, ALIGN_INVERSE_SOURCE = 2 };

struct AlignView {
    ViewMaps maps;       // depth = the source map
    const float* target;
    const void* mask;    // uint8 [H,W], or float32 [H,W] compared with the threshold
    float* out;          // apply: the aligned map
    uint32_t block_base; // the view's first row of the partials
    uint32_t n_blocks;   // ceil(W H / ALIGN_SPAN)
};

struct CueView {
    VisRay ray;
    float Rw[9];  // Rw[3 i + j] = world_view_transform[i][j]
    ViewMaps maps;  // depth = the mono disparity
    const float* warp;
    const float* alpha;
    unsigned char* visibility;
    float *mono, *aligned, *merged, *normal_world, *normal_cam;
};

struct PlaneView {
    float o[3];
    float R[9];  // camera -> world rotation, row-major
    float fx, fy;
    ViewMaps maps;  // depth = the depth map that is read
    float* out;
    const int* mask;
    int id_base, n_ids;  // the view's run of the id table
};

struct RefillView {
    ViewMaps maps;  // depth = the mono depth
    float* depth;
    const int* mask;
    const unsigned char* conf;
};

// t and d of a masked pixel in the entry point's domain
__device__ __forceinline__ void align_terms(int domain, float src, float tgt, float& t, float& d) {
    t = domain == ALIGN_DEPTH ? tgt : 1.0f / tgt;
    d = domain == ALIGN_INVERSE_SOURCE ? 1.0f / src : src;
}

// the aligned value of a source value: 1 / (alpha + beta d), or alpha + beta d in the depth domain
__device__ __forceinline__ float align_value(int domain, float alpha, float beta, float src) {
    const float d = domain == ALIGN_INVERSE_SOURCE ? 1.0f / src : src;
    const float lin = alpha + beta * d;
    return domain == ALIGN_DEPTH ? lin : 1.0f / lin;
}

__global__ void __launch_bounds__(256) align_sums_kernel(const AlignView* __restrict__ views, int domain, int mask_is_map,
                                                         float threshold, double* __restrict__ partials) {
    const AlignView& v = views[blockIdx.y];
    if (blockIdx.x >= v.n_blocks) return;  // block-uniform
    const int n = v.maps.W * v.maps.H;
    double s[ALIGN_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const size_t first = (size_t)blockIdx.x * ALIGN_SPAN + threadIdx.x;
    for (int k = 0; k < ALIGN_ITEMS; k++) {
        const size_t q = first + (size_t)k * 256;
        if (q >= (size_t)n) break;
        const bool set = mask_is_map ? ((const float*)v.mask)[q] > threshold : ((const unsigned char*)v.mask)[q] != 0;
        if (!set) continue;
        float tf, df;
        align_terms(domain, v.maps.depth[q], v.target[q], tf, df);
        const double t = (double)tf, d = (double)df;
        s[0] += 1.0;
        s[1] += t;
        s[2] += d;
        s[3] += t * d;  // exact: two float32 factors
        s[4] += d * d;
    }
    __shared__ double waves[4][ALIGN_TERMS];
#pragma unroll
    for (int c = 0; c < ALIGN_TERMS; c++) moment_fold(s[c], waves, c);
    moment_store(waves, ALIGN_TERMS, partials + ((size_t)v.block_base + blockIdx.x) * ALIGN_TERMS);
}

// grid = views, 64 threads
__global__ void __launch_bounds__(64) align_coeffs_kernel(const AlignView* __restrict__ views, const double* __restrict__ partials,
                                                          float* __restrict__ coeffs, int* __restrict__ counts) {
    const AlignView& v = views[blockIdx.x];
    double s[ALIGN_TERMS];
    column_fold(partials + (size_t)v.block_base * ALIGN_TERMS, v.n_blocks, ALIGN_TERMS, s);
    if (threadIdx.x == 0) scale_shift_solve(s, coeffs + 2 * (size_t)blockIdx.x, counts + blockIdx.x);
}

__global__ void __launch_bounds__(256) align_apply_kernel(const AlignView* __restrict__ views, int domain,
                                                          const float* __restrict__ coeffs) {
    const AlignView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    v.out[q] = align_value(domain, coeffs[2 * blockIdx.y], coeffs[2 * blockIdx.y + 1], v.maps.depth[q]);
}

// the world point of pixel (x, y) at its own aligned depth
__device__ __forceinline__ void cue_point(const CueView& v, float alpha, float beta, int x, int y, float (&p)[3]) {
    const int i = y * v.maps.W + x;
    pixel_point(v.ray, v.maps.W, i, align_value(ALIGN_DISPARITY, alpha, beta, v.maps.depth[i]), p);
}

__global__ void __launch_bounds__(256) cue_maps_kernel(const CueView* __restrict__ views, float threshold,
                                                       const float* __restrict__ coeffs) {
    const CueView& v = views[blockIdx.y];
    const int W = v.maps.W, H = v.maps.H;
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= W * H) return;
    const float alpha = coeffs[2 * blockIdx.y], beta = coeffs[2 * blockIdx.y + 1];
    const float d = v.maps.depth[q];
    const bool vis = v.alpha[q] > threshold;
    const float a = align_value(ALIGN_DISPARITY, alpha, beta, d);
    v.visibility[q] = vis ? 1 : 0;
    v.mono[q] = 1.0f / d;
    v.aligned[q] = a;
    v.merged[q] = vis ? v.warp[q] : a;
    const int x = q % W, y = q / W;
    float nw[3] = {0.0f, 0.0f, 0.0f}, nc[3] = {0.0f, 0.0f, 0.0f};
    if (x >= 1 && x < W - 1 && y >= 1 && y < H - 1) {  // an interior pixel exists only with W, H >= 3
        float up[3], down[3], left[3], right[3];
        cue_point(v, alpha, beta, x, y - 1, up);
        cue_point(v, alpha, beta, x, y + 1, down);
        cue_point(v, alpha, beta, x - 1, y, left);
        cue_point(v, alpha, beta, x + 1, y, right);
        float dx[3], dy[3];
#pragma unroll
        for (int c = 0; c < 3; c++) dx[c] = down[c] - up[c], dy[c] = right[c] - left[c];
        const float n0 = dx[1] * dy[2] - dx[2] * dy[1];
        const float n1 = dx[2] * dy[0] - dx[0] * dy[2];
        const float n2 = dx[0] * dy[1] - dx[1] * dy[0];
        const float len = fmaxf(sqrtf((n0 * n0 + n1 * n1) + n2 * n2), 1e-12f);
        nw[0] = n0 / len, nw[1] = n1 / len, nw[2] = n2 / len;
#pragma unroll
        for (int j = 0; j < 3; j++) nc[j] = (nw[0] * v.Rw[j] + nw[1] * v.Rw[3 + j]) + nw[2] * v.Rw[6 + j];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        v.normal_world[3 * (size_t)q + c] = nw[c];
        v.normal_cam[3 * (size_t)q + c] = nc[c];
    }
}

// no early return: the waves vote
__global__ void __launch_bounds__(256) plane_depths_kernel(const PlaneView* __restrict__ views, int n_views,
                                                           const int* __restrict__ ids, const int* __restrict__ entry_plane,
                                                           const float* __restrict__ planes, uint32_t* __restrict__ counts) {
    const PlaneView& v = views[blockIdx.y];
    const int W = v.maps.W, H = v.maps.H;
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool inside = q < W * H;
    bool replaced = false, zeroed = false;
    if (inside) {
        float depth = v.maps.depth[q];
        const int id = v.mask[q];
        int k = -1;
        if (id > 0) {  // the view's ids are strictly ascending
            int lo = 0, hi = v.n_ids;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ids[v.id_base + mid] < id) lo = mid + 1; else hi = mid;
            }
            if (lo < v.n_ids && ids[v.id_base + lo] == id) k = entry_plane[v.id_base + lo];
        }
        if (k >= 0) {
            const float* P = planes + 6 * (size_t)k;
            const float dcx = ((float)(q % W) - (float)W * 0.5f) / v.fx;
            const float dcy = ((float)(q / W) - (float)H * 0.5f) / v.fy;
            float w[3];
#pragma unroll
            for (int r = 0; r < 3; r++) w[r] = (v.R[3 * r] * dcx + v.R[3 * r + 1] * dcy) + v.R[3 * r + 2];
            const float len = fmaxf(sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]), 1e-12f);
            const float nd = (P[0] * (w[0] / len) + P[1] * (w[1] / len)) + P[2] * (w[2] / len);
            const float ndc = copysignf(fmaxf(fabsf(nd), 1e-8f), nd);
            const float num = (P[0] * (P[3] - v.o[0]) + P[1] * (P[4] - v.o[1])) + P[2] * (P[5] - v.o[2]);
            const float t = num / ndc;
            const float z = t / len;
            const bool valid = t > 0.0f && z > 0.0f;
            depth = valid ? z : 0.0f;
            replaced = valid;
            zeroed = !valid;
        }
        v.out[q] = depth;
    }
    wave_count(counts, blockIdx.y, replaced);
    wave_count(counts, (uint32_t)n_views + blockIdx.y, zeroed);
}

// grid y = the inpainted views; first_view = n_input_views
__global__ void __launch_bounds__(256) refill_kernel(const RefillView* __restrict__ views, int first_view,
                                                     const float* __restrict__ coeffs) {
    const int view = first_view + (int)blockIdx.y;
    const RefillView& v = views[view];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    if (v.mask[q] != 0 || v.conf[q] != 0) return;
    v.depth[q] = align_value(ALIGN_INVERSE_SOURCE, coeffs[2 * (size_t)view], coeffs[2 * (size_t)view + 1], v.maps.depth[q]);
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

inline long long spans(long long pixels) { return (pixels + ALIGN_SPAN - 1) / ALIGN_SPAN; }

int check_domain(int domain) {
    return domain >= ALIGN_DISPARITY && domain <= ALIGN_INVERSE_SOURCE
               ? G4S_OK
               : fail(G4S_ERR_INVALID_ARGUMENT, "domain must be 0 (disparity), 1 (depth) or 2 (inverse source)");
}

// byte offsets into the workspace, after the view table
struct AlignLayout { size_t partials, bytes; };
AlignLayout align_layout(int n_views, const int* sizes) {  // sizes have passed view_sizes_ok
    long long total_spans = 0;
    for (int v = 0; v < n_views; v++) total_spans += spans((long long)sizes[2 * v] * sizes[2 * v + 1]);
    WorkspaceCursor c;
    take_view_table<AlignView>(c, n_views);
    const size_t partials = c.take((size_t)total_spans * ALIGN_TERMS * sizeof(double));
    return {partials, c.off};
}

struct PlaneDepthsLayout { size_t ids, planes, bytes; };  // ids: the ids [n_entries], then entry_plane [n_entries]
PlaneDepthsLayout plane_depths_layout(int n_views, int n_entries, int n_planes) {
    WorkspaceCursor c;
    take_view_table<PlaneView>(c, n_views);
    const size_t ids = c.take((size_t)n_entries * 8), planes = c.take((size_t)n_planes * 24);
    return {ids, planes, c.off};
}

}  // namespace

extern "C" size_t g4s_depth_align_workspace(int n_views, const int* sizes) {
    long long largest, total;
    if (!grid_views_ok(n_views) || !view_sizes_ok(n_views, sizes, &largest, &total)) return 0;
    return align_layout(n_views, sizes).bytes + VIEW_TABLE_SLACK + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_depth_align(int domain, int mask_is_map, float mask_threshold, int n_views, const int* sizes,
                               const float* const* source, const float* const* target, const void* const* masks,
                               float* coeffs, int* counts, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_domain(domain) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (mask_is_map && mask_threshold != mask_threshold) return fail(G4S_ERR_INVALID_ARGUMENT, "mask_threshold must not be NaN");
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return G4S_OK;
    if (check_pointers("source", source, n_views) != G4S_OK || check_pointers("target", target, n_views) != G4S_OK ||
        check_pointers("masks", masks, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!coeffs || !counts) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_depth_align_workspace(n_views, sizes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    double* partials = workspace_at<double>(workspace, align_layout(n_views, sizes).partials);
    uint32_t base = 0, most = 0;
    const AlignView* table;
    const int rc = stage_views("depth align", n_views, true, sizes, source, nullptr, false, workspace,
                               view_table_bytes<AlignView>(n_views), stream, &table, [&](AlignView& u, int v) {
                                   u.target = target[v];
                                   u.mask = masks[v];
                                   u.out = nullptr;
                                   u.block_base = base;
                                   u.n_blocks = (uint32_t)spans((long long)sizes[2 * v] * sizes[2 * v + 1]);
                                   base += u.n_blocks;
                                   if (u.n_blocks > most) most = u.n_blocks;
                               });
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(align_sums_kernel, dim3(most, (unsigned)n_views), dim3(256), 0, stream, table, domain, mask_is_map != 0,
                       mask_threshold, partials);
    hipLaunchKernelGGL(align_coeffs_kernel, dim3((unsigned)n_views), dim3(64), 0, stream, table, (const double*)partials, coeffs,
                       counts);
    return finish(hipSuccess, "depth align");
}

extern "C" size_t g4s_depth_align_apply_workspace(int n_views) {
    return !grid_views_ok(n_views) ? 0 : view_table_bytes<AlignView>(n_views);
}

extern "C" int g4s_depth_align_apply(int domain, int n_views, const int* sizes, const float* const* source,
                                     const float* coeffs, float* const* aligned, char* workspace, size_t workspace_bytes,
                                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_domain(domain) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return G4S_OK;
    if (check_pointers("source", source, n_views) != G4S_OK || check_pointers("aligned", aligned, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!coeffs) return null_pointer();
    const AlignView* table;
    const int rc = stage_views("depth align apply", n_views, true, sizes, source, nullptr, false, workspace, workspace_bytes,
                               stream, &table, [&](AlignView& u, int v) {
                                   u.target = nullptr;
                                   u.mask = nullptr;
                                   u.out = aligned[v];
                                   u.block_base = u.n_blocks = 0u;
                               });
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(align_apply_kernel, dim3(blocks256(largest), (unsigned)n_views), dim3(256), 0, stream, table, domain,
                       coeffs);
    return finish(hipSuccess, "depth align apply");
}

extern "C" size_t g4s_depth_cue_maps_workspace(int n_views) {
    return !grid_views_ok(n_views) ? 0 : view_table_bytes<CueView>(n_views);
}

extern "C" int g4s_depth_cue_maps(int n_views, const float* world_view, const float* rays, const int* sizes,
                                  const float* const* disparity, const float* const* warp_depth,
                                  const float* const* alpha_map, float visible_threshold, const float* coeffs,
                                  unsigned char* const* visibility, float* const* mono_depth, float* const* aligned_depth,
                                  float* const* merged_depth, float* const* normal_world, float* const* normal_cam,
                                  char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (visible_threshold != visible_threshold) return fail(G4S_ERR_INVALID_ARGUMENT, "visible_threshold must not be NaN");
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return G4S_OK;
    if (!world_view || !rays || !coeffs) return null_pointer();
    if (check_pointers("disparity", disparity, n_views) != G4S_OK || check_pointers("warp_depth", warp_depth, n_views) != G4S_OK ||
        check_pointers("alpha_map", alpha_map, n_views) != G4S_OK || check_pointers("visibility", visibility, n_views) != G4S_OK ||
        check_pointers("mono_depth", mono_depth, n_views) != G4S_OK || check_pointers("aligned_depth", aligned_depth, n_views) != G4S_OK ||
        check_pointers("merged_depth", merged_depth, n_views) != G4S_OK || check_pointers("normal_world", normal_world, n_views) != G4S_OK ||
        check_pointers("normal_cam", normal_cam, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const CueView* table;
    const int rc = stage_views("depth cue maps", n_views, true, sizes, disparity, nullptr, false, workspace, workspace_bytes,
                               stream, &table, [&](CueView& u, int v) {
                                   u.ray = ray_record(rays + 12 * (size_t)v);
                                   for (int i = 0; i < 3; i++) {
                                       for (int j = 0; j < 3; j++) u.Rw[3 * i + j] = world_view[16 * (size_t)v + 4 * i + j];
                                   }
                                   u.warp = warp_depth[v];
                                   u.alpha = alpha_map[v];
                                   u.visibility = visibility[v];
                                   u.mono = mono_depth[v];
                                   u.aligned = aligned_depth[v];
                                   u.merged = merged_depth[v];
                                   u.normal_world = normal_world[v];
                                   u.normal_cam = normal_cam[v];
                               });
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(cue_maps_kernel, dim3(blocks256(largest), (unsigned)n_views), dim3(256), 0, stream, table,
                       visible_threshold, coeffs);
    return finish(hipSuccess, "depth cue maps");
}

extern "C" size_t g4s_plane_depths_workspace(int n_views, int n_entries, int n_planes) {
    if (!grid_views_ok(n_views) || n_entries < 0 || n_planes < 0) return 0;
    return plane_depths_layout(n_views, n_entries, n_planes).bytes + VIEW_TABLE_SLACK + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_plane_depths(int n_views, const float* cameras, const int* sizes, const float* const* depth,
                                float* const* depth_out, const int* const* masks, const int* view_offset, const int* ids,
                                const int* entry_plane, int n_planes, const float* planes, int* counts, char* workspace,
                                size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_planes < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_planes must not be negative");
    if (n_views == 0) return G4S_OK;
    if (!cameras || !counts) return null_pointer();
    if (check_pointers("depth", depth, n_views) != G4S_OK || check_pointers("depth_out", depth_out, n_views) != G4S_OK ||
        check_pointers("masks", masks, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 14 * n_views; i++) {
        if (!finite(cameras[i])) return fail(G4S_ERR_INVALID_ARGUMENT, "cameras: view %d is not finite", i / 14);
    }
    for (int v = 0; v < n_views; v++) {
        if (!(cameras[14 * v + 12] > 0.0f) || !(cameras[14 * v + 13] > 0.0f))
            return fail(G4S_ERR_INVALID_ARGUMENT, "cameras: view %d: the focal lengths must be positive", v);
    }
    if (!view_offset) return fail(G4S_ERR_INVALID_ARGUMENT, "view_offset: NULL array");
    if (view_offset[0] != 0) return fail(G4S_ERR_INVALID_ARGUMENT, "view_offset[0] must be 0");
    for (int v = 0; v < n_views; v++) {
        if (view_offset[v + 1] < view_offset[v]) return fail(G4S_ERR_INVALID_ARGUMENT, "view_offset[%d] must not decrease", v + 1);
    }
    const int n_entries = view_offset[n_views];
    if (n_entries > 0 && (!ids || !entry_plane)) return fail(G4S_ERR_INVALID_ARGUMENT, "ids, entry_plane: NULL array");
    if (n_planes > 0 && !planes) return fail(G4S_ERR_INVALID_ARGUMENT, "planes: NULL array");
    for (int v = 0; v < n_views; v++) {
        for (int e = view_offset[v]; e < view_offset[v + 1]; e++) {
            if (ids[e] <= 0 || (e > view_offset[v] && ids[e] <= ids[e - 1]))
                return fail(G4S_ERR_INVALID_ARGUMENT, "ids[%d]: the ids of view %d must be positive and strictly ascending", e, v);
            if (entry_plane[e] < 0 || entry_plane[e] >= n_planes)
                return fail(G4S_ERR_INVALID_ARGUMENT, "entry_plane[%d] must be a plane below n_planes", e);
        }
    }
    for (int i = 0; i < 6 * n_planes; i++) {
        if (!finite(planes[i])) return fail(G4S_ERR_INVALID_ARGUMENT, "planes: plane %d is not finite", i / 6);
    }
    if (check_workspace(workspace, workspace_bytes, g4s_plane_depths_workspace(n_views, n_entries, n_planes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const PlaneDepthsLayout L = plane_depths_layout(n_views, n_entries, n_planes);
    int* dev_ids = workspace_at<int>(workspace, L.ids);
    int* dev_plane = dev_ids + n_entries;
    float* dev_planes = workspace_at<float>(workspace, L.planes);
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_views * 8, stream);
    if (e == hipSuccess && n_entries > 0) e = upload_pair(dev_ids, ids, n_entries, entry_plane, n_entries, stream);
    if (e == hipSuccess && n_planes > 0) e = upload(dev_planes, planes, (size_t)n_planes * 24, stream);
    if (e != hipSuccess) return finish(e, "plane depths");
    const PlaneView* table;
    const int rc = stage_views("plane depths", n_views, true, sizes, depth, nullptr, false, workspace,
                               view_table_bytes<PlaneView>(n_views), stream, &table, [&](PlaneView& u, int v) {
                                   const float* c = cameras + 14 * (size_t)v;
                                   for (int i = 0; i < 3; i++) u.o[i] = c[i];
                                   for (int i = 0; i < 9; i++) u.R[i] = c[3 + i];
                                   u.fx = c[12];
                                   u.fy = c[13];
                                   u.out = depth_out[v];
                                   u.mask = masks[v];
                                   u.id_base = view_offset[v];
                                   u.n_ids = view_offset[v + 1] - view_offset[v];
                               });
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(plane_depths_kernel, dim3(blocks256(largest), (unsigned)n_views), dim3(256), 0, stream, table, n_views,
                       (const int*)dev_ids, (const int*)dev_plane, (const float*)dev_planes, (uint32_t*)counts);
    return finish(hipSuccess, "plane depths");
}

extern "C" size_t g4s_depth_refill_workspace(int n_views) {
    return !grid_views_ok(n_views) ? 0 : view_table_bytes<RefillView>(n_views);
}

extern "C" int g4s_depth_refill(int n_views, int n_input_views, const int* sizes, float* const* depth,
                                const float* const* mono_depth, const int* const* masks, const unsigned char* const* conf,
                                const float* coeffs, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_input_views < 0 || n_input_views > n_views)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_input_views must be in 0 .. n_views");
    if (n_views == 0) return G4S_OK;
    if (check_pointers("depth", depth, n_views) != G4S_OK || check_pointers("mono_depth", mono_depth, n_views) != G4S_OK ||
        check_pointers("masks", masks, n_views) != G4S_OK || check_pointers("conf", conf, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!coeffs) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_depth_refill_workspace(n_views)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_input_views == n_views) return G4S_OK;
    long long largest_inpainted;  // the sizes have passed: this only measures the inpainted views
    view_sizes_ok(n_views - n_input_views, sizes + 2 * n_input_views, &largest_inpainted, &total);
    const RefillView* table;
    const int rc = stage_views("depth refill", n_views, true, sizes, mono_depth, nullptr, false, workspace, workspace_bytes,
                               stream, &table, [&](RefillView& u, int v) {
                                   u.depth = depth[v];
                                   u.mask = masks[v];
                                   u.conf = conf[v];
                               });
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(refill_kernel, dim3(blocks256(largest_inpainted), (unsigned)(n_views - n_input_views)), dim3(256), 0,
                       stream, table, n_input_views, coeffs);
    return finish(hipSuccess, "depth refill");
}
