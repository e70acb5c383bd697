// Visibility grid for novel-view selection (include/g4s_render_maps.h, "Visibility grid"; the semantics stated there are
// the contract, tests/visibility_ref.py restates them in numpy).
//
// Build:  one thread per voxel, 64 consecutive flat indices per wave, so a wave is a run of voxels along z (and a few row
// ends) whose taps into a view fall along one image line.  Each thread walks the view table (view_stack.h: records in the
// workspace, indexed by the loop counter alone, so their reads are wave-uniform) and leaves at the first view that sees
// its centre in free space; the 64 answers become one 64-bit ballot that one lane stores.  No atomics, every word is
// written exactly once, tail bits are zero because out-of-range lanes vote 0.
// March:  one thread per pixel walks its ray through the bit grid (256^3 voxels = 2 MiB) and leaves at its first
// invisible sample; no sample point is ever stored.
// Counts:  points x view stack with the FREE or the SURFACE predicate, for explicit points or for the pixels of a depth map
// back-projected in the kernel.
// Compaction:  per word the number of selected voxels -> fixed-order exclusive scan (scan.h) -> [host: size] -> emit, one
// thread per voxel, its rank inside the word from the lanes below.  The order is the flat index's.
#include <math.h>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "scan.h"
#include "vis_view.h"

namespace g4s {

struct VisGrid {
    float lo[3], extent[3], cell[3];  // bbox_min, bbox_max - bbox_min, extent / R
    int R;
};

enum { VIS_FREE = 0, VIS_SURFACE = 1 };

// The predicate of one (point, view) pair.  A NaN fails every comparison, so the map is read only at a pixel inside it.
template <int MODE>
__device__ __forceinline__ bool vis_pass(const VisView& v, float px, float py, float pz, float threshold) {
    VisProj q;
    if (!vis_project(v, px, py, pz, q)) return false;
    const float z = q.z;
    const float d = v.maps.depth[vis_tap(v, q)];
    if (MODE == VIS_FREE) return z > 0.0f && z < d;
    return vis_surface(z, d, threshold);
}

__device__ __forceinline__ float voxel_centre(const VisGrid& g, int axis, int i) {
    return g.lo[axis] + ((float)i + 0.5f) * g.cell[axis];
}

// flat < R^3
__device__ __forceinline__ void voxel_of_flat(const VisGrid& g, uint32_t flat, float& x, float& y, float& z) {
    const uint32_t R = (uint32_t)g.R;
    const uint32_t iz = flat % R, r = flat / R;
    x = voxel_centre(g, 0, (int)(r / R));
    y = voxel_centre(g, 1, (int)(r % R));
    z = voxel_centre(g, 2, (int)iz);
}

// Flat index of the voxel a point falls into; always below R^3 (minNum / maxNum: a NaN coordinate gives index 0).
__device__ __forceinline__ uint32_t voxel_of_point(const VisGrid& g, float px, float py, float pz) {
    const float top = (float)(g.R - 1), Rf = (float)g.R;
    const int ix = (int)fminf(fmaxf(((px - g.lo[0]) / g.extent[0]) * Rf, 0.0f), top);
    const int iy = (int)fminf(fmaxf(((py - g.lo[1]) / g.extent[1]) * Rf, 0.0f), top);
    const int iz = (int)fminf(fmaxf(((pz - g.lo[2]) / g.extent[2]) * Rf, 0.0f), top);
    return ((uint32_t)ix * (uint32_t)g.R + (uint32_t)iy) * (uint32_t)g.R + (uint32_t)iz;
}

__device__ __forceinline__ bool voxel_bit(const unsigned long long* __restrict__ words, uint32_t flat) {
    return (words[flat >> 6] >> (flat & 63u)) & 1ull;
}
__device__ __forceinline__ bool voxel_bit(const unsigned char* __restrict__ bytes, uint32_t flat) { return bytes[flat] != 0; }

// ---------------------------------------------------------------------------------------------------------------------
// grid

// 256 threads = 4 words; grid = ceil(total / 256)
__global__ void __launch_bounds__(256) visgrid_build_kernel(VisGrid g, uint32_t total, const VisView* __restrict__ views,
                                                            int n_views, unsigned long long* __restrict__ words) {
    const uint32_t flat = blockIdx.x * 256u + threadIdx.x;
    bool vis = false;
    if (flat < total) {
        float x, y, z;
        voxel_of_flat(g, flat, x, y, z);
        for (int v = 0; v < n_views; v++) {
            if (vis_pass<VIS_FREE>(views[v], x, y, z, 0.0f)) {
                vis = true;
                break;
            }
        }
    }
    const unsigned long long word = __ballot(vis);
    // the wave's first lane is in range iff the wave has a word to write
    if (lane_id() == 0 && flat < total) words[flat >> 6] = word;
}

__global__ void __launch_bounds__(256) visgrid_sample_kernel(VisGrid g, const unsigned long long* __restrict__ words, int n,
                                                             const float* __restrict__ points,
                                                             unsigned char* __restrict__ visible) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const uint32_t flat = voxel_of_point(g, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
    visible[i] = voxel_bit(words, flat) ? 1 : 0;
}

// n_samples = S of the contract: sample k < S - 10 sits at t_k of linspace(0, 1, S) along the pixel's ray.  Grid = the packed
// words, or one byte per voxel (the storage the packing is measured against, tools/bench_visibility.py).
template <class Grid>
__global__ void __launch_bounds__(256) visgrid_march_kernel(VisGrid g, const Grid* __restrict__ grid, int W, int n_pixels,
                                                            const float* __restrict__ depth, VisRay ray, int S,
                                                            float* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n_pixels) return;
    const float d = depth[i];
    if (d <= 1e-6f) {
        out[i] = 0.0f;
        return;
    }
    float dir[3];
    ray_dir(ray, i % W, i / W, dir);
    // torch.linspace(0, 1, S) in float32: the lower half counts up from 0, the upper half down from 1, and the upper
    // half's multiply-subtract is one fused operation there -- the one fmaf of this unit, spelled for that reason
    const float step = 1.0f / (float)(S - 1);
    const int half = S / 2;
    float res = 1.0f;
    for (int k = 0; k < S - 10; k++) {
        const float tk = k < half ? step * (float)k : fmaf(-step, (float)(S - 1 - k), 1.0f);
        const float t = tk * d;
        if (!voxel_bit(grid, voxel_of_point(g, ray.o[0] + t * dir[0], ray.o[1] + t * dir[1], ray.o[2] + t * dir[2]))) {
            res = 0.0f;
            break;
        }
    }
    out[i] = res;
}

__global__ void __launch_bounds__(256) visgrid_expand_kernel(const unsigned long long* __restrict__ words, uint32_t total,
                                                             float* __restrict__ grid) {
    const uint32_t flat = blockIdx.x * 256u + threadIdx.x;
    if (flat < total) grid[flat] = voxel_bit(words, flat) ? 1.0f : 0.0f;
}

// the selected voxels of word w: the visible ones, or the invisible ones among the voxels that exist
__device__ __forceinline__ unsigned long long selected_word(const unsigned long long* __restrict__ words, uint32_t w,
                                                            uint32_t total, int invisible) {
    unsigned long long m = words[w];
    if (invisible) {
        const uint32_t left = total - (w << 6);  // voxels from this word on, >= 1
        m = ~m & (left >= 64u ? ~0ull : (1ull << left) - 1ull);
    }
    return m;
}

__global__ void __launch_bounds__(256) visgrid_compact_count_kernel(const unsigned long long* __restrict__ words,
                                                                    uint32_t n_words, uint32_t total, int invisible,
                                                                    uint32_t* __restrict__ counts) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < n_words) counts[w] = (uint32_t)__builtin_popcountll(selected_word(words, w, total, invisible));
}

__global__ void __launch_bounds__(256) visgrid_compact_emit_kernel(VisGrid g, const unsigned long long* __restrict__ words,
                                                                   uint32_t total, int invisible,
                                                                   const uint32_t* __restrict__ offs, uint32_t capacity,
                                                                   float* __restrict__ centres) {
    const uint32_t flat = blockIdx.x * 256u + threadIdx.x;
    if (flat >= total) return;
    const uint32_t w = flat >> 6, l = flat & 63u;
    const unsigned long long m = selected_word(words, w, total, invisible);
    if (!((m >> l) & 1ull)) return;
    const uint32_t at = offs[w] + (uint32_t)__builtin_popcountll(m & ((1ull << l) - 1ull));
    if (at >= capacity) return;
    float x, y, z;
    voxel_of_flat(g, flat, x, y, z);
    centres[3 * (size_t)at] = x;
    centres[3 * (size_t)at + 1] = y;
    centres[3 * (size_t)at + 2] = z;
}

// ---------------------------------------------------------------------------------------------------------------------
// view counts

template <int MODE>
__device__ __forceinline__ int count_views(const VisView* __restrict__ views, int n_views, int skip_view, float threshold,
                                           float x, float y, float z) {
    int c = 0;
    for (int v = 0; v < n_views; v++) {
        if (v != skip_view && vis_pass<MODE>(views[v], x, y, z, threshold)) c++;
    }
    return c;
}

template <int MODE>
__global__ void __launch_bounds__(256) view_counts_points_kernel(int n, const float* __restrict__ points,
                                                                 const VisView* __restrict__ views, int n_views,
                                                                 int skip_view, float threshold, int* __restrict__ counts) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    counts[i] = count_views<MODE>(views, n_views, skip_view, threshold, points[3 * (size_t)i], points[3 * (size_t)i + 1],
                                  points[3 * (size_t)i + 2]);
}

template <int MODE>
__global__ void __launch_bounds__(256) view_counts_pixels_kernel(int W, int n_pixels, const float* __restrict__ depth,
                                                                 VisRay ray, const VisView* __restrict__ views, int n_views,
                                                                 int skip_view, float threshold, int* __restrict__ counts) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n_pixels) return;
    float p[3];
    pixel_point(ray, W, i, depth[i], p);
    counts[i] = count_views<MODE>(views, n_views, skip_view, threshold, p[0], p[1], p[2]);
}

__global__ void __launch_bounds__(256) depth_to_points_kernel(int W, int n_pixels, const float* __restrict__ depth,
                                                              VisRay ray, float* __restrict__ points) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n_pixels) return;
    float p[3];
    pixel_point(ray, W, i, depth[i], p);
#pragma unroll
    for (int c = 0; c < 3; c++) points[3 * (size_t)i + c] = p[c];
}

struct VisCompactLayout {  // byte offsets into the workspace
    size_t counts, offs, chunks, words, bytes;
    uint32_t n_words;
};

VisCompactLayout vis_compact_layout(int R) {
    VisCompactLayout L{};
    const size_t total = (size_t)R * R * R;
    L.n_words = (uint32_t)((total + 63) / 64);
    WorkspaceCursor c;
    L.counts = c.take((size_t)L.n_words * 4);
    L.offs = c.take((size_t)L.n_words * 4);
    L.chunks = c.take((size_t)scan_chunks((long)L.n_words) * 4 + 4);
    L.words = c.take(64);
    L.bytes = c.off;
    return L;
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

bool grid_resolution_ok(int R) { return R >= 1 && (long long)R * R * R < (1ll << 31); }

int check_grid(int R, const float* bbox_min, const float* bbox_max, VisGrid* g) {
    if (!grid_resolution_ok(R)) return fail(G4S_ERR_INVALID_ARGUMENT, "resolution must be at least 1 and resolution^3 below 2^31");
    if (!bbox_min || !bbox_max) return null_pointer();
    g->R = R;
    for (int a = 0; a < 3; a++) {
        if (!finite(bbox_min[a]) || !finite(bbox_max[a]) || !(bbox_max[a] > bbox_min[a]))
            return fail(G4S_ERR_INVALID_ARGUMENT, "bbox must be finite with bbox_max > bbox_min on every axis");
        g->lo[a] = bbox_min[a];
        g->extent[a] = bbox_max[a] - bbox_min[a];
        g->cell[a] = g->extent[a] / (float)R;
    }
    return G4S_OK;
}

int check_map(int width, int height) {
    return width > 0 && height > 0 && (long long)width * height <= (1ll << 30)
               ? G4S_OK
               : fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive and width * height at most 2^30");
}

int check_mode(int mode, int skip_view) {
    if (mode != VIS_FREE && mode != VIS_SURFACE) return fail(G4S_ERR_INVALID_ARGUMENT, "mode must be 0 (free) or 1 (surface)");
    return skip_view >= -1 ? G4S_OK : fail(G4S_ERR_INVALID_ARGUMENT, "skip_view must be a view index or -1");
}

// the view table of this unit in the workspace (view_stack.h)
int vis_table(int n_views, const float* world_view, const float* focal, const int* sizes, const float* const* depth,
              char* workspace, size_t workspace_bytes, hipStream_t stream, const VisView** table) {
    return stage_views("visibility", n_views, world_view != nullptr && focal != nullptr, sizes, depth, nullptr, false,
                       workspace, workspace_bytes, stream, table,
                       [=](VisView& u, int v) { vis_pose(u, world_view, focal, v); });
}

}  // namespace

extern "C" size_t g4s_visgrid_workspace(int n_views) { return view_table_bytes<VisView>(n_views); }

extern "C" int g4s_visgrid_build(int resolution, const float* bbox_min, const float* bbox_max, int n_views,
                                 const float* world_view, const float* focal, const int* sizes, const float* const* depth,
                                 unsigned long long* words, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    VisGrid g;
    if (check_grid(resolution, bbox_min, bbox_max, &g) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!words) return null_pointer();
    const VisView* table;
    const int rc = vis_table(n_views, world_view, focal, sizes, depth, workspace, workspace_bytes, stream, &table);
    if (rc != G4S_OK) return rc;
    const uint32_t total = (uint32_t)resolution * resolution * resolution;
    hipLaunchKernelGGL(visgrid_build_kernel, dim3(blocks256(total)), dim3(256), 0, stream, g, total, table, n_views, words);
    return finish(hipSuccess, "visgrid build");
}

extern "C" int g4s_visgrid_sample(int resolution, const float* bbox_min, const float* bbox_max,
                                  const unsigned long long* words, int n_points, const float* points,
                                  unsigned char* visible, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    (void)workspace_bytes;
    clear_error();
    VisGrid g;
    if (check_grid(resolution, bbox_min, bbox_max, &g) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_points < 0 || n_points > (1 << 30)) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must be in 0 .. 2^30");
    if (!words || (n_points > 0 && (!points || !visible))) return null_pointer();
    if (n_points == 0) return G4S_OK;
    hipLaunchKernelGGL(visgrid_sample_kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, g, words, n_points,
                       points, visible);
    return finish(hipSuccess, "visgrid sample");
}

namespace {

template <class Grid>
int visgrid_march(int resolution, const float* bbox_min, const float* bbox_max, const Grid* grid, int width, int height,
                  const float* depth, const float* ray, int n_samples, float* visibility, hipStream_t stream) {
    clear_error();
    VisGrid g;
    if (check_grid(resolution, bbox_min, bbox_max, &g) != G4S_OK || check_map(width, height) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_samples < 1) return fail(G4S_ERR_INVALID_ARGUMENT, "n_samples must be at least 1");
    if (!grid || !depth || !visibility || !ray) return null_pointer();
    const int n = width * height;
    hipLaunchKernelGGL(visgrid_march_kernel<Grid>, dim3(blocks256(n)), dim3(256), 0, stream, g, grid, width, n, depth,
                       ray_record(ray), n_samples, visibility);
    return finish(hipSuccess, "visgrid march");
}

}  // namespace

extern "C" int g4s_visgrid_march(int resolution, const float* bbox_min, const float* bbox_max,
                                 const unsigned long long* words, int width, int height, const float* depth,
                                 const float* ray, int n_samples, float* visibility, char* workspace,
                                 size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    return visgrid_march(resolution, bbox_min, bbox_max, words, width, height, depth, ray, n_samples, visibility,
                         (hipStream_t)stream);
}

extern "C" int g4s_visgrid_march_bytes(int resolution, const float* bbox_min, const float* bbox_max,
                                       const unsigned char* grid, int width, int height, const float* depth,
                                       const float* ray, int n_samples, float* visibility, char* workspace,
                                       size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    return visgrid_march(resolution, bbox_min, bbox_max, grid, width, height, depth, ray, n_samples, visibility,
                         (hipStream_t)stream);
}

extern "C" int g4s_visgrid_expand(int resolution, const unsigned long long* words, float* grid, char* workspace,
                                  size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    (void)workspace_bytes;
    clear_error();
    if (!grid_resolution_ok(resolution))
        return fail(G4S_ERR_INVALID_ARGUMENT, "resolution must be at least 1 and resolution^3 below 2^31");
    if (!words || !grid) return null_pointer();
    const uint32_t total = (uint32_t)resolution * resolution * resolution;
    hipLaunchKernelGGL(visgrid_expand_kernel, dim3(blocks256(total)), dim3(256), 0, stream, words, total, grid);
    return finish(hipSuccess, "visgrid expand");
}

extern "C" size_t g4s_visgrid_compact_workspace(int resolution) {
    return grid_resolution_ok(resolution) ? vis_compact_layout(resolution).bytes + WORKSPACE_BASE_SLACK : 0;
}

extern "C" int g4s_visgrid_compact_count(int resolution, const unsigned long long* words, int invisible, int* n_points,
                                         char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (!grid_resolution_ok(resolution))
        return fail(G4S_ERR_INVALID_ARGUMENT, "resolution must be at least 1 and resolution^3 below 2^31");
    if (!words || !n_points) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_visgrid_compact_workspace(resolution)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const VisCompactLayout L = vis_compact_layout(resolution);
    char* ws = align_ptr(workspace);
    uint32_t* counts = (uint32_t*)(ws + L.counts);
    uint32_t* totals = (uint32_t*)(ws + L.words);
    const uint32_t total = (uint32_t)resolution * resolution * resolution;
    hipError_t e = hipMemsetAsync(totals, 0, 8, stream);  // read_totals copies two words; the scan writes the first
    if (e != hipSuccess) return finish(e, "visgrid compact count");
    hipLaunchKernelGGL(visgrid_compact_count_kernel, dim3(blocks256(L.n_words)), dim3(256), 0, stream, words, L.n_words, total,
                       invisible != 0, counts);
    scan_u32(counts, (uint32_t*)(ws + L.offs), (int)L.n_words, (uint32_t*)(ws + L.chunks), totals, stream);
    int t[2];
    e = read_totals(totals, t, stream);
    if (e != hipSuccess) return finish(e, "visgrid compact count");
    *n_points = t[0];
    return G4S_OK;
}

extern "C" int g4s_visgrid_compact_emit(int resolution, const float* bbox_min, const float* bbox_max,
                                        const unsigned long long* words, int invisible, int n_points, float* centres,
                                        char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    VisGrid g;
    if (check_grid(resolution, bbox_min, bbox_max, &g) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_points < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must not be negative");
    if (!words || (n_points > 0 && !centres)) return null_pointer();
    if (n_points == 0) return G4S_OK;  // nothing selected: nothing to write
    if (check_workspace(workspace, workspace_bytes, g4s_visgrid_compact_workspace(resolution)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const VisCompactLayout L = vis_compact_layout(resolution);
    char* ws = align_ptr(workspace);
    const uint32_t total = (uint32_t)resolution * resolution * resolution;
    hipLaunchKernelGGL(visgrid_compact_emit_kernel, dim3(blocks256(total)), dim3(256), 0, stream, g, words, total,
                       invisible != 0, (const uint32_t*)(ws + L.offs), (uint32_t)n_points, centres);
    return finish(hipSuccess, "visgrid compact emit");
}

extern "C" int g4s_view_counts_points(int n_points, const float* points, int mode, float depth_threshold, int skip_view,
                                      int n_views, const float* world_view, const float* focal, const int* sizes,
                                      const float* const* depth, int* counts, char* workspace, size_t workspace_bytes,
                                      void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_points < 0 || n_points > (1 << 30)) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must be in 0 .. 2^30");
    if (check_mode(mode, skip_view) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_points > 0 && (!points || !counts)) return null_pointer();
    const VisView* table;
    const int rc = vis_table(n_views, world_view, focal, sizes, depth, workspace, workspace_bytes, stream, &table);
    if (rc != G4S_OK) return rc;
    if (n_points == 0) return G4S_OK;
    const auto kernel = mode == VIS_FREE ? view_counts_points_kernel<VIS_FREE> : view_counts_points_kernel<VIS_SURFACE>;
    hipLaunchKernelGGL(kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, n_points, points, table, n_views,
                       skip_view, depth_threshold, counts);
    return finish(hipSuccess, "view counts points");
}

extern "C" int g4s_view_counts_pixels(int width, int height, const float* pixel_depth, const float* ray, int mode,
                                      float depth_threshold, int skip_view, int n_views, const float* world_view,
                                      const float* focal, const int* sizes, const float* const* depth, int* counts,
                                      char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_map(width, height) != G4S_OK || check_mode(mode, skip_view) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!pixel_depth || !counts || !ray) return null_pointer();
    const VisRay r = ray_record(ray);
    const VisView* table;
    const int rc = vis_table(n_views, world_view, focal, sizes, depth, workspace, workspace_bytes, stream, &table);
    if (rc != G4S_OK) return rc;
    const int n = width * height;
    const auto kernel = mode == VIS_FREE ? view_counts_pixels_kernel<VIS_FREE> : view_counts_pixels_kernel<VIS_SURFACE>;
    hipLaunchKernelGGL(kernel, dim3(blocks256(n)), dim3(256), 0, stream, width, n, pixel_depth, r, table, n_views,
                       skip_view, depth_threshold, counts);
    return finish(hipSuccess, "view counts pixels");
}

extern "C" int g4s_depth_to_points(int width, int height, const float* depth, const float* ray, float* points,
                                   char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    (void)workspace_bytes;
    clear_error();
    if (check_map(width, height) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!depth || !points || !ray) return null_pointer();
    const VisRay r = ray_record(ray);
    const int n = width * height;
    hipLaunchKernelGGL(depth_to_points_kernel, dim3(blocks256(n)), dim3(256), 0, stream, width, n, depth, r, points);
    return finish(hipSuccess, "depth to points");
}
