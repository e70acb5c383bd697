// Cross-view consistency (include/g4s_render_maps.h, "Cross-view consistency"; the semantics stated there are the contract,
// tests/consistency_ref.py restates them in numpy): the confident maps and the anchor colours of the inpainted views.
//
// Point solver.  Nothing is stored per (point, view) pair.
//   fill    one thread per pixel of every view: conf = 1, the winner word of an inpainted view = 0.
//   points  one thread per point walks the view table (vis_view.h: THE projection, records indexed by the loop counter
//           alone, so their reads are wave-uniform; the points are read coalesced).  The input views give `seen`.  A seen
//           point stores a plain byte 0 into conf at its tap of every inpainted view that sees it.  An unseen point fixes its
//           colour at the first view that sees it and raises the pixel's winner word to i + 1 with an integer atomic max at
//           every view that sees it: the largest index wins whatever the order of execution.  One packed word per point
//           leaves the kernel: three colour bytes, `seen`, "visible somewhere".
//   paint   one thread per pixel of every view: the winner's colour, or the input image's pixel.
// Plane solver.  No launch per (plane, view, anchor) triple.
//   counts  one thread per pixel of every view: the pixel's slot names its global plane, the pixel's point is tested in
//           every anchor view, a wave folds its lanes' equal (plane, anchor) keys before one integer atomic.
//   source  one thread per pixel: (step, source view, source pixel), or step = none.
//   resolve one thread per pixel follows its chain -- steps strictly decrease along it -- and copies the ORIGINAL colour
//           at the chain's end.  That is the reference's sequential in-place repaint, without its order of execution.
// No float atomics, no sort; integer max and integer sums do not depend on the order.
#include <math.h>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "vis_view.h"
#include "wave_count.h"

namespace g4s {

// VisView's fields (vis_project and stage_views read them by name), then the point solver's own.
struct ConsPointView {
    float R[9];
    float T[3];
    float fx, fy;
    ViewMaps maps;
    const float* image;   // [H,W,3] or [3,H,W]
    float* out;           // [H,W,3], or NULL: no outputs
    unsigned char* conf;  // [H,W], or NULL: no outputs
    uint32_t* winner;     // [H,W] in the workspace; NULL for an input view and without outputs
    int pixel_stride, channel_stride;  // of `image`, in floats
};
static_assert(sizeof(ConsPointView) == 120, "g4s_consistency_points_workspace is stated in records of 120 bytes");

// ... and the plane solver's.
struct ConsPlaneView {
    float R[9];
    float T[3];
    float fx, fy;
    ViewMaps maps;
    const int* mask;             // [H,W] slots 0 .. n_slots - 1
    const float* points;         // [H*W,3]
    const unsigned char* image;  // [H,W,3] or NULL (counts)
    unsigned char* out;          // [H,W,3] or NULL (counts)
    int slot_base, n_slots;      // the view's run of the slot tables
    uint32_t pixel_base;         // the view's first pixel in the source arrays
    int pad_;
};
static_assert(sizeof(ConsPlaneView) == 128, "g4s_consistency_plane_*_workspace are stated in records of 128 bytes");

enum : uint32_t { CONS_SEEN = 1u << 24, CONS_VISIBLE = 1u << 25, CONS_NO_STEP = 0xFFFFFFFFu };

// The tap (row-major pixel index) of a point that passes SURFACE in view v, -1 otherwise.  Sizes are at most 2^30 pixels.
template <class View>
__device__ __forceinline__ int cons_surface(const View& v, float px, float py, float pz, float threshold) {
    VisProj q;
    if (!vis_project(v, px, py, pz, q)) return -1;
    const size_t tap = vis_tap(v, q);
    return vis_surface(q.z, v.maps.depth[tap], threshold) ? (int)tap : -1;
}

// uint8(trunc(x * 255)); outside 0 .. 1 the product is clamped to 0 .. 255 first (minNum / maxNum: a NaN gives 0)
__device__ __forceinline__ uint32_t colour_byte(float x) { return (uint32_t)(int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }

// ---------------------------------------------------------------------------------------------------------------------
// point solver

// grid = (blocks of 256 pixels of the largest view, views)
__global__ void __launch_bounds__(256) cons_fill_kernel(const ConsPointView* __restrict__ views) {
    const ConsPointView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    if (v.conf != nullptr) v.conf[q] = 1;
    if (v.winner != nullptr) v.winner[q] = 0u;
}

__global__ void __launch_bounds__(256) cons_point_kernel(int n, const float* __restrict__ points,
                                                         const ConsPointView* __restrict__ views, int n_views, int n_input,
                                                         float threshold, int resume, uint32_t* __restrict__ state) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const float px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
    uint32_t s = resume ? state[i] : 0u;
    for (int v = 0; v < n_input && !(s & CONS_SEEN); v++) {
        if (cons_surface(views[v], px, py, pz, threshold) >= 0) s = CONS_SEEN | CONS_VISIBLE;  // a seen point has no colour
    }
    for (int v = n_input; v < n_views; v++) {
        const ConsPointView& view = views[v];
        const int pix = cons_surface(view, px, py, pz, threshold);
        if (pix < 0) continue;
        if (s & CONS_SEEN) {
            if (view.conf != nullptr) view.conf[pix] = 0;
            continue;
        }
        if (!(s & CONS_VISIBLE)) {  // the first view that sees the point: its colour, from the input image
            const float* c = view.image + (size_t)pix * view.pixel_stride;
            const size_t cs = (size_t)view.channel_stride;
            s = CONS_VISIBLE | colour_byte(c[0]) | (colour_byte(c[cs]) << 8) | (colour_byte(c[2 * cs]) << 16);
        }
        if (view.winner != nullptr) {
            uint32_t* cell = view.winner + pix;
            // the cell only ever grows: a value read here is a lower bound of the final one, so skipping is safe
            if ((uint32_t)i + 1u > *(volatile uint32_t*)cell) atomicMax(cell, (uint32_t)i + 1u);
        }
    }
    state[i] = s;
}

// grid = (blocks of 256 pixels of the largest view, views); state may be NULL if no winner word is non-zero
__global__ void __launch_bounds__(256) cons_paint_kernel(const ConsPointView* __restrict__ views,
                                                         const uint32_t* __restrict__ state) {
    const ConsPointView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    const uint32_t w = v.winner != nullptr ? v.winner[q] : 0u;
    float* o = v.out + 3 * (size_t)q;
    if (w != 0u) {
        const uint32_t s = state[w - 1u];
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = (float)((s >> (8 * c)) & 255u) / 255.0f;
    } else {
        const float* im = v.image + (size_t)q * v.pixel_stride;
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = im[(size_t)c * v.channel_stride];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// plane solver

// the entry of the view's slot table that pixel q's mask value names; slot 0 and values outside the table name entry 0
__device__ __forceinline__ int cons_slot(const ConsPlaneView& v, int q) {
    const int s = v.mask[q];
    return v.slot_base + (s > 0 && s < v.n_slots ? s : 0);
}

// grid = (a capped number of blocks, views); grid-stride over the view's pixels, no early return: the waves vote
__global__ void __launch_bounds__(256) cons_plane_count_kernel(const ConsPlaneView* __restrict__ views,
                                                               const int* __restrict__ slot_plane, int n_anchors,
                                                               const int* __restrict__ anchors, float threshold,
                                                               uint32_t* __restrict__ counts) {
    const ConsPlaneView& v = views[blockIdx.y];
    const int n = v.maps.W * v.maps.H;
    for (int first = (int)(blockIdx.x * 256u); first < n; first += (int)(gridDim.x * 256u)) {  // n <= 2^30: no overflow
        const int q = first + (int)threadIdx.x;
        const int k = q < n ? slot_plane[cons_slot(v, q)] : -1;
        if (__ballot(k >= 0) == 0ull) continue;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        if (k >= 0) px = v.points[3 * (size_t)q], py = v.points[3 * (size_t)q + 1], pz = v.points[3 * (size_t)q + 2];
        for (int j = 0; j < n_anchors; j++) {
            const bool pass = k >= 0 && cons_surface(views[anchors[j]], px, py, pz, threshold) >= 0;
            wave_count(counts, (uint32_t)(k * n_anchors + j), pass);
        }
    }
}

// grid = (blocks of 256 pixels of the largest view, views)
__global__ void __launch_bounds__(256) cons_plane_source_kernel(const ConsPlaneView* __restrict__ views,
                                                                const int* __restrict__ slot_step,
                                                                const int* __restrict__ slot_anchor, float threshold,
                                                                uint32_t* __restrict__ step, int* __restrict__ src_view,
                                                                int* __restrict__ src_pix) {
    const ConsPlaneView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    const int e = cons_slot(v, q);
    const int t = slot_step[e];
    uint32_t st = CONS_NO_STEP;
    int a = 0, pix = 0;
    if (t >= 0) {
        a = slot_anchor[e];
        pix = cons_surface(views[a], v.points[3 * (size_t)q], v.points[3 * (size_t)q + 1], v.points[3 * (size_t)q + 2], threshold);
        if (pix >= 0) st = (uint32_t)t;
    }
    const size_t g = (size_t)v.pixel_base + (size_t)q;
    step[g] = st;
    src_view[g] = a;
    src_pix[g] = pix;
}

// grid = (blocks of 256 pixels of the largest view, views)
__global__ void __launch_bounds__(256) cons_plane_resolve_kernel(const ConsPlaneView* __restrict__ views,
                                                                 const uint32_t* __restrict__ step,
                                                                 const int* __restrict__ src_view,
                                                                 const int* __restrict__ src_pix) {
    const ConsPlaneView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    // value(x, T) = value(src(x), step(x)) if step(x) < T, else original(x); T starts at "no step", above every step
    int w = (int)blockIdx.y, p = q;
    uint32_t T = CONS_NO_STEP;
    for (;;) {
        const size_t g = (size_t)views[w].pixel_base + (size_t)p;
        const uint32_t s = step[g];
        if (!(s < T)) break;  // T strictly decreases: the walk ends
        T = s;
        w = src_view[g];
        p = src_pix[g];
    }
    const unsigned char* im = views[w].image + 3 * (size_t)p;
    unsigned char* o = v.out + 3 * (size_t)q;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = im[c];
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

constexpr unsigned CONS_COUNT_BLOCKS = 256;

int check_threshold(float depth_threshold) {
    return depth_threshold == depth_threshold ? G4S_OK : fail(G4S_ERR_INVALID_ARGUMENT, "depth_threshold must not be NaN");
}

struct ConsPointsLayout {  // byte offsets into the workspace, after the view table
    std::vector<size_t> winner;  // per view; an input view has no winner map
    size_t bytes;
};
ConsPointsLayout cons_points_layout(int n_views, int n_input_views, const int* sizes) {  // sizes have passed view_sizes_ok
    ConsPointsLayout L{std::vector<size_t>((size_t)n_views, 0), 0};
    WorkspaceCursor c;
    take_view_table<ConsPointView>(c, n_views);
    for (int v = n_input_views; v < n_views; v++) L.winner[(size_t)v] = c.take((size_t)sizes[2 * v] * sizes[2 * v + 1] * 4);
    L.bytes = c.off;
    return L;
}

struct ConsCountsLayout { size_t ints, bytes; };  // ints: slot_plane [n_slots], then anchor_views [n_anchors]
ConsCountsLayout cons_counts_layout(int n_views, int n_slots, int n_anchors) {
    WorkspaceCursor c;
    take_view_table<ConsPlaneView>(c, n_views);
    const size_t ints = c.take(((size_t)n_slots + (size_t)n_anchors) * 4);
    return {ints, c.off};
}

struct ConsRepaintLayout { size_t ints, step, src_view, src_pix, bytes; };  // ints: slot_step, then slot_anchor [n_slots]
ConsRepaintLayout cons_repaint_layout(int n_views, int n_slots, long long total_pixels) {
    WorkspaceCursor c;
    take_view_table<ConsPlaneView>(c, n_views);
    const size_t ints = c.take((size_t)n_slots * 8), map = (size_t)total_pixels * 4;
    const size_t step = c.take(map), src_view = c.take(map), src_pix = c.take(map);
    return {ints, step, src_view, src_pix, c.off};
}

// The checks both plane entry points share.  *total_slots = slot_offset[n_views].
int check_plane_views(int n_views, const float* world_view, const float* focal, const float* const* depth,
                      const int* const* masks, const float* const* points, const int* slot_offset, int* total_slots) {
    *total_slots = 0;
    if (n_views == 0) return G4S_OK;
    if (!world_view || !focal) return null_pointer();
    if (check_pointers("depth", depth, n_views) != G4S_OK || check_pointers("masks", masks, n_views) != G4S_OK ||
        check_pointers("points", points, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!slot_offset) return fail(G4S_ERR_INVALID_ARGUMENT, "slot_offset: NULL array");
    if (slot_offset[0] != 0) return fail(G4S_ERR_INVALID_ARGUMENT, "slot_offset[0] must be 0");
    for (int v = 0; v < n_views; v++) {
        if (slot_offset[v + 1] <= slot_offset[v])
            return fail(G4S_ERR_INVALID_ARGUMENT, "slot_offset[%d]: every view has at least slot 0", v + 1);
    }
    *total_slots = slot_offset[n_views];
    return G4S_OK;
}

}  // namespace

extern "C" size_t g4s_consistency_points_workspace(int n_views, int n_input_views, const int* sizes) {
    long long largest, total;
    if (!grid_views_ok(n_views) || n_input_views < 0 || n_input_views > n_views || !view_sizes_ok(n_views, sizes, &largest, &total))
        return 0;
    return cons_points_layout(n_views, n_input_views, sizes).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_consistency_points(int n_points, const float* points, float depth_threshold, int n_views,
                                      int n_input_views, const float* world_view, const float* focal, const int* sizes,
                                      const float* const* depth, const float* const* images, const int* image_chw,
                                      float* const* images_out, unsigned char* const* conf, int resume, unsigned int* state,
                                      char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (n_points < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_points must be in 0 .. 2^31 - 1");
    if (check_threshold(depth_threshold) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_input_views < 0 || n_input_views > n_views)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_input_views must be in 0 .. n_views");
    if ((images_out == nullptr) != (conf == nullptr))
        return fail(G4S_ERR_INVALID_ARGUMENT, "images_out and conf must both be there or both be NULL");
    const bool outputs = images_out != nullptr;
    // the point pass: its state is wanted, or an inpainted view needs it
    const bool point_pass = n_points > 0 && n_views > 0 && (state != nullptr || (outputs && n_input_views < n_views));
    if (point_pass && !state) return fail(G4S_ERR_INVALID_ARGUMENT, "state: NULL, but an inpainted view needs the point pass");
    if (point_pass && !points) return fail(G4S_ERR_INVALID_ARGUMENT, "points: NULL pointer");
    if (n_views == 0) return G4S_OK;
    if (!world_view || !focal) return null_pointer();
    if (check_pointers("depth", depth, n_views) != G4S_OK || check_pointers("images", images, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!image_chw) return fail(G4S_ERR_INVALID_ARGUMENT, "image_chw: NULL array");
    if (outputs && (check_pointers("images_out", images_out, n_views) != G4S_OK || check_pointers("conf", conf, n_views) != G4S_OK))
        return G4S_ERR_INVALID_ARGUMENT;
    if (check_workspace(workspace, workspace_bytes, g4s_consistency_points_workspace(n_views, n_input_views, sizes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!outputs && !point_pass) return G4S_OK;
    // nothing below can fail a check: the first device call comes after every one of them
    const ConsPointsLayout L = cons_points_layout(n_views, n_input_views, sizes);
    char* ws = align_ptr(workspace);
    const ConsPointView* table;
    const int rc = stage_views("consistency points", n_views, true, sizes, depth, nullptr, false, workspace,
                               view_table_bytes<ConsPointView>(n_views), stream, &table, [&](ConsPointView& u, int v) {
                                   vis_pose(u, world_view, focal, v);
                                   const int W = sizes[2 * v], H = sizes[2 * v + 1];
                                   u.image = images[v];
                                   u.out = outputs ? images_out[v] : nullptr;
                                   u.conf = outputs ? conf[v] : nullptr;
                                   u.winner = outputs && point_pass && v >= n_input_views ? (uint32_t*)(ws + L.winner[(size_t)v]) : nullptr;
                                   u.pixel_stride = image_chw[v] ? 1 : 3;
                                   u.channel_stride = image_chw[v] ? W * H : 1;
                               });
    if (rc != G4S_OK) return rc;
    const dim3 pixel_grid(blocks256(largest), (unsigned)n_views);
    if (outputs) hipLaunchKernelGGL(cons_fill_kernel, pixel_grid, dim3(256), 0, stream, table);
    if (point_pass)
        hipLaunchKernelGGL(cons_point_kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, n_points, points, table, n_views,
                           n_input_views, depth_threshold, resume != 0, state);
    if (outputs) hipLaunchKernelGGL(cons_paint_kernel, pixel_grid, dim3(256), 0, stream, table, (const uint32_t*)state);
    return finish(hipSuccess, "consistency points");
}

extern "C" size_t g4s_consistency_plane_counts_workspace(int n_views, int n_slots, int n_anchors) {
    if (!grid_views_ok(n_views) || n_slots < 0 || n_anchors < 0) return 0;
    return cons_counts_layout(n_views, n_slots, n_anchors).bytes + VIEW_TABLE_SLACK + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_consistency_plane_counts(float depth_threshold, int n_views, const float* world_view, const float* focal,
                                            const int* sizes, const float* const* depth, const int* const* masks,
                                            const float* const* points, const int* slot_offset, const int* slot_plane,
                                            int n_planes, int n_anchors, const int* anchor_views, unsigned int* counts,
                                            char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_threshold(depth_threshold) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_planes < 0 || n_anchors < 0 || (long long)n_planes * n_anchors > (1ll << 30))
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_planes, n_anchors must not be negative and n_planes * n_anchors at most 2^30");
    if (n_anchors > 0 && !anchor_views) return fail(G4S_ERR_INVALID_ARGUMENT, "anchor_views: NULL array");
    for (int j = 0; j < n_anchors; j++) {
        if (anchor_views[j] < 0 || anchor_views[j] >= n_views)
            return fail(G4S_ERR_INVALID_ARGUMENT, "anchor_views[%d] must be a view index below n_views", j);
    }
    int n_slots;
    if (check_plane_views(n_views, world_view, focal, depth, masks, points, slot_offset, &n_slots) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_slots > 0 && !slot_plane) return fail(G4S_ERR_INVALID_ARGUMENT, "slot_plane: NULL array");
    for (int e = 0; e < n_slots; e++) {
        if (slot_plane[e] < -1 || slot_plane[e] >= n_planes)
            return fail(G4S_ERR_INVALID_ARGUMENT, "slot_plane[%d] must be -1 or a plane below n_planes", e);
    }
    const size_t n_counts = (size_t)n_planes * (size_t)n_anchors;
    if (n_counts == 0) return G4S_OK;
    if (!counts) return fail(G4S_ERR_INVALID_ARGUMENT, "counts: NULL pointer");
    if (check_workspace(workspace, workspace_bytes, g4s_consistency_plane_counts_workspace(n_views, n_slots, n_anchors)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    hipError_t e = hipMemsetAsync(counts, 0, n_counts * 4, stream);
    if (e != hipSuccess) return finish(e, "consistency plane counts");
    if (n_views == 0) return G4S_OK;
    int* ints = workspace_at<int>(workspace, cons_counts_layout(n_views, n_slots, n_anchors).ints);
    e = upload_pair(ints, slot_plane, n_slots, anchor_views, n_anchors, stream);
    if (e != hipSuccess) return finish(e, "consistency plane counts");
    const ConsPlaneView* table;
    const int rc = stage_views("consistency plane counts", n_views, true, sizes, depth, nullptr, false, workspace,
                               view_table_bytes<ConsPlaneView>(n_views), stream, &table, [&](ConsPlaneView& u, int v) {
                                   vis_pose(u, world_view, focal, v);
                                   u.mask = masks[v];
                                   u.points = points[v];
                                   u.image = nullptr;
                                   u.out = nullptr;
                                   u.slot_base = slot_offset[v];
                                   u.n_slots = slot_offset[v + 1] - slot_offset[v];
                                   u.pixel_base = 0u;
                                   u.pad_ = 0;
                               });
    if (rc != G4S_OK) return rc;
    const unsigned bx = blocks256(largest) < CONS_COUNT_BLOCKS ? blocks256(largest) : CONS_COUNT_BLOCKS;
    hipLaunchKernelGGL(cons_plane_count_kernel, dim3(bx, (unsigned)n_views), dim3(256), 0, stream, table, (const int*)ints,
                       n_anchors, (const int*)(ints + n_slots), depth_threshold, counts);
    return finish(hipSuccess, "consistency plane counts");
}

extern "C" size_t g4s_consistency_plane_repaint_workspace(int n_views, const int* sizes, int n_slots) {
    long long largest, total;
    if (!grid_views_ok(n_views) || n_slots < 0 || !view_sizes_ok(n_views, sizes, &largest, &total) || total >= (1ll << 31))
        return 0;
    return cons_repaint_layout(n_views, n_slots, total).bytes + VIEW_TABLE_SLACK + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_consistency_plane_repaint(float depth_threshold, int n_views, const float* world_view, const float* focal,
                                             const int* sizes, const float* const* depth, const int* const* masks,
                                             const float* const* points, const unsigned char* const* images,
                                             unsigned char* const* images_out, const int* slot_offset, const int* slot_step,
                                             const int* slot_anchor, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_threshold(depth_threshold) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (total >= (1ll << 31)) return fail(G4S_ERR_INVALID_ARGUMENT, "sizes: the views must have fewer than 2^31 pixels in all");
    int n_slots;
    if (check_plane_views(n_views, world_view, focal, depth, masks, points, slot_offset, &n_slots) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return G4S_OK;
    if (check_pointers("images", images, n_views) != G4S_OK || check_pointers("images_out", images_out, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!slot_step) return fail(G4S_ERR_INVALID_ARGUMENT, "slot_step: NULL array");
    if (!slot_anchor) return fail(G4S_ERR_INVALID_ARGUMENT, "slot_anchor: NULL array");
    for (int e = 0; e < n_slots; e++) {
        if (slot_step[e] < -1) return fail(G4S_ERR_INVALID_ARGUMENT, "slot_step[%d] must be -1 or a step", e);
        if (slot_step[e] >= 0 && (slot_anchor[e] < 0 || slot_anchor[e] >= n_views))
            return fail(G4S_ERR_INVALID_ARGUMENT, "slot_anchor[%d] must be a view index below n_views", e);
    }
    if (check_workspace(workspace, workspace_bytes, g4s_consistency_plane_repaint_workspace(n_views, sizes, n_slots)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const ConsRepaintLayout L = cons_repaint_layout(n_views, n_slots, total);
    int* ints = workspace_at<int>(workspace, L.ints);
    uint32_t* step = workspace_at<uint32_t>(workspace, L.step);
    int* src_view = workspace_at<int>(workspace, L.src_view);
    int* src_pix = workspace_at<int>(workspace, L.src_pix);
    const hipError_t e = upload_pair(ints, slot_step, n_slots, slot_anchor, n_slots, stream);
    if (e != hipSuccess) return finish(e, "consistency plane repaint");
    std::vector<uint32_t> pixel_base((size_t)n_views);
    uint32_t at = 0;
    for (int v = 0; v < n_views; v++) {
        pixel_base[(size_t)v] = at;
        at += (uint32_t)(sizes[2 * v] * sizes[2 * v + 1]);
    }
    const ConsPlaneView* table;
    const int rc = stage_views("consistency plane repaint", n_views, true, sizes, depth, nullptr, false, workspace,
                               view_table_bytes<ConsPlaneView>(n_views), stream, &table, [&](ConsPlaneView& u, int v) {
                                   vis_pose(u, world_view, focal, v);
                                   u.mask = masks[v];
                                   u.points = points[v];
                                   u.image = images[v];
                                   u.out = images_out[v];
                                   u.slot_base = slot_offset[v];
                                   u.n_slots = slot_offset[v + 1] - slot_offset[v];
                                   u.pixel_base = pixel_base[(size_t)v];
                                   u.pad_ = 0;
                               });
    if (rc != G4S_OK) return rc;
    const dim3 grid(blocks256(largest), (unsigned)n_views);
    hipLaunchKernelGGL(cons_plane_source_kernel, grid, dim3(256), 0, stream, table, (const int*)ints, (const int*)(ints + n_slots),
                       depth_threshold, step, src_view, src_pix);
    hipLaunchKernelGGL(cons_plane_resolve_kernel, grid, dim3(256), 0, stream, table, (const uint32_t*)step, (const int*)src_view,
                       (const int*)src_pix);
    return finish(hipSuccess, "consistency plane repaint");
}
