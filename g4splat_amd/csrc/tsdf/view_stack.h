// What the units over a stack of views share.  All of them -- the two fields (unbounded.hip, tetra.hip) and, through
// vis_view.h, visibility.hip, planes.hip, consistency.hip, view_select.hip, depth_cues.hip, chart_init.hip, warp_init.hip, plane_masks.hip --: the tail of a
// view record, the host checks of a view stack, and the staging of the view table into the caller's workspace with its size.
// The two fields alone: the bilinear tap and the point-sample kernel; a field differs in its matrices, in which points a view
// accepts and in its running-mean update, and those stay in its unit.
#pragma once
#include <vector>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "mesh_common.h"

namespace g4s {

// The tail of every view record, after the field's matrices.
struct ViewMaps {
    int W, H;
    const float* depth;  // [H,W]
    const float* rgb;    // [3,H,W] or NULL (no colour output)
};

// The four texels around (ix, iy) and their weights.  The caller has established 0 <= ix <= W-1 and 0 <= iy <= H-1; the
// clamps never change a value and keep every tap inside the map.
struct ViewTap {
    size_t i00, i10, i01, i11;
    float w00, w10, w01, w11;
    __device__ __forceinline__ ViewTap(float ix, float iy, int W, int H) {
        const float fx0 = floorf(ix), fy0 = floorf(iy);
        const int x0 = imin_(imax_((int)fx0, 0), W - 1), y0 = imin_(imax_((int)fy0, 0), H - 1);
        const int x1 = imin_(x0 + 1, W - 1), y1 = imin_(y0 + 1, H - 1);
        const float fx = ix - fx0, fy = iy - fy0;
        w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
        i00 = (size_t)y0 * W + x0, i10 = (size_t)y0 * W + x1, i01 = (size_t)y1 * W + x0, i11 = (size_t)y1 * W + x1;
    }
    // one [H,W] plane at the tap
    __device__ __forceinline__ float blend(const float* P) const {
        return ((P[i00] * w00 + P[i10] * w10) + P[i01] * w01) + P[i11] * w11;
    }
};

// ---- host checks of a view stack ----
constexpr int GRID_MAX_VIEWS = 65535;  // where the views are the grid's y
inline bool grid_views_ok(int n_views) { return n_views >= 0 && n_views <= GRID_MAX_VIEWS; }

// The sizes [n_views,2] = (W, H) are there and positive with W * H at most 2^30: the largest pixel count of the views and
// the sum of the counts.  No cap on n_views: that is grid_views_ok, for the units it binds.
inline bool view_sizes_ok(int n_views, const int* sizes, long long* largest, long long* total) {
    *largest = *total = 0;
    if (n_views < 0 || (n_views > 0 && !sizes)) return false;
    for (int v = 0; v < n_views; v++) {
        const long long W = sizes[2 * v], H = sizes[2 * v + 1];
        if (W <= 0 || H <= 0 || W * H > (1ll << 30)) return false;
        *total += W * H;
        if (W * H > *largest) *largest = W * H;
    }
    return true;
}
// the same with the grid cap and the messages; a unit with a wording of its own calls the bool form
inline int check_grid_views(int n_views, const int* sizes, long long* largest, long long* total) {
    if (!grid_views_ok(n_views)) return fail(G4S_ERR_INVALID_ARGUMENT, "n_views must be in 0 .. 65535");
    if (view_sizes_ok(n_views, sizes, largest, total)) return G4S_OK;
    if (!sizes) return null_pointer();
    return fail(G4S_ERR_INVALID_ARGUMENT, "sizes: width, height must be positive and width * height at most 2^30");
}
// a host pointer array with one non-NULL entry per view
template <class T>
int check_pointers(const char* name, T* const* a, int n_views) {
    if (!a) return fail(G4S_ERR_INVALID_ARGUMENT, "%s: NULL array", name);
    for (int v = 0; v < n_views; v++) {
        if (!a[v]) return fail(G4S_ERR_INVALID_ARGUMENT, "%s[%d]: NULL pointer", name, v);
    }
    return G4S_OK;
}

// ---- the view table in the workspace ----
// bytes of the workspace that holds a table of n_views records
template <class View>
size_t view_table_bytes(int n_views) {
    return (n_views > 0 ? (size_t)n_views * sizeof(View) : 0) + WORKSPACE_BASE_SLACK;
}
// The table in a layout that holds more: stage_views puts it at the aligned base, so a layout takes this range first.
template <class View>
void take_view_table(WorkspaceCursor& c, int n_views) { c.take(n_views > 0 ? (size_t)n_views * sizeof(View) : 0); }
// Some queries were stated as align_up(view_table_bytes) + ... + 256 and so count the base alignment twice.  Callers size
// buffers by them: those queries add this to their layout besides WORKSPACE_BASE_SLACK.
constexpr size_t VIEW_TABLE_SLACK = 256;

// Checks the view stack, builds the table on the host and copies it into the workspace.  `matrices` says that the
// field's matrix arrays are there; fill(record, v) copies those of view v.  `name` opens the message of a failed upload.
template <class View, class Fill>
int stage_views(const char* name, int n_views, bool matrices, const int* sizes, const float* const* depth,
                const float* const* rgb, bool need_rgb, char* workspace, size_t workspace_bytes, hipStream_t stream,
                const View** table, Fill fill) {
    if (n_views < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_views must not be negative");
    *table = nullptr;
    if (n_views == 0) return G4S_OK;
    if (!matrices || !sizes || !depth || (need_rgb && !rgb)) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, view_table_bytes<View>(n_views)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    std::vector<View> host((size_t)n_views);
    for (int v = 0; v < n_views; v++) {
        View& u = host[(size_t)v];
        const int W = sizes[2 * v], H = sizes[2 * v + 1];
        if (W <= 0 || H <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "view %d: width, height must be positive", v);
        if (!depth[v] || (need_rgb && !rgb[v])) return fail(G4S_ERR_INVALID_ARGUMENT, "view %d: NULL map pointer", v);
        fill(u, v);
        u.maps = ViewMaps{W, H, depth[v], need_rgb ? rgb[v] : nullptr};
    }
    View* dev = (View*)align_ptr(workspace);
    const hipError_t e = upload(dev, host.data(), host.size() * sizeof(View), stream);  // `host` dies with this frame
    if (e != hipSuccess) return fail(G4S_ERR_HIP, "%s view table: %s", name, hipGetErrorString(e));
    *table = dev;
    return G4S_OK;
}

// The field of a whole view stack at explicit points, one thread per point.  Field names the record (View), the point
// state (Point), the by-value parameter block (Params) and two static __device__ functions: init(s, x, y, z, a) and
// view<RGB>(s, record, a).
template <class Field, bool RGB>
__global__ void __launch_bounds__(256) point_sample_kernel(int n, const float* __restrict__ points,
                                                           const typename Field::View* __restrict__ views, int n_views,
                                                           typename Field::Params a, float* __restrict__ tsdf,
                                                           float* __restrict__ colour) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    typename Field::Point s;
    Field::init(s, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], a);
    for (int v = 0; v < n_views; v++) Field::template view<RGB>(s, views[v], a);
    if (tsdf != nullptr) tsdf[i] = s.tsdf;
    if (RGB) {
#pragma unroll
        for (int c = 0; c < 3; c++) colour[3 * (size_t)i + c] = s.col[c];
    }
}

// n_points > 0; the colour instantiation runs iff `colour` is there
template <class Field>
void launch_point_sample(int n_points, const float* points, const typename Field::View* table, int n_views,
                         const typename Field::Params& a, float* tsdf, float* colour, hipStream_t stream) {
    const auto kernel = colour ? point_sample_kernel<Field, true> : point_sample_kernel<Field, false>;
    hipLaunchKernelGGL(kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, n_points, points, table,
                       n_views, a, tsdf, colour);
}

}  // namespace g4s
