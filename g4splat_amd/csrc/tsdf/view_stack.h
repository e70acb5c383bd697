// What the two view-stack fields (unbounded.hip, tetra.hip) share: the tail of a view record, the bilinear tap into a
// view's maps, the staging of the view table into the caller's workspace with its size, and the point-sample kernel.
// A field differs in its matrices, in which points a view accepts and in its running-mean update; those stay in its unit.
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

// bytes of the workspace that holds a table of n_views records
template <class View>
size_t view_table_bytes(int n_views) {
    return (n_views > 0 ? (size_t)n_views * sizeof(View) : 0) + 256;  // + alignment of the base pointer
}

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
    hipError_t e = hipMemcpyAsync(dev, host.data(), host.size() * sizeof(View), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // `host` dies with this frame
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
    hipLaunchKernelGGL(kernel, dim3(((unsigned)n_points + 255u) / 256u), dim3(256), 0, stream, n_points, points, table,
                       n_views, a, tsdf, colour);
}

}  // namespace g4s
