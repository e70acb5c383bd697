// What the units over the Visibility section's views share.  visibility.hip, planes.hip, consistency.hip, view_select.hip: the
// head of a view record -- world -> camera rotation, translation, focal lengths, then view_stack.h's maps --, its fill from
// the host arrays, THE projection of include/g4s_render_maps.h ("Projection of a point p into a view"), its truncating tap and
// the SURFACE test.  visibility.hip, depth_cues.hip, chart_init.hip, warp_init.hip: the ray record with THE back-projection
// (warp_init.hip reads both halves: it projects the points it back-projects).  There is no
// second one of any of them.  The host checks and the table's staging that all six share are view_stack.h's.
#pragma once
#include "view_stack.h"

namespace g4s {

// One view of the stack as the visibility kernels read it (80 bytes; the table is an array of these in the workspace).
// A unit that needs more per view declares a record that begins with the same fields (planes.hip, consistency.hip).
struct VisView {
    float R[9];  // world -> camera rotation, R[3 j + i] = world_view_transform[i][j]
    float T[3];  // world_view_transform[3][j]
    float fx, fy;
    ViewMaps maps;
};
static_assert(sizeof(VisView) == 80, "g4s_visgrid_workspace is stated in records of 80 bytes");

// z = c_2 and the image coordinates (u, v) of the contract
struct VisProj {
    float z, u, v;
};

// The projection; true iff the point is "in image" (every comparison with a NaN is false).  View: R, T, fx, fy, maps.
template <class View>
__device__ __forceinline__ bool vis_project(const View& v, float px, float py, float pz, VisProj& q) {
    const float x = ((px * v.R[0] + py * v.R[1]) + pz * v.R[2]) + v.T[0];
    const float y = ((px * v.R[3] + py * v.R[4]) + pz * v.R[5]) + v.T[1];
    const float z = ((px * v.R[6] + py * v.R[7]) + pz * v.R[8]) + v.T[2];
    const int W = v.maps.W, H = v.maps.H;
    const float a = (x / z) * v.fx + (float)W * 0.5f;
    const float b = (y / z) * v.fy + (float)H * 0.5f;
    q = VisProj{z, a, b};
    return a >= 0.0f && a < (float)W && b >= 0.0f && b < (float)H;
}

// The truncating tap of a point that is in the image: the row-major index of depth[min(int(v), H-1)][min(int(u), W-1)].
template <class View>
__device__ __forceinline__ size_t vis_tap(const View& v, const VisProj& q) {
    return (size_t)imin_((int)q.v, v.maps.H - 1) * v.maps.W + imin_((int)q.u, v.maps.W - 1);
}

// SURFACE of a point in the image with depth z whose tap reads d
__device__ __forceinline__ bool vis_surface(float z, float d, float threshold) {
    return z > 0.0f && fabsf(z - d) / (z + 1e-6f) < threshold;
}

// host: the pose fields of view v's record from world_view [V,16] and focal [V,2]
template <class View>
inline void vis_pose(View& u, const float* world_view, const float* focal, int v) {
    const float* M = world_view + 16 * (size_t)v;
    for (int j = 0; j < 3; j++) {
        for (int i = 0; i < 3; i++) u.R[3 * j + i] = M[4 * i + j];
        u.T[j] = M[12 + j];
    }
    u.fx = focal[2 * (size_t)v];
    u.fy = focal[2 * (size_t)v + 1];
}

// The ray record of the contract ("Ray record of a camera"): origin, then D row-major.
struct VisRay {
    float o[3], D[9];
};
// host: ray != NULL, the twelve floats of a ray record
inline VisRay ray_record(const float* ray) {
    VisRay r;
    for (int i = 0; i < 3; i++) r.o[i] = ray[i];
    for (int i = 0; i < 9; i++) r.D[i] = ray[3 + i];
    return r;
}

// dir = D (x, y, 1) at integer pixel coordinates
__device__ __forceinline__ void ray_dir(const VisRay& r, int x, int y, float (&dir)[3]) {
    const float xf = (float)x, yf = (float)y;
#pragma unroll
    for (int c = 0; c < 3; c++) dir[c] = (r.D[3 * c] * xf + r.D[3 * c + 1] * yf) + r.D[3 * c + 2];
}

// THE back-projection: the point of pixel i = y * W + x at depth d (g4s_depth_to_points, the pixel view counts, the depth cues)
__device__ __forceinline__ void pixel_point(const VisRay& ray, int W, int i, float d, float (&p)[3]) {
    float dir[3];
    ray_dir(ray, i % W, i / W, dir);
#pragma unroll
    for (int c = 0; c < 3; c++) p[c] = ray.o[c] + d * dir[c];
}

}  // namespace g4s
