// The warp initialiser (include/g4s_render_maps.h, "Warp surfels"; the semantics stated there are the contract,
// tests/warp_init_ref.py restates them in numpy): one surfel per pixel that no earlier view already explains under
// depth-consistent warping, views in order, kept pixels of a view in row-major order.
//
// Shape.  The coverage of view i reads only the depths and poses of the views j < i, so every view is independent: ONE
// launch over (view, lattice cell) with an inner loop over the earlier views.  A view has C = ceil(H/g) ceil(W/g) lattice
// cells and ceil(C / 256) workgroups of 256 consecutive row-major cells; views of different sizes share the launch through
// the first-workgroup number in every view record (ascending; the kernel finds its view by bisection, a wave-uniform walk
// over the table).  Workgroups are LAUNCHED in descending order, so the views with the most earlier views start first.
//   count: keep byte per cell -> __ballot -> popcount per workgroup  ->  scan_u32  ->  [host: n_rows]  ->  emit: re-reads
//   the keep bytes, row = workgroup base + the waves before + the kept lanes below, and writes the surfel.
// The emit kernel re-READS the keep bytes instead of re-deriving them: the rows cannot disagree with the count.
// The inner loop walks j = i-1 .. 0 (the order changes no bit: covered is an OR); a lane stops testing once it is covered
// and the wave leaves the loop when no lane is left.  Measured on tools/bench_warp_init.py's stack, whose poses are in random
// order, the two directions are within 1.5 % of each other; the nearest earlier view first is
// kept for captured sequences, where the neighbours in time overlap most.  The depth gathers of a wave fall on a short line of the target map
// and are left to L2; nothing is staged.  The points (five for the scale, four more for the normal) are formed in registers
// from the depth and the ray record; no point map is stored.
// No atomics; every output is a function of the inputs alone.
#include "../../../include/g4s_render_maps.h"
#include "scan.h"
#include "vis_view.h"

namespace g4s {

// Begins like VisView (vis_project reads R, T, fx, fy, maps).
struct WarpView {
    float R[9], T[3], fx, fy;
    VisRay ray;
    ViewMaps maps;        // depth [H,W]; rgb = the image [3,H,W] (emit) or NULL
    unsigned char* keep;  // [LH,LW]
    int LW, LH;           // the lattice: ceil(W / g), ceil(H / g)
    int first;            // the view's first workgroup in view order
};

struct WarpLayout {
    size_t table, counts, offs, chunks, words, bytes;
    long long cells, groups;  // over all views
};

inline int lattice(int n, int g) { return (n + g - 1) / g; }

// sizes are view_sizes_ok; g >= 1
static WarpLayout warp_layout(int V, const int* sizes, int g) {
    WarpLayout L{};
    for (int v = 0; v < V; v++) {
        const long long c = (long long)lattice(sizes[2 * v], g) * lattice(sizes[2 * v + 1], g);
        L.cells += c;
        L.groups += blocks256(c);
    }
    const size_t e = L.groups > 0 ? (size_t)L.groups : 1;
    WorkspaceCursor c;
    L.table = c.take((size_t)(V > 0 ? V : 1) * sizeof(WarpView));
    L.counts = c.take(e * 4);
    L.offs = c.take(e * 4);
    L.chunks = c.take((size_t)scan_chunks((long)e) * 4 + 4);
    L.words = c.take(64);  // [0] rows, [1] unused
    L.bytes = c.off;
    return L;
}

constexpr float WARP_EPS = 1e-12f;

// the NaN-propagating forms of this section (torch.min, torch.clamp): NOT the minNum / maxNum of the other sections
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ float at_least(float t, float lo) { return t < lo ? lo : t; }  // a NaN stays
__device__ __forceinline__ float sign_of(float t) { return t > 0.0f ? 1.0f : (t < 0.0f ? -1.0f : t); }  // 0 and a NaN stay

__device__ __forceinline__ float dist3(const float (&a)[3], const float (&b)[3]) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}
__device__ __forceinline__ void normalize3(float (&a)[3]) {
    const float d = at_least(sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]), WARP_EPS);
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = a[k] / d;
}
__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void warp_point(const WarpView& v, int x, int y, float (&p)[3]) {
    const int i = y * v.maps.W + x;
    pixel_point(v.ray, v.maps.W, i, v.maps.depth[i], p);
}

// s of the contract at pixel (x, y) whose point is P
__device__ __forceinline__ float warp_scale(const WarpView& v, int x, int y, const float (&P)[3], int grid) {
    const int W = v.maps.W, H = v.maps.H;
    float s = 1e-3f;
    if (W > 1 && H > 1) {
        float q[3];
        warp_point(v, x < W - 1 ? x + 1 : x - 1, y, q);  // the missing neighbour's distance is the opposite one's
        const float r = dist3(q, P);
        warp_point(v, x > 0 ? x - 1 : x + 1, y, q);
        const float l = dist3(P, q);
        warp_point(v, x, y < H - 1 ? y + 1 : y - 1, q);
        const float d = dist3(q, P);
        warp_point(v, x, y > 0 ? y - 1 : y + 1, q);
        const float u = dist3(P, q);
        s = min_nan(min_nan(min_nan(r, l), d), u);
    }
    s = s * 0.5f;
    return grid > 0 ? s * (float)grid : s;
}

// the view and the workgroup within it of launch position blockIdx.x: descending, the last view first
__device__ __forceinline__ int warp_find_view(const WarpView* __restrict__ views, int V, int block) {
    int lo = 0, hi = V - 1;  // views[lo].first <= block
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (views[mid].first <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) warp_count_kernel(const WarpView* __restrict__ views, int V, int groups, int grid,
                                                         float depth_error_thresh, float max_scale,
                                                         uint32_t* __restrict__ counts) {
    __shared__ uint32_t sm[4];
    const int block = groups - 1 - (int)blockIdx.x;
    const int i = warp_find_view(views, V, block);
    const WarpView& view = views[i];
    const int g = grid > 0 ? grid : 1;
    const int c = (block - view.first) * 256 + (int)threadIdx.x;
    const bool inside = c < view.LW * view.LH;
    bool open = false;  // a candidate below the scale cut that no view has covered yet
    float P[3] = {0.0f, 0.0f, 0.0f};
    if (inside) {
        const int y = (c / view.LW) * g, x = (c % view.LW) * g;
        if (view.maps.depth[y * view.maps.W + x] > 0.0f) {
            warp_point(view, x, y, P);
            open = warp_scale(view, x, y, P, grid) < max_scale;
        }
    }
    for (int j = i - 1; j >= 0; j--) {  // wave-uniform
        if (__ballot(open) == 0ull) break;
        if (open) {
            const WarpView& t = views[j];
            VisProj q;
            vis_project(t, P[0], P[1], P[2], q);
            const int W = t.maps.W, H = t.maps.H;
            if (q.u >= 0.0f && q.u <= (float)(W - 1) && q.v >= 0.0f && q.v <= (float)(H - 1) && q.z > 0.0f) {
                const float d = t.maps.depth[(size_t)(int)rintf(q.v) * W + (int)rintf(q.u)];
                if (d > 0.0f && vis_surface(q.z, d, depth_error_thresh)) open = false;
            }
        }
    }
    if (inside) view.keep[c] = open ? 1 : 0;
    const unsigned long long w = __ballot(open);
    if (lane_id() == 0) sm[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(w);
    __syncthreads();
    if (threadIdx.x == 0) counts[block] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// The surfel of the contract for the kept pixel (x, y) of `view`, written to row `row`.
__device__ __forceinline__ void warp_surfel(const WarpView& view, int x, int y, int grid, float min_scale, size_t row,
                                            float* __restrict__ means, float* __restrict__ scales, float* __restrict__ quats,
                                            float* __restrict__ colors) {
    const int W = view.maps.W, H = view.maps.H;
    float P[3];
    warp_point(view, x, y, P);
    const float s = at_least(warp_scale(view, x, y, P, grid), min_scale);
    float n[3] = {0.0f, 0.0f, 1.0f};
    if (H >= 3 && W >= 3) {
        const int sy = imin_(imax_(y, 1), H - 2), sx = imin_(imax_(x, 1), W - 2);
        float a[3], b[3], dy[3], dx[3];
        warp_point(view, sx, sy + 1, a);
        warp_point(view, sx, sy - 1, b);
#pragma unroll
        for (int k = 0; k < 3; k++) dy[k] = a[k] - b[k];
        warp_point(view, sx + 1, sy, a);
        warp_point(view, sx - 1, sy, b);
#pragma unroll
        for (int k = 0; k < 3; k++) dx[k] = a[k] - b[k];
        cross3(dy, dx, n);
        normalize3(n);
    }
    float z[3] = {n[0], n[1], n[2]};
    normalize3(z);
    const bool par = fabsf(z[0]) > 0.9f;
    const float ref[3] = {par ? 0.0f : 1.0f, par ? 1.0f : 0.0f, 0.0f};
    float xa[3], ya[3];
    cross3(ref, z, xa);
    normalize3(xa);
    cross3(z, xa, ya);
    // the matrix has the columns (xa, ya, z): m_ij = column j, component i
    const float m00 = xa[0], m01 = ya[0], m02 = z[0];
    const float m10 = xa[1], m11 = ya[1], m12 = z[1];
    const float m20 = xa[2], m21 = ya[2], m22 = z[2];
    float q[4];
    q[0] = sqrtf(at_least(((1.0f + m00) + m11) + m22, 0.0f)) / 2.0f;
    q[1] = sqrtf(at_least(((1.0f + m00) - m11) - m22, 0.0f)) / 2.0f;
    q[2] = sqrtf(at_least(((1.0f - m00) + m11) - m22, 0.0f)) / 2.0f;
    q[3] = sqrtf(at_least(((1.0f - m00) - m11) + m22, 0.0f)) / 2.0f;
    q[1] = q[1] * sign_of((m21 - m12) + WARP_EPS);
    q[2] = q[2] * sign_of((m02 - m20) + WARP_EPS);
    q[3] = q[3] * sign_of((m10 - m01) + WARP_EPS);
    const float d = at_least(sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]), WARP_EPS);
    const size_t pixel = (size_t)y * W + x, plane = (size_t)H * W;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        means[3 * row + k] = P[k];
        colors[3 * row + k] = view.maps.rgb[k * plane + pixel];
    }
    scales[2 * row] = s;
    scales[2 * row + 1] = s;
#pragma unroll
    for (int k = 0; k < 4; k++) quats[4 * row + k] = q[k] / d;
}

__global__ void __launch_bounds__(256) warp_emit_kernel(const WarpView* __restrict__ views, int V, int groups, int grid,
                                                        float min_scale, const uint32_t* __restrict__ offs, uint32_t n_rows,
                                                        float* __restrict__ means, float* __restrict__ scales,
                                                        float* __restrict__ quats, float* __restrict__ colors) {
    __shared__ uint32_t sm[4];
    const int block = (int)blockIdx.x;
    const int i = warp_find_view(views, V, block);
    const WarpView& view = views[i];
    const int g = grid > 0 ? grid : 1;
    const int c = (block - view.first) * 256 + (int)threadIdx.x;
    const bool kept = c < view.LW * view.LH && view.keep[c] != 0;
    const unsigned long long w = __ballot(kept);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (lane == 0) sm[wave] = (uint32_t)__builtin_popcountll(w);
    __syncthreads();
    if (!kept) return;
    uint32_t row = offs[block] + (uint32_t)__builtin_popcountll(w & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; k++) row += sm[k];
    if (row >= n_rows) return;  // the caller's capacity
    warp_surfel(view, (c % view.LW) * g, (c / view.LW) * g, grid, min_scale, row, means, scales, quats, colors);
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

// the sizes are those of a view stack and the lattice cells of all views stay below 2^31
bool warp_sizes_ok(int V, const int* sizes, int g) {
    long long largest, total;
    if (!view_sizes_ok(V, sizes, &largest, &total)) return false;
    long long cells = 0;
    for (int v = 0; v < V; v++) {
        cells += (long long)lattice(sizes[2 * v], g) * lattice(sizes[2 * v + 1], g);
        if (cells >= (1ll << 31)) return false;
    }
    return true;
}

int check_warp_sizes(int V, const int* sizes, int g) {
    if (V < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_views must not be negative");
    if (V > 0 && !sizes) return null_pointer();
    if (!warp_sizes_ok(V, sizes, g))
        return fail(G4S_ERR_INVALID_ARGUMENT,
                    "sizes: width, height must be positive, width * height at most 2^30 and the lattice cells of all views below 2^31");
    return G4S_OK;
}

// the view table of both phases
int warp_table(const char* name, int V, const float* world_view, const float* focal, const int* sizes, const float* const* depth,
               const float* rays, const float* const* images, unsigned char* const* keep, int g, char* workspace,
               size_t workspace_bytes, hipStream_t stream, const WarpView** table) {
    int first = 0;
    return stage_views(name, V, world_view && focal && rays, sizes, depth, images, images != nullptr, workspace, workspace_bytes,
                       stream, table, [&](WarpView& u, int v) {
                           vis_pose(u, world_view, focal, v);
                           u.ray = ray_record(rays + 12 * (size_t)v);
                           u.keep = keep[v];
                           u.LW = lattice(sizes[2 * v], g);
                           u.LH = lattice(sizes[2 * v + 1], g);
                           u.first = first;
                           first += (int)blocks256((long long)u.LW * u.LH);
                       });
}

}  // namespace

extern "C" size_t g4s_warp_init_workspace(int n_views, const int* sizes, int grid) {
    const int g = grid > 0 ? grid : 1;
    if (n_views < 0 || !warp_sizes_ok(n_views, sizes, g)) return 0;
    return warp_layout(n_views, sizes, g).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_warp_init_count(int n_views, const float* world_view, const float* focal, const int* sizes,
                                   const float* const* depth, const float* rays, int grid, float depth_error_thresh,
                                   float max_scale, unsigned char* const* keep, int* n_rows, char* workspace,
                                   size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    const int g = grid > 0 ? grid : 1;
    if (check_warp_sizes(n_views, sizes, g) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!n_rows) return null_pointer();
    *n_rows = 0;
    if (n_views == 0) return G4S_OK;
    if (!world_view || !focal || !rays) return null_pointer();
    if (check_pointers("depth", depth, n_views) != G4S_OK || check_pointers("keep", keep, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (check_workspace(workspace, workspace_bytes, g4s_warp_init_workspace(n_views, sizes, grid)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const WarpLayout L = warp_layout(n_views, sizes, g);
    char* ws = align_ptr(workspace);
    uint32_t* words = (uint32_t*)(ws + L.words);
    uint32_t* counts = (uint32_t*)(ws + L.counts);
    hipError_t e = hipMemsetAsync(words, 0, 64, s);
    if (e != hipSuccess) return finish(e, "warp init count");
    const WarpView* table;
    const int rc = warp_table("warp init count", n_views, world_view, focal, sizes, depth, rays, nullptr, keep, g, workspace,
                              workspace_bytes, s, &table);
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(warp_count_kernel, dim3((unsigned)L.groups), dim3(256), 0, s, table, n_views, (int)L.groups, grid,
                       depth_error_thresh, max_scale, counts);
    scan_u32(counts, (uint32_t*)(ws + L.offs), (int)L.groups, (uint32_t*)(ws + L.chunks), words + 0, s);
    int t[2];
    e = read_totals(words, t, s);
    if (e != hipSuccess) return finish(e, "warp init count");
    *n_rows = t[0];
    return finish(hipSuccess, "warp init count");
}

extern "C" int g4s_warp_init_emit(int n_views, const float* world_view, const float* focal, const int* sizes,
                                  const float* const* depth, const float* rays, const float* const* images, int grid,
                                  float min_scale, const unsigned char* const* keep, int n_rows, float* means, float* scales,
                                  float* quaternions, float* colors, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    const int g = grid > 0 ? grid : 1;
    if (check_warp_sizes(n_views, sizes, g) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const WarpLayout L = warp_layout(n_views, sizes, g);
    if (n_rows < 0 || n_rows > L.cells)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_rows must lie in 0 .. the lattice cells of all views");
    if (n_rows == 0) return G4S_OK;
    if (!world_view || !focal || !rays || !means || !scales || !quaternions || !colors) return null_pointer();
    if (check_pointers("depth", depth, n_views) != G4S_OK || check_pointers("images", images, n_views) != G4S_OK ||
        check_pointers("keep", keep, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (check_workspace(workspace, workspace_bytes, g4s_warp_init_workspace(n_views, sizes, grid)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    char* ws = align_ptr(workspace);
    const WarpView* table;
    const int rc = warp_table("warp init emit", n_views, world_view, focal, sizes, depth, rays, images,
                              (unsigned char* const*)keep, g, workspace, workspace_bytes, s, &table);
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(warp_emit_kernel, dim3((unsigned)L.groups), dim3(256), 0, s, table, n_views, (int)L.groups, grid,
                       min_scale, (const uint32_t*)(ws + L.offs), (uint32_t)n_rows, means, scales, quaternions, colors);
    return finish(hipSuccess, "warp init emit");
}
