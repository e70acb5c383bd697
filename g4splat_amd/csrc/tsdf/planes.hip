// Global 3D planes (include/g4s_render_maps.h, "Global planes"; the semantics stated there are the contract,
// tests/planes_ref.py restates them in numpy): which points of a chart cloud each view's plane mask claims, and the integer
// counts the covisibility merge decides on.
//
// Two facts make the merge cheap (g4splat_amd/planes.py decides on the host, tests/planes_ref.py asserts both):
//   1. The local planes of one view are disjoint: a point has at most one label per view.  Absorbing S_p into G_g therefore
//      leaves |G_g' ∩ S_q| unchanged for every other local plane q of that view and every g', so ONE overlap launch per view
//      yields every count its sequential decisions need; sizes follow |G ∪ S| = |G| + |S| - |G ∩ S|.
//   2. The final sweep does not decompose like that: after a merge the counts against the grown row are needed, which is
//      one row-overlap launch per sweep step.
//
// Labels:   one thread per point walks the view table (vis_view.h: THE projection, records read wave-uniformly).  Pass 1
//           takes the per-pixel minimum of z over the candidates as an unsigned atomic min of the float's bits (z > 0, so
//           the bits order like the values; any execution order gives the same word).  Pass 2 projects again -- 12 bytes of
//           point against 8 bytes per (point, view) of a stored pixel and depth -- and writes the mask value or 0.
// Membership: point i's word w holds global planes 64 w .. 64 w + 63 and sits at member[w * N + i]: every kernel reads and
//           writes it coalesced, a thread owns its point's words (no atomics on the membership, ever), and capacity grows
//           by whole blocks of N words.
// Counts:   integer.  A wave first folds its lanes' equal keys (ballot), the first lane of each key adds the population
//           count with one integer atomic -- into the workgroup's table in LDS when the table fits, which a capped grid
//           flushes with one global atomic per non-zero entry; integer sums do not depend on the order.  No float
//           atomics anywhere.
#include <math.h>

#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "vis_view.h"
#include "wave_count.h"

namespace g4s {

// VisView's fields (vis_project and stage_views read them by name), then this unit's own.  The map of a plane view is its
// int32 slot mask: the table keeps its address in maps.depth, mask_of() gives it back its type.
struct PlaneView {
    float R[9];
    float T[3];
    float fx, fy;
    ViewMaps maps;
    uint32_t* zmin;  // [H,W] float bits, in the workspace
};
static_assert(sizeof(PlaneView) == 88, "g4s_plane_labels_workspace is stated in records of 88 bytes");

__device__ __forceinline__ const int* mask_of(const PlaneView& v) { return (const int*)v.maps.depth; }

// The pixel of candidate point i in view v (row-major index) and its z; -1 if the point is no candidate.
__device__ __forceinline__ int plane_pixel(const PlaneView& v, int i, float px, float py, float pz, float& z) {
    VisProj q;
    if (i == 0 || !vis_project(v, px, py, pz, q) || !(q.z > 0.0f)) return -1;
    // in image: 0 <= u < W, so rint(u) is in 0 .. W
    const int x = imin_((int)rintf(q.u), v.maps.W - 1), y = imin_((int)rintf(q.v), v.maps.H - 1);
    z = q.z;
    return y * v.maps.W + x;
}

__global__ void __launch_bounds__(256) plane_zmin_kernel(int n, const float* __restrict__ points,
                                                         const PlaneView* __restrict__ views, int n_views) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const float px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
    for (int v = 0; v < n_views; v++) {
        float z;
        const int pix = plane_pixel(views[v], i, px, py, pz, z);
        if (pix < 0) continue;
        uint32_t* cell = views[v].zmin + pix;
        const uint32_t bits = __float_as_uint(z);
        // the cell only ever decreases: a value read here is an upper bound of the final one, so skipping is safe
        if (bits < *(volatile uint32_t*)cell) atomicMin(cell, bits);
    }
}

__global__ void __launch_bounds__(256) plane_label_kernel(int n, const float* __restrict__ points,
                                                          const PlaneView* __restrict__ views, int n_views,
                                                          float depth_thresh, int depth_test, int* __restrict__ labels) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const float px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
    for (int v = 0; v < n_views; v++) {
        float z;
        const int pix = plane_pixel(views[v], i, px, py, pz, z);
        int label = 0;
        if (pix >= 0 && (!depth_test || z < __uint_as_float(views[v].zmin[pix]) + depth_thresh)) label = mask_of(views[v])[pix];
        labels[(size_t)v * (size_t)n + (size_t)i] = label;
    }
}

// the bits of word w that name a global plane below n_global
__device__ __forceinline__ unsigned long long word_planes(int w, int n_global) {
    const int left = n_global - 64 * w;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
}

// table[base + 64 w + b] += 1 for every set bit b of m (m = 0 in lanes that take no part); wave-uniform control flow
__device__ __forceinline__ void wave_count_bits(uint32_t* __restrict__ table, uint32_t base, int w, unsigned long long m) {
    while (__ballot(m != 0ull) != 0ull) {
        const bool a = m != 0ull;
        const uint32_t b = a ? (uint32_t)__builtin_ctzll(m) : 0u;
        wave_count(table, base + 64u * (uint32_t)w + b, a);
        m &= m - 1ull;
    }
}

// A workgroup's count table: in LDS when it has at most COUNT_LDS_MAX entries -- a capped grid walks the points, the waves
// add into LDS and every workgroup ends with one global atomic per non-zero entry, so a hot entry sees at most
// COUNT_MAX_BLOCKS global atomics instead of one per wave -- and the global table itself otherwise.
constexpr int COUNT_LDS_MAX = 8192;  // 32 KiB
constexpr unsigned COUNT_MAX_BLOCKS = 2048;

__device__ __forceinline__ void lds_table_clear(uint32_t* lds, int entries) {
    for (int k = (int)threadIdx.x; k < entries; k += 256) lds[k] = 0u;
    __syncthreads();
}
__device__ __forceinline__ void lds_table_flush(const uint32_t* lds, uint32_t* __restrict__ table, int entries) {
    for (int k = (int)threadIdx.x; k < entries; k += 256) {
        const uint32_t c = lds[k];
        if (c != 0u) atomicAdd(table + k, c);
    }
}

// grid-stride over blocks of 256 points; no early return, the waves vote.  LDS: dynamic shared memory of
// (n_planes * n_global + n_planes) words.
template <bool LDS>
__global__ void __launch_bounds__(256) plane_overlap_kernel(int n, const int* __restrict__ labels, int n_planes, int n_global,
                                                            int n_words, const unsigned long long* __restrict__ member,
                                                            uint32_t* __restrict__ counts, uint32_t* __restrict__ sizes) {
    extern __shared__ uint32_t lds_table[];
    const int n_counts = n_planes * n_global;
    uint32_t* ct = LDS ? lds_table : counts;
    uint32_t* st = LDS ? lds_table + n_counts : sizes;
    if (LDS) lds_table_clear(lds_table, n_counts + n_planes);
    for (int first = (int)(blockIdx.x * 256u); first < n; first += (int)(gridDim.x * 256u)) {  // n <= 2^30: no overflow
        const int i = first + (int)threadIdx.x;
        const int p = i < n ? labels[i] : 0;
        const bool labelled = p >= 1 && p <= n_planes;
        wave_count(st, (uint32_t)(p - 1), labelled);
        if (__ballot(labelled) == 0ull) continue;
        const uint32_t base = labelled ? (uint32_t)(p - 1) * (uint32_t)n_global : 0u;
        for (int w = 0; w < n_words; w++) {
            const unsigned long long m = labelled ? member[(size_t)w * (size_t)n + (size_t)i] & word_planes(w, n_global) : 0ull;
            wave_count_bits(ct, base, w, m);
        }
    }
    if (LDS) {
        __syncthreads();
        lds_table_flush(lds_table, counts, n_counts);
        lds_table_flush(lds_table + n_counts, sizes, n_planes);
    }
}

__global__ void __launch_bounds__(256) plane_assign_kernel(int n, const int* __restrict__ labels, int n_planes,
                                                           const int* __restrict__ target,
                                                           unsigned long long* __restrict__ member) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int p = labels[i];
    if (p < 1 || p > n_planes) return;
    const int t = target[p - 1];  // checked on the host: -1 or below 64 * n_words
    if (t < 0) return;
    member[(size_t)(t >> 6) * (size_t)n + (size_t)i] |= 1ull << (t & 63);
}

__device__ __forceinline__ bool member_bit(const unsigned long long* __restrict__ member, int n, int row, int i) {
    return (member[(size_t)(row >> 6) * (size_t)n + (size_t)i] >> (row & 63)) & 1ull;
}

// LDS: dynamic shared memory of n_global words
template <bool LDS>
__global__ void __launch_bounds__(256) plane_row_overlap_kernel(int n, int n_global, int n_words,
                                                                const unsigned long long* __restrict__ member, int row,
                                                                uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t lds_table[];
    uint32_t* ct = LDS ? lds_table : counts;
    if (LDS) lds_table_clear(lds_table, n_global);
    for (int first = (int)(blockIdx.x * 256u); first < n; first += (int)(gridDim.x * 256u)) {
        const int i = first + (int)threadIdx.x;
        const bool in_row = i < n && member_bit(member, n, row, i);
        if (__ballot(in_row) == 0ull) continue;
        for (int w = 0; w < n_words; w++) {
            const unsigned long long m = in_row ? member[(size_t)w * (size_t)n + (size_t)i] & word_planes(w, n_global) : 0ull;
            wave_count_bits(ct, 0u, w, m);
        }
    }
    if (LDS) {
        __syncthreads();
        lds_table_flush(lds_table, counts, n_global);
    }
}

__global__ void __launch_bounds__(256) plane_row_merge_kernel(int n, unsigned long long* __restrict__ member, int src, int dst) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n || !member_bit(member, n, src, i)) return;
    member[(size_t)(dst >> 6) * (size_t)n + (size_t)i] |= 1ull << (dst & 63);
}

__global__ void __launch_bounds__(256) plane_row_mask_kernel(int n, const unsigned long long* __restrict__ member, int row,
                                                             unsigned char* __restrict__ mask) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < n) mask[i] = member_bit(member, n, row, i) ? 1 : 0;
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

int check_points(int n_points) {
    return n_points >= 0 && n_points <= (1 << 30) ? G4S_OK : fail(G4S_ERR_INVALID_ARGUMENT, "n_points must be in 0 .. 2^30");
}

struct PlaneLabelsLayout {  // byte offsets into the workspace, after the view table
    std::vector<size_t> zmin;  // per view; the maps are one run, from zmin[0] to the end
    size_t bytes;
};
PlaneLabelsLayout plane_labels_layout(int n_views, const int* sizes) {  // sizes have passed view_sizes_ok
    PlaneLabelsLayout L{std::vector<size_t>((size_t)n_views), 0};
    WorkspaceCursor c;
    take_view_table<PlaneView>(c, n_views);
    for (int v = 0; v < n_views; v++) L.zmin[(size_t)v] = c.take((size_t)sizes[2 * v] * sizes[2 * v + 1] * 4);
    L.bytes = c.off;
    return L;
}

struct PlaneAssignLayout { size_t target, bytes; };
PlaneAssignLayout plane_assign_layout(int n_planes) {
    const size_t bytes = n_planes > 0 ? (size_t)n_planes * 4 : 0;
    WorkspaceCursor c;
    const size_t target = c.take(bytes);
    return {target, target + bytes};  // the one range's own end, not c.off: the query has always been stated without the rounding
}

int check_member(int n_global, int n_words, const void* member) {
    if (n_words < 1 || n_words > (1 << 20) || n_global < 0 || n_global > 64 * n_words)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_words must be in 1 .. 2^20 and n_global in 0 .. 64 * n_words");
    return member ? G4S_OK : null_pointer();
}

int check_row(int row, int n_global, const char* name) {
    return row >= 0 && row < n_global ? G4S_OK : fail(G4S_ERR_INVALID_ARGUMENT, "%s must be a global plane below n_global", name);
}

}  // namespace

extern "C" size_t g4s_plane_labels_workspace(int n_views, const int* sizes) {
    long long largest, total;
    if (!view_sizes_ok(n_views, sizes, &largest, &total)) return 0;  // no cap on n_views: the views are no grid dimension
    return plane_labels_layout(n_views, sizes).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_plane_labels(int n_points, const float* points, float depth_thresh, int n_views, const float* world_view,
                                const float* focal, const int* sizes, const int* const* masks, int* labels, char* workspace,
                                size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_points(n_points) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!(depth_thresh == depth_thresh)) return fail(G4S_ERR_INVALID_ARGUMENT, "depth_thresh must not be NaN");
    if (n_views < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_views must not be negative");
    if (n_views == 0) return G4S_OK;
    if (!world_view || !focal || !sizes || !masks || (n_points > 0 && (!points || !labels))) return null_pointer();
    long long largest, total;
    if (!view_sizes_ok(n_views, sizes, &largest, &total))  // this unit's own wording, and no cap on n_views
        return fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive and width * height at most 2^30");
    if (check_workspace(workspace, workspace_bytes, g4s_plane_labels_workspace(n_views, sizes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    for (int v = 0; v < n_views; v++) {
        if (!masks[v]) return fail(G4S_ERR_INVALID_ARGUMENT, "view %d: NULL map pointer", v);
    }
    if (n_points == 0) return G4S_OK;
    // nothing below can fail a check: the first device call comes after every one of them
    const PlaneLabelsLayout L = plane_labels_layout(n_views, sizes);
    char* ws = align_ptr(workspace);
    const bool depth_test = depth_thresh >= 0.0f;
    // 0xFFFFFFFF: above the bits of every positive float
    hipError_t e = depth_test ? hipMemsetAsync(ws + L.zmin[0], 0xFF, L.bytes - L.zmin[0], stream) : hipSuccess;
    if (e != hipSuccess) return finish(e, "plane labels");
    const PlaneView* table;
    const int rc = stage_views("plane labels", n_views, true, sizes, (const float* const*)masks, nullptr, false, workspace,
                               view_table_bytes<PlaneView>(n_views), stream, &table, [&](PlaneView& u, int v) {
                                   vis_pose(u, world_view, focal, v);
                                   u.zmin = (uint32_t*)(ws + L.zmin[(size_t)v]);
                               });
    if (rc != G4S_OK) return rc;
    if (depth_test)
        hipLaunchKernelGGL(plane_zmin_kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, n_points, points, table, n_views);
    hipLaunchKernelGGL(plane_label_kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, n_points, points, table, n_views,
                       depth_thresh, depth_test ? 1 : 0, labels);
    return finish(hipSuccess, "plane labels");
}

extern "C" int g4s_plane_overlap(int n_points, const int* labels, int n_planes, int n_global, int n_words,
                                 const unsigned long long* member, unsigned int* counts, unsigned int* sizes, char* workspace,
                                 size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    (void)workspace_bytes;
    clear_error();
    if (check_points(n_points) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_planes < 0 || (long long)n_planes * (n_global > 0 ? n_global : 1) > (1ll << 30))
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_planes must not be negative and n_planes * n_global at most 2^30");
    if (check_member(n_global, n_words, member) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_planes == 0) return G4S_OK;
    if (!sizes || (n_global > 0 && !counts) || (n_points > 0 && !labels)) return null_pointer();
    hipError_t e = hipMemsetAsync(sizes, 0, (size_t)n_planes * 4, stream);
    if (e == hipSuccess && n_global > 0) e = hipMemsetAsync(counts, 0, (size_t)n_planes * n_global * 4, stream);
    if (e != hipSuccess) return finish(e, "plane overlap");
    if (n_points == 0) return G4S_OK;
    const int entries = n_planes * n_global + n_planes;
    const dim3 grid(blocks256(n_points) < COUNT_MAX_BLOCKS ? blocks256(n_points) : COUNT_MAX_BLOCKS);
    if (entries <= COUNT_LDS_MAX)
        hipLaunchKernelGGL(plane_overlap_kernel<true>, grid, dim3(256), (size_t)entries * 4, stream, n_points, labels, n_planes,
                           n_global, (n_global + 63) / 64, member, counts, sizes);
    else
        hipLaunchKernelGGL(plane_overlap_kernel<false>, grid, dim3(256), 0, stream, n_points, labels, n_planes, n_global,
                           (n_global + 63) / 64, member, counts, sizes);
    return finish(hipSuccess, "plane overlap");
}

extern "C" size_t g4s_plane_assign_workspace(int n_planes) { return plane_assign_layout(n_planes).bytes + WORKSPACE_BASE_SLACK; }

extern "C" int g4s_plane_assign(int n_points, const int* labels, int n_planes, const int* target, int n_global, int n_words,
                                unsigned long long* member, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_points(n_points) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_planes < 0 || n_planes > (1 << 30)) return fail(G4S_ERR_INVALID_ARGUMENT, "n_planes must be in 0 .. 2^30");
    if (check_member(n_global, n_words, member) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_planes == 0) return G4S_OK;
    if (!target || (n_points > 0 && !labels)) return null_pointer();
    for (int p = 0; p < n_planes; p++) {
        if (target[p] < -1 || target[p] >= n_global)
            return fail(G4S_ERR_INVALID_ARGUMENT, "target[%d] must be -1 or a global plane below n_global", p);
    }
    if (check_workspace(workspace, workspace_bytes, g4s_plane_assign_workspace(n_planes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_points == 0) return G4S_OK;
    int* dev = workspace_at<int>(workspace, plane_assign_layout(n_planes).target);
    const hipError_t e = upload(dev, target, (size_t)n_planes * 4, stream);
    if (e != hipSuccess) return finish(e, "plane assign");
    hipLaunchKernelGGL(plane_assign_kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, n_points, labels, n_planes, dev, member);
    return finish(hipSuccess, "plane assign");
}

extern "C" int g4s_plane_row_overlap(int n_points, int n_global, int n_words, const unsigned long long* member, int row,
                                     unsigned int* counts, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    (void)workspace_bytes;
    clear_error();
    if (check_points(n_points) != G4S_OK || check_member(n_global, n_words, member) != G4S_OK ||
        check_row(row, n_global, "row") != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!counts) return null_pointer();
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_global * 4, stream);
    if (e != hipSuccess) return finish(e, "plane row overlap");
    if (n_points == 0) return G4S_OK;
    const dim3 grid(blocks256(n_points) < COUNT_MAX_BLOCKS ? blocks256(n_points) : COUNT_MAX_BLOCKS);
    if (n_global <= COUNT_LDS_MAX)
        hipLaunchKernelGGL(plane_row_overlap_kernel<true>, grid, dim3(256), (size_t)n_global * 4, stream, n_points, n_global,
                           (n_global + 63) / 64, member, row, counts);
    else
        hipLaunchKernelGGL(plane_row_overlap_kernel<false>, grid, dim3(256), 0, stream, n_points, n_global,
                           (n_global + 63) / 64, member, row, counts);
    return finish(hipSuccess, "plane row overlap");
}

extern "C" int g4s_plane_row_merge(int n_points, int n_global, int n_words, unsigned long long* member, int src, int dst,
                                   char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    (void)workspace_bytes;
    clear_error();
    if (check_points(n_points) != G4S_OK || check_member(n_global, n_words, member) != G4S_OK ||
        check_row(src, n_global, "src") != G4S_OK || check_row(dst, n_global, "dst") != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_points == 0 || src == dst) return G4S_OK;
    hipLaunchKernelGGL(plane_row_merge_kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, n_points, member, src, dst);
    return finish(hipSuccess, "plane row merge");
}

extern "C" int g4s_plane_row_mask(int n_points, int n_global, int n_words, const unsigned long long* member, int row,
                                  unsigned char* mask, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)workspace;
    (void)workspace_bytes;
    clear_error();
    if (check_points(n_points) != G4S_OK || check_member(n_global, n_words, member) != G4S_OK ||
        check_row(row, n_global, "row") != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_points == 0) return G4S_OK;
    if (!mask) return null_pointer();
    hipLaunchKernelGGL(plane_row_mask_kernel, dim3(blocks256(n_points)), dim3(256), 0, stream, n_points, member, row, mask);
    return finish(hipSuccess, "plane row mask");
}
