// Mesh operations of the multi-resolution export (include/g4s_render_maps.h, "mesh operations" section; the semantics
// stated there are the contract, tests/mesh_ops_ref.py restates them in numpy).
//
// Observed-vertex test: one thread per vertex, the cameras staged through LDS 64 at a time (the three columns of
//   full_proj_transform and the one of world_view_transform that the test reads), early exit once observed.
// Clustering: every non-degenerate edge (min, max) of every triangle is entered into an open-addressing table (64-bit
//   CAS on the key); the slot's owner word takes the minimum of the triangles that came by (32-bit atomicMin), and every
//   triangle that finds an earlier one there unites with it in a lock-free union-find that always links the larger root
//   under the smaller.  Whatever the interleaving, the root of a finished tree is the smallest triangle of its cluster:
//   the labels are a function of the mesh alone.  Sizes are integer counts at the roots.
// Compaction: keep flags -> fixed-order exclusive scans (scan_u32 of scan.hip) -> [host: sizes] -> gather.
// Only integer atomics (CAS / min / add); every output is bit-reproducible.
#include "../g4s_internal.h"
#include "../g4s_device.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "scan.h"
#include "union_find.h"

namespace g4s {

constexpr int CAM_CHUNK = 64;                 // cameras staged in LDS at a time (4 KiB)
constexpr uint64_t EDGE_EMPTY = ~0ull;        // no edge key has all bits set (its low half is the larger index, lo < hi)
constexpr uint32_t OWNER_NONE = 0xFFFFFFFFu;  // above every triangle index

// ---------------------------------------------------------------------------------------------------------------------
// A. observed vertices

__global__ void __launch_bounds__(256) mesh_observed_kernel(int V, const float* __restrict__ verts, int C,
                                                            const float* __restrict__ world_view,
                                                            const float* __restrict__ full_proj, float near_trunc,
                                                            uint8_t* __restrict__ observed) {
    __shared__ float cam[CAM_CHUNK][16];  // per camera, row r of [p,1]: (proj[r][0], proj[r][1], proj[r][3], view[r][2])
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < V;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (valid) {
        x = verts[3 * i + 0];
        y = verts[3 * i + 1];
        z = verts[3 * i + 2];
    }
    bool obs = false;
    for (int c0 = 0; c0 < C; c0 += CAM_CHUNK) {
        const int n = C - c0 < CAM_CHUNK ? C - c0 : CAM_CHUNK;
        for (int j = (int)threadIdx.x; j < n * 16; j += 256) {
            const int ci = j >> 4, r = (j >> 2) & 3, k = j & 3;
            const size_t base = (size_t)(c0 + ci) * 16 + (size_t)r * 4;
            cam[ci][r * 4 + k] = k == 3 ? world_view[base + 2] : full_proj[base + (k == 2 ? 3 : k)];
        }
        __syncthreads();
        if (valid && !obs) {
            for (int c = 0; c < n; c++) {
                const float* m = cam[c];
                const float hx = ((x * m[0] + y * m[4]) + z * m[8]) + m[12];
                const float hy = ((x * m[1] + y * m[5]) + z * m[9]) + m[13];
                const float hw = ((x * m[2] + y * m[6]) + z * m[10]) + m[14];
                const float zc = ((x * m[3] + y * m[7]) + z * m[11]) + m[15];
                const float w = hw > 1.0e-6f ? hw : 1.0e-6f;
                if (fabsf(hx / w) < 1.0f && fabsf(hy / w) < 1.0f && zc < near_trunc) {
                    obs = true;
                    break;
                }
            }
        }
        if (__syncthreads_and(!valid || obs)) break;  // also the barrier before the next chunk overwrites the LDS
    }
    if (valid) observed[i] = obs ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// keep masks (one thread per triangle)

__device__ inline bool index_ok(int i, int V) { return (uint32_t)i < (uint32_t)V; }

__global__ void __launch_bounds__(256) mesh_keep_unobserved_kernel(int F, const int* __restrict__ tris, int V,
                                                                   const uint8_t* __restrict__ observed,
                                                                   uint8_t* __restrict__ keep) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    bool all = true;
    for (int k = 0; k < 3; k++) {
        const int i = tris[3 * t + k];
        all = all && index_ok(i, V) && observed[i] != 0;
    }
    keep[t] = all ? 0 : 1;
}

__global__ void __launch_bounds__(256) mesh_keep_min_size_kernel(int F, const int* __restrict__ sizes, int min_size,
                                                                 uint8_t* __restrict__ keep) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < F) keep[t] = sizes[t] >= min_size ? 1 : 0;
}

__global__ void __launch_bounds__(256) mesh_keep_nondegenerate_kernel(int F, const int* __restrict__ tris,
                                                                      uint8_t* __restrict__ keep) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    keep[t] = (a != b && b != c && a != c) ? 1 : 0;
}

__device__ inline double edge_length(const float* __restrict__ v, int a, int b) {
    const double dx = (double)v[3 * (long)a + 0] - (double)v[3 * (long)b + 0];
    const double dy = (double)v[3 * (long)a + 1] - (double)v[3 * (long)b + 1];
    const double dz = (double)v[3 * (long)a + 2] - (double)v[3 * (long)b + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ void __launch_bounds__(256) mesh_keep_short_edges_kernel(int F, const int* __restrict__ tris, int V,
                                                                    const float* __restrict__ verts, double threshold,
                                                                    uint8_t* __restrict__ keep) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    bool ok = index_ok(a, V) && index_ok(b, V) && index_ok(c, V);
    if (ok)
        ok = edge_length(verts, a, b) <= threshold && edge_length(verts, b, c) <= threshold &&
             edge_length(verts, c, a) <= threshold;
    keep[t] = ok ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// B. clustering

// the union-find (uf_find, uf_unite) is in union_find.h

__device__ inline uint64_t mix64(uint64_t k) {  // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

__global__ void __launch_bounds__(256) mesh_cluster_init_kernel(int F, uint32_t* __restrict__ parent,
                                                                uint32_t* __restrict__ count) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < F) {
        parent[t] = (uint32_t)t;
        count[t] = 0u;
    }
}

__global__ void __launch_bounds__(256) mesh_cluster_hook_kernel(int F, const int* __restrict__ tris,
                                                                unsigned long long* __restrict__ keys,
                                                                uint32_t* __restrict__ owner, uint64_t mask,
                                                                uint32_t* __restrict__ parent) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    uint32_t v[3];
    for (int k = 0; k < 3; k++) v[k] = (uint32_t)tris[3 * t + k];
    for (int k = 0; k < 3; k++) {
        const uint32_t a = v[k], b = v[k == 2 ? 0 : k + 1];
        if (a == b) continue;
        const uint64_t key = ((uint64_t)(a < b ? a : b) << 32) | (uint64_t)(a < b ? b : a);
        uint64_t h = mix64(key) & mask;
        for (uint64_t probe = 0; probe <= mask; probe++) {  // the table is at most half full: an empty slot exists
            const unsigned long long prev = atomicCAS(keys + h, (unsigned long long)EDGE_EMPTY, (unsigned long long)key);
            if (prev == EDGE_EMPTY || prev == key) {
                const uint32_t old = atomicMin(owner + h, (uint32_t)t);
                if (old != OWNER_NONE && old != (uint32_t)t) uf_unite(parent, (uint32_t)t, old);
                break;
            }
            h = (h + 1) & mask;
        }
    }
}

// labels = roots; count[root] += 1 per triangle, one atomic per distinct root of a wave
__global__ void __launch_bounds__(256) mesh_cluster_label_kernel(int F, uint32_t* __restrict__ parent,
                                                                 int* __restrict__ labels, uint32_t* __restrict__ count) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = t < F;
    uint32_t root = 0;
    if (valid) {
        root = uf_find(parent, (uint32_t)t);
        labels[t] = (int)root;
    }
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t l = (uint32_t)__shfl((int)root, leader, 64);
        const unsigned long long same = __ballot(valid && root == l);
        if (lane_id() == leader) atomicAdd(count + l, (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(256) mesh_cluster_sizes_kernel(int F, const int* __restrict__ labels,
                                                                 const uint32_t* __restrict__ count,
                                                                 int* __restrict__ sizes) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < F) sizes[t] = (int)count[labels[t]];
}

struct ClusterLayout {
    size_t slots, keys, owner, parent, count, bytes;
};
ClusterLayout cluster_layout(int F) {
    ClusterLayout L{};
    size_t slots = 1024;
    while (slots < (size_t)6 * (size_t)F) slots <<= 1;  // at most 3 F edges: load <= 1/2
    L.slots = slots;
    WorkspaceCursor c;
    L.keys = c.take(slots * 8);
    L.owner = c.take(slots * 4);
    L.parent = c.take((size_t)F * 4);
    L.count = c.take((size_t)F * 4);
    L.bytes = c.off;
    return L;
}

hipError_t mesh_cluster(int F, const int* tris, int* labels, int* sizes, char* ws, hipStream_t s) {
    const ClusterLayout L = cluster_layout(F);
    unsigned long long* keys = (unsigned long long*)(ws + L.keys);
    uint32_t* owner = (uint32_t*)(ws + L.owner);
    uint32_t* parent = (uint32_t*)(ws + L.parent);
    uint32_t* count = (uint32_t*)(ws + L.count);
    hipError_t e = hipMemsetAsync(keys, 0xFF, L.slots * 8, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(owner, 0xFF, L.slots * 4, s);
    if (e != hipSuccess) return e;
    const int g = (F + 255) / 256;
    hipLaunchKernelGGL(mesh_cluster_init_kernel, dim3(g), dim3(256), 0, s, F, parent, count);
    hipLaunchKernelGGL(mesh_cluster_hook_kernel, dim3(g), dim3(256), 0, s, F, tris, keys, owner, (uint64_t)(L.slots - 1), parent);
    hipLaunchKernelGGL(mesh_cluster_label_kernel, dim3(g), dim3(256), 0, s, F, parent, labels, count);
    hipLaunchKernelGGL(mesh_cluster_sizes_kernel, dim3(g), dim3(256), 0, s, F, labels, count, sizes);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// E. stable compaction

__global__ void __launch_bounds__(256) mesh_tri_flags_kernel(int F, const uint8_t* __restrict__ keep,
                                                             uint32_t* __restrict__ tflag) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < F) tflag[t] = (keep == nullptr || keep[t] != 0) ? 1u : 0u;
}

// every writer stores the same 1 (vflag was cleared): no atomic needed
__global__ void __launch_bounds__(256) mesh_mark_vertices_kernel(int F, const int* __restrict__ tris,
                                                                 const uint32_t* __restrict__ tflag, int V,
                                                                 uint32_t* __restrict__ vflag) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F || tflag[t] == 0u) return;
    for (int k = 0; k < 3; k++) {
        const int i = tris[3 * t + k];
        if (index_ok(i, V)) vflag[i] = 1u;
    }
}

__global__ void __launch_bounds__(256) mesh_gather_tris_kernel(int F, const int* __restrict__ tris,
                                                               const uint32_t* __restrict__ tflag,
                                                               const uint32_t* __restrict__ tpos, int V,
                                                               const uint32_t* __restrict__ vpos, int* __restrict__ out,
                                                               uint32_t F_out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F || tflag[t] == 0u) return;
    const uint32_t o = tpos[t];
    if (o >= F_out) return;  // the caller's capacity
    for (int k = 0; k < 3; k++) {
        const int i = tris[3 * t + k];
        out[3 * (size_t)o + k] = !index_ok(i, V) ? -1 : (vpos != nullptr ? (int)vpos[i] : i);
    }
}

__global__ void __launch_bounds__(256) mesh_gather_verts_kernel(int V, const float* __restrict__ verts,
                                                                const float* __restrict__ cols,
                                                                const uint32_t* __restrict__ vflag,
                                                                const uint32_t* __restrict__ vpos,
                                                                float* __restrict__ verts_out, float* __restrict__ cols_out,
                                                                uint32_t V_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= V || vflag[i] == 0u) return;
    const uint32_t o = vpos[i];
    if (o >= V_out) return;
    for (int k = 0; k < 3; k++) {
        verts_out[3 * (size_t)o + k] = verts[3 * i + k];
        if (cols_out != nullptr) cols_out[3 * (size_t)o + k] = cols[3 * i + k];
    }
}

struct CompactLayout {
    size_t tflag, tpos, vflag, vpos, chunks, words, bytes;
};
CompactLayout compact_layout(int V, int F) {
    CompactLayout L{};
    WorkspaceCursor c;
    L.tflag = c.take((size_t)F * 4);
    L.tpos = c.take((size_t)F * 4);
    L.vflag = c.take((size_t)V * 4);
    L.vpos = c.take((size_t)V * 4);
    L.chunks = c.take((size_t)scan_chunks((long)(V > F ? V : F)) * 4 + 4);
    L.words = c.take(64);
    L.bytes = c.off;
    return L;
}

hipError_t mesh_compact_count(int V, int F, const int* tris, const uint8_t* keep, bool compact_vertices, char* ws,
                              int* totals, hipStream_t s) {
    const CompactLayout L = compact_layout(V, F);
    uint32_t* tflag = (uint32_t*)(ws + L.tflag);
    uint32_t* vflag = (uint32_t*)(ws + L.vflag);
    uint32_t* chunks = (uint32_t*)(ws + L.chunks);
    uint32_t* words = (uint32_t*)(ws + L.words);
    hipError_t e = hipMemsetAsync(words, 0, 64, s);
    if (e != hipSuccess) return e;
    const int g = (F + 255) / 256;
    if (F > 0) hipLaunchKernelGGL(mesh_tri_flags_kernel, dim3(g), dim3(256), 0, s, F, keep, tflag);
    scan_u32(tflag, (uint32_t*)(ws + L.tpos), F, chunks, words + 0, s);
    if (compact_vertices) {
        if (V > 0) {
            e = hipMemsetAsync(vflag, 0, (size_t)V * 4, s);
            if (e != hipSuccess) return e;
        }
        if (F > 0 && V > 0) hipLaunchKernelGGL(mesh_mark_vertices_kernel, dim3(g), dim3(256), 0, s, F, tris, tflag, V, vflag);
        scan_u32(vflag, (uint32_t*)(ws + L.vpos), V, chunks, words + 1, s);
    }
    int t[2];  // (kept triangles, referenced vertices)
    e = read_totals(words, t, s);
    if (e != hipSuccess) return e;
    totals[0] = compact_vertices ? t[1] : V;
    totals[1] = t[0];
    return hipSuccess;
}

hipError_t mesh_compact_emit(int V, int F, const float* verts, const float* cols, const int* tris, bool compact_vertices,
                             float* verts_out, float* cols_out, int* tris_out, int V_out, int F_out, char* ws,
                             hipStream_t s) {
    const CompactLayout L = compact_layout(V, F);
    const uint32_t* vpos = compact_vertices ? (const uint32_t*)(ws + L.vpos) : nullptr;
    if (F > 0 && F_out > 0)
        hipLaunchKernelGGL(mesh_gather_tris_kernel, dim3((F + 255) / 256), dim3(256), 0, s, F, tris,
                           (const uint32_t*)(ws + L.tflag), (const uint32_t*)(ws + L.tpos), V, vpos, tris_out,
                           (uint32_t)F_out);
    if (compact_vertices && V > 0 && V_out > 0)
        hipLaunchKernelGGL(mesh_gather_verts_kernel, dim3((V + 255) / 256), dim3(256), 0, s, V, verts, cols,
                           (const uint32_t*)(ws + L.vflag), vpos, verts_out, cols_out, (uint32_t)V_out);
    return hipGetLastError();
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points (include/g4s_render_maps.h, mesh operations); every argument is checked before any launch
namespace {

constexpr int MAX_TRIANGLES = 2147483647 / 3;  // 3 * n_triangles < 2^31

int check_triangles(int n_triangles) {
    if (n_triangles < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_triangles must not be negative");
    if (n_triangles > MAX_TRIANGLES) return fail(G4S_ERR_INVALID_ARGUMENT, "3 * n_triangles exceeds 2^31 - 1");
    return G4S_OK;
}
int check_vertices(int n_vertices) {
    if (n_vertices < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_vertices must not be negative");
    if (n_vertices > MAX_TRIANGLES) return fail(G4S_ERR_INVALID_ARGUMENT, "3 * n_vertices exceeds 2^31 - 1");
    return G4S_OK;
}

}  // namespace

extern "C" int g4s_mesh_observed_vertices(int n_vertices, const float* vertices, int n_cameras,
                                          const float* world_view_transforms, const float* full_proj_transforms,
                                          float near_trunc, unsigned char* observed, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_vertices(n_vertices) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_cameras < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_cameras must not be negative");
    if (near_trunc != near_trunc) return fail(G4S_ERR_INVALID_ARGUMENT, "near_trunc must not be NaN");
    if ((n_vertices > 0 && (!vertices || !observed)) || (n_cameras > 0 && (!world_view_transforms || !full_proj_transforms)))
        return null_pointer();
    if (n_vertices == 0) return G4S_OK;
    hipLaunchKernelGGL(mesh_observed_kernel, dim3((n_vertices + 255) / 256), dim3(256), 0, stream, n_vertices, vertices,
                       n_cameras, world_view_transforms, full_proj_transforms, near_trunc, observed);
    return finish(hipSuccess, "mesh observed_vertices");
}

extern "C" int g4s_mesh_keep_unobserved(int n_triangles, const int* triangles, int n_vertices,
                                        const unsigned char* observed, unsigned char* keep, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_triangles(n_triangles) != G4S_OK || check_vertices(n_vertices) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if ((n_triangles > 0 && (!triangles || !keep)) || (n_triangles > 0 && n_vertices > 0 && !observed)) return null_pointer();
    if (n_triangles == 0) return G4S_OK;
    hipLaunchKernelGGL(mesh_keep_unobserved_kernel, dim3((n_triangles + 255) / 256), dim3(256), 0, stream, n_triangles,
                       triangles, n_vertices, observed, keep);
    return finish(hipSuccess, "mesh keep_unobserved");
}

extern "C" int g4s_mesh_keep_min_size(int n_triangles, const int* sizes, int min_size, unsigned char* keep, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_triangles(n_triangles) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_triangles > 0 && (!sizes || !keep)) return null_pointer();
    if (n_triangles == 0) return G4S_OK;
    hipLaunchKernelGGL(mesh_keep_min_size_kernel, dim3((n_triangles + 255) / 256), dim3(256), 0, stream, n_triangles,
                       sizes, min_size, keep);
    return finish(hipSuccess, "mesh keep_min_size");
}

extern "C" int g4s_mesh_keep_nondegenerate(int n_triangles, const int* triangles, unsigned char* keep, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_triangles(n_triangles) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_triangles > 0 && (!triangles || !keep)) return null_pointer();
    if (n_triangles == 0) return G4S_OK;
    hipLaunchKernelGGL(mesh_keep_nondegenerate_kernel, dim3((n_triangles + 255) / 256), dim3(256), 0, stream,
                       n_triangles, triangles, keep);
    return finish(hipSuccess, "mesh keep_nondegenerate");
}

extern "C" int g4s_mesh_keep_short_edges(int n_triangles, const int* triangles, int n_vertices, const float* vertices,
                                         double length_threshold, unsigned char* keep, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_triangles(n_triangles) != G4S_OK || check_vertices(n_vertices) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (length_threshold != length_threshold) return fail(G4S_ERR_INVALID_ARGUMENT, "length_threshold must not be NaN");
    if ((n_triangles > 0 && (!triangles || !keep)) || (n_triangles > 0 && n_vertices > 0 && !vertices)) return null_pointer();
    if (n_triangles == 0) return G4S_OK;
    hipLaunchKernelGGL(mesh_keep_short_edges_kernel, dim3((n_triangles + 255) / 256), dim3(256), 0, stream, n_triangles,
                       triangles, n_vertices, vertices, length_threshold, keep);
    return finish(hipSuccess, "mesh keep_short_edges");
}

extern "C" size_t g4s_mesh_cluster_workspace(int n_triangles) {
    if (n_triangles <= 0 || n_triangles > MAX_TRIANGLES) return 256;
    return cluster_layout(n_triangles).bytes + 256;  // + alignment of the base pointer
}

extern "C" int g4s_mesh_cluster_triangles(int n_triangles, const int* triangles, int* labels, int* sizes, char* workspace,
                                          size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_triangles(n_triangles) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_triangles > 0 && (!triangles || !labels || !sizes)) return null_pointer();
    if (n_triangles == 0) return G4S_OK;
    if (check_workspace(workspace, workspace_bytes, g4s_mesh_cluster_workspace(n_triangles)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    return finish(mesh_cluster(n_triangles, triangles, labels, sizes, align_ptr(workspace), stream), "mesh cluster_triangles");
}

extern "C" size_t g4s_mesh_compact_workspace(int n_vertices, int n_triangles) {
    const int V = n_vertices > 0 && n_vertices <= MAX_TRIANGLES ? n_vertices : 0;
    const int F = n_triangles > 0 && n_triangles <= MAX_TRIANGLES ? n_triangles : 0;
    return compact_layout(V, F).bytes + 256;
}

extern "C" int g4s_mesh_compact_count(int n_vertices, int n_triangles, const int* triangles, const unsigned char* keep,
                                      int compact_vertices, int* totals, char* workspace, size_t workspace_bytes,
                                      void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_vertices(n_vertices) != G4S_OK || check_triangles(n_triangles) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!totals || (n_triangles > 0 && !triangles)) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_mesh_compact_workspace(n_vertices, n_triangles)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const hipError_t e = mesh_compact_count(n_vertices, n_triangles, triangles, keep, compact_vertices != 0,
                                            align_ptr(workspace), totals, stream);
    return finish(e, "mesh compact_count");
}

extern "C" int g4s_mesh_compact_emit(int n_vertices, int n_triangles, const float* vertices, const float* vertex_colors,
                                     const int* triangles, int compact_vertices, float* vertices_out,
                                     float* vertex_colors_out, int* triangles_out, int n_vertices_out, int n_triangles_out,
                                     char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_vertices(n_vertices) != G4S_OK || check_triangles(n_triangles) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_vertices_out < 0 || n_triangles_out < 0 || n_vertices_out > n_vertices || n_triangles_out > n_triangles)
        return fail(G4S_ERR_INVALID_ARGUMENT, "output counts must lie in 0..input counts");
    if ((n_triangles > 0 && !triangles) || (n_triangles_out > 0 && !triangles_out)) return null_pointer();
    if (compact_vertices && n_vertices_out > 0 && (!vertices || !vertices_out)) return null_pointer();
    if (compact_vertices && n_vertices_out > 0 && ((vertex_colors == nullptr) != (vertex_colors_out == nullptr)))
        return fail(G4S_ERR_INVALID_ARGUMENT, "vertex_colors and vertex_colors_out go together");
    if ((const void*)triangles == (const void*)triangles_out || (vertices && (const void*)vertices == (const void*)vertices_out))
        return fail(G4S_ERR_INVALID_ARGUMENT, "outputs must not alias the inputs");
    if (check_workspace(workspace, workspace_bytes, g4s_mesh_compact_workspace(n_vertices, n_triangles)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const hipError_t e = mesh_compact_emit(n_vertices, n_triangles, vertices, vertex_colors, triangles, compact_vertices != 0,
                                           vertices_out, vertex_colors_out, triangles_out, n_vertices_out, n_triangles_out,
                                           align_ptr(workspace), stream);
    return finish(e, "mesh compact_emit");
}
