// What the units under tsdf/ share that is not about views -- the mesh units (tsdf.hip, unbounded.hip, tetra.hip, mesh_ops.hip,
// mesh_eval.hip) and the view-stack units (visibility.hip, planes.hip, consistency.hip, view_select.hip, depth_cues.hip,
// chart_init.hip, plane_masks.hip): the argument checks of their entry points beyond those of g4s_internal.h (null_pointer,
// check_workspace; blocks256 and workspace_at are there too), the upload of host values and the read-back of the two scan
// totals; for the mesh units alone, the index arithmetic of the marching-cubes table (tsdf_mc_table.h).  What is about a
// stack of views is in view_stack.h.
#pragma once
#include <math.h>
#include <vector>

#include "../g4s_internal.h"

namespace g4s {

// ---- argument checks: each leaves its message behind and returns the entry point's status ----
inline bool finite_pos(float x) { return x > 0.0f && x < 3.0e38f; }
inline bool finite(float x) { return fabsf(x) < 3.0e38f; }
inline bool lattice_ok(int n) { return n >= 2 && (long long)n * n * n < (1ll << 31); }
inline int check_lattice(int n) {
    return lattice_ok(n) ? G4S_OK : fail(G4S_ERR_INVALID_ARGUMENT, "n must be at least 2 and n^3 below 2^31");
}

// host values -> device memory; synchronises, so `host` is the caller's again on return
inline hipError_t upload(void* dev, const void* host, size_t bytes, hipStream_t stream) {
    hipError_t e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e;
}
// two host int arrays -> one device range, b behind a, in one upload
inline hipError_t upload_pair(int* dev, const int* a, int na, const int* b, int nb, hipStream_t stream) {
    std::vector<int> host(a, a + na);
    host.insert(host.end(), b, b + nb);
    return upload(dev, host.data(), host.size() * sizeof(int), stream);
}

// out[0..1] = the two adjacent scan totals words[0..1]: pending launch errors first, then one copy and the one host
// synchronisation of a count call.  `out` is written on success only.
inline hipError_t read_totals(const uint32_t* words, int out[2], hipStream_t s) {
    uint32_t host[2];
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, words, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    out[0] = (int)host[0];
    out[1] = (int)host[1];
    return hipSuccess;
}

// ---- the cube table's encoding (tsdf_mc_table.h): edge id = 4 * axis + n, n = the lower corner's other two coordinates ----
struct McEdge {
    int x, y, z, a;  // the lattice point that owns the edge's vertex (the edge's lower end), and the edge's axis
};
// edge e of the cube whose lower corner is (x, y, z)
__device__ __forceinline__ McEdge mc_edge(int e, int x, int y, int z) {
    const int a = e >> 2, n = e & 3;
    const int o1 = n & 1, o2 = n >> 1;  // the lower corner's other two coordinates, in axis order
    return McEdge{x + (a == 0 ? 0 : o1), y + (a == 1 ? 0 : (a == 0 ? o1 : o2)), z + (a == 2 ? 0 : o2), a};
}
// rank of the +a vertex among the vertices before and of its owner, whose word is w = exclusive vertex prefix << 3 |
// owned-edge mask
__device__ __forceinline__ uint32_t mc_vertex_rank(uint32_t w, int a) {
    return (w >> 3) + (uint32_t)__builtin_popcount(w & 7u & ((1u << a) - 1u));
}

}  // namespace g4s
