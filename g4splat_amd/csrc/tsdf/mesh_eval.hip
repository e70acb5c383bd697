// Mesh evaluation (include/g4s_render_maps.h, "mesh evaluation" section; the semantics stated there are the contract,
// tests/mesh_eval_ref.py restates them in numpy): what the reference's eval/mesh_eval.py takes from scikit-learn's
// KDTree, open3d's VoxelDownSample and trimesh's sample_surface.
//
// A. Nearest neighbour from a query cloud into a reference cloud.  The reference cloud gets distCUDA2's tree
//    (../knn_tree.h: extent, cubic 1024^3 Z-curve, LDS radix sort, float4 leaves of 64, two levels of 64-ary boxes).
//    The queries are ordered along the SAME curve -- the reference cloud's extent, cells clamped, so a query far outside
//    lands in a border cell -- and one wave answers 64 consecutive ones: neighbours on the curve want the same
//    candidates.  The wave's radius is seeded from the reference leaf whose first curve code is nearest the code of its
//    first query (binary search over the sorted codes); then tops, mids and leaves are walked with knn.hip's two-stage
//    pruning: box against the union box of the wave's live queries with the wave's largest current best, then every
//    lane's point against the leaf's box.  Both bounds never exceed the distance of a candidate inside the box (knn.hip),
//    and a box is dropped only on `bound > best`: an equal distance at a smaller index must still be seen.  (So a cloud
//    of coincident reference points is scanned whole: every leaf holds a tie.)
//    A lane keeps (d, j) as ONE 64-bit word, float bits of d above j, and takes the unsigned minimum: d is a sum of
//    squares, never negative, so its bits order as its value does and the word orders as (d, j) does -- the rule
//    `d < best || (d == best && j < best_j)` in one compare.  The word starts at (FLT_MAX, 0xFFFFFFFF): +inf and every
//    NaN have larger bits and never win, and a query that meets no finite candidate reads back FLT_MAX and -1.
//    No atomics; the result is a function of the two clouds alone.
// B. Voxel down-sample: extent -> plan (one thread: lower corner, cells per axis, key width) -> key = linear cell <<
//    index_bits | index -> radix_sort_u64_keys over the cell bits (stable: indices stay ascending inside a cell) ->
//    segment heads -> scan_u32 -> [host: n_voxels] -> one thread per voxel sums its points in float64 in index order.
// C. Surface sampling: one thread per sample, binary search in the caller's cumulative areas.
#include "../knn_tree.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "scan.h"

namespace g4s {

// ---------------------------------------------------------------------------------------------------------------------
// A. nearest neighbour

constexpr uint64_t NN_NONE = ((uint64_t)0x7F7FFFFFu << 32) | 0xFFFFFFFFull;  // (FLT_MAX, -1)

struct NnLayout {
    KnnLayout ref;  // the reference cloud's tree, at offset 0
    size_t keys_a, keys_b, vals_a, vals_b, hist, bin_total, bytes;  // the queries' curve order
};
static NnLayout nn_layout(size_t n_ref, size_t n_query) {
    NnLayout L{};
    L.ref = knn_layout(n_ref);
    WorkspaceCursor c;
    c.off = align_up(L.ref.bytes);
    L.keys_a = c.take(n_query * 4); L.keys_b = c.take(n_query * 4); L.vals_a = c.take(n_query * 4); L.vals_b = c.take(n_query * 4);
    L.hist = c.take((size_t)256 * (sort_blocks(n_query, SORT_ITEMS_U32) + 1) * 4);
    L.bin_total = c.take(256 * 4);
    L.bytes = c.off + 256;
    return L;
}

// All 64 candidates of a staged leaf against this lane's query (padding slots: NaN coordinates, index bits all set).
__device__ __forceinline__ void nn_scan_leaf(const float4* __restrict__ cand, float qx, float qy, float qz, uint64_t& best) {
#pragma unroll 8
    for (int k = 0; k < KNN_LEAF; k++) {
        const float4 c = cand[k];  // wave-uniform address: broadcast read
        const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
        const float d = dx * dx + dy * dy + dz * dz;
        const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)__float_as_uint(c.w);
        best = key < best ? key : best;
    }
}

__global__ void __launch_bounds__(256) nn_search_kernel(int n_query, const float* __restrict__ query,
                                                        const uint32_t* __restrict__ q_order, const uint32_t* __restrict__ q_codes,
                                                        const uint32_t* __restrict__ r_codes, const float4* __restrict__ sorted,
                                                        const Box* __restrict__ leaves, const Box* __restrict__ mids,
                                                        const Box* __restrict__ tops, int n0, int n1, int n2,
                                                        float* __restrict__ dist2_out, int* __restrict__ index_out) {
    __shared__ float4 s_cand[4][KNN_LEAF];
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const long first = ((long)blockIdx.x * 4 + wv) * KNN_LEAF;  // this wave's first query on the curve
    if (first >= n_query) return;
    float4* stage = s_cand[wv];
    const bool valid = first + lane < n_query;
    uint32_t src = 0;
    float x = __uint_as_float(0x7FC00000u), y = x, z = x;
    if (valid) {
        src = q_order[first + lane];
        x = query[3 * (size_t)src], y = query[3 * (size_t)src + 1], z = query[3 * (size_t)src + 2];
    }
    // a query with a non-finite coordinate has no finite candidate: it keeps NN_NONE and steers nothing
    const bool live = valid && fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;
    uint64_t best = NN_NONE;
    if (__ballot(live) != 0ull) {
        const Box q = box_wave_join(live ? Box{x, y, z, x, y, z, 0, 0} : box_empty());  // the live queries' box (uniform)
        // the start: the reference leaf whose first code is nearest the first query's
        const uint32_t code = q_codes[first];
        int lo = 0, hi = n0;  // leaves [0, lo) begin at or below `code`, leaves [hi, n0) above it
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (r_codes[(size_t)mid * KNN_LEAF] <= code) lo = mid + 1; else hi = mid;
        }
        int seed = lo > 0 ? lo - 1 : 0;
        if (lo > 0 && lo < n0 && r_codes[(size_t)lo * KNN_LEAF] - code < code - r_codes[(size_t)seed * KNN_LEAF]) seed = lo;
        seed = __builtin_amdgcn_readfirstlane(seed);
        stage_leaf(sorted, seed, lane, stage);
        nn_scan_leaf(stage, x, y, z, best);
        float r2 = wave_max_nonneg(live ? __uint_as_float((uint32_t)(best >> 32)) : 0.0f);  // wave-uniform

        for (int c2 = 0; c2 < n2; c2 += KNN_FAN) {
            const bool in2 = c2 + lane < n2;
            const float g2 = in2 ? gap2_box_box(tops[c2 + lane], q) : FLT_MAX;
            uint64_t m2 = __ballot(in2 && g2 <= r2);
            while (m2) {
                const int j2 = (int)__builtin_ctzll(m2);
                m2 &= m2 - 1;
                if (!(lane_value(g2, j2) <= r2)) continue;  // r2 has shrunk since
                const int i1 = (c2 + j2) * KNN_FAN + lane;
                const bool in1 = i1 < n1;
                const float g1 = in1 ? gap2_box_box(mids[i1], q) : FLT_MAX;
                uint64_t m1 = __ballot(in1 && g1 <= r2);
                while (m1) {
                    const int j1 = (int)__builtin_ctzll(m1);
                    m1 &= m1 - 1;
                    if (!(lane_value(g1, j1) <= r2)) continue;
                    const int base0 = ((c2 + j2) * KNN_FAN + j1) * KNN_FAN;
                    const int i0 = base0 + lane;
                    Box lf = box_empty();
                    if (i0 < n0) lf = leaves[i0];
                    const bool fresh = i0 < n0 && i0 != seed;
                    uint64_t m0 = __ballot(fresh && gap2_box_box(lf, q) <= r2);
                    while (m0) {
                        const int j0 = (int)__builtin_ctzll(m0);
                        m0 &= m0 - 1;
                        // stage 2: could ANY lane still improve on, or tie with, its best inside this leaf's box?
                        const float lx = lane_value(lf.lx, j0), ly = lane_value(lf.ly, j0), lz = lane_value(lf.lz, j0);
                        const float hx = lane_value(lf.hx, j0), hy = lane_value(lf.hy, j0), hz = lane_value(lf.hz, j0);
                        const float gp = gap2_box_point(lx, ly, lz, hx, hy, hz, x, y, z);
                        if (__ballot(live && gp <= __uint_as_float((uint32_t)(best >> 32))) == 0ull) continue;
                        stage_leaf(sorted, base0 + j0, lane, stage);
                        nn_scan_leaf(stage, x, y, z, best);
                        r2 = wave_max_nonneg(live ? __uint_as_float((uint32_t)(best >> 32)) : 0.0f);
                    }
                }
            }
        }
    }
    if (valid) {
        dist2_out[src] = __uint_as_float((uint32_t)(best >> 32));
        index_out[src] = (int)(uint32_t)best;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// B. voxel down-sample

constexpr uint32_t VDS_NONFINITE = 1u, VDS_TOO_WIDE = 2u;  // the status word of a count call

struct VdsPlan {
    float lo[3];
    uint32_t pad;
    unsigned long long nx, ny, nz;  // cells per axis (0: no plan, see the status word)
};
struct VdsLayout {
    size_t keys_a, keys_b, hist, bin_total, flag, pos, chunks, partial, extent, plan, words, bytes;
    int nparts;
};
static VdsLayout vds_layout(size_t n) {
    VdsLayout L{};
    const size_t k = n ? n : 1;
    WorkspaceCursor c;
    L.nparts = (int)((k + 1023) / 1024);
    L.keys_a = c.take(k * 8);
    L.keys_b = c.take(k * 8);
    L.hist = c.take((size_t)256 * (sort_blocks(k, SORT_ITEMS_U64) + 1) * 4);
    L.bin_total = c.take(512 * 4);
    L.flag = c.take(k * 4);
    L.pos = c.take(k * 4);
    L.chunks = c.take((size_t)scan_chunks((long)k) * 4 + 4);
    L.partial = c.take((size_t)L.nparts * 32);
    L.extent = c.take(32);
    L.plan = c.take(sizeof(VdsPlan));
    L.words = c.take(64);  // [0] voxels, [1] status
    L.bytes = c.off;
    return L;
}
static int vds_index_bits(int n) {  // bits(n - 1)
    int b = 0;
    while (b < 31 && ((unsigned)(n - 1) >> b) != 0u) b++;
    return b;
}

__device__ __forceinline__ unsigned long long vds_cell(float p, float lo, float voxel_size) {
    return (unsigned long long)floor(((double)p - (double)lo) / (double)voxel_size);
}

// One thread: the lattice of the cloud, and whether cell and index fit one 64-bit key.
__global__ void vds_plan_kernel(const Box* __restrict__ extent, float voxel_size, int index_bits, VdsPlan* __restrict__ plan,
                                uint32_t* __restrict__ status) {
    const Box b = *extent;
    VdsPlan p{};
    const float mn[3] = {b.lx, b.ly, b.lz}, mx[3] = {b.hx, b.hy, b.hz};
    bool ok = true;
    double cells[3];
    for (int a = 0; a < 3; a++) {
        // (a NaN coordinate is invisible to the extent: the key kernel reports it)
        if (!(fabsf(mn[a]) <= FLT_MAX) || !(fabsf(mx[a]) <= FLT_MAX)) {
            *status = VDS_NONFINITE;
            *plan = p;
            return;
        }
        p.lo[a] = mn[a] - voxel_size * 0.5f;
        cells[a] = floor(((double)mx[a] - (double)p.lo[a]) / (double)voxel_size) + 1.0;
        ok = ok && cells[a] < 9.0e18;
    }
    unsigned long long total = 0;
    if (ok) {
        const unsigned long long nx = (unsigned long long)cells[0], ny = (unsigned long long)cells[1], nz = (unsigned long long)cells[2];
        ok = __umul64hi(nx, ny) == 0ull && __umul64hi(nx * ny, nz) == 0ull;
        total = nx * ny * nz;
        // the largest linear cell, total - 1, must fit 64 - index_bits bits
        if (ok && index_bits > 0) ok = ((total - 1ull) >> (64 - index_bits)) == 0ull;
        if (ok) p.nx = nx, p.ny = ny, p.nz = nz;
    }
    if (!ok) *status = VDS_TOO_WIDE;
    *plan = p;
}

__global__ void __launch_bounds__(256) vds_keys_kernel(int n, const float* __restrict__ pts, float voxel_size, int index_bits,
                                                       const VdsPlan* __restrict__ plan, unsigned long long* __restrict__ keys,
                                                       uint32_t* __restrict__ status) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const VdsPlan p = *plan;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    unsigned long long cell = 0;
    if (!(fabsf(x) <= FLT_MAX) || !(fabsf(y) <= FLT_MAX) || !(fabsf(z) <= FLT_MAX)) {
        *status = VDS_NONFINITE;  // every writer stores the same word: no atomic needed
    } else if (p.nx != 0ull) {
        // p >= the axis minimum > lo and the quotient is monotonic in p: 0 <= cell < cells per axis
        const unsigned long long cx = vds_cell(x, p.lo[0], voxel_size), cy = vds_cell(y, p.lo[1], voxel_size),
                                 cz = vds_cell(z, p.lo[2], voxel_size);
        cell = (cz * p.ny + cy) * p.nx + cx;
    }
    keys[i] = index_bits > 0 ? (cell << index_bits) | (unsigned long long)i : cell;
}

__global__ void __launch_bounds__(256) vds_heads_kernel(int n, const unsigned long long* __restrict__ keys, int index_bits,
                                                        uint32_t* __restrict__ flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // index_bits == 0 is n == 1: the one point heads the one voxel
    flag[i] = (i == 0 || (keys[i] >> index_bits) != (keys[i - 1] >> index_bits)) ? 1u : 0u;
}

// The thread of a segment's head walks the segment: ascending input index, float64 sums, one rounding to float32.
__global__ void __launch_bounds__(256) vds_emit_kernel(int n, const float* __restrict__ pts, const unsigned long long* __restrict__ keys,
                                                       int index_bits, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                       int n_voxels, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || flag[i] == 0u) return;
    const uint32_t o = pos[i];
    if (o >= (uint32_t)n_voxels) return;  // the caller's capacity
    const unsigned long long mask = index_bits > 0 ? (1ull << index_bits) - 1ull : 0ull;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    long e = i;
    do {
        const size_t src = (size_t)(keys[e] & mask);
        sx += (double)pts[3 * src], sy += (double)pts[3 * src + 1], sz += (double)pts[3 * src + 2];
        e++;
    } while (e < n && flag[e] == 0u);
    const double count = (double)(e - i);
    out[3 * (size_t)o] = (float)(sx / count), out[3 * (size_t)o + 1] = (float)(sy / count), out[3 * (size_t)o + 2] = (float)(sz / count);
}

// The same walk for the index variant: s = sum of (double)i / (double)n in ascending input index, a = s / count, and the
// voxel's index is a * (double)n rounded half to even (rint under the default rounding mode).
__global__ void __launch_bounds__(256) vds_emit_index_kernel(int n, const unsigned long long* __restrict__ keys, int index_bits,
                                                             const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                             int n_voxels, long long* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || flag[i] == 0u) return;
    const uint32_t o = pos[i];
    if (o >= (uint32_t)n_voxels) return;  // the caller's capacity
    const unsigned long long mask = index_bits > 0 ? (1ull << index_bits) - 1ull : 0ull;
    const double total = (double)n;
    double sum = 0.0;
    long e = i;
    do {
        sum += (double)(keys[e] & mask) / total;
        e++;
    } while (e < n && flag[e] == 0u);
    const double mean = sum / (double)(e - i);
    out[o] = (long long)rint(mean * total);
}

// ---------------------------------------------------------------------------------------------------------------------
// C. surface sampling

__global__ void __launch_bounds__(256) mesh_sample_kernel(int n_samples, const float* __restrict__ u, const double* __restrict__ cum_area,
                                                          int F, const int* __restrict__ tris, int V, const float* __restrict__ verts,
                                                          float* __restrict__ points, float* __restrict__ normals, int* __restrict__ face_out) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_samples) return;
    const double t = (double)u[3 * s] * cum_area[F - 1];
    int lo = 0, hi = F;  // cum_area[0, lo) <= t < cum_area[hi, F)
    while (lo < hi) {
        const int mid = (int)(((long)lo + hi) >> 1);
        if (cum_area[mid] <= t) lo = mid + 1; else hi = mid;
    }
    const int f = lo < F - 1 ? lo : F - 1;
    face_out[s] = f;
    const int i0 = tris[3 * (size_t)f], i1 = tris[3 * (size_t)f + 1], i2 = tris[3 * (size_t)f + 2];
    float p[3] = {__uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u)};
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if ((uint32_t)i0 < (uint32_t)V && (uint32_t)i1 < (uint32_t)V && (uint32_t)i2 < (uint32_t)V) {
        float a = u[3 * s + 1], b = u[3 * s + 2];
        if (a + b > 1.0f) a = 1.0f - a, b = 1.0f - b;
        float e1[3], e2[3];
        for (int k = 0; k < 3; k++) {
            const float v0 = verts[3 * (size_t)i0 + k];
            e1[k] = verts[3 * (size_t)i1 + k] - v0;
            e2[k] = verts[3 * (size_t)i2 + k] - v0;
            p[k] = v0 + (a * e1[k] + b * e2[k]);
        }
        const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
        if (len > 0.0f) nrm[0] = cx / len, nrm[1] = cy / len, nrm[2] = cz / len;
    }
    for (int k = 0; k < 3; k++) {
        points[3 * s + k] = p[k];
        normals[3 * s + k] = nrm[k];
    }
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points (include/g4s_render_maps.h, mesh evaluation); every argument is checked before any launch
namespace {

constexpr int MAX_POINTS = 2147483647 / 3;  // 3 * n < 2^31

int check_count(int n, const char* what) {
    if (n < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "%s must not be negative", what);
    if (n > MAX_POINTS) return fail(G4S_ERR_INVALID_ARGUMENT, "3 * %s exceeds 2^31 - 1", what);
    return G4S_OK;
}

}  // namespace

extern "C" size_t g4s_nn_workspace(int n_ref, int n_query) {
    const size_t r = n_ref > 0 && n_ref <= MAX_POINTS ? (size_t)n_ref : 0, q = n_query > 0 && n_query <= MAX_POINTS ? (size_t)n_query : 0;
    return nn_layout(r, q).bytes;
}

extern "C" int g4s_nn_search(int n_ref, const float* ref, int n_query, const float* query, float* dist2_out, int* index_out,
                             char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (n_ref <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_ref must be positive");
    if (check_count(n_ref, "n_ref") != G4S_OK || check_count(n_query, "n_query") != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_query == 0) return G4S_OK;
    if (!ref || !query || !dist2_out || !index_out) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_nn_workspace(n_ref, n_query)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const NnLayout L = nn_layout((size_t)n_ref, (size_t)n_query);
    char* w = align_ptr(workspace);
    const int r_cur = knn_build_tree(L.ref, n_ref, ref, w, s);
    const uint32_t* r_codes = (const uint32_t*)(w + (r_cur ? L.ref.keys_b : L.ref.keys_a));
    // the queries along the reference cloud's curve
    uint32_t* keys_a = (uint32_t*)(w + L.keys_a);
    uint32_t* keys_b = (uint32_t*)(w + L.keys_b);
    uint32_t* vals_a = (uint32_t*)(w + L.vals_a);
    uint32_t* vals_b = (uint32_t*)(w + L.vals_b);
    hipLaunchKernelGGL(knn_curve_kernel, dim3((n_query + 255) / 256), dim3(256), 0, s, n_query, query, (const Box*)(w + L.ref.extent),
                       keys_a, vals_a);
    const int q_cur = radix_sort_u32_pairs(keys_a, keys_b, vals_a, vals_b, n_query, (uint32_t*)(w + L.hist),
                                           (uint32_t*)(w + L.bin_total), s);
    const Box* leaves = (const Box*)(w + L.ref.nodes);
    const int waves = (n_query + KNN_LEAF - 1) / KNN_LEAF;
    hipLaunchKernelGGL(nn_search_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, n_query, query, q_cur ? vals_b : vals_a,
                       q_cur ? keys_b : keys_a, r_codes, (const float4*)(w + L.ref.sorted), leaves, leaves + L.ref.n0,
                       leaves + L.ref.n0 + L.ref.n1, L.ref.n0, L.ref.n1, L.ref.n2, dist2_out, index_out);
    return finish(hipSuccess, "nn search");
}

extern "C" size_t g4s_voxel_downsample_workspace(int n) {
    return vds_layout(n > 0 && n <= MAX_POINTS ? (size_t)n : 0).bytes + 256;  // + alignment of the base pointer
}

extern "C" int g4s_voxel_downsample_count(int n, const float* points, float voxel_size, int* n_voxels, char* workspace,
                                          size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (check_count(n, "n") != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!finite_pos(voxel_size)) return fail(G4S_ERR_INVALID_ARGUMENT, "voxel_size must be finite and positive");
    if (!n_voxels || (n > 0 && !points)) return null_pointer();
    *n_voxels = 0;
    if (n == 0) return G4S_OK;
    if (check_workspace(workspace, workspace_bytes, g4s_voxel_downsample_workspace(n)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const VdsLayout L = vds_layout((size_t)n);
    char* ws = align_ptr(workspace);
    unsigned long long* ka = (unsigned long long*)(ws + L.keys_a);
    unsigned long long* kb = (unsigned long long*)(ws + L.keys_b);
    Box* partial = (Box*)(ws + L.partial);
    Box* extent = (Box*)(ws + L.extent);
    VdsPlan* plan = (VdsPlan*)(ws + L.plan);
    uint32_t* words = (uint32_t*)(ws + L.words);
    uint32_t* flag = (uint32_t*)(ws + L.flag);
    const int index_bits = vds_index_bits(n);
    hipError_t e = hipMemsetAsync(words, 0, 64, s);
    if (e != hipSuccess) return finish(e, "voxel_downsample count");
    const dim3 grid(((unsigned)n + 255u) / 256u);
    hipLaunchKernelGGL(knn_extent_partial_kernel, dim3(L.nparts), dim3(1024), 0, s, n, points, partial);
    hipLaunchKernelGGL(knn_extent_final_kernel, dim3(1), dim3(1024), 0, s, L.nparts, partial, extent);
    hipLaunchKernelGGL(vds_plan_kernel, dim3(1), dim3(1), 0, s, extent, voxel_size, index_bits, plan, words + 1);
    hipLaunchKernelGGL(vds_keys_kernel, grid, dim3(256), 0, s, n, points, voxel_size, index_bits, plan, ka, words + 1);
    // The width of the cell field is known on the device only: every bit above the index is sorted.  The keys come in
    // ascending index and the sort is stable, so the index bits need no pass.
    const int cur = radix_sort_u64_keys((uint64_t*)ka, (uint64_t*)kb, n, index_bits, 64, (uint32_t*)(ws + L.hist),
                                        (uint32_t*)(ws + L.bin_total), s);
    if (cur != 0) {  // g4s_voxel_downsample_emit finds the sorted keys in the first buffer
        e = hipMemcpyAsync(ka, kb, (size_t)n * 8, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return finish(e, "voxel_downsample count");
    }
    hipLaunchKernelGGL(vds_heads_kernel, grid, dim3(256), 0, s, n, ka, index_bits, flag);
    scan_u32(flag, (uint32_t*)(ws + L.pos), n, (uint32_t*)(ws + L.chunks), words + 0, s);
    int t[2];  // (voxels, status)
    e = read_totals(words, t, s);
    if (e != hipSuccess) return finish(e, "voxel_downsample count");
    if ((uint32_t)t[1] == VDS_NONFINITE) return fail(G4S_ERR_INVALID_ARGUMENT, "points must be finite");
    if (t[1] != 0)
        return fail(G4S_ERR_INVALID_ARGUMENT, "cell bits and index bits exceed 64: the cloud spans too many voxels of this size");
    *n_voxels = t[0];
    return finish(hipSuccess, "voxel_downsample count");
}

extern "C" int g4s_voxel_downsample_emit(int n, const float* points, int n_voxels, float* points_out, char* workspace,
                                         size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (check_count(n, "n") != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_voxels < 0 || n_voxels > n) return fail(G4S_ERR_INVALID_ARGUMENT, "n_voxels must lie in 0..n");
    if (n_voxels == 0) return G4S_OK;
    if (!points || !points_out) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_voxel_downsample_workspace(n)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const VdsLayout L = vds_layout((size_t)n);
    char* ws = align_ptr(workspace);
    hipLaunchKernelGGL(vds_emit_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, s, n, points,
                       (const unsigned long long*)(ws + L.keys_a), vds_index_bits(n), (const uint32_t*)(ws + L.flag),
                       (const uint32_t*)(ws + L.pos), n_voxels, points_out);
    return finish(hipSuccess, "voxel_downsample emit");
}

extern "C" int g4s_voxel_downsample_emit_index(int n, int n_voxels, long long* index_out, char* workspace,
                                               size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (check_count(n, "n") != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_voxels < 0 || n_voxels > n) return fail(G4S_ERR_INVALID_ARGUMENT, "n_voxels must lie in 0..n");
    if (n_voxels == 0) return G4S_OK;
    if (!index_out) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_voxel_downsample_workspace(n)) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    const VdsLayout L = vds_layout((size_t)n);
    char* ws = align_ptr(workspace);
    hipLaunchKernelGGL(vds_emit_index_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, s, n,
                       (const unsigned long long*)(ws + L.keys_a), vds_index_bits(n), (const uint32_t*)(ws + L.flag),
                       (const uint32_t*)(ws + L.pos), n_voxels, index_out);
    return finish(hipSuccess, "voxel_downsample emit index");
}

extern "C" int g4s_mesh_sample_surface(int n_samples, const float* u, const double* cum_area, int n_triangles, const int* triangles,
                                       int n_vertices, const float* vertices, float* points_out, float* normals_out, int* face_out,
                                       void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (check_count(n_samples, "n_samples") != G4S_OK || check_count(n_vertices, "n_vertices") != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_triangles <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_triangles must be positive");
    if (check_count(n_triangles, "n_triangles") != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_samples == 0) return G4S_OK;
    if (!u || !cum_area || !triangles || !points_out || !normals_out || !face_out || (n_vertices > 0 && !vertices)) return null_pointer();
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(((unsigned)n_samples + 255u) / 256u), dim3(256), 0, s, n_samples, u, cum_area,
                       n_triangles, triangles, n_vertices, vertices, points_out, normals_out, face_out);
    return finish(hipSuccess, "mesh sample_surface");
}
