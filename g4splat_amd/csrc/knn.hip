// simple-knn replacement: mean squared distance to the 3 nearest other points (distCUDA2).
//
// WHAT is computed is the reference's (knn/simple_knn.cu:131-183, restated by brute force in
// oracle/surfel_oracle.c oracle_knn): for every point the three smallest values of
//     d(j) = (x_j - x)^2 + (y_j - y)^2 + (z_j - z)^2        (separate multiplies and adds, this association)
// over all j with a different INDEX (duplicates give 0, fewer than three other points leave FLT_MAX terms), summed
// smallest first and divided by 3.  The three smallest values are a property of the point set, so every exact search
// returns the same bits.  HOW it is searched here has nothing in common with the reference (one thread per point walking
// every 1 024-point box of a per-axis Morton order):
//
//   * the points are ordered along a Z-curve over a CUBIC lattice (one scale for the three axes: the cells of a
//     6 x 4 x 3 m room are cubes, not bricks, and the bounding boxes of consecutive runs are compact) with the library's
//     own LDS radix sort, and gathered once into a float4 array (x, y, z, index) padded to a multiple of 64;
//   * over that order sits an implicit 64-ary tree of axis-aligned boxes: a LEAF is 64 consecutive points -- what a
//     wave64 fetches with one coalesced 1-KB request --, an inner node has 64 children -- what a wave tests in ONE step,
//     one child per lane and a ballot.  Three levels cover 262 144 points per top node; the top nodes are walked 64 at a
//     time (10 M points: 39 of them);
//   * ONE WAVE ANSWERS THE 64 QUERIES OF A LEAF TOGETHER.  Its lanes are neighbours on the curve, so they want the
//     same candidates: a candidate leaf is fetched once per wave, parked in LDS and read back as broadcast
//     ds_read_b128 -- one LDS instruction per 64 (query, candidate) pairs -- and every lane keeps its own sorted
//     triple with v_min_f32 + 2 x v_med3_f32 (three independent instructions per pair, no compare / select chain);
//   * pruning is wave-level and two-stage: (1) box against box -- the query leaf's own box against a node's, compared
//     with the wave's largest third-best distance -- decides 64 nodes per step; (2) before a surviving leaf is
//     fetched, every lane measures ITS point against the leaf's box and the leaf is skipped unless some lane could
//     still improve.  Both bounds are computed with the distance's own operations in the distance's own order, so by
//     monotonicity of IEEE rounding they never exceed the distance a candidate inside the box would get: pruning on
//     `bound >= third best` is exact (an equal value changes nothing), and a cloud of coincident points costs one leaf
//     instead of the whole scene;
//   * the search starts from the wave's own leaf and its two neighbours on the curve, so the radius is already a few
//     point spacings when the tree walk begins; nothing is reset and nothing is scanned twice.
//   No host synchronisation, no allocation (caller's workspace), 11 launches of which 8 are the sort's.
#include "knn_tree.h"

namespace g4s {

// sorted triple t0 <= t1 <= t2 of the smallest distances seen; insertion = min and two medians of the OLD values
struct Best3 {
    float t0, t1, t2;
};
__device__ __forceinline__ void best3_insert(Best3& b, float d) {
    const float n0 = fminf(b.t0, d);
    const float n1 = __builtin_amdgcn_fmed3f(b.t0, b.t1, d);
    const float n2 = __builtin_amdgcn_fmed3f(b.t1, b.t2, d);
    b.t0 = n0; b.t1 = n1; b.t2 = n2;
}
// All 64 candidates of a staged leaf against this lane's query.  OWN: the leaf is the wave's own, candidate k is lane
// k's point and is excluded for that lane (by index, like the reference: a duplicate elsewhere counts with distance 0).
// A candidate whose distance is NaN or inf (padding slots, non-finite input) is clamped to FLT_MAX, which inserts as a
// no-op -- exactly what the reference's `best[j] > dist` does with it.
template <bool OWN>
__device__ __forceinline__ void scan_leaf(const float4* __restrict__ cand, float qx, float qy, float qz, int lane, Best3& b) {
#pragma unroll 8
    for (int k = 0; k < KNN_LEAF; k++) {
        const float4 c = cand[k];  // wave-uniform address: broadcast read
        const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
        float d = fminf(dx * dx + dy * dy + dz * dz, FLT_MAX);
        if (OWN) d = k == lane ? FLT_MAX : d;
        best3_insert(b, d);
    }
}

__global__ void __launch_bounds__(256) knn_search_kernel(int P, const float4* __restrict__ sorted, const Box* __restrict__ leaves,
                                                         const Box* __restrict__ mids, const Box* __restrict__ tops, int n0, int n1, int n2,
                                                         float* __restrict__ dists) {
    __shared__ float4 s_cand[4][KNN_LEAF];
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int own = (int)(blockIdx.x * 4) + wv;  // this wave's leaf
    if (own >= n0) return;
    float4* stage = s_cand[wv];
    const float4 me = sorted[(size_t)own * KNN_LEAF + lane];
    const bool valid = own * KNN_LEAF + lane < P;
    Best3 b{FLT_MAX, FLT_MAX, FLT_MAX};
    // the start: own leaf, then its neighbours on the curve
    stage_leaf(sorted, own, lane, stage);
    scan_leaf<true>(stage, me.x, me.y, me.z, lane, b);
    const int near_lo = own > 0 ? own - 1 : own, near_hi = own + 1 < n0 ? own + 1 : own;
    if (near_lo != own) { stage_leaf(sorted, near_lo, lane, stage); scan_leaf<false>(stage, me.x, me.y, me.z, lane, b); }
    if (near_hi != own) { stage_leaf(sorted, near_hi, lane, stage); scan_leaf<false>(stage, me.x, me.y, me.z, lane, b); }
    float r2 = wave_max_nonneg(valid ? b.t2 : 0.0f);  // wave-uniform: nothing at or beyond it can matter to any lane

    const Box q = leaves[own];  // the 64 queries' own box (uniform)
    for (int c2 = 0; c2 < n2; c2 += KNN_FAN) {
        const float g2 = c2 + lane < n2 ? gap2_box_box(tops[c2 + lane], q) : FLT_MAX;
        uint64_t m2 = __ballot(g2 < r2);
        while (m2) {
            const int j2 = (int)__builtin_ctzll(m2);
            m2 &= m2 - 1;
            if (!(lane_value(g2, j2) < r2)) continue;  // r2 has shrunk since
            const int i1 = (c2 + j2) * KNN_FAN + lane;
            const float g1 = i1 < n1 ? gap2_box_box(mids[i1], q) : FLT_MAX;
            uint64_t m1 = __ballot(g1 < r2);
            while (m1) {
                const int j1 = (int)__builtin_ctzll(m1);
                m1 &= m1 - 1;
                if (!(lane_value(g1, j1) < r2)) continue;
                const int base0 = ((c2 + j2) * KNN_FAN + j1) * KNN_FAN;
                const int i0 = base0 + lane;
                Box lf = box_empty();
                if (i0 < n0) lf = leaves[i0];
                const bool fresh = i0 < n0 && (i0 < near_lo || i0 > near_hi);  // not one of the three leaves of the start
                uint64_t m0 = __ballot(fresh && gap2_box_box(lf, q) < r2);
                while (m0) {
                    const int j0 = (int)__builtin_ctzll(m0);
                    m0 &= m0 - 1;
                    // stage 2: could ANY lane still improve on its third best inside this leaf's box?
                    const float lx = lane_value(lf.lx, j0), ly = lane_value(lf.ly, j0), lz = lane_value(lf.lz, j0);
                    const float hx = lane_value(lf.hx, j0), hy = lane_value(lf.hy, j0), hz = lane_value(lf.hz, j0);
                    const float gp = gap2_box_point(lx, ly, lz, hx, hy, hz, me.x, me.y, me.z);
                    if (__ballot(valid && gp < b.t2) == 0ull) continue;
                    stage_leaf(sorted, base0 + j0, lane, stage);
                    scan_leaf<false>(stage, me.x, me.y, me.z, lane, b);
                    r2 = wave_max_nonneg(valid ? b.t2 : 0.0f);
                }
            }
        }
    }
    if (valid) dists[__float_as_uint(me.w)] = (b.t0 + b.t1 + b.t2) / 3.0f;
}

}  // namespace g4s

using namespace g4s;

extern "C" size_t g4s_knn_workspace(int P) { return knn_layout(P > 0 ? (size_t)P : 0).bytes; }

// SimpleKNN::knn (knn/simple_knn.cu:185-221)
extern "C" int g4s_knn_mean_dist(int P, const float* points, float* meanDists, char* workspace,
                                 size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P < 0");
    if (P == 0) return G4S_OK;
    if (!points || !meanDists || !workspace) return fail(G4S_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (int rc = check_workspace(workspace, workspace_bytes, g4s_knn_workspace(P))) return rc;
    const KnnLayout L = knn_layout((size_t)P);
    char* w = align_ptr(workspace);
    knn_build_tree(L, P, points, w, s);
    const Box* leaves = (const Box*)(w + L.nodes);
    hipLaunchKernelGGL(knn_search_kernel, dim3((L.n0 + 3) / 4), dim3(256), 0, s, P, (const float4*)(w + L.sorted), leaves,
                       leaves + L.n0, leaves + L.n0 + L.n1, L.n0, L.n1, L.n2, meanDists);
    return stage_done("knn", s);
}
