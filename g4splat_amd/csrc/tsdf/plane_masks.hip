// Per-view plane masks (include/g4s_render_maps.h, "Plane masks"; the semantics stated there are the contract,
// tests/plane_masks_ref.py restates them in numpy): Lloyd's k-means over the normals of a view, the 9x9 opening and the
// 8-connected components of the kept clusters, and the join of the components with the caller's segmentation masks.
//
//   k-means     grid = (spans of KM_SPAN pixels of the largest view, views).  A thread labels its KM_ITEMS pixels and adds the
//               members of every cluster in ascending order in float64, a wave folds its lanes by the fixed shuffle tree
//               (wave_count.h), lane 0 of wave 0 adds the four wave sums in wave order; one wave per (cluster, view) adds the
//               workgroups' partials by index.  A one-wave launch per view and iteration writes the view's done flag; the
//               launches of later iterations read it and return.  The host reads the flags every KM_POLL iterations.
//   open        one workgroup per 32x8 tile, the ranks staged with an 8-pixel halo in LDS; erode and dilate are separable.
//   components  label-equivalence union-find on pixel indices (union_find.h), sizes by integer atomics at the roots, the
//               kept roots compacted by scan_u32 and ranked per (view, rank) by a block scan.
//   join        one thread per pixel walks the view's masks; counts are integer, one atomic per wave and key (wave_count.h);
//               the normal sums are 64-bit integers of fixed-point values.
// Every launch count is independent of the number of views, masks and components.  No float atomics.
#include <math.h>
#include <vector>

#include "../g4s_internal.h"
#include "../fixed_sums.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "scan.h"
#include "union_find.h"
#include "view_stack.h"
#include "wave_count.h"

namespace g4s {

constexpr int KM_ITEMS = 16;               // pixels per thread of the k-means kernels
constexpr int KM_SPAN = 256 * KM_ITEMS;    // pixels one workgroup labels and reduces
constexpr int KM_MAX_K = G4S_KMEANS_MAX_K;
constexpr int KM_STRIDE = 4 * KM_MAX_K;    // doubles per workgroup partial: (count, x, y, z) per cluster; the moments use 7
constexpr int KM_POLL = 8;                 // iterations between two reads of the done flags
static_assert(KM_SPAN == G4S_KMEANS_SPAN, "the header states the span the workspace is sized by");
enum { KM_RUNNING = 0, KM_STABLE = 1, KM_REASSIGN = 2 };  // state[0]; state[1] = iterations, state[2] = a label changed

constexpr int OPEN_R = 4;                   // the 9x9 window
constexpr int OPEN_TX = 32, OPEN_TY = 8;    // output tile
constexpr int OPEN_AX = OPEN_TX + 4 * OPEN_R, OPEN_AY = OPEN_TY + 4 * OPEN_R;  // staged ranks: 8-pixel halo
constexpr int OPEN_HX = OPEN_TX + 2 * OPEN_R;                                  // erode: 4-pixel halo
constexpr int OPEN_EY = OPEN_TY + 2 * OPEN_R;
constexpr signed char RANK_NONE = -1, RANK_OUTSIDE = -2;
constexpr int CC_MAX_RANKS = 16;

struct KmView {
    ViewMaps maps;  // depth = the normals [H,W,3]
    signed char* labels;
    uint32_t block_base, n_blocks;  // the view's rows of the partials
};

struct CcView {
    ViewMaps maps;  // depth = the int8 labels (count), unused (sizes)
    int* out;       // count: components [H,W]; sizes: the sizes [n]
    signed char* opened;  // count: optional [H,W]
    uint32_t pix_base;    // the view's first pixel in the workspace arrays
    int min_size;
    signed char lut[CC_MAX_RANKS];
};

struct JoinView {
    ViewMaps maps;  // depth = the int32 components (pair counts, paint), the normals (relabel)
    const unsigned char* masks;  // [M,H,W]
    int* seg;
    int M, n, n_ids;  // masks, components, pair ids
    int mask_base, pair_base, id_base, sum_base;
};

// ---------------------------------------------------------------------------------------------------------------------
// A. k-means


__global__ void __launch_bounds__(256) km_moments_kernel(const KmView* __restrict__ views, double* __restrict__ partials) {
    const KmView& v = views[blockIdx.y];
    if (blockIdx.x >= v.n_blocks) return;  // block-uniform
    const int n = v.maps.W * v.maps.H;
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const size_t first = (size_t)blockIdx.x * KM_SPAN + threadIdx.x;
    for (int k = 0; k < KM_ITEMS; k++) {
        const size_t q = first + (size_t)k * 256;
        if (q >= (size_t)n) break;
        const float xf = v.maps.depth[3 * q], yf = v.maps.depth[3 * q + 1], zf = v.maps.depth[3 * q + 2];
        if (xf != xf || yf != yf || zf != zf) continue;
        const double x = (double)xf, y = (double)yf, z = (double)zf;
        s[0] += 1.0;
        s[1] += x;
        s[2] += y;
        s[3] += z;
        s[4] += x * x;  // exact: two float32 factors
        s[5] += y * y;
        s[6] += z * z;
    }
    __shared__ double waves[4][KM_STRIDE];
#pragma unroll
    for (int c = 0; c < 7; c++) moment_fold(s[c], waves, c);
    moment_store(waves, 7, partials + ((size_t)v.block_base + blockIdx.x) * KM_STRIDE);
}

// grid = views, 64 threads: the absolute tolerance of the view, and its state cleared
__global__ void __launch_bounds__(64) km_tolerance_kernel(const KmView* __restrict__ views, const double* __restrict__ partials,
                                                          double tol, double* __restrict__ tol_abs, int* __restrict__ state) {
    const KmView& v = views[blockIdx.x];
    double s[7];
    column_fold(partials + (size_t)v.block_base * KM_STRIDE, v.n_blocks, KM_STRIDE, s);
    if (threadIdx.x != 0) return;
    const double n = s[0];
    const double vx = (s[4] - s[1] * s[1] / n) / n, vy = (s[5] - s[2] * s[2] / n) / n, vz = (s[6] - s[3] * s[3] / n) / n;
    tol_abs[blockIdx.x] = tol * (((vx + vy) + vz) / 3.0);
    int* st = state + 4 * (size_t)blockIdx.x;
    st[0] = KM_RUNNING;
    st[1] = st[2] = st[3] = 0;
}

// pass = KM_RUNNING: an iteration's labels and sums, for views still running; `first`: there are no earlier labels.
// pass = KM_REASSIGN: the final labels and counts, for views that stopped by the tolerance or at max_iter.
__global__ void __launch_bounds__(256) km_assign_kernel(const KmView* __restrict__ views, int K, const float* __restrict__ centres,
                                                        int* __restrict__ state, double* __restrict__ partials, int pass,
                                                        int first) {
    const KmView& v = views[blockIdx.y];
    if (blockIdx.x >= v.n_blocks) return;  // block-uniform, as the next
    int* st = state + 4 * (size_t)blockIdx.y;
    if (st[0] != pass) return;
    __shared__ float c[3 * KM_MAX_K];
    __shared__ double waves[4][KM_STRIDE];
    if ((int)threadIdx.x < 3 * K) c[threadIdx.x] = centres[(size_t)blockIdx.y * 3 * K + threadIdx.x];
    __syncthreads();
    const int n = v.maps.W * v.maps.H;
    const size_t q0 = (size_t)blockIdx.x * KM_SPAN + threadIdx.x;
    float x[KM_ITEMS], y[KM_ITEMS], z[KM_ITEMS];
    int lab[KM_ITEMS];
    bool changed = false;
#pragma unroll
    for (int i = 0; i < KM_ITEMS; i++) {
        const size_t q = q0 + (size_t)i * 256;
        lab[i] = -2;  // no pixel
        x[i] = y[i] = z[i] = 0.0f;
        if (q >= (size_t)n) continue;
        x[i] = v.maps.depth[3 * q], y[i] = v.maps.depth[3 * q + 1], z[i] = v.maps.depth[3 * q + 2];
        int best = -1;
        if (x[i] == x[i] && y[i] == y[i] && z[i] == z[i]) {
            float bd = 0.0f;
            for (int k = 0; k < K; k++) {
                const float dx = x[i] - c[3 * k], dy = y[i] - c[3 * k + 1], dz = z[i] - c[3 * k + 2];
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (k == 0 || d < bd) bd = d, best = k;
            }
        }
        lab[i] = best;
        if (pass == KM_RUNNING && !first && (int)v.labels[q] != best) changed = true;
        v.labels[q] = (signed char)best;
    }
    if (pass == KM_RUNNING && __ballot(changed) != 0ull && lane_id() == 0) atomicOr(st + 2, 1);
    for (int k = 0; k < K; k++) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int i = 0; i < KM_ITEMS; i++) {
            if (lab[i] != k) continue;
            s0 += 1.0;
            s1 += (double)x[i];
            s2 += (double)y[i];
            s3 += (double)z[i];
        }
        moment_fold(s0, waves, 4 * k);
        moment_fold(s1, waves, 4 * k + 1);
        moment_fold(s2, waves, 4 * k + 2);
        moment_fold(s3, waves, 4 * k + 3);
    }
    moment_store(waves, 4 * K, partials + ((size_t)v.block_base + blockIdx.x) * KM_STRIDE);
}

// grid = (K, views), 64 threads: the cluster's count, and in an iteration its next centre and the squared shift
__global__ void __launch_bounds__(64) km_update_kernel(const KmView* __restrict__ views, int K, const float* __restrict__ centres,
                                                       float* __restrict__ next, double* __restrict__ shift2,
                                                       int* __restrict__ counts, const int* __restrict__ state,
                                                       const double* __restrict__ partials, int pass) {
    const KmView& v = views[blockIdx.y];
    if (state[4 * (size_t)blockIdx.y] != pass) return;
    const int k = (int)blockIdx.x;
    double s[4];
    column_fold(partials + (size_t)v.block_base * KM_STRIDE + 4 * k, v.n_blocks, KM_STRIDE, s);
    if (threadIdx.x != 0) return;
    const size_t row = (size_t)blockIdx.y * K + k;
    counts[row] = (int)s[0];
    if (pass != KM_RUNNING) return;
    double d[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float old = centres[3 * row + c];
        const float nw = s[0] > 0.0 ? (float)(s[1 + c] / s[0]) : old;  // an empty cluster keeps its centre
        next[3 * row + c] = nw;
        d[c] = (double)nw - (double)old;
    }
    shift2[row] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

// grid = views, 64 threads: the centres take the next ones and the view's stop rule is evaluated; iter counts from 1
__global__ void __launch_bounds__(64) km_finalise_kernel(int K, float* __restrict__ centres, const float* __restrict__ next,
                                                         const double* __restrict__ shift2, const double* __restrict__ tol_abs,
                                                         int* __restrict__ state, int iter, int max_iter) {
    int* st = state + 4 * (size_t)blockIdx.x;
    if (st[0] != KM_RUNNING) return;  // wave-uniform: one wave
    if ((int)threadIdx.x < 3 * K) {
        const size_t i = (size_t)blockIdx.x * 3 * K + threadIdx.x;
        centres[i] = next[i];
    }
    if (threadIdx.x != 0) return;
    const bool changed = iter == 1 || st[2] != 0;
    st[1] = iter;
    st[2] = 0;
    if (!changed) {
        st[0] = KM_STABLE;
        return;
    }
    double total = 0.0;
    for (int k = 0; k < K; k++) total += shift2[(size_t)blockIdx.x * K + k];
    if (total <= tol_abs[blockIdx.x] || iter == max_iter) st[0] = KM_REASSIGN;
}

// ---------------------------------------------------------------------------------------------------------------------
// B. opening and components

__device__ __forceinline__ signed char rank_of(const CcView& v, signed char label) {
    return label >= 0 && label < CC_MAX_RANKS ? v.lut[label] : RANK_NONE;
}

// per pixel: rank, parent = itself, size = 0
__device__ __forceinline__ void cc_seed(const CcView& v, int q, signed char r, signed char* __restrict__ rank,
                                        uint32_t* __restrict__ parent, uint32_t* __restrict__ size) {
    const uint32_t p = v.pix_base + (uint32_t)q;
    rank[p] = r;
    parent[p] = p;
    size[p] = 0u;
    if (v.opened) v.opened[q] = r;
}

// without the opening: grid = (blocks of 256 pixels of the largest view, views)
__global__ void __launch_bounds__(256) cc_ranks_kernel(const CcView* __restrict__ views, signed char* __restrict__ rank,
                                                       uint32_t* __restrict__ parent, uint32_t* __restrict__ size) {
    const CcView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    cc_seed(v, q, rank_of(v, ((const signed char*)v.maps.depth)[q]), rank, parent, size);
}

// grid = (tiles of the view with the most, views)
__global__ void __launch_bounds__(256) cc_open_kernel(const CcView* __restrict__ views, signed char* __restrict__ rank,
                                                      uint32_t* __restrict__ parent, uint32_t* __restrict__ size) {
    const CcView& v = views[blockIdx.y];
    const int W = v.maps.W, H = v.maps.H;
    const int tiles_x = (W + OPEN_TX - 1) / OPEN_TX, tiles_y = (H + OPEN_TY - 1) / OPEN_TY;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // block-uniform
    const int x0 = ((int)blockIdx.x % tiles_x) * OPEN_TX, y0 = ((int)blockIdx.x / tiles_x) * OPEN_TY;
    const signed char* labels = (const signed char*)v.maps.depth;
    __shared__ signed char A[OPEN_AY][OPEN_AX];     // ranks, image (y0 - 8 + ay, x0 - 8 + ax)
    __shared__ signed char Hh[OPEN_AY][OPEN_HX];    // row erode, image (y0 - 8 + hy, x0 - 4 + hx)
    __shared__ unsigned char E[OPEN_EY][OPEN_HX];   // erode, image (y0 - 4 + ey, x0 - 4 + ex)
    __shared__ unsigned char D[OPEN_EY][OPEN_TX];   // row dilate, image (y0 - 4 + dy, x0 + dx)
    for (int i = (int)threadIdx.x; i < OPEN_AY * OPEN_AX; i += 256) {
        const int ay = i / OPEN_AX, ax = i % OPEN_AX;
        const int x = x0 - 2 * OPEN_R + ax, y = y0 - 2 * OPEN_R + ay;
        A[ay][ax] = x >= 0 && x < W && y >= 0 && y < H ? rank_of(v, labels[(size_t)y * W + x]) : RANK_OUTSIDE;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < OPEN_AY * OPEN_HX; i += 256) {
        const int hy = i / OPEN_HX, hx = i % OPEN_HX;
        const int x = x0 - OPEN_R + hx, y = y0 - 2 * OPEN_R + hy;
        signed char h = RANK_NONE;
        if (x >= 0 && x < W) {
            if (y < 0 || y >= H) {
                h = RANK_OUTSIDE;  // a row outside the image belongs to every cluster
            } else {
                const signed char r = A[hy][hx + OPEN_R];
                bool ok = r >= 0;
#pragma unroll
                for (int d = 0; d <= 2 * OPEN_R; d++) {
                    const signed char a = A[hy][hx + d];
                    ok = ok && (a == r || a == RANK_OUTSIDE);
                }
                if (ok) h = r;
            }
        }
        Hh[hy][hx] = h;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < OPEN_EY * OPEN_HX; i += 256) {
        const int ey = i / OPEN_HX, ex = i % OPEN_HX;
        const int x = x0 - OPEN_R + ex, y = y0 - OPEN_R + ey;
        bool ok = false;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const signed char r = Hh[ey + OPEN_R][ex];
            ok = r >= 0;
#pragma unroll
            for (int d = 0; d <= 2 * OPEN_R; d++) {
                const signed char a = Hh[ey + d][ex];
                ok = ok && (a == r || a == RANK_OUTSIDE);
            }
        }
        E[ey][ex] = ok ? 1 : 0;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < OPEN_EY * OPEN_TX; i += 256) {
        const int dy = i / OPEN_TX, dx = i % OPEN_TX;
        unsigned char any = 0;
#pragma unroll
        for (int d = 0; d <= 2 * OPEN_R; d++) any |= E[dy][dx + d];
        D[dy][dx] = any;
    }
    __syncthreads();
    const int ox = (int)threadIdx.x % OPEN_TX, oy = (int)threadIdx.x / OPEN_TX;
    const int x = x0 + ox, y = y0 + oy;
    if (x >= W || y >= H) return;
    unsigned char any = 0;
#pragma unroll
    for (int d = 0; d <= 2 * OPEN_R; d++) any |= D[oy + d][ox];
    // a survivor within the window of (x, y) has (x, y) within its own window: it has the rank of (x, y)
    const signed char r = A[oy + 2 * OPEN_R][ox + 2 * OPEN_R];
    cc_seed(v, y * W + x, any && r >= 0 ? r : RANK_NONE, rank, parent, size);
}

__global__ void __launch_bounds__(256) cc_unite_kernel(const CcView* __restrict__ views, const signed char* __restrict__ rank,
                                                       uint32_t* __restrict__ parent) {
    const CcView& v = views[blockIdx.y];
    const int W = v.maps.W, H = v.maps.H;
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= W * H) return;
    const uint32_t p = v.pix_base + (uint32_t)q;
    const signed char r = rank[p];
    if (r < 0) return;
    const int x = q % W, y = q / W;
    if (x > 0 && rank[p - 1] == r) uf_unite(parent, p, p - 1);
    if (y > 0) {
        const uint32_t up = p - (uint32_t)W;
        if (x > 0 && rank[up - 1] == r) uf_unite(parent, p, up - 1);
        if (rank[up] == r) uf_unite(parent, p, up);
        if (x < W - 1 && rank[up + 1] == r) uf_unite(parent, p, up + 1);
    }
}

// size[root] = the pixels below it; no early return: the waves vote.  The root is not stored: a halving store of another
// thread's find, which writes an ancestor it read earlier, could land on top of it.
__global__ void __launch_bounds__(256) cc_roots_kernel(const CcView* __restrict__ views, const signed char* __restrict__ rank,
                                                       uint32_t* __restrict__ parent, uint32_t* __restrict__ size) {
    const CcView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    const uint32_t p = v.pix_base + (uint32_t)q;
    const bool member = q < v.maps.W * v.maps.H && rank[p] >= 0;
    uint32_t root = 0u;
    if (member) root = uf_find(parent, p);
    wave_count(size, root, member);
}

__global__ void __launch_bounds__(256) cc_flags_kernel(const CcView* __restrict__ views, const signed char* __restrict__ rank,
                                                       const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                       uint32_t* __restrict__ flag) {
    const CcView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    const uint32_t p = v.pix_base + (uint32_t)q;
    flag[p] = rank[p] >= 0 && parent[p] == p && size[p] >= (uint32_t)v.min_size ? 1u : 0u;
}

// roots[pos] = the kept roots in pixel order; grid y = views
__global__ void __launch_bounds__(256) cc_compact_kernel(const CcView* __restrict__ views, const uint32_t* __restrict__ flag,
                                                         const uint32_t* __restrict__ pos, uint32_t* __restrict__ roots) {
    const CcView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    const uint32_t p = v.pix_base + (uint32_t)q;
    if (flag[p]) roots[pos[p]] = p;
}

// first[v] = the view's first kept root, first[n_views] = all of them; one workgroup
__global__ void __launch_bounds__(256) cc_first_kernel(const CcView* __restrict__ views, int n_views,
                                                       const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total,
                                                       uint32_t* __restrict__ first) {
    for (int v = (int)threadIdx.x; v <= n_views; v += 256) first[v] = v < n_views ? pos[views[v].pix_base] : *total;
}

// grid = (CC_MAX_RANKS, views): within[j] = the kept roots of j's rank before j in the view, rank_total = their number
__global__ void __launch_bounds__(256) cc_rank_index_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ roots,
                                                            const signed char* __restrict__ rank, uint32_t* __restrict__ within,
                                                            uint32_t* __restrict__ rank_total) {
    __shared__ uint32_t sm4[4];
    const uint32_t begin = first[blockIdx.y], end = first[blockIdx.y + 1];
    const int r = (int)blockIdx.x;
    uint32_t run = 0u;
    for (uint32_t b = begin; b < end; b += 256u) {  // block-uniform
        const uint32_t j = b + threadIdx.x;
        const bool match = j < end && rank[roots[j]] == r;
        uint32_t t;
        const uint32_t ex = block256_excl_scan_u32(match ? 1u : 0u, sm4, &t);
        if (match) within[j] = run + ex;
        run += t;
    }
    if (threadIdx.x == 0) rank_total[(size_t)blockIdx.y * CC_MAX_RANKS + r] = run;
}

// grid = (blocks of 256 roots of the largest view, views): id[root] and by_id[first + id] = root
__global__ void __launch_bounds__(256) cc_ids_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ roots,
                                                     const signed char* __restrict__ rank, const uint32_t* __restrict__ within,
                                                     const uint32_t* __restrict__ rank_total, uint32_t* __restrict__ id,
                                                     uint32_t* __restrict__ by_id) {
    const uint32_t begin = first[blockIdx.y], end = first[blockIdx.y + 1];
    const uint32_t j = begin + blockIdx.x * 256u + threadIdx.x;
    if (j >= end) return;
    const uint32_t root = roots[j];
    const int r = rank[root];
    uint32_t i = within[j];
    for (int s = 0; s < r; s++) i += rank_total[(size_t)blockIdx.y * CC_MAX_RANKS + s];
    id[root] = i;
    by_id[begin + i] = root;
}

__global__ void __launch_bounds__(256) cc_write_kernel(const CcView* __restrict__ views, const signed char* __restrict__ rank,
                                                       uint32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                       const uint32_t* __restrict__ id) {
    const CcView& v = views[blockIdx.y];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= v.maps.W * v.maps.H) return;
    const uint32_t p = v.pix_base + (uint32_t)q;
    int c = -1;
    if (rank[p] >= 0) {
        const uint32_t root = uf_find(parent, p);
        if (size[root] >= (uint32_t)v.min_size) c = (int)id[root];
    }
    v.out[q] = c;
}

// grid = (blocks of 256 components of the view with the most, views)
__global__ void __launch_bounds__(256) cc_sizes_kernel(const CcView* __restrict__ views, const uint32_t* __restrict__ first,
                                                       const uint32_t* __restrict__ by_id, const uint32_t* __restrict__ size) {
    const uint32_t begin = first[blockIdx.y], end = first[blockIdx.y + 1];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (begin + i >= end) return;
    views[blockIdx.y].out[i] = (int)size[by_id[begin + i]];
}

// ---------------------------------------------------------------------------------------------------------------------
// C. the join with the masks

// no early return: the waves vote
__global__ void __launch_bounds__(256) join_counts_kernel(const JoinView* __restrict__ views, uint32_t* __restrict__ areas,
                                                          uint32_t* __restrict__ pairs) {
    const JoinView& v = views[blockIdx.y];
    const size_t P = (size_t)v.maps.W * v.maps.H;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool inside = q < P;
    const int c = inside && v.n > 0 ? ((const int*)v.maps.depth)[q] : -1;
    for (int m = 0; m < v.M; m++) {
        const bool set = inside && v.masks[(size_t)m * P + q] != 0;
        const unsigned long long vote = __ballot(set);
        if (vote == 0ull) continue;  // wave-uniform
        if (lane_id() == 0) atomicAdd(areas + v.mask_base + m, (uint32_t)__builtin_popcountll(vote));
        wave_count(pairs + v.pair_base + (size_t)m * v.n, (uint32_t)c, set && c >= 0 && c < v.n);
    }
}

__global__ void __launch_bounds__(256) join_paint_kernel(const JoinView* __restrict__ views, const int* __restrict__ order,
                                                         const int* __restrict__ pair_ids, uint32_t* __restrict__ id_areas) {
    const JoinView& v = views[blockIdx.y];
    const size_t P = (size_t)v.maps.W * v.maps.H;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool inside = q < P;
    int id = 0;
    if (inside) {
        const int c = v.n > 0 ? ((const int*)v.maps.depth)[q] : -1;
        if (c >= 0 && c < v.n) {
            for (int j = v.M - 1; j >= 0; j--) {  // the last mask of the order that qualifies and holds the pixel
                const int m = order[v.mask_base + j];
                const int pid = pair_ids[v.pair_base + (size_t)m * v.n + c];
                if (pid != 0 && v.masks[(size_t)m * P + q] != 0) {
                    id = pid;
                    break;
                }
            }
        }
        v.seg[q] = id;
    }
    wave_count(id_areas + v.id_base, (uint32_t)id, inside && id > 0);
}

// round(clamp(x, -2, 2) 2^32), 0 for a NaN
__device__ __forceinline__ long long fixed32(float x) {
    if (x != x) return 0ll;
    const double c = fmin(fmax((double)x, -2.0), 2.0);
    return llrint(c * 4294967296.0);
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// no early return: the waves vote
__global__ void __launch_bounds__(256) join_relabel_kernel(const JoinView* __restrict__ views, const int* __restrict__ relabel,
                                                           unsigned long long* __restrict__ sums) {
    const JoinView& v = views[blockIdx.y];
    const size_t P = (size_t)v.maps.W * v.maps.H;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool inside = q < P;
    int id = 0;
    long long f[3] = {0ll, 0ll, 0ll};
    if (inside) {
        const int old = v.seg[q];
        id = old > 0 && old <= v.n_ids ? relabel[v.id_base + old] : 0;
        v.seg[q] = id;
        if (id > 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) f[c] = fixed32(v.maps.depth[3 * q + c]);
        }
    }
    unsigned long long todo = __ballot(id > 0);
    while (todo != 0ull) {  // wave-uniform
        const int k = __shfl(id, __builtin_ctzll(todo));
        const bool mine = id == k;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const long long s = wave_sum_i64(mine ? f[c] : 0ll);  // integer: any order gives the same sum
            if (lane_id() == 0) atomicAdd(sums + 3 * ((size_t)v.sum_base + k) + c, (unsigned long long)s);
        }
        todo &= ~__ballot(mine);
    }
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

inline long long km_spans(long long pixels) { return (pixels + KM_SPAN - 1) / KM_SPAN; }

struct KmLayout { size_t partials, next, shift2, tol_abs, state, bytes; };
KmLayout km_layout(int n_views, const int* sizes) {  // sizes have passed view_sizes_ok
    long long total_spans = 0;
    for (int v = 0; v < n_views; v++) total_spans += km_spans((long long)sizes[2 * v] * sizes[2 * v + 1]);
    WorkspaceCursor c;
    take_view_table<KmView>(c, n_views);
    KmLayout L{};
    L.partials = c.take((size_t)total_spans * KM_STRIDE * sizeof(double));
    L.next = c.take((size_t)n_views * KM_MAX_K * 3 * sizeof(float));
    L.shift2 = c.take((size_t)n_views * KM_MAX_K * sizeof(double));
    L.tol_abs = c.take((size_t)n_views * sizeof(double));
    L.state = c.take((size_t)n_views * 4 * sizeof(int));
    L.bytes = c.off;
    return L;
}

struct CcLayout { size_t rank, parent, size, flag, pos, roots, within, chunks, total, first, rank_total, bytes; };
CcLayout cc_layout(int n_views, long long pixels) {
    WorkspaceCursor c;
    take_view_table<CcView>(c, n_views);
    CcLayout L{};
    const size_t n = (size_t)pixels;
    L.rank = c.take(n);
    L.parent = c.take(n * 4);
    L.size = c.take(n * 4);
    L.flag = c.take(n * 4);  // the keep flags, then by_id
    L.pos = c.take(n * 4);   // the scan, then id
    L.roots = c.take(n * 4);
    L.within = c.take(n * 4);
    L.chunks = c.take((size_t)scan_chunks((long)pixels) * 4);
    L.total = c.take(8);
    L.first = c.take(((size_t)n_views + 1) * 4);
    L.rank_total = c.take((size_t)n_views * CC_MAX_RANKS * 4);
    L.bytes = c.off;
    return L;
}
constexpr long long CC_MAX_PIXELS = (1ll << 31) - 1;  // of all views: pixel indices are 32-bit and scan_u32 takes an int

// the checks of the counts [n_views] that size a join's tables: sum_i a[i] (+ extra each), below 2^31
bool table_total(int n_views, const int* a, const int* b, int extra, long long* total) {
    *total = 0;
    for (int v = 0; v < n_views; v++) {
        if (a[v] < 0 || (b && b[v] < 0)) return false;
        *total += (long long)(a[v] + extra) * (b ? b[v] : 1);
        if (*total >= (1ll << 31)) return false;
    }
    return true;
}

struct JoinLayout { size_t a, b, bytes; };  // two uploaded host tables behind the view table
JoinLayout join_layout(int n_views, long long na, long long nb) {
    WorkspaceCursor c;
    take_view_table<JoinView>(c, n_views);
    JoinLayout L{};
    L.a = c.take((size_t)na * 4);
    L.b = c.take((size_t)nb * 4);
    L.bytes = c.off;
    return L;
}

// the join's view table; `first` = the stack's leading map (components or normals)
int stage_join(const char* name, int n_views, const int* sizes, const void* const* first, const unsigned char* const* masks,
               int* const* seg, const int* n_masks, const int* n_components, const int* n_ids, const int* n_planes,
               char* workspace, hipStream_t stream, const JoinView** table) {
    int mask_base = 0, pair_base = 0, id_base = 0, sum_base = 0;
    return stage_views(name, n_views, true, sizes, (const float* const*)first, nullptr, false, workspace,
                       view_table_bytes<JoinView>(n_views), stream, table, [&](JoinView& u, int v) {
                           u.masks = masks ? masks[v] : nullptr;
                           u.seg = seg ? seg[v] : nullptr;
                           u.M = n_masks ? n_masks[v] : 0;
                           u.n = n_components ? n_components[v] : 0;
                           u.n_ids = n_ids ? n_ids[v] : 0;
                           u.mask_base = mask_base;
                           u.pair_base = pair_base;
                           u.id_base = id_base;
                           u.sum_base = sum_base;
                           mask_base += u.M;
                           pair_base += u.M * u.n;
                           id_base += n_ids ? n_ids[v] + 1 : 0;
                           sum_base += n_planes ? n_planes[v] + 1 : 0;
                       });
}

int check_masks(int n_views, const unsigned char* const* masks, const int* n_masks) {
    if (!masks || !n_masks) return null_pointer();
    for (int v = 0; v < n_views; v++) {
        if (n_masks[v] < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "n_masks[%d] must not be negative", v);
        if (n_masks[v] > 0 && !masks[v]) return fail(G4S_ERR_INVALID_ARGUMENT, "masks[%d]: NULL pointer", v);
    }
    return G4S_OK;
}

}  // namespace

extern "C" size_t g4s_kmeans_normals_workspace(int n_views, const int* sizes) {
    long long largest, total;
    if (!grid_views_ok(n_views) || !view_sizes_ok(n_views, sizes, &largest, &total)) return 0;
    return km_layout(n_views, sizes).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_kmeans_normals(int n_views, const int* sizes, const float* const* normals, int k, const float* init,
                                  int max_iter, double tol, signed char* const* labels, float* centres, int* counts,
                                  int* n_iter, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (k < 1 || k > KM_MAX_K) return fail(G4S_ERR_INVALID_ARGUMENT, "k must be in 1 .. %d", KM_MAX_K);
    if (max_iter < 1) return fail(G4S_ERR_INVALID_ARGUMENT, "max_iter must be at least 1");
    if (!(tol >= 0.0)) return fail(G4S_ERR_INVALID_ARGUMENT, "tol must not be negative or NaN");
    if (n_views == 0) return G4S_OK;
    if (check_pointers("normals", normals, n_views) != G4S_OK || check_pointers("labels", labels, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!init || !centres || !counts || !n_iter) return null_pointer();
    for (int i = 0; i < 3 * k * n_views; i++) {
        if (!finite(init[i])) return fail(G4S_ERR_INVALID_ARGUMENT, "init: view %d is not finite", i / (3 * k));
    }
    if (check_workspace(workspace, workspace_bytes, g4s_kmeans_normals_workspace(n_views, sizes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const KmLayout L = km_layout(n_views, sizes);
    double* partials = workspace_at<double>(workspace, L.partials);
    float* next = workspace_at<float>(workspace, L.next);
    double* shift2 = workspace_at<double>(workspace, L.shift2);
    double* tol_abs = workspace_at<double>(workspace, L.tol_abs);
    int* state = workspace_at<int>(workspace, L.state);
    hipError_t e = upload(centres, init, (size_t)n_views * k * 3 * sizeof(float), stream);
    if (e != hipSuccess) return finish(e, "k-means");
    uint32_t base = 0, most = 0;
    const KmView* table;
    const int rc = stage_views("k-means", n_views, true, sizes, normals, nullptr, false, workspace,
                               view_table_bytes<KmView>(n_views), stream, &table, [&](KmView& u, int v) {
                                   u.labels = labels[v];
                                   u.block_base = base;
                                   u.n_blocks = (uint32_t)km_spans((long long)sizes[2 * v] * sizes[2 * v + 1]);
                                   base += u.n_blocks;
                                   if (u.n_blocks > most) most = u.n_blocks;
                               });
    if (rc != G4S_OK) return rc;
    const dim3 spans(most, (unsigned)n_views), per_cluster((unsigned)k, (unsigned)n_views), per_view((unsigned)n_views);
    hipLaunchKernelGGL(km_moments_kernel, spans, dim3(256), 0, stream, table, partials);
    hipLaunchKernelGGL(km_tolerance_kernel, per_view, dim3(64), 0, stream, table, (const double*)partials, tol, tol_abs, state);
    std::vector<int> host((size_t)n_views * 4);
    const auto read_state = [&]() {
        hipError_t r = hipGetLastError();
        if (r == hipSuccess) r = hipMemcpyAsync(host.data(), state, host.size() * sizeof(int), hipMemcpyDeviceToHost, stream);
        if (r == hipSuccess) r = hipStreamSynchronize(stream);
        return r;
    };
    for (int iter = 1; iter <= max_iter; iter++) {
        hipLaunchKernelGGL(km_assign_kernel, spans, dim3(256), 0, stream, table, k, (const float*)centres, state, partials,
                           (int)KM_RUNNING, iter == 1 ? 1 : 0);
        hipLaunchKernelGGL(km_update_kernel, per_cluster, dim3(64), 0, stream, table, k, (const float*)centres, next, shift2,
                           counts, (const int*)state, (const double*)partials, (int)KM_RUNNING);
        hipLaunchKernelGGL(km_finalise_kernel, per_view, dim3(64), 0, stream, k, centres, (const float*)next,
                           (const double*)shift2, (const double*)tol_abs, state, iter, max_iter);
        if (iter % KM_POLL != 0 || iter == max_iter) continue;
        if ((e = read_state()) != hipSuccess) return finish(e, "k-means");
        bool running = false;
        for (int v = 0; v < n_views; v++) running = running || host[4 * (size_t)v] == KM_RUNNING;
        if (!running) break;
    }
    hipLaunchKernelGGL(km_assign_kernel, spans, dim3(256), 0, stream, table, k, (const float*)centres, state, partials,
                       (int)KM_REASSIGN, 0);
    hipLaunchKernelGGL(km_update_kernel, per_cluster, dim3(64), 0, stream, table, k, (const float*)centres, next, shift2, counts,
                       (const int*)state, (const double*)partials, (int)KM_REASSIGN);
    if ((e = read_state()) != hipSuccess) return finish(e, "k-means");
    for (int v = 0; v < n_views; v++) n_iter[v] = host[4 * (size_t)v + 1];
    return finish(hipSuccess, "k-means");
}

extern "C" size_t g4s_normal_components_workspace(int n_views, const int* sizes) {
    long long largest, total;
    if (!grid_views_ok(n_views) || !view_sizes_ok(n_views, sizes, &largest, &total) || total > CC_MAX_PIXELS) return 0;
    return cc_layout(n_views, total).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_normal_components_count(int n_views, const int* sizes, const signed char* const* labels, const int* lut,
                                           int open, const int* min_size, signed char* const* opened, int* const* components,
                                           int* n, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (total > CC_MAX_PIXELS) return fail(G4S_ERR_INVALID_ARGUMENT, "the views must have fewer than 2^31 pixels together");
    if (n_views == 0) return G4S_OK;
    if (check_pointers("labels", labels, n_views) != G4S_OK || check_pointers("components", components, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!lut || !min_size || !n) return null_pointer();
    for (int i = 0; i < CC_MAX_RANKS * n_views; i++) {
        if (lut[i] < -1 || lut[i] >= CC_MAX_RANKS)
            return fail(G4S_ERR_INVALID_ARGUMENT, "lut: view %d: a rank must be in -1 .. %d", i / CC_MAX_RANKS, CC_MAX_RANKS - 1);
    }
    for (int v = 0; v < n_views; v++) {
        if (min_size[v] < 1) return fail(G4S_ERR_INVALID_ARGUMENT, "min_size[%d] must be at least 1", v);
    }
    if (check_workspace(workspace, workspace_bytes, g4s_normal_components_workspace(n_views, sizes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const CcLayout L = cc_layout(n_views, total);
    signed char* rank = workspace_at<signed char>(workspace, L.rank);
    uint32_t* parent = workspace_at<uint32_t>(workspace, L.parent);
    uint32_t* size = workspace_at<uint32_t>(workspace, L.size);
    uint32_t* flag = workspace_at<uint32_t>(workspace, L.flag);
    uint32_t* pos = workspace_at<uint32_t>(workspace, L.pos);
    uint32_t* roots = workspace_at<uint32_t>(workspace, L.roots);
    uint32_t* within = workspace_at<uint32_t>(workspace, L.within);
    uint32_t* chunks = workspace_at<uint32_t>(workspace, L.chunks);
    uint32_t* d_total = workspace_at<uint32_t>(workspace, L.total);
    uint32_t* first = workspace_at<uint32_t>(workspace, L.first);
    uint32_t* rank_total = workspace_at<uint32_t>(workspace, L.rank_total);
    uint32_t base = 0;
    unsigned most_tiles = 0;
    const CcView* table;
    const int rc = stage_views("normal components", n_views, true, sizes, (const float* const*)labels, nullptr, false, workspace,
                               view_table_bytes<CcView>(n_views), stream, &table, [&](CcView& u, int v) {
                                   const int W = sizes[2 * v], H = sizes[2 * v + 1];
                                   u.out = components[v];
                                   u.opened = opened ? opened[v] : nullptr;
                                   u.pix_base = base;
                                   u.min_size = min_size[v];
                                   for (int i = 0; i < CC_MAX_RANKS; i++) u.lut[i] = (signed char)lut[CC_MAX_RANKS * v + i];
                                   base += (uint32_t)(W * H);
                                   const unsigned tiles = (unsigned)(((W + OPEN_TX - 1) / OPEN_TX) * ((H + OPEN_TY - 1) / OPEN_TY));
                                   if (tiles > most_tiles) most_tiles = tiles;
                               });
    if (rc != G4S_OK) return rc;
    const dim3 pixels(blocks256(largest), (unsigned)n_views);
    if (open)
        hipLaunchKernelGGL(cc_open_kernel, dim3(most_tiles, (unsigned)n_views), dim3(256), 0, stream, table, rank, parent, size);
    else
        hipLaunchKernelGGL(cc_ranks_kernel, pixels, dim3(256), 0, stream, table, rank, parent, size);
    hipLaunchKernelGGL(cc_unite_kernel, pixels, dim3(256), 0, stream, table, (const signed char*)rank, parent);
    hipLaunchKernelGGL(cc_roots_kernel, pixels, dim3(256), 0, stream, table, (const signed char*)rank, parent, size);
    hipLaunchKernelGGL(cc_flags_kernel, pixels, dim3(256), 0, stream, table, (const signed char*)rank, (const uint32_t*)parent,
                       (const uint32_t*)size, flag);
    scan_u32(flag, pos, (int)total, chunks, d_total, stream);
    hipLaunchKernelGGL(cc_compact_kernel, pixels, dim3(256), 0, stream, table, (const uint32_t*)flag, (const uint32_t*)pos, roots);
    hipLaunchKernelGGL(cc_first_kernel, dim3(1), dim3(256), 0, stream, table, n_views, (const uint32_t*)pos,
                       (const uint32_t*)d_total, first);
    hipLaunchKernelGGL(cc_rank_index_kernel, dim3(CC_MAX_RANKS, (unsigned)n_views), dim3(256), 0, stream, (const uint32_t*)first,
                       (const uint32_t*)roots, (const signed char*)rank, within, rank_total);
    // a view has at most a root per pixel: the grid of the largest view covers every view's roots
    hipLaunchKernelGGL(cc_ids_kernel, pixels, dim3(256), 0, stream, (const uint32_t*)first, (const uint32_t*)roots,
                       (const signed char*)rank, (const uint32_t*)within, (const uint32_t*)rank_total, pos, flag);
    hipLaunchKernelGGL(cc_write_kernel, pixels, dim3(256), 0, stream, table, (const signed char*)rank, parent,
                       (const uint32_t*)size, (const uint32_t*)pos);
    std::vector<uint32_t> host((size_t)n_views + 1);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), first, host.size() * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return finish(e, "normal components");
    for (int v = 0; v < n_views; v++) n[v] = (int)(host[(size_t)v + 1] - host[(size_t)v]);
    return finish(hipSuccess, "normal components");
}

extern "C" int g4s_normal_components_sizes(int n_views, const int* sizes, const int* n, int* const* component_sizes,
                                           char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (total > CC_MAX_PIXELS) return fail(G4S_ERR_INVALID_ARGUMENT, "the views must have fewer than 2^31 pixels together");
    if (n_views == 0) return G4S_OK;
    if (!n || !component_sizes) return null_pointer();
    int most = 0;
    for (int v = 0; v < n_views; v++) {
        if (n[v] < 0 || n[v] > (long long)sizes[2 * v] * sizes[2 * v + 1])
            return fail(G4S_ERR_INVALID_ARGUMENT, "n[%d] must be the count of the view", v);
        if (n[v] > 0 && !component_sizes[v]) return fail(G4S_ERR_INVALID_ARGUMENT, "component_sizes[%d]: NULL pointer", v);
        if (n[v] > most) most = n[v];
    }
    if (check_workspace(workspace, workspace_bytes, g4s_normal_components_workspace(n_views, sizes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (most == 0) return G4S_OK;
    const CcLayout L = cc_layout(n_views, total);
    // The count phase left the arrays behind the table; the table is staged again with the outputs of this phase.  The
    // kernel reads the bounds of a view from `first`, which the count phase wrote: an n[v] that is not the count is ignored.
    const std::vector<const float*> unused((size_t)n_views, (const float*)workspace);
    const CcView* table;
    const int rc = stage_views("normal component sizes", n_views, true, sizes, unused.data(), nullptr, false, workspace,
                               view_table_bytes<CcView>(n_views), stream, &table, [&](CcView& u, int v) {
                                   u.out = component_sizes[v];
                                   u.opened = nullptr;
                                   u.pix_base = 0;
                                   u.min_size = 0;
                                   for (int i = 0; i < CC_MAX_RANKS; i++) u.lut[i] = RANK_NONE;
                               });
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(blocks256(most), (unsigned)n_views), dim3(256), 0, stream, table,
                       (const uint32_t*)workspace_at<uint32_t>(workspace, L.first),
                       (const uint32_t*)workspace_at<uint32_t>(workspace, L.flag),
                       (const uint32_t*)workspace_at<uint32_t>(workspace, L.size));
    return finish(hipSuccess, "normal component sizes");
}

extern "C" size_t g4s_plane_pair_counts_workspace(int n_views) {
    return !grid_views_ok(n_views) ? 0 : view_table_bytes<JoinView>(n_views);
}

extern "C" int g4s_plane_pair_counts(int n_views, const int* sizes, const int* const* components,
                                     const unsigned char* const* masks, const int* n_masks, const int* n_components, int* areas,
                                     int* pairs, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return G4S_OK;
    if (check_pointers("components", components, n_views) != G4S_OK || check_masks(n_views, masks, n_masks) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!n_components) return null_pointer();
    long long total_masks, total_pairs;
    if (!table_total(n_views, n_masks, nullptr, 0, &total_masks) || !table_total(n_views, n_masks, n_components, 0, &total_pairs))
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_masks, n_components: not negative, and fewer than 2^31 pairs");
    if ((total_masks > 0 && !areas) || (total_pairs > 0 && !pairs)) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_plane_pair_counts_workspace(n_views)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (total_masks == 0) return G4S_OK;
    hipError_t e = hipMemsetAsync(areas, 0, (size_t)total_masks * 4, stream);
    if (e == hipSuccess && total_pairs > 0) e = hipMemsetAsync(pairs, 0, (size_t)total_pairs * 4, stream);
    if (e != hipSuccess) return finish(e, "plane pair counts");
    const JoinView* table;
    const int rc = stage_join("plane pair counts", n_views, sizes, (const void* const*)components, masks, nullptr, n_masks,
                              n_components, nullptr, nullptr, workspace, stream, &table);
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(join_counts_kernel, dim3(blocks256(largest), (unsigned)n_views), dim3(256), 0, stream, table,
                       (uint32_t*)areas, (uint32_t*)pairs);
    return finish(hipSuccess, "plane pair counts");
}

extern "C" size_t g4s_plane_paint_workspace(int n_views, int total_masks, int total_pairs) {
    if (!grid_views_ok(n_views) || total_masks < 0 || total_pairs < 0) return 0;
    return join_layout(n_views, total_masks, total_pairs).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_plane_paint(int n_views, const int* sizes, const int* const* components, const unsigned char* const* masks,
                               const int* n_masks, const int* n_components, const int* order, const int* pair_ids,
                               const int* n_ids, int* const* seg, int* id_areas, char* workspace, size_t workspace_bytes,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return G4S_OK;
    if (check_pointers("components", components, n_views) != G4S_OK || check_masks(n_views, masks, n_masks) != G4S_OK ||
        check_pointers("seg", seg, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!n_components || !n_ids || !id_areas) return null_pointer();
    long long total_masks, total_pairs, total_ids;
    if (!table_total(n_views, n_masks, nullptr, 0, &total_masks) ||
        !table_total(n_views, n_masks, n_components, 0, &total_pairs) || !table_total(n_views, n_ids, nullptr, 1, &total_ids))
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_masks, n_components, n_ids: not negative, and fewer than 2^31 pairs and ids");
    if ((total_masks > 0 && !order) || (total_pairs > 0 && !pair_ids)) return null_pointer();
    int mask_base = 0, pair_base = 0;
    for (int v = 0; v < n_views; v++) {  // order: a permutation of the view's masks; pair ids: 0 or 1 .. n_ids
        std::vector<char> seen((size_t)n_masks[v], 0);
        for (int j = 0; j < n_masks[v]; j++) {
            const int m = order[mask_base + j];
            if (m < 0 || m >= n_masks[v] || seen[(size_t)m])
                return fail(G4S_ERR_INVALID_ARGUMENT, "order: view %d: not a permutation of its masks", v);
            seen[(size_t)m] = 1;
        }
        for (int i = 0; i < n_masks[v] * n_components[v]; i++) {
            if (pair_ids[pair_base + i] < 0 || pair_ids[pair_base + i] > n_ids[v])
                return fail(G4S_ERR_INVALID_ARGUMENT, "pair_ids: view %d: an id must be in 0 .. n_ids", v);
        }
        mask_base += n_masks[v];
        pair_base += n_masks[v] * n_components[v];
    }
    if (check_workspace(workspace, workspace_bytes, g4s_plane_paint_workspace(n_views, (int)total_masks, (int)total_pairs)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const JoinLayout L = join_layout(n_views, total_masks, total_pairs);
    int* dev_order = workspace_at<int>(workspace, L.a);
    int* dev_pairs = workspace_at<int>(workspace, L.b);
    hipError_t e = hipMemsetAsync(id_areas, 0, (size_t)total_ids * 4, stream);
    if (e == hipSuccess && total_masks > 0) e = upload(dev_order, order, (size_t)total_masks * 4, stream);
    if (e == hipSuccess && total_pairs > 0) e = upload(dev_pairs, pair_ids, (size_t)total_pairs * 4, stream);
    if (e != hipSuccess) return finish(e, "plane paint");
    const JoinView* table;
    const int rc = stage_join("plane paint", n_views, sizes, (const void* const*)components, masks, seg, n_masks, n_components,
                              n_ids, nullptr, workspace, stream, &table);
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(join_paint_kernel, dim3(blocks256(largest), (unsigned)n_views), dim3(256), 0, stream, table,
                       (const int*)dev_order, (const int*)dev_pairs, (uint32_t*)id_areas);
    return finish(hipSuccess, "plane paint");
}

extern "C" size_t g4s_plane_relabel_workspace(int n_views, int total_ids) {
    if (!grid_views_ok(n_views) || total_ids < 0) return 0;
    return join_layout(n_views, total_ids, 0).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_plane_relabel(int n_views, const int* sizes, int* const* seg, const float* const* normals, const int* n_ids,
                                 const int* relabel, const int* n_planes, long long* sums, char* workspace,
                                 size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_views == 0) return G4S_OK;
    if (check_pointers("seg", seg, n_views) != G4S_OK || check_pointers("normals", normals, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (!n_ids || !relabel || !n_planes || !sums) return null_pointer();
    long long total_ids, total_planes;
    if (!table_total(n_views, n_ids, nullptr, 1, &total_ids) || !table_total(n_views, n_planes, nullptr, 1, &total_planes))
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_ids, n_planes: not negative, and fewer than 2^31 together");
    int id_base = 0;
    for (int v = 0; v < n_views; v++) {
        for (int i = 0; i <= n_ids[v]; i++) {
            const int r = relabel[id_base + i];
            if (r < 0 || r > n_planes[v] || (i == 0 && r != 0))
                return fail(G4S_ERR_INVALID_ARGUMENT, "relabel: view %d: a plane must be in 0 .. n_planes, and 0 stays 0", v);
        }
        id_base += n_ids[v] + 1;
    }
    if (check_workspace(workspace, workspace_bytes, g4s_plane_relabel_workspace(n_views, (int)total_ids)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    int* dev_relabel = workspace_at<int>(workspace, join_layout(n_views, total_ids, 0).a);
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)total_planes * 3 * sizeof(long long), stream);
    if (e == hipSuccess) e = upload(dev_relabel, relabel, (size_t)total_ids * 4, stream);
    if (e != hipSuccess) return finish(e, "plane relabel");
    const JoinView* table;
    const int rc = stage_join("plane relabel", n_views, sizes, (const void* const*)normals, nullptr, seg, nullptr, nullptr, n_ids,
                              n_planes, workspace, stream, &table);
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(join_relabel_kernel, dim3(blocks256(largest), (unsigned)n_views), dim3(256), 0, stream, table,
                       (const int*)dev_relabel, (unsigned long long*)sums);
    return finish(hipSuccess, "plane relabel");
}
