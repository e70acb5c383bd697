// Global plane fit (include/g4s_render_maps.h, "Plane fit"; the semantics stated there are the contract, tests/plane_fit_ref.py
// restates them in numpy): the valid pixels of every (plane, view) pair as world points and normals, the members of every
// pair's top normal cluster per plane, the plane hypotheses of sampled point triples, their inlier counts, and the refit
// over the inliers of the chosen hypothesis.
//
//   gather      grid = (blocks of 256 pixels of the largest view, pairs): count, scan.h's scan over the blocks of all pairs,
//               emit by the block's rank.  The point is vis_view.h's back-projection, the one g4s_depth_to_points uses.
//   members     a flag per gathered row (its k-means label is its pair's top label), the scan, the copy.
//   hypotheses  one thread per (plane, trial): pf_solve, float64, + - * / sqrt only.
//   score       grid = (spans of SC_SPAN points of the largest plane, planes).  A thread keeps SC_ITEMS points in registers
//               as float64; the plane's hypotheses pass through LDS in chunks of SC_CHUNK, every lane reads the same address;
//               a wave counts by ballot and population count into the chunk's integer LDS counters, and the workgroup adds
//               each counter to the global table once.
//   refit       the inlier mask and the float64 sums of x and x x^T in the k-means kernels' order (a workgroup per
//               RF_SPAN points, the fixed tree, the fold by index), then one wave per plane folds and lane 0 solves.
// No float atomics; the integer ones are sums, which do not depend on the order.
#include <math.h>
#include <vector>

#include "../g4s_internal.h"
#include "../fixed_sums.h"
#include "../../../include/g4s_render_maps.h"
#include "mesh_common.h"
#include "scan.h"
#include "vis_view.h"
#include "view_stack.h"
#include "wave_count.h"

namespace g4s {

constexpr int SC_ITEMS = 8;                // points per thread of the scoring kernel
constexpr int SC_SPAN = 256 * SC_ITEMS;    // points one workgroup of the scoring kernel holds
constexpr int SC_CHUNK = 256;              // hypotheses staged in LDS at a time
constexpr int RF_ITEMS = 16;
constexpr int RF_SPAN = 256 * RF_ITEMS;    // points one workgroup of the moment sums reduces
constexpr int RF_TERMS = 10;               // count, x, y, z, xx, xy, xz, yy, yz, zz
constexpr int PF_SWEEPS = G4S_PLANE_FIT_SWEEPS;
constexpr int PF_BISECT = G4S_PLANE_FIT_BISECTIONS;
static_assert(SC_SPAN == G4S_PLANE_FIT_SCORE_SPAN && RF_SPAN == G4S_PLANE_FIT_SUM_SPAN, "the header states the spans");
constexpr int PF_MAX_TRIALS = 1 << 20;

struct PfView {
    ViewMaps maps;  // depth
    const float* normals;
    const int* mask;
    const unsigned char* conf;
    VisRay ray;
};

struct PfPair {
    int view, id;
    uint32_t block_base, n_blocks;  // the pair's blocks of 256 pixels among all pairs' blocks
    long long out;                  // first output row, or -1: the pair is skipped
    uint32_t count;                 // the rows the pair may write
};

struct PfRun {  // the gathered rows of one pair
    uint32_t begin, n;
    int top;
};

struct PfPlane {
    long long begin;  // first row of plane_points
    int n, best;
    uint32_t sc_blocks, rf_base, rf_blocks;
    double prior[3];
};

// ---------------------------------------------------------------------------------------------------------------------
// A. gather

__device__ __forceinline__ bool pf_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }

__device__ __forceinline__ bool pf_valid(const PfView& v, size_t q, int id) {
    if (v.mask[q] != id || v.conf[q] == 0) return false;
    return pf_finite(v.normals[3 * q]) && pf_finite(v.normals[3 * q + 1]) && pf_finite(v.normals[3 * q + 2]) &&
           pf_finite(v.maps.depth[q]);
}

__global__ void __launch_bounds__(256) pf_gather_count_kernel(const PfView* __restrict__ views, const PfPair* __restrict__ pairs,
                                                              uint32_t* __restrict__ counts) {
    __shared__ uint32_t sm4[4];
    const PfPair& pr = pairs[blockIdx.y];
    if (blockIdx.x >= pr.n_blocks) return;  // block-uniform
    const PfView& v = views[pr.view];
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < (size_t)v.maps.W * v.maps.H && pf_valid(v, q, pr.id);
    uint32_t total;
    (void)block256_excl_scan_u32(valid ? 1u : 0u, sm4, &total);
    if (threadIdx.x == 0) counts[pr.block_base + blockIdx.x] = total;
}

// first[e] = the rows before pair e among all pairs' valid pixels, first[n_pairs] = all of them; one workgroup
__global__ void __launch_bounds__(256) pf_pair_first_kernel(const PfPair* __restrict__ pairs, int n_pairs,
                                                            const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total,
                                                            uint32_t* __restrict__ first) {
    for (int e = (int)threadIdx.x; e <= n_pairs; e += 256) first[e] = e < n_pairs ? pos[pairs[e].block_base] : *total;
}

__global__ void __launch_bounds__(256) pf_gather_emit_kernel(const PfView* __restrict__ views, const PfPair* __restrict__ pairs,
                                                             const uint32_t* __restrict__ pos, float* __restrict__ points,
                                                             float* __restrict__ normals) {
    __shared__ uint32_t sm4[4];
    const PfPair& pr = pairs[blockIdx.y];
    if (blockIdx.x >= pr.n_blocks || pr.out < 0) return;  // block-uniform
    const PfView& v = views[pr.view];
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < (size_t)v.maps.W * v.maps.H && pf_valid(v, q, pr.id);
    uint32_t total;
    const uint32_t rank = block256_excl_scan_u32(valid ? 1u : 0u, sm4, &total);
    if (!valid) return;
    const uint32_t local = (pos[pr.block_base + blockIdx.x] - pos[pr.block_base]) + rank;
    if (local >= pr.count) return;  // maps that changed since the count phase cannot write past the pair's rows
    const size_t row = (size_t)pr.out + local;
    float p[3];
    pixel_point(v.ray, v.maps.W, (int)q, v.maps.depth[q], p);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        points[3 * row + c] = p[c];
        normals[3 * row + c] = v.normals[3 * q + c];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// B. members

__global__ void __launch_bounds__(256) pf_member_flags_kernel(const PfRun* __restrict__ runs, const signed char* __restrict__ labels,
                                                              uint32_t* __restrict__ flag) {
    const PfRun& r = runs[blockIdx.y];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n) return;
    flag[r.begin + i] = (int)labels[r.begin + i] == r.top ? 1u : 0u;
}

// first[p] = the members before plane p, first[n_planes] = all of them; rows[p] = the plane's first gathered row
__global__ void __launch_bounds__(256) pf_plane_first_kernel(const int* __restrict__ rows, int n_planes, int n_rows,
                                                             const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total,
                                                             uint32_t* __restrict__ first) {
    for (int p = (int)threadIdx.x; p <= n_planes; p += 256) first[p] = rows[p] < n_rows ? pos[rows[p]] : *total;
}

__global__ void __launch_bounds__(256) pf_member_emit_kernel(int n_rows, uint32_t n_members, const uint32_t* __restrict__ flag,
                                                             const uint32_t* __restrict__ pos, const float* __restrict__ points,
                                                             float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n_rows || flag[i] == 0u || pos[i] >= n_members) return;
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * (size_t)pos[i] + c] = points[3 * i + c];
}

// ---------------------------------------------------------------------------------------------------------------------
// C. the solver: the unit n that minimises n^T C n + alpha (1 - |n . p|)^2, and d = -n . c.  Every operation is the
// header's, in its order; a select evaluates both sides (a division by zero is harmless here and its result unused).

__device__ __forceinline__ void pf_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                          double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double tf = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double ts = theta < 0.0 ? -tf : tf;
    const double t = apq != 0.0 ? ts : 0.0;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0;
    v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1;
    v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2;
    v2q = s * a2 + c * b2;
}

// columns i and j of (l, V) change places when l[j] < l[i]
__device__ __forceinline__ void pf_order(double& li, double& lj, double& v0i, double& v0j, double& v1i, double& v1j, double& v2i,
                                         double& v2j) {
    if (lj < li) {
        double t = li; li = lj; lj = t;
        t = v0i; v0i = v0j; v0j = t;
        t = v1i; v1i = v1j; v1j = t;
        t = v2i; v2i = v2j; v2j = t;
    }
}

// the component of largest magnitude (the first of equals) becomes positive
__device__ __forceinline__ void pf_sign(double& v0, double& v1, double& v2) {
    double big = v0;
    if (fabs(v1) > fabs(big)) big = v1;
    if (fabs(v2) > fabs(big)) big = v2;
    if (big < 0.0) v0 = -v0, v1 = -v1, v2 = -v2;
}

__device__ __forceinline__ double pf_ratio(double b, double den) { return b == 0.0 ? 0.0 : b / den; }

// C = (xx, xy, xz, yy, yz, zz)
__device__ __forceinline__ void pf_solve(const double (&cen)[3], const double (&C)[6], bool has_prior, const double (&p)[3],
                                      double alpha, double (&out)[4]) {
    double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
    if (has_prior) {
        const double q0 = alpha * p[0], q1 = alpha * p[1], q2 = alpha * p[2];
        a00 = a00 + q0 * p[0];
        a01 = a01 + q0 * p[1];
        a02 = a02 + q0 * p[2];
        a11 = a11 + q1 * p[1];
        a12 = a12 + q1 * p[2];
        a22 = a22 + q2 * p[2];
    }
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < PF_SWEEPS; sweep++) {
        pf_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        pf_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        pf_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    double l0 = a00, l1 = a11, l2 = a22;
    pf_order(l0, l1, v00, v01, v10, v11, v20, v21);
    pf_order(l1, l2, v01, v02, v11, v12, v21, v22);
    pf_order(l0, l1, v00, v01, v10, v11, v20, v21);
    pf_sign(v00, v10, v20);
    pf_sign(v01, v11, v21);
    pf_sign(v02, v12, v22);
    double y0 = 1.0, y1 = 0.0, y2 = 0.0;
    if (has_prior) {
        const double b0 = alpha * ((v00 * p[0] + v10 * p[1]) + v20 * p[2]);
        const double b1 = alpha * ((v01 * p[0] + v11 * p[1]) + v21 * p[2]);
        const double b2 = alpha * ((v02 * p[0] + v12 * p[1]) + v22 * p[2]);
        const double g1 = l1 - l0, g2 = l2 - l0;
        const double h1 = pf_ratio(b1, g1), h2 = pf_ratio(b2, g2);
        const double hh = h1 * h1 + h2 * h2;
        double lo = 0.0, hi = alpha;
#pragma unroll 1
        for (int it = 0; it < PF_BISECT; it++) {
            const double mid = (lo + hi) * 0.5;
            const double t0 = pf_ratio(b0, mid), t1 = pf_ratio(b1, g1 + mid), t2 = pf_ratio(b2, g2 + mid);
            const double s = (t0 * t0 + t1 * t1) + t2 * t2;
            if (s > 1.0) lo = mid; else hi = mid;
        }
        if (b0 == 0.0 && hh < 1.0) {  // the hard case: the vector is completed along the smallest eigenvector
            y0 = sqrt(1.0 - hh);
            y1 = h1;
            y2 = h2;
        } else {
            y0 = pf_ratio(b0, hi);
            y1 = pf_ratio(b1, g1 + hi);
            y2 = pf_ratio(b2, g2 + hi);
        }
    }
    const double n0 = (v00 * y0 + v01 * y1) + v02 * y2;
    const double n1 = (v10 * y0 + v11 * y1) + v12 * y2;
    const double n2 = (v20 * y0 + v21 * y1) + v22 * y2;
    const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    out[0] = n0 / nn;
    out[1] = n1 / nn;
    out[2] = n2 / nn;
    out[3] = -((out[0] * cen[0] + out[1] * cen[1]) + out[2] * cen[2]);
}

// grid = (blocks of 256 trials, planes)
__global__ void __launch_bounds__(256) pf_hypotheses_kernel(const PfPlane* __restrict__ planes, const float* __restrict__ points,
                                                            int T, const int* __restrict__ samples, int has_prior, double alpha,
                                                            double* __restrict__ hyp) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= T) return;
    const PfPlane& pl = planes[blockIdx.y];
    const size_t row = (size_t)blockIdx.y * T + t;
    const int i0 = samples[3 * row], i1 = samples[3 * row + 1], i2 = samples[3 * row + 2];
    double* out = hyp + 4 * row;
    if (i0 < 0 || i0 >= pl.n || i1 < 0 || i1 >= pl.n || i2 < 0 || i2 >= pl.n) {  // never read outside the plane's points
        out[0] = out[1] = out[2] = out[3] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const float* a = points + 3 * ((size_t)pl.begin + i0);
    const float* b = points + 3 * ((size_t)pl.begin + i1);
    const float* c = points + 3 * ((size_t)pl.begin + i2);
    double cen[3], d[3][3], C[6], r[4];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x0 = (double)a[k], x1 = (double)b[k], x2 = (double)c[k];
        cen[k] = ((x0 + x1) + x2) / 3.0;
        d[0][k] = x0 - cen[k];
        d[1][k] = x1 - cen[k];
        d[2][k] = x2 - cen[k];
    }
    int m = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = i; j < 3; j++) C[m++] = ((d[0][i] * d[0][j] + d[1][i] * d[1][j]) + d[2][i] * d[2][j]) / 3.0;
    }
    pf_solve(cen, C, has_prior != 0, pl.prior, alpha, r);
    out[0] = r[0], out[1] = r[1], out[2] = r[2], out[3] = r[3];
}

// ---------------------------------------------------------------------------------------------------------------------
// D. scoring

__global__ void __launch_bounds__(256) pf_score_kernel(const PfPlane* __restrict__ planes, const float* __restrict__ points, int T,
                                                       const double* __restrict__ hyp, double threshold, int* __restrict__ counts) {
    const PfPlane& pl = planes[blockIdx.y];
    if (blockIdx.x >= pl.sc_blocks) return;  // block-uniform
    __shared__ double h[4 * SC_CHUNK];
    __shared__ int cnt[SC_CHUNK];
    double x[SC_ITEMS], y[SC_ITEMS], z[SC_ITEMS];
#pragma unroll
    for (int k = 0; k < SC_ITEMS; k++) {
        const size_t i = (size_t)blockIdx.x * SC_SPAN + (size_t)k * 256 + threadIdx.x;
        x[k] = __longlong_as_double(0x7ff8000000000000ll);  // no point: a NaN is within no threshold
        y[k] = z[k] = 0.0;
        if (i < (size_t)pl.n) {
            const float* p = points + 3 * ((size_t)pl.begin + i);
            x[k] = (double)p[0], y[k] = (double)p[1], z[k] = (double)p[2];
        }
    }
    const double* mine = hyp + 4 * (size_t)blockIdx.y * T;
    int* table = counts + (size_t)blockIdx.y * T;
    for (int t0 = 0; t0 < T; t0 += SC_CHUNK) {  // block-uniform
        const int m = T - t0 < SC_CHUNK ? T - t0 : SC_CHUNK;
        __syncthreads();  // the chunk before is done with h and cnt
        for (int j = (int)threadIdx.x; j < 4 * m; j += 256) h[j] = mine[4 * (size_t)t0 + j];
        if ((int)threadIdx.x < m) cnt[threadIdx.x] = 0;
        __syncthreads();
        for (int j = 0; j < m; j++) {
            const double a = h[4 * j], b = h[4 * j + 1], c = h[4 * j + 2], d = h[4 * j + 3];  // one address for the wave
            int n = 0;
#pragma unroll
            for (int k = 0; k < SC_ITEMS; k++) {
                const double r = ((x[k] * a + y[k] * b) + z[k] * c) + d;
                n += __builtin_popcountll(__ballot(fabs(r) <= threshold));
            }
            if (n != 0 && lane_id() == 0) atomicAdd(cnt + j, n);
        }
        __syncthreads();
        if ((int)threadIdx.x < m && cnt[threadIdx.x] != 0) atomicAdd(table + t0 + threadIdx.x, cnt[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// E. refit

// grid = (spans of RF_SPAN points of the largest plane, planes)
__global__ void __launch_bounds__(256) pf_refit_sums_kernel(const PfPlane* __restrict__ planes, const float* __restrict__ points,
                                                            int T, const double* __restrict__ hyp, double threshold,
                                                            unsigned char* __restrict__ mask, double* __restrict__ partials) {
    const PfPlane& pl = planes[blockIdx.y];
    if (blockIdx.x >= pl.rf_blocks) return;  // block-uniform
    __shared__ double waves[4][RF_TERMS];
    double s[RF_TERMS];
#pragma unroll
    for (int c = 0; c < RF_TERMS; c++) s[c] = 0.0;
    double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
    if (pl.best >= 0) {
        const double* h = hyp + 4 * ((size_t)blockIdx.y * T + pl.best);
        a = h[0], b = h[1], c = h[2], d = h[3];
    }
    for (int k = 0; k < RF_ITEMS; k++) {
        const size_t i = (size_t)blockIdx.x * RF_SPAN + (size_t)k * 256 + threadIdx.x;
        if (i >= (size_t)pl.n) break;
        const float* p = points + 3 * ((size_t)pl.begin + i);
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        const double r = ((x * a + y * b) + z * c) + d;
        const bool in = pl.best >= 0 && fabs(r) <= threshold;
        mask[(size_t)pl.begin + i] = in ? 1 : 0;
        if (!in) continue;
        s[0] += 1.0;
        s[1] += x;
        s[2] += y;
        s[3] += z;
        s[4] += x * x;  // exact: two float32 factors
        s[5] += x * y;
        s[6] += x * z;
        s[7] += y * y;
        s[8] += y * z;
        s[9] += z * z;
    }
#pragma unroll
    for (int t = 0; t < RF_TERMS; t++) moment_fold(s[t], waves, t);
    moment_store(waves, RF_TERMS, partials + ((size_t)pl.rf_base + blockIdx.x) * RF_TERMS);
}

// grid = planes, 64 threads
__global__ void __launch_bounds__(64) pf_refit_solve_kernel(const PfPlane* __restrict__ planes, const double* __restrict__ partials,
                                                            int has_prior, double alpha, double* __restrict__ moments,
                                                            double* __restrict__ coef) {
    const PfPlane& pl = planes[blockIdx.x];
    double s[RF_TERMS];
    column_fold(partials + (size_t)pl.rf_base * RF_TERMS, pl.rf_blocks, RF_TERMS, s);
    if (threadIdx.x != 0) return;
    double* mo = moments + (size_t)blockIdx.x * RF_TERMS;
    double* out = coef + 4 * (size_t)blockIdx.x;
#pragma unroll
    for (int t = 0; t < RF_TERMS; t++) mo[t] = s[t];
    if (!(s[0] > 0.0)) {
        out[0] = out[1] = out[2] = out[3] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double n = s[0];
    double cen[3], C[6], r[4];
#pragma unroll
    for (int k = 0; k < 3; k++) cen[k] = s[1 + k] / n;
    C[0] = s[4] / n - cen[0] * cen[0];
    C[1] = s[5] / n - cen[0] * cen[1];
    C[2] = s[6] / n - cen[0] * cen[2];
    C[3] = s[7] / n - cen[1] * cen[1];
    C[4] = s[8] / n - cen[1] * cen[2];
    C[5] = s[9] / n - cen[2] * cen[2];
    pf_solve(cen, C, has_prior != 0, pl.prior, alpha, r);
    out[0] = r[0], out[1] = r[1], out[2] = r[2], out[3] = r[3];
}

}  // namespace g4s

using namespace g4s;

// ---------------------------------------------------------------------------------------------------------------------
// extern "C" entry points; every argument is checked before any launch
namespace {

constexpr int PF_MAX_GRID_Y = 65535;
constexpr long long PF_MAX_ROWS = (1ll << 31) - 1;

struct GatherLayout { size_t pairs, counts, pos, chunks, total, first, bytes; long long blocks; };
// sizes have passed view_sizes_ok, pair_view[e] is in 0 .. n_views - 1
GatherLayout gather_layout(int n_views, const int* sizes, int n_pairs, const int* pair_view) {
    GatherLayout L{};
    for (int e = 0; e < n_pairs; e++) L.blocks += blocks256((long long)sizes[2 * pair_view[e]] * sizes[2 * pair_view[e] + 1]);
    WorkspaceCursor c;
    take_view_table<PfView>(c, n_views);
    L.pairs = c.take((size_t)n_pairs * sizeof(PfPair));
    L.counts = c.take((size_t)L.blocks * 4);
    L.pos = c.take((size_t)L.blocks * 4);
    L.chunks = c.take((size_t)scan_chunks((long)L.blocks) * 4);
    L.total = c.take(8);
    L.first = c.take(((size_t)n_pairs + 1) * 4);
    L.bytes = c.off;
    return L;
}

bool pairs_ok(int n_views, int n_pairs, const int* pair_view) {
    if (n_pairs < 0 || n_pairs > PF_MAX_GRID_Y || (n_pairs > 0 && !pair_view)) return false;
    for (int e = 0; e < n_pairs; e++) {
        if (pair_view[e] < 0 || pair_view[e] >= n_views) return false;
    }
    return true;
}

int check_gather(int n_views, const int* sizes, const float* const* depth, const float* const* normals, const int* const* masks,
                 const unsigned char* const* conf, int n_pairs, const int* pair_view, const int* pair_id, long long* blocks) {
    long long largest, total;
    if (check_grid_views(n_views, sizes, &largest, &total) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!pairs_ok(n_views, n_pairs, pair_view) || (n_pairs > 0 && !pair_id))
        return fail(G4S_ERR_INVALID_ARGUMENT, "pairs: at most 65535, each with a view in 0 .. n_views - 1");
    if (check_pointers("depth", depth, n_views) != G4S_OK || check_pointers("normals", normals, n_views) != G4S_OK ||
        check_pointers("plane_masks", masks, n_views) != G4S_OK || check_pointers("conf", conf, n_views) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    *blocks = 0;
    for (int e = 0; e < n_pairs; e++) *blocks += blocks256((long long)sizes[2 * pair_view[e]] * sizes[2 * pair_view[e] + 1]);
    if (*blocks > PF_MAX_ROWS / 256) return fail(G4S_ERR_INVALID_ARGUMENT, "the pairs' views must have fewer than 2^31 pixels together");
    return G4S_OK;
}

// the view and pair tables of a gather call; out == NULL: no pair has an output row yet
int stage_gather(const char* name, int n_views, const int* sizes, const float* rays, const float* const* depth,
                 const float* const* normals, const int* const* masks, const unsigned char* const* conf, int n_pairs,
                 const int* pair_view, const int* pair_id, const int* count, const long long* out, char* workspace, const GatherLayout& L,
                 hipStream_t stream, const PfView** views, const PfPair** pairs, unsigned* most) {
    const int rc = stage_views(name, n_views, true, sizes, depth, nullptr, false, workspace, view_table_bytes<PfView>(n_views), stream,
                               views, [&](PfView& u, int v) {
                                   u.normals = normals[v];
                                   u.mask = masks[v];
                                   u.conf = conf[v];
                                   u.ray = rays ? ray_record(rays + 12 * (size_t)v) : VisRay{};
                               });
    if (rc != G4S_OK) return rc;
    std::vector<PfPair> host((size_t)n_pairs);
    uint32_t base = 0;
    *most = 0;
    for (int e = 0; e < n_pairs; e++) {
        PfPair& p = host[(size_t)e];
        p.view = pair_view[e];
        p.id = pair_id[e];
        p.block_base = base;
        p.n_blocks = blocks256((long long)sizes[2 * p.view] * sizes[2 * p.view + 1]);
        p.out = out ? out[e] : -1;
        p.count = count ? (uint32_t)count[e] : 0u;
        base += p.n_blocks;
        if (p.n_blocks > *most) *most = p.n_blocks;
    }
    PfPair* dev = workspace_at<PfPair>(workspace, L.pairs);
    const hipError_t e = upload(dev, host.data(), host.size() * sizeof(PfPair), stream);
    if (e != hipSuccess) return fail(G4S_ERR_HIP, "%s pair table: %s", name, hipGetErrorString(e));
    *pairs = dev;
    return G4S_OK;
}

struct MemberLayout { size_t runs, flag, pos, chunks, total, rows, first, bytes; };
MemberLayout member_layout(int n_rows, int n_pairs, int n_planes) {
    MemberLayout L{};
    WorkspaceCursor c;
    L.runs = c.take((size_t)n_pairs * sizeof(PfRun));
    L.flag = c.take((size_t)n_rows * 4);
    L.pos = c.take((size_t)n_rows * 4);
    L.chunks = c.take((size_t)scan_chunks(n_rows) * 4);
    L.total = c.take(8);
    L.rows = c.take(((size_t)n_planes + 1) * 4);
    L.first = c.take(((size_t)n_planes + 1) * 4);
    L.bytes = c.off;
    return L;
}
bool member_sizes_ok(int n_rows, int n_pairs, int n_planes) {
    return n_rows >= 0 && n_pairs >= 0 && n_pairs <= PF_MAX_GRID_Y && n_planes >= 0 && n_planes <= PF_MAX_GRID_Y;
}

long long rf_spans(long long n) { return (n + RF_SPAN - 1) / RF_SPAN; }
long long sc_spans(long long n) { return (n + SC_SPAN - 1) / SC_SPAN; }

// plane_offset [n_planes + 1]: from 0, ascending, below 2^31
bool plane_offsets_ok(int n_planes, const int* plane_offset) {
    if (n_planes < 0 || n_planes > PF_MAX_GRID_Y || !plane_offset || plane_offset[0] != 0) return false;
    for (int p = 0; p < n_planes; p++) {
        if (plane_offset[p + 1] < plane_offset[p]) return false;
    }
    return true;
}

struct PlaneLayout { size_t planes, partials, bytes; };
PlaneLayout plane_layout(int n_planes, const int* plane_offset, bool partials) {
    PlaneLayout L{};
    WorkspaceCursor c;
    L.planes = c.take((size_t)n_planes * sizeof(PfPlane));
    long long spans = 0;
    if (partials) {
        for (int p = 0; p < n_planes; p++) spans += rf_spans(plane_offset[p + 1] - plane_offset[p]);
    }
    L.partials = c.take((size_t)spans * RF_TERMS * sizeof(double));
    L.bytes = c.off;
    return L;
}

// the plane table of the hypotheses, the scoring and the refit
int stage_planes(const char* name, int n_planes, const int* plane_offset, const double* priors, const int* best, char* workspace,
                 hipStream_t stream, const PfPlane** table, unsigned* most_sc, unsigned* most_rf) {
    std::vector<PfPlane> host((size_t)n_planes);
    uint32_t base = 0;
    *most_sc = *most_rf = 0;
    for (int p = 0; p < n_planes; p++) {
        PfPlane& u = host[(size_t)p];
        u.begin = plane_offset[p];
        u.n = plane_offset[p + 1] - plane_offset[p];
        u.best = best ? best[p] : -1;
        u.sc_blocks = (uint32_t)sc_spans(u.n);
        u.rf_base = base;
        u.rf_blocks = (uint32_t)rf_spans(u.n);
        base += u.rf_blocks;
        for (int c = 0; c < 3; c++) u.prior[c] = priors ? priors[3 * (size_t)p + c] : 0.0;
        if (u.sc_blocks > *most_sc) *most_sc = u.sc_blocks;
        if (u.rf_blocks > *most_rf) *most_rf = u.rf_blocks;
    }
    PfPlane* dev = workspace_at<PfPlane>(workspace, 0);
    const hipError_t e = upload(dev, host.data(), host.size() * sizeof(PfPlane), stream);
    if (e != hipSuccess) return fail(G4S_ERR_HIP, "%s plane table: %s", name, hipGetErrorString(e));
    *table = dev;
    return G4S_OK;
}

int check_fit(int n_planes, const int* plane_offset, const float* points, int n_trials, const double* priors, double alpha) {
    if (!plane_offsets_ok(n_planes, plane_offset))
        return fail(G4S_ERR_INVALID_ARGUMENT, "plane_offset: at most 65535 planes, from 0, ascending");
    if (n_trials < 1 || n_trials > PF_MAX_TRIALS) return fail(G4S_ERR_INVALID_ARGUMENT, "n_trials must be in 1 .. 2^20");
    if (plane_offset[n_planes] > 0 && !points) return null_pointer();
    if (priors) {
        if (!(alpha > 0.0) || !(alpha < 1.0e300)) return fail(G4S_ERR_INVALID_ARGUMENT, "alpha must be positive and finite");
        for (int i = 0; i < 3 * n_planes; i++) {
            if (!(fabs(priors[i]) < 1.0e300)) return fail(G4S_ERR_INVALID_ARGUMENT, "priors: plane %d is not finite", i / 3);
        }
    }
    return G4S_OK;
}

bool threshold_ok(double t) { return t >= 0.0 && t < 1.0e300; }

}  // namespace

extern "C" size_t g4s_plane_fit_gather_workspace(int n_views, const int* sizes, int n_pairs, const int* pair_view) {
    long long largest, total;
    if (!grid_views_ok(n_views) || !view_sizes_ok(n_views, sizes, &largest, &total) || !pairs_ok(n_views, n_pairs, pair_view)) return 0;
    const GatherLayout L = gather_layout(n_views, sizes, n_pairs, pair_view);
    return L.blocks > PF_MAX_ROWS / 256 ? 0 : L.bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_plane_fit_gather_count(int n_views, const int* sizes, const float* const* depth, const float* const* normals,
                                          const int* const* plane_masks, const unsigned char* const* conf, int n_pairs,
                                          const int* pair_view, const int* pair_id, int* pair_count, char* workspace,
                                          size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long blocks;
    if (check_gather(n_views, sizes, depth, normals, plane_masks, conf, n_pairs, pair_view, pair_id, &blocks) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_pairs == 0) return G4S_OK;
    if (!pair_count) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_plane_fit_gather_workspace(n_views, sizes, n_pairs, pair_view)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const GatherLayout L = gather_layout(n_views, sizes, n_pairs, pair_view);
    const PfView* views;
    const PfPair* pairs;
    unsigned most;
    const int rc = stage_gather("plane fit gather", n_views, sizes, nullptr, depth, normals, plane_masks, conf, n_pairs, pair_view,
                                pair_id, nullptr, nullptr, workspace, L, stream, &views, &pairs, &most);
    if (rc != G4S_OK) return rc;
    uint32_t* counts = workspace_at<uint32_t>(workspace, L.counts);
    uint32_t* pos = workspace_at<uint32_t>(workspace, L.pos);
    uint32_t* d_total = workspace_at<uint32_t>(workspace, L.total);
    uint32_t* first = workspace_at<uint32_t>(workspace, L.first);
    hipLaunchKernelGGL(pf_gather_count_kernel, dim3(most, (unsigned)n_pairs), dim3(256), 0, stream, views, pairs, counts);
    scan_u32(counts, pos, (int)blocks, workspace_at<uint32_t>(workspace, L.chunks), d_total, stream);
    hipLaunchKernelGGL(pf_pair_first_kernel, dim3(1), dim3(256), 0, stream, pairs, n_pairs, (const uint32_t*)pos,
                       (const uint32_t*)d_total, first);
    std::vector<uint32_t> host((size_t)n_pairs + 1);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), first, host.size() * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return finish(e, "plane fit gather");
    for (int p = 0; p < n_pairs; p++) pair_count[p] = (int)(host[(size_t)p + 1] - host[(size_t)p]);
    return finish(hipSuccess, "plane fit gather");
}

extern "C" int g4s_plane_fit_gather_emit(int n_views, const int* sizes, const float* rays, const float* const* depth,
                                         const float* const* normals, const int* const* plane_masks,
                                         const unsigned char* const* conf, int n_pairs, const int* pair_view, const int* pair_id,
                                         const int* pair_count, const long long* pair_row, long long n_rows, float* points,
                                         float* out_normals, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    long long blocks;
    if (check_gather(n_views, sizes, depth, normals, plane_masks, conf, n_pairs, pair_view, pair_id, &blocks) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_rows < 0 || n_rows > PF_MAX_ROWS) return fail(G4S_ERR_INVALID_ARGUMENT, "n_rows must be in 0 .. 2^31 - 1");
    if (n_pairs == 0 || n_rows == 0) return G4S_OK;
    if (!rays || !pair_count || !pair_row || !points || !out_normals) return null_pointer();
    for (int i = 0; i < 12 * n_views; i++) {
        if (!finite(rays[i])) return fail(G4S_ERR_INVALID_ARGUMENT, "rays: view %d is not finite", i / 12);
    }
    for (int e = 0; e < n_pairs; e++) {  // a pair's rows lie inside the outputs: the kernel writes pair_count[e] rows from pair_row[e]
        if (pair_count[e] < 0 || pair_row[e] < -1 || (pair_row[e] >= 0 && pair_row[e] + pair_count[e] > n_rows))
            return fail(G4S_ERR_INVALID_ARGUMENT, "pair %d: its rows must lie in 0 .. n_rows", e);
    }
    if (check_workspace(workspace, workspace_bytes, g4s_plane_fit_gather_workspace(n_views, sizes, n_pairs, pair_view)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const GatherLayout L = gather_layout(n_views, sizes, n_pairs, pair_view);
    // pair_count must be what the count phase returned: it is compared with the scan the phase left in the workspace
    std::vector<uint32_t> first((size_t)n_pairs + 1);
    hipError_t e = hipMemcpyAsync(first.data(), workspace_at<uint32_t>(workspace, L.first), first.size() * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return finish(e, "plane fit gather");
    for (int p = 0; p < n_pairs; p++) {
        if ((long long)first[(size_t)p + 1] - (long long)first[(size_t)p] != pair_count[p])
            return fail(G4S_ERR_INVALID_ARGUMENT, "pair_count[%d] is not the count phase's", p);
    }
    const PfView* views;
    const PfPair* pairs;
    unsigned most;
    const int rc = stage_gather("plane fit gather", n_views, sizes, rays, depth, normals, plane_masks, conf, n_pairs, pair_view,
                                pair_id, pair_count, pair_row, workspace, L, stream, &views, &pairs, &most);
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(pf_gather_emit_kernel, dim3(most, (unsigned)n_pairs), dim3(256), 0, stream, views, pairs,
                       (const uint32_t*)workspace_at<uint32_t>(workspace, L.pos), points, out_normals);
    return finish(hipSuccess, "plane fit gather");
}

extern "C" size_t g4s_plane_fit_members_workspace(int n_rows, int n_pairs, int n_planes) {
    return member_sizes_ok(n_rows, n_pairs, n_planes) ? member_layout(n_rows, n_pairs, n_planes).bytes + WORKSPACE_BASE_SLACK : 0;
}

extern "C" int g4s_plane_fit_members_count(int n_rows, int n_pairs, const int* pair_offset, const signed char* labels,
                                           const int* top, int n_planes, const int* plane_pair, int* plane_offset, char* workspace,
                                           size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (!member_sizes_ok(n_rows, n_pairs, n_planes))
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_rows must not be negative, n_pairs and n_planes in 0 .. 65535");
    if (!pair_offset || !plane_pair || !plane_offset || (n_pairs > 0 && !top) || (n_rows > 0 && !labels)) return null_pointer();
    if (pair_offset[0] != 0 || pair_offset[n_pairs] != n_rows || plane_pair[0] != 0 || plane_pair[n_planes] != n_pairs)
        return fail(G4S_ERR_INVALID_ARGUMENT, "pair_offset runs from 0 to n_rows, plane_pair from 0 to n_pairs");
    for (int e = 0; e < n_pairs; e++) {
        if (pair_offset[e + 1] < pair_offset[e]) return fail(G4S_ERR_INVALID_ARGUMENT, "pair_offset must ascend");
    }
    for (int p = 0; p < n_planes; p++) {
        if (plane_pair[p + 1] < plane_pair[p]) return fail(G4S_ERR_INVALID_ARGUMENT, "plane_pair must ascend");
    }
    if (check_workspace(workspace, workspace_bytes, g4s_plane_fit_members_workspace(n_rows, n_pairs, n_planes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    if (n_rows == 0) {
        for (int p = 0; p <= n_planes; p++) plane_offset[p] = 0;
        return G4S_OK;
    }
    const MemberLayout L = member_layout(n_rows, n_pairs, n_planes);
    std::vector<PfRun> runs((size_t)n_pairs);
    uint32_t most = 0;
    for (int e = 0; e < n_pairs; e++) {
        runs[(size_t)e] = PfRun{(uint32_t)pair_offset[e], (uint32_t)(pair_offset[e + 1] - pair_offset[e]), top[e]};
        if (runs[(size_t)e].n > most) most = runs[(size_t)e].n;
    }
    std::vector<int> rows((size_t)n_planes + 1);
    for (int p = 0; p <= n_planes; p++) rows[(size_t)p] = pair_offset[plane_pair[p]];
    PfRun* d_runs = workspace_at<PfRun>(workspace, L.runs);
    int* d_rows = workspace_at<int>(workspace, L.rows);
    uint32_t* flag = workspace_at<uint32_t>(workspace, L.flag);
    uint32_t* pos = workspace_at<uint32_t>(workspace, L.pos);
    uint32_t* d_total = workspace_at<uint32_t>(workspace, L.total);
    uint32_t* first = workspace_at<uint32_t>(workspace, L.first);
    hipError_t e = upload(d_runs, runs.data(), runs.size() * sizeof(PfRun), stream);
    if (e == hipSuccess) e = upload(d_rows, rows.data(), rows.size() * 4, stream);
    if (e != hipSuccess) return finish(e, "plane fit members");
    hipLaunchKernelGGL(pf_member_flags_kernel, dim3(blocks256(most), (unsigned)n_pairs), dim3(256), 0, stream, (const PfRun*)d_runs,
                       labels, flag);
    scan_u32(flag, pos, n_rows, workspace_at<uint32_t>(workspace, L.chunks), d_total, stream);
    hipLaunchKernelGGL(pf_plane_first_kernel, dim3(1), dim3(256), 0, stream, (const int*)d_rows, n_planes, n_rows,
                       (const uint32_t*)pos, (const uint32_t*)d_total, first);
    std::vector<uint32_t> host((size_t)n_planes + 1);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), first, host.size() * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return finish(e, "plane fit members");
    for (int p = 0; p <= n_planes; p++) plane_offset[p] = (int)host[(size_t)p];
    return finish(hipSuccess, "plane fit members");
}

extern "C" int g4s_plane_fit_members_emit(int n_rows, int n_pairs, int n_planes, const float* points, int n_members,
                                          float* plane_points, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (!member_sizes_ok(n_rows, n_pairs, n_planes) || n_members < 0 || n_members > n_rows)
        return fail(G4S_ERR_INVALID_ARGUMENT, "n_rows must not be negative, n_pairs and n_planes in 0 .. 65535, n_members in 0 .. n_rows");
    if (n_members == 0) return G4S_OK;
    if (!points || !plane_points) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_plane_fit_members_workspace(n_rows, n_pairs, n_planes)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const MemberLayout L = member_layout(n_rows, n_pairs, n_planes);
    hipLaunchKernelGGL(pf_member_emit_kernel, dim3(blocks256(n_rows)), dim3(256), 0, stream, n_rows, (uint32_t)n_members,
                       (const uint32_t*)workspace_at<uint32_t>(workspace, L.flag),
                       (const uint32_t*)workspace_at<uint32_t>(workspace, L.pos), points, plane_points);
    return finish(hipSuccess, "plane fit members");
}

extern "C" size_t g4s_plane_fit_workspace(int n_planes, const int* plane_offset) {
    if (!plane_offsets_ok(n_planes, plane_offset)) return 0;
    return plane_layout(n_planes, plane_offset, true).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_plane_fit_hypotheses(int n_planes, const int* plane_offset, const float* points, int n_trials,
                                        const int* samples, const double* priors, double alpha, double* hypotheses,
                                        char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_fit(n_planes, plane_offset, points, n_trials, priors, alpha) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (n_planes == 0) return G4S_OK;
    if (!samples || !hypotheses) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_plane_fit_workspace(n_planes, plane_offset)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const PfPlane* table;
    unsigned most_sc, most_rf;
    const int rc = stage_planes("plane fit hypotheses", n_planes, plane_offset, priors, nullptr, workspace, stream, &table, &most_sc,
                                &most_rf);
    if (rc != G4S_OK) return rc;
    hipLaunchKernelGGL(pf_hypotheses_kernel, dim3(blocks256(n_trials), (unsigned)n_planes), dim3(256), 0, stream, table, points,
                       n_trials, samples, priors ? 1 : 0, alpha, hypotheses);
    return finish(hipSuccess, "plane fit hypotheses");
}

extern "C" int g4s_plane_fit_score(int n_planes, const int* plane_offset, const float* points, int n_trials,
                                   const double* hypotheses, double threshold, int* counts, char* workspace, size_t workspace_bytes,
                                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_fit(n_planes, plane_offset, points, n_trials, nullptr, 0.0) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!threshold_ok(threshold)) return fail(G4S_ERR_INVALID_ARGUMENT, "threshold must be finite and not negative");
    if (n_planes == 0) return G4S_OK;
    if (!hypotheses || !counts) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_plane_fit_workspace(n_planes, plane_offset)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_planes * n_trials * sizeof(int), stream);
    if (e != hipSuccess) return finish(e, "plane fit score");
    const PfPlane* table;
    unsigned most_sc, most_rf;
    const int rc = stage_planes("plane fit score", n_planes, plane_offset, nullptr, nullptr, workspace, stream, &table, &most_sc, &most_rf);
    if (rc != G4S_OK) return rc;
    if (most_sc > 0)
        hipLaunchKernelGGL(pf_score_kernel, dim3(most_sc, (unsigned)n_planes), dim3(256), 0, stream, table, points, n_trials,
                           hypotheses, threshold, counts);
    return finish(hipSuccess, "plane fit score");
}

extern "C" int g4s_plane_fit_refit(int n_planes, const int* plane_offset, const float* points, int n_trials,
                                   const double* hypotheses, const int* best, double threshold, const double* priors, double alpha,
                                   unsigned char* inlier_mask, double* moments, double* coefficients, char* workspace,
                                   size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    clear_error();
    if (check_fit(n_planes, plane_offset, points, n_trials, priors, alpha) != G4S_OK) return G4S_ERR_INVALID_ARGUMENT;
    if (!threshold_ok(threshold)) return fail(G4S_ERR_INVALID_ARGUMENT, "threshold must be finite and not negative");
    if (n_planes == 0) return G4S_OK;
    if (!hypotheses || !best || !moments || !coefficients || (plane_offset[n_planes] > 0 && !inlier_mask)) return null_pointer();
    for (int p = 0; p < n_planes; p++) {
        if (best[p] < -1 || best[p] >= n_trials) return fail(G4S_ERR_INVALID_ARGUMENT, "best[%d] must be -1 or a trial", p);
    }
    if (check_workspace(workspace, workspace_bytes, g4s_plane_fit_workspace(n_planes, plane_offset)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const PlaneLayout L = plane_layout(n_planes, plane_offset, true);
    double* partials = workspace_at<double>(workspace, L.partials);
    const PfPlane* table;
    unsigned most_sc, most_rf;
    const int rc = stage_planes("plane fit refit", n_planes, plane_offset, priors, best, workspace, stream, &table, &most_sc, &most_rf);
    if (rc != G4S_OK) return rc;
    if (most_rf > 0)
        hipLaunchKernelGGL(pf_refit_sums_kernel, dim3(most_rf, (unsigned)n_planes), dim3(256), 0, stream, table, points, n_trials,
                           hypotheses, threshold, inlier_mask, partials);
    hipLaunchKernelGGL(pf_refit_solve_kernel, dim3((unsigned)n_planes), dim3(64), 0, stream, table, (const double*)partials,
                       priors ? 1 : 0, alpha, moments, coefficients);
    return finish(hipSuccess, "plane fit refit");
}
