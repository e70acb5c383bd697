// Chart points (include/g4s_losses.h, "Chart points": g4s_chart_points_*), kernels and entry points.
//
// Reference semantics: matcha/pointmap/depthanythingv2.py:82-117, 156-253 -- get_points_depth_in_depthmap and
// fit_depth_to_point_cloud, looped per chart with grid_sample and two .item() read-backs each -- and the point form of
// ParallelAligner.loss (matcha/dm_scene/parallel_aligner.py:423-453), which calls the same sampler per chart on the predicted
// depths and on the confidence in every iteration and lets autograd scatter the gradient with float atomics.
//
// MI355X design: one primitive, "project a chart's points, tap a map under them", with two consumers.
//   project     one thread per point of the packed list, once per point set: the chart of the point (a search in the n + 1
//               offsets), its view depth z and its pixel coordinates (ix, iy).  A clipped point gets (-2, -2), whose four taps
//               lie outside every map, so no consumer needs the flag.
//   sample      a gather: one thread per point recomputes the four weights from (ix, iy) and taps any [n,H,W] map.
//   moments     grid (spans of the largest chart, charts): a thread adds its CP_ITEMS points in ascending order in float64, a
//               fixed shuffle tree folds the lanes, the four wave sums are added in wave order.  coeffs: one wave per chart
//               adds the chart's partials by index.  The order of the depth cues' alignment (tsdf/depth_cues.hip), no atomics.
//   loss        the same sum over spans of the whole list, one double per span, folded by one workgroup.
//   backward    no float atomics: a store pass writes dL/ds_p (and dL/dk_p) per point, and one thread per PIXEL adds its taps
//               through an inverted index built once per point set -- keys (chart pixel << 32 | 4 point + corner) emitted in
//               ascending (point, corner) order, partitioned by the pixel bits with the stable radix_sort_u64_keys, counted
//               per pixel with integer atomics and scanned (tsdf/scan.hip) into tap ranges.  A pixel's list is summed in
//               chunks of CP_CHUNK taps, the chunk sums added in chunk order: bit-identical from run to run whatever piles up.
//               A pixel with more than one chunk (SfM points pile up) is summed by its whole wave, a chunk per lane.
// Every launch is on the caller's stream; nothing allocates, synchronises or reads back.
#include "g4s_internal.h"
#include "fixed_sums.h"
#include "chart_common.h"
#include "tsdf/scan.h"
#include "../../include/g4s_losses.h"

namespace g4s {

constexpr int CP_CAM_FLOATS = 32;          // world_view_transform[4][4], full_proj_transform[4][4]
constexpr int CP_ITEMS = 16;               // points per thread of the sums
constexpr int CP_SPAN = 256 * CP_ITEMS;    // points one workgroup reduces
constexpr int CP_TERMS = 5;                // n, sum t, sum d, sum t d, sum d d
constexpr int CP_CHUNK = G4S_CHART_POINTS_CHUNK;
constexpr int CP_MAX_POINTS = (1 << 29) - 1;          // 4 N < 2^31: tap ids are 32-bit and the sort takes an int
constexpr long long CP_MAX_PIXELS = (1ll << 31) - 2;  // n H W + 1 fits the scan's int
static_assert(CP_SPAN == G4S_CHART_POINTS_SPAN, "the header states the span the workspace is sized by");

struct PointArgs {
    int n, W, H, N;
    const int* chart;    // [N]
    const float* ixy;    // [N][2]
    const float* z;      // [N]
    const float* depths; // [n][H][W]
    const float* conf;   // [n][H][W] or NULL
    float cw;
};

struct Taps {
    int idx[4];   // index into the chart's map, -1 outside
    float w[4];   // nw, ne, sw, se
};

// the four taps of pixel coordinates (ix, iy): grid_sample's bilinear rule with zeros padding
__device__ __forceinline__ void cp_taps(float ix, float iy, int W, int H, Taps& t) {
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float wx1 = ix - fx0, wy1 = iy - fy0;
    const float wx0 = (fx0 + 1.0f) - ix, wy0 = (fy0 + 1.0f) - iy;
    // the edge tests in float: a coordinate of any size is decided before it becomes an index (a NaN fails all four)
    const bool inx0 = fx0 >= 0.0f && fx0 <= (float)(W - 1), inx1 = fx0 >= -1.0f && fx0 <= (float)(W - 2);
    const bool iny0 = fy0 >= 0.0f && fy0 <= (float)(H - 1), iny1 = fy0 >= -1.0f && fy0 <= (float)(H - 2);
    const int x0 = (inx0 || inx1) ? (int)fx0 : 0, y0 = (iny0 || iny1) ? (int)fy0 : 0;
    const bool in[4] = {inx0 && iny0, inx1 && iny0, inx0 && iny1, inx1 && iny1};
    t.w[0] = wx0 * wy0; t.w[1] = wx1 * wy0; t.w[2] = wx0 * wy1; t.w[3] = wx1 * wy1;
#pragma unroll
    for (int c = 0; c < 4; c++) t.idx[c] = in[c] ? (y0 + (c >> 1)) * W + (x0 + (c & 1)) : -1;
}

// ((nw m(x0,y0) + ne m(x1,y0)) + sw m(x0,y1)) + se m(x1,y1), a tap outside the map contributing 0
__device__ __forceinline__ float cp_value(const Taps& t, const float* __restrict__ m) {
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = t.idx[c] >= 0 ? t.w[c] * m[t.idx[c]] : 0.0f;
    return ((v[0] + v[1]) + v[2]) + v[3];
}

__device__ __forceinline__ float cp_rows(float p0, float p1, float p2, const float* __restrict__ M, int c) {
    return ((p0 * M[c] + p1 * M[4 + c]) + p2 * M[8 + c]) + M[12 + c];
}

__global__ void __launch_bounds__(256) cp_project_kernel(int n, int W, int H, int N, const float* __restrict__ cams,
        const float* __restrict__ points, const int* __restrict__ offsets, int* __restrict__ chart, float* __restrict__ z,
        float* __restrict__ ixy, unsigned char* __restrict__ clipped) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= N) return;
    int lo = 0, hi = n;  // the last chart whose first point is at or before i (empty charts own nothing)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const float* V = cams + (size_t)lo * CP_CAM_FLOATS;
    const float* F = V + 16;
    const float p0 = points[3 * (size_t)i], p1 = points[3 * (size_t)i + 1], p2 = points[3 * (size_t)i + 2];
    const float q0 = cp_rows(p0, p1, p2, F, 0), q1 = cp_rows(p0, p1, p2, F, 1), q3 = cp_rows(p0, p1, p2, F, 3);
    const float gx = q0 / q3, gy = q1 / q3;
    const bool clip = !(q3 > 0.0f) || !isfinite(gx) || !isfinite(gy);
    const float ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f, iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
    chart[i] = lo;
    z[i] = cp_rows(p0, p1, p2, V, 2);
    ixy[2 * (size_t)i] = clip ? -2.0f : ix;
    ixy[2 * (size_t)i + 1] = clip ? -2.0f : iy;
    if (clipped) clipped[i] = clip ? 1 : 0;
}

__global__ void __launch_bounds__(256) cp_sample_kernel(int W, int H, int N, const int* __restrict__ chart,
        const float* __restrict__ ixy, const float* __restrict__ map, float* __restrict__ values,
        unsigned char* __restrict__ fov) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= N) return;
    Taps t;
    cp_taps(ixy[2 * (size_t)i], ixy[2 * (size_t)i + 1], W, H, t);
    const float v = cp_value(t, map + (size_t)chart[i] * W * H);
    values[i] = v;
    if (fov) fov[i] = v > 0.0f ? 1 : 0;
}

// the first row of chart c's partials: its spans never reach the next chart's (floor(a/S) + ceil((b-a)/S) <= floor(b/S) + 1)
__device__ __forceinline__ size_t cp_partial_base(const int* __restrict__ offsets, int c) {
    return (size_t)(offsets[c] / CP_SPAN) + (size_t)c;
}

// grid = (spans of the largest chart, charts)
__global__ void __launch_bounds__(256) cp_moments_kernel(const int* __restrict__ offsets, const float* __restrict__ z,
        const float* __restrict__ d, int use_fov, double* __restrict__ partials) {
    const int c = (int)blockIdx.y;
    const int begin = offsets[c], end = offsets[c + 1];
    if ((long long)blockIdx.x * CP_SPAN >= (long long)(end - begin)) return;  // block-uniform
    double s[CP_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const long long first = (long long)begin + (long long)blockIdx.x * CP_SPAN + threadIdx.x;
    for (int k = 0; k < CP_ITEMS; k++) {
        const long long q = first + (long long)k * 256;
        if (q >= end) break;
        const float df = d[q];
        if (use_fov && !(df > 0.0f)) continue;
        const double t = (double)(1.0f / z[q]), dd = (double)df;
        s[0] += 1.0;
        s[1] += t;
        s[2] += dd;
        s[3] += t * dd;  // exact: two float32 factors
        s[4] += dd * dd;
    }
    __shared__ double waves[4][CP_TERMS];
#pragma unroll
    for (int k = 0; k < CP_TERMS; k++) moment_fold(s[k], waves, k);
    moment_store(waves, CP_TERMS, partials + (cp_partial_base(offsets, c) + blockIdx.x) * CP_TERMS);
}

// grid = charts, 64 threads
__global__ void __launch_bounds__(64) cp_coeffs_kernel(const int* __restrict__ offsets, const double* __restrict__ partials,
        float* __restrict__ coeffs, int* __restrict__ counts) {
    const int c = (int)blockIdx.x;
    const int nb = (offsets[c + 1] - offsets[c] + CP_SPAN - 1) / CP_SPAN;
    double s[CP_TERMS];
    column_fold(partials + cp_partial_base(offsets, c) * CP_TERMS, (uint32_t)nb, CP_TERMS, s);
    if (threadIdx.x == 0) scale_shift_solve(s, coeffs + 2 * (size_t)c, counts + c);
}

__global__ void __launch_bounds__(256) cp_apply_kernel(long long total, int per_chart, const float* __restrict__ disp,
        const float* __restrict__ coeffs, float scale, float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= total) return;
    const int c = (int)(v / per_chart);
    const float lin = coeffs[2 * c] + coeffs[2 * c + 1] * disp[v];
    out[v] = scale * (1.0f / lin);
}

// z of scale P: chart == NULL means `per_chart` consecutive points per chart (point maps)
__global__ void __launch_bounds__(256) cp_view_depths_kernel(long long total, long long per_chart, const int* __restrict__ chart,
        const float* __restrict__ cams, const float* __restrict__ points, float scale, float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= total) return;
    const int c = chart ? chart[v] : (int)(v / per_chart);
    const float* V = cams + (size_t)c * CP_CAM_FLOATS;
    out[v] = cp_rows(scale * points[3 * v], scale * points[3 * v + 1], scale * points[3 * v + 2], V, 2);
}

// ---- the inverted index ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cp_keys_kernel(int n, int W, int H, int N, const int* __restrict__ chart,
        const float* __restrict__ ixy, unsigned long long* __restrict__ keys, uint32_t* __restrict__ counts) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= N) return;
    Taps t;
    cp_taps(ixy[2 * (size_t)i], ixy[2 * (size_t)i + 1], W, H, t);
    const uint32_t per = (uint32_t)W * (uint32_t)H, none = (uint32_t)n * per;  // taps outside sort behind every pixel
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t pix = t.idx[c] >= 0 ? (uint32_t)chart[i] * per + (uint32_t)t.idx[c] : none;
        keys[4 * (size_t)i + c] = ((unsigned long long)pix << 32) | (unsigned long long)(4u * (uint32_t)i + (uint32_t)c);
        if (t.idx[c] >= 0) atomicAdd(counts + pix, 1u);  // integers: the same counts in every run
    }
}

__global__ void __launch_bounds__(256) cp_tap_ids_kernel(long long total, const unsigned long long* __restrict__ keys,
        int* __restrict__ taps) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < total) taps[v] = (int)(uint32_t)keys[v];
}

// ---- the point-reference term ---------------------------------------------------------------------------------------------
struct PointTerm {
    float s, k, e;
};
__device__ __forceinline__ void cp_point_term(const PointArgs& a, int i, PointTerm& o) {
    Taps t;
    cp_taps(a.ixy[2 * (size_t)i], a.ixy[2 * (size_t)i + 1], a.W, a.H, t);
    const size_t base = (size_t)a.chart[i] * a.W * a.H;
    o.s = cp_value(t, a.depths + base);
    o.k = a.conf ? cp_value(t, a.conf + base) : 1.0f;
    o.e = fabsf(o.s - a.z[i]);
}

// grid = spans of the packed list; one double per span
__global__ void __launch_bounds__(256) cp_loss_kernel(PointArgs a, double* __restrict__ partials) {
    double s = 0.0;
    const long long first = (long long)blockIdx.x * CP_SPAN + threadIdx.x;
    for (int k = 0; k < CP_ITEMS; k++) {
        const long long q = first + (long long)k * 256;
        if (q >= a.N) break;
        PointTerm p;
        cp_point_term(a, (int)q, p);
        s += (double)(a.conf ? p.k * p.e - a.cw * logf(p.k) : p.e);
    }
    __shared__ double waves[4];
    const double b = block_sum_chain(s, waves);
    if (threadIdx.x == 0) partials[blockIdx.x] = b;
}

// one workgroup: thread t adds partials t, t + 256, ... in ascending order, then the same fold
__global__ void __launch_bounds__(256) cp_loss_fold_kernel(int nparts, int N, const double* __restrict__ partials,
        float* __restrict__ out1) {
    double s = 0.0;
    for (int b = (int)threadIdx.x; b < nparts; b += 256) s += partials[b];
    __shared__ double waves[4];
    const double b = block_sum_chain(s, waves);
    if (threadIdx.x == 0) out1[0] = (float)(b / (double)N);
}

// the store pass: dL/ds_p and dL/dk_p per point
__global__ void __launch_bounds__(256) cp_point_grad_kernel(PointArgs a, const float* __restrict__ g1, float* __restrict__ ds,
        float* __restrict__ dk) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= a.N) return;
    PointTerm p;
    cp_point_term(a, i, p);
    const float c = g1[0] / (float)a.N;
    const float sg = signf(p.s - a.z[i]);
    ds[i] = a.conf ? (c * p.k) * sg : c * sg;
    if (a.conf) dk[i] = c * (p.e - a.cw / p.k);
}

// taps [at, stop) of one chunk, added from 0 in ascending order
__device__ __forceinline__ void cp_chunk_sum(uint32_t at, uint32_t stop, int W, int H, const float* __restrict__ ixy,
        const int* __restrict__ taps, const float* __restrict__ ga, const float* __restrict__ gb, float& acc_a, float& acc_b) {
    acc_a = 0.0f;
    acc_b = 0.0f;
    for (uint32_t k = at; k < stop; k++) {
        const uint32_t id = (uint32_t)taps[k];
        const uint32_t pt = id >> 2, c = id & 3u;
        Taps t;
        cp_taps(ixy[2 * (size_t)pt], ixy[2 * (size_t)pt + 1], W, H, t);
        const float w = c == 0 ? t.w[0] : (c == 1 ? t.w[1] : (c == 2 ? t.w[2] : t.w[3]));
        acc_a += ga[pt] * w;
        if (gb) acc_b += gb[pt] * w;
    }
}

// one thread per pixel: the float32 sum of its taps in ascending (point, corner) order, in chunks of CP_CHUNK
__global__ void __launch_bounds__(256) cp_gather_kernel(long long pixels, int W, int H, const float* __restrict__ ixy,
        const int* __restrict__ taps, const uint32_t* __restrict__ starts, const float* __restrict__ ga,
        const float* __restrict__ gb, float* __restrict__ out_a, float* __restrict__ out_b) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = v < pixels;  // no early return: the whole wave helps with its piled-up pixels below
    const uint32_t begin = valid ? starts[v] : 0u, end = valid ? starts[v + 1] : 0u;
    const bool piled = end - begin > (uint32_t)CP_CHUNK;
    float total_a = 0.0f, total_b = 0.0f;
    if (!piled) {  // at most one chunk
        cp_chunk_sum(begin, end, W, H, ixy, taps, ga, gb, total_a, total_b);
        total_a = 0.0f + total_a;
        total_b = 0.0f + total_b;
    }
    // SfM points pile up on some pixels.  The wave takes its piled-up pixels one after the other: lane l sums chunk l of a
    // round of 64 chunks, then the round's chunk sums are added in chunk order -- the order of the contract, whoever adds.
    unsigned long long todo = __ballot(piled);
    while (todo != 0ull) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const uint32_t b = (uint32_t)__shfl((int)begin, src), e = (uint32_t)__shfl((int)end, src);
        const uint32_t nchunks = (e - b + CP_CHUNK - 1) / CP_CHUNK;
        float tot_a = 0.0f, tot_b = 0.0f;
        for (uint32_t c0 = 0; c0 < nchunks; c0 += 64u) {
            const uint32_t c = c0 + (uint32_t)lane_id();
            float acc_a = 0.0f, acc_b = 0.0f;
            if (c < nchunks) {
                const uint32_t at = b + c * CP_CHUNK;
                cp_chunk_sum(at, e - at < (uint32_t)CP_CHUNK ? e : at + CP_CHUNK, W, H, ixy, taps, ga, gb, acc_a, acc_b);
            }
            const int live = nchunks - c0 < 64u ? (int)(nchunks - c0) : 64;
            for (int l = 0; l < live; l++) {
                tot_a += __shfl(acc_a, l);
                tot_b += __shfl(acc_b, l);
            }
        }
        if (lane_id() == src) {
            total_a = tot_a;
            total_b = tot_b;
        }
    }
    if (!valid) return;
    out_a[v] = total_a;
    if (out_b) out_b[v] = total_b;
}

namespace {

bool cp_shape_ok(int n, int height, int width, int n_points) {
    return n > 0 && n <= 65535 && height > 0 && width > 0 && (long long)n * height * width <= CP_MAX_PIXELS && n_points >= 0 &&
           n_points <= CP_MAX_POINTS;
}

int cp_check_shape(int n, int height, int width, int n_points) {
    if (n <= 0 || n > 65535) return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: n must lie in 1..65535");
    if (height <= 0 || width <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: width, height must be positive");
    if ((long long)n * height * width > CP_MAX_PIXELS) return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: n H W must be below 2^31 - 1");
    if (n_points < 0 || n_points > CP_MAX_POINTS)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: the number of points must lie in 0..2^29 - 1");
    return G4S_OK;
}

// spans of the packed list, and an upper bound on the rows of the per-chart partials
size_t cp_spans(int n_points) { return ((size_t)n_points + CP_SPAN - 1) / CP_SPAN; }

struct CpLayout { size_t partials, ds, dk, bytes; };
CpLayout cp_layout(int n, int n_points) {
    WorkspaceCursor c;
    CpLayout L;
    L.partials = c.take(((size_t)n_points / CP_SPAN + (size_t)n + 1) * CP_TERMS * 8);
    L.ds = c.take((size_t)n_points * 4);
    L.dk = c.take((size_t)n_points * 4);
    L.bytes = c.off;
    return L;
}

struct CpIndexLayout { size_t keys_a, keys_b, hist, bin_total, counts, chunks, total, bytes; };
CpIndexLayout cp_index_layout(long long pixels, int n_points) {
    WorkspaceCursor c;
    CpIndexLayout L;
    const size_t k = (size_t)n_points * 4;
    L.keys_a = c.take(k * 8);
    L.keys_b = c.take(k * 8);
    L.hist = c.take((size_t)256 * (sort_blocks(k, SORT_ITEMS_U64) + 1) * 4);
    L.bin_total = c.take(512 * 4);
    L.counts = c.take((size_t)(pixels + 1) * 4);
    L.chunks = c.take((size_t)scan_chunks(pixels + 1) * 4);
    L.total = c.take(4);
    L.bytes = c.off;
    return L;
}

PointArgs cp_point_args(int n, int height, int width, int n_points, const int* chart, const float* ixy, const float* z,
                        const float* depths, const float* confidence, float cw) {
    PointArgs a{};
    a.n = n; a.W = width; a.H = height; a.N = n_points;
    a.chart = chart; a.ixy = ixy; a.z = z; a.depths = depths; a.conf = confidence; a.cw = cw;
    return a;
}

}  // namespace

}  // namespace g4s

using namespace g4s;

extern "C" size_t g4s_chart_points_workspace(int n, int height, int width, int n_points) {
    if (!cp_shape_ok(n, height, width, n_points)) return 0;
    return cp_layout(n, n_points).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" size_t g4s_chart_points_index_workspace(int n, int height, int width, int n_points) {
    if (!cp_shape_ok(n, height, width, n_points)) return 0;
    return cp_index_layout((long long)n * height * width, n_points).bytes + WORKSPACE_BASE_SLACK;
}

extern "C" int g4s_chart_points_project(int n, int height, int width, const float* cameras, int n_points, const float* points,
                                        const int* offsets, int* chart, float* z, float* ixy, unsigned char* clipped,
                                        void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cp_check_shape(n, height, width, n_points)) return rc;
    if (n_points == 0) return G4S_OK;
    if (!cameras || !points || !offsets || !chart || !z || !ixy) return null_pointer();
    hipLaunchKernelGGL(cp_project_kernel, dim3(blocks256(n_points)), dim3(256), 0, s, n, width, height, n_points, cameras, points,
                       offsets, chart, z, ixy, clipped);
    return stage_done("chart_points_project", s);
}

extern "C" int g4s_chart_points_sample(int n, int height, int width, int n_points, const int* chart, const float* ixy,
                                       const float* map, float* values, unsigned char* fov, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cp_check_shape(n, height, width, n_points)) return rc;
    if (n_points == 0) return G4S_OK;
    if (!chart || !ixy || !map || !values) return null_pointer();
    hipLaunchKernelGGL(cp_sample_kernel, dim3(blocks256(n_points)), dim3(256), 0, s, width, height, n_points, chart, ixy, map,
                       values, fov);
    return stage_done("chart_points_sample", s);
}

extern "C" int g4s_chart_points_fit(int n, int n_points, const int* offsets, int max_count, const float* z, const float* values,
                                    int use_fov_mask, float* coeffs, int* counts, char* workspace, size_t workspace_bytes,
                                    void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cp_check_shape(n, 1, 1, n_points)) return rc;
    if (max_count < 0 || max_count > n_points) return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: max_count must lie in 0..n_points");
    if (!offsets || !coeffs || !counts || (n_points > 0 && (!z || !values))) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_chart_points_workspace(n, 1, 1, n_points)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    double* partials = workspace_at<double>(workspace, cp_layout(n, n_points).partials);
    const unsigned most = (unsigned)cp_spans(max_count);
    if (most > 0)
        hipLaunchKernelGGL(cp_moments_kernel, dim3(most, (unsigned)n), dim3(256), 0, s, offsets, z, values, use_fov_mask != 0,
                           partials);
    hipLaunchKernelGGL(cp_coeffs_kernel, dim3((unsigned)n), dim3(64), 0, s, offsets, (const double*)partials, coeffs, counts);
    return stage_done("chart_points_fit", s);
}

extern "C" int g4s_chart_points_apply(int n, int height, int width, const float* disparities, const float* coeffs, float scale,
                                      float* depths, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cp_check_shape(n, height, width, 0)) return rc;
    if (!disparities || !coeffs || !depths) return null_pointer();
    const long long total = (long long)n * height * width;
    hipLaunchKernelGGL(cp_apply_kernel, dim3(blocks256(total)), dim3(256), 0, s, total, height * width, disparities, coeffs, scale,
                       depths);
    return stage_done("chart_points_apply", s);
}

extern "C" int g4s_chart_points_view_depths(int n, const float* cameras, long long count, long long per_chart, const int* chart,
                                            const float* points, float scale, float* depths, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (n <= 0 || n > 65535) return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: n must lie in 1..65535");
    if (count < 0 || count > (1ll << 31) - 1) return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: the number of points must lie in 0..2^31 - 1");
    if (!chart && (per_chart <= 0 || count != per_chart * n))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: without a chart list the points must be n runs of per_chart > 0");
    if (count == 0) return G4S_OK;
    if (!cameras || !points || !depths) return null_pointer();
    hipLaunchKernelGGL(cp_view_depths_kernel, dim3(blocks256(count)), dim3(256), 0, s, count, per_chart, chart, cameras, points, scale,
                       depths);
    return stage_done("chart_points_view_depths", s);
}

extern "C" int g4s_chart_points_index(int n, int height, int width, int n_points, const int* chart, const float* ixy, int* taps,
                                      unsigned int* starts, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cp_check_shape(n, height, width, n_points)) return rc;
    if (!starts || (n_points > 0 && (!chart || !ixy || !taps))) return null_pointer();
    if (check_workspace(workspace, workspace_bytes, g4s_chart_points_index_workspace(n, height, width, n_points)) != G4S_OK)
        return G4S_ERR_INVALID_ARGUMENT;
    const long long pixels = (long long)n * height * width;
    const CpIndexLayout L = cp_index_layout(pixels, n_points);
    char* ws = align_ptr(workspace);
    unsigned long long* ka = (unsigned long long*)(ws + L.keys_a);
    unsigned long long* kb = (unsigned long long*)(ws + L.keys_b);
    uint32_t* counts = (uint32_t*)(ws + L.counts);
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)(pixels + 1) * 4, s);
    if (e != hipSuccess) return finish(e, "chart_points_index");
    int cur = 0;
    if (n_points > 0) {
        hipLaunchKernelGGL(cp_keys_kernel, dim3(blocks256(n_points)), dim3(256), 0, s, n, width, height, n_points, chart, ixy, ka,
                           counts);
        // The keys come in ascending (point, corner) order and the sort is stable: only the pixel bits need passes.
        int bits = 1;
        while ((pixels >> bits) != 0) bits++;
        cur = radix_sort_u64_keys((uint64_t*)ka, (uint64_t*)kb, 4 * n_points, 32, 32 + bits, (uint32_t*)(ws + L.hist),
                                  (uint32_t*)(ws + L.bin_total), s);
        hipLaunchKernelGGL(cp_tap_ids_kernel, dim3(blocks256(4ll * n_points)), dim3(256), 0, s, 4ll * n_points,
                           (const unsigned long long*)(cur ? kb : ka), taps);
    }
    scan_u32(counts, starts, (int)(pixels + 1), (uint32_t*)(ws + L.chunks), (uint32_t*)(ws + L.total), s);
    return stage_done("chart_points_index", s);
}

static int cp_check_loss(int n, int height, int width, int n_points, const int* chart, const float* ixy, const float* z,
                         const float* depths, char* workspace, size_t workspace_bytes) {
    if (int rc = cp_check_shape(n, height, width, n_points)) return rc;
    if (n_points == 0) return fail(G4S_ERR_INVALID_ARGUMENT, "chart points: the point-reference term needs at least one point (a mean over none)");
    if (!chart || !ixy || !z || !depths) return null_pointer();
    return check_workspace(workspace, workspace_bytes, g4s_chart_points_workspace(n, height, width, n_points));
}

extern "C" int g4s_chart_points_loss_forward(int n, int height, int width, int n_points, const int* chart, const float* ixy,
                                             const float* z, const float* depths, const float* confidence,
                                             float confidence_weighting, float* out1, char* workspace, size_t workspace_bytes,
                                             void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cp_check_loss(n, height, width, n_points, chart, ixy, z, depths, workspace, workspace_bytes)) return rc;
    if (!out1) return null_pointer();
    const PointArgs a = cp_point_args(n, height, width, n_points, chart, ixy, z, depths, confidence, confidence_weighting);
    double* partials = workspace_at<double>(workspace, cp_layout(n, n_points).partials);
    const int spans = (int)cp_spans(n_points);
    hipLaunchKernelGGL(cp_loss_kernel, dim3((unsigned)spans), dim3(256), 0, s, a, partials);
    hipLaunchKernelGGL(cp_loss_fold_kernel, dim3(1), dim3(256), 0, s, spans, n_points, (const double*)partials, out1);
    return stage_done("chart_points_loss_forward", s);
}

extern "C" int g4s_chart_points_loss_backward(int n, int height, int width, int n_points, const int* chart, const float* ixy,
                                              const float* z, const float* depths, const float* confidence,
                                              float confidence_weighting, const int* taps, const unsigned int* starts,
                                              const float* grad_out1, float* dL_ddepths, float* dL_dconfidence, char* workspace,
                                              size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cp_check_loss(n, height, width, n_points, chart, ixy, z, depths, workspace, workspace_bytes)) return rc;
    if (!taps || !starts || !grad_out1 || !dL_ddepths || (confidence && !dL_dconfidence)) return null_pointer();
    const PointArgs a = cp_point_args(n, height, width, n_points, chart, ixy, z, depths, confidence, confidence_weighting);
    const CpLayout L = cp_layout(n, n_points);
    float* ds = workspace_at<float>(workspace, L.ds);
    float* dk = workspace_at<float>(workspace, L.dk);
    const long long pixels = (long long)n * height * width;
    hipLaunchKernelGGL(cp_point_grad_kernel, dim3(blocks256(n_points)), dim3(256), 0, s, a, grad_out1, ds, dk);
    hipLaunchKernelGGL(cp_gather_kernel, dim3(blocks256(pixels)), dim3(256), 0, s, pixels, width, height, ixy, taps, starts,
                       (const float*)ds, confidence ? (const float*)dk : (const float*)nullptr, dL_ddepths,
                       confidence ? dL_dconfidence : (float*)nullptr);
    return stage_done("chart_points_loss_backward", s);
}

extern "C" int g4s_chart_points_sample_backward(int n, int height, int width, int n_points, const float* ixy, const int* taps,
                                                const unsigned int* starts, const float* grad_values, float* dL_dmap,
                                                void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cp_check_shape(n, height, width, n_points)) return rc;
    if (!starts || !dL_dmap || (n_points > 0 && (!ixy || !taps || !grad_values))) return null_pointer();
    const long long pixels = (long long)n * height * width;
    hipLaunchKernelGGL(cp_gather_kernel, dim3(blocks256(pixels)), dim3(256), 0, s, pixels, width, height, ixy, taps, starts,
                       grad_values, (const float*)nullptr, dL_dmap, (float*)nullptr);
    return stage_done("chart_points_sample_backward", s);
}
