// The chart matcher of MAtCha's chart alignment (include/g4s_losses.h, "Chart matcher": g4s_chart_match*), kernels and
// entry points.
//
// Reference semantics: matcha/dm_modules/matcher_3d.py:6-187 -- Matcher3D.match and compute_reprojection_errors -- and the
// matching loss of ParallelAligner.optimize (matcha/dm_scene/parallel_aligner.py:790-797), which repeats the n N points n
// times, multiplies them by every camera, calls grid_sample on every depth map and keeps [n,n,H,W] tensors for autograd.
//
// MI355X design: one thread owns a source pixel (j, p), back-projects it once and walks the n target cameras in a
// wave-uniform loop.  The camera records and the depth maps are kernel parameters of their own, const and __restrict__, apart
// from the argument block whose other pointers the kernels store through: only then can the compiler prove that no store of
// the kernel clobbers a record, and read its 44 floats through the uniform address with scalar loads into SGPRs instead of
// once per lane (as members of the block, two of the three kernels loaded them per lane).  The pair is evaluated in registers (one projection, four gathered taps) and reduced on the spot: the match kernel
// ballots a bit per lane and stores whole words, the loss kernel adds into a per-thread sum that waves, blocks and a
// one-block pass fold in a fixed order, the backward keeps the source-point part in a register and scatters the tap part
// as 2^36 fixed-point integers with 64-bit integer atomics (associative: bit-identical from run to run), which a finishing
// pass scales into dL/dD.  Nothing of size n n N exists except the match bits.
#include "g4s_internal.h"
#include "fixed_sums.h"
#include "chart_common.h"
#include "../../include/g4s_losses.h"

namespace g4s {

constexpr long long CM_MAX_TERMS = 1ll << 26;     // n H W max(1, weight_max): that many terms of at most 2^36 stay below 2^62
constexpr double CM_FIXED_ONE = 68719476736.0;    // 2^36
constexpr int CM_CAM_FLOATS = 44;                 // o[3], D[3][3], V[4][4], P[4][4]
constexpr float CM_ZNEAR = 1e-6f;
constexpr float CM_NO_MATCH = 1e8f;

struct MatchArgs {
    int n, W, H, N, nwords;   // N = H W, nwords = ceil(N / 32)
    float fax, fay, fbx, fby; // float(W/m), float(H/m), float(-m/W), float(-m/H)
    const float* weights;     // [n][N] or NULL
    float thr, weight_max;
    uint32_t* words;          // [n][n][nwords]
    const uint32_t* words_in;
    float* errors;            // [n][n][N] or NULL
    int raw_errors;
    uint8_t* fov_mask;        // [n][n][N] or NULL
    float* partials;          // [n * blocks per view]
    int nblocks;
    float* out1;
    const float* g1;
    float* d_depths;          // [n][N]
    unsigned long long* acc;  // [n][N] fixed-point sums of the tap scatter
};

struct Source {
    float dir[3], q[3];
};
// One (target, source pixel) pair in the contract's order of operations.
struct Pair {
    float z, s, e;
    bool fov;
    // what the backward needs on top
    float dsrc;       // dz - (s_x dix + s_y diy)
    int tap[4];       // index into the target map, -1 outside
    float wt[4];
};

__device__ __forceinline__ void cm_source(const float* __restrict__ c, float x, float y, float d, Source& o) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.dir[k] = (c[3 + 3 * k] * x + c[4 + 3 * k] * y) + c[5 + 3 * k];
        o.q[k] = d * o.dir[k] + c[k];
    }
}

__device__ __forceinline__ float cm_rows3(float a0, float a1, float a2, const float* __restrict__ M, int c) {
    return (a0 * M[c] + a1 * M[4 + c]) + a2 * M[8 + c];
}

// `c`: the target's camera record, `Di`: its depth map; both wave-uniform addresses.
template <bool GRAD>
__device__ __forceinline__ void cm_pair(const MatchArgs& a, const float* __restrict__ c, const float* __restrict__ Di,
                                        const Source& src, Pair& o) {
    const float* V = c + 12;
    const float* P = c + 28;
    const float v0 = cm_rows3(src.q[0], src.q[1], src.q[2], V, 0) + V[12];
    const float v1 = cm_rows3(src.q[0], src.q[1], src.q[2], V, 1) + V[13];
    const float z = cm_rows3(src.q[0], src.q[1], src.q[2], V, 2) + V[14];
    const float r0 = cm_rows3(-v0, -v1, z, P, 0) + P[12];
    const float r1 = cm_rows3(-v0, -v1, z, P, 1) + P[13];
    const float r3 = cm_rows3(-v0, -v1, z, P, 3) + P[15];
    const float wc = r3 < CM_ZNEAR ? CM_ZNEAR : r3;  // clamp_min: a NaN stays
    float ux = r0 / wc, uy = r1 / wc;
    const bool fin = isfinite(ux) && isfinite(uy);
    if (!isfinite(ux)) ux = 0.0f;
    if (!isfinite(uy)) uy = 0.0f;
    const float gx = (ux * a.fax) * a.fbx, gy = (uy * a.fay) * a.fby;
    const float ix = ((gx + 1.0f) * (float)a.W - 1.0f) / 2.0f, iy = ((gy + 1.0f) * (float)a.H - 1.0f) / 2.0f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float wx1 = ix - fx0, wy1 = iy - fy0;
    const float wx0 = (fx0 + 1.0f) - ix, wy0 = (fy0 + 1.0f) - iy;
    // the edge tests in float: a coordinate of any size (or inf, from an overflow) is decided before it becomes an index
    const bool inx0 = fx0 >= 0.0f && fx0 <= (float)(a.W - 1), inx1 = fx0 >= -1.0f && fx0 <= (float)(a.W - 2);
    const bool iny0 = fy0 >= 0.0f && fy0 <= (float)(a.H - 1), iny1 = fy0 >= -1.0f && fy0 <= (float)(a.H - 2);
    const int x0 = (inx0 || inx1) ? (int)fx0 : 0, y0 = (iny0 || iny1) ? (int)fy0 : 0;
    const bool in[4] = {inx0 && iny0, inx1 && iny0, inx0 && iny1, inx1 && iny1};
    const float wt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
    const float sxw[4] = {-wy0, wy0, -wy1, wy1}, syw[4] = {-wx0, -wx1, wx0, wx1};
    float s = 0.0f, s_x = 0.0f, s_y = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int idx = (y0 + (t >> 1)) * a.W + (x0 + (t & 1));
        if (in[t]) {
            const float val = Di[idx];
            s = s + wt[t] * val;
            if (GRAD) {
                s_x = s_x + val * sxw[t];
                s_y = s_y + val * syw[t];
            }
        }
        if (GRAD) {
            o.tap[t] = in[t] ? idx : -1;
            o.wt[t] = wt[t];
        }
    }
    o.z = z;
    o.s = s;
    o.fov = z > 0.0f && fin && s > 0.0f;
    o.e = fabsf(z - s * (o.fov ? 1.0f : 0.0f));
    if (GRAD) {
        const float dv0 = cm_rows3(src.dir[0], src.dir[1], src.dir[2], V, 0);
        const float dv1 = cm_rows3(src.dir[0], src.dir[1], src.dir[2], V, 1);
        const float dz = cm_rows3(src.dir[0], src.dir[1], src.dir[2], V, 2);
        const float dr0 = cm_rows3(-dv0, -dv1, dz, P, 0), dr1 = cm_rows3(-dv0, -dv1, dz, P, 1);
        const float dwc = r3 >= CM_ZNEAR ? cm_rows3(-dv0, -dv1, dz, P, 3) : 0.0f;
        const float dgx = ((dr0 / wc - (ux / wc) * dwc) * a.fax) * a.fbx;
        const float dgy = ((dr1 / wc - (uy / wc) * dwc) * a.fay) * a.fby;
        const float dix = dgx * ((float)a.W / 2.0f), diy = dgy * ((float)a.H / 2.0f);
        o.dsrc = dz - (s_x * dix + s_y * diy);
    }
}

__device__ __forceinline__ float cm_nan_to_num(float e) {
    return e != e ? 0.0f : (e > 3.4028234663852886e38f ? 3.4028234663852886e38f : e);  // e >= 0 or NaN
}

// grid (ceil(N / 256), n): block (b, j) owns pixels 256 b .. 256 b + 255 of source view j
__global__ void __launch_bounds__(256) chart_match_kernel(MatchArgs a, const float* __restrict__ cams,
        const float* __restrict__ depths) {
    const int j = (int)blockIdx.y, p = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool valid = p < a.N;
    Source src{};
    if (valid) cm_source(cams + (size_t)j * CM_CAM_FLOATS, (float)(p % a.W), (float)(p / a.W), depths[(size_t)j * a.N + p], src);
    const int word0 = (int)(blockIdx.x * 8 + (threadIdx.x >> 6) * 2);  // the wave's two words
    for (int i = 0; i < a.n; i++) {
        bool bit = false;
        if (valid) {
            Pair r;
            cm_pair<false>(a, cams + (size_t)i * CM_CAM_FLOATS, depths + (size_t)i * a.N, src, r);
            bit = (r.fov ? r.e : CM_NO_MATCH) < a.thr;
            const size_t at = ((size_t)i * a.n + j) * a.N + p;
            if (a.errors) a.errors[at] = a.raw_errors ? cm_nan_to_num(r.e) : (r.fov ? r.e : CM_NO_MATCH);
            if (a.fov_mask) a.fov_mask[at] = r.fov ? 1 : 0;
        }
        const unsigned long long m = __ballot(bit);  // lanes beyond the map vote 0: the tail word's unused bits
        if (a.words && lane_id() < 2 && word0 + lane_id() < a.nwords)
            a.words[((size_t)i * a.n + j) * a.nwords + word0 + lane_id()] = (uint32_t)(m >> (32 * lane_id()));
    }
}

__global__ void __launch_bounds__(256) chart_match_loss_fwd_kernel(MatchArgs a, const float* __restrict__ cams,
        const float* __restrict__ depths) {
    __shared__ float s_red[4];
    const int j = (int)blockIdx.y, p = (int)(blockIdx.x * 256 + threadIdx.x);
    float sum = 0.0f;
    if (p < a.N) {
        Source src;
        cm_source(cams + (size_t)j * CM_CAM_FLOATS, (float)(p % a.W), (float)(p / a.W), depths[(size_t)j * a.N + p], src);
        const float w = a.weights ? fminf(fmaxf(a.weights[(size_t)j * a.N + p], -a.weight_max), a.weight_max) : 1.0f;  // as the backward
        for (int i = 0; i < a.n; i++) {
            const uint32_t word = a.words_in[((size_t)i * a.n + j) * a.nwords + (p >> 5)];
            Pair r;
            cm_pair<false>(a, cams + (size_t)i * CM_CAM_FLOATS, depths + (size_t)i * a.N, src, r);
            if (((word >> (p & 31)) & 1u) && r.fov) sum += cm_nan_to_num(r.e) * w;
        }
    }
    const float b = block_sum(sum, s_red);
    if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = b;
}

// one block of 1024 threads folds the block partials in double; fixed association => bit-reproducible
__global__ void __launch_bounds__(1024) chart_match_reduce_kernel(MatchArgs a) {
    __shared__ double s_v[1][1024];
    fold_partials<1>(a.partials, a.nblocks, s_v);
    if (threadIdx.x == 0) a.out1[0] = (float)(s_v[0][0] / ((double)a.n * (double)a.n * (double)a.N));
}

__global__ void __launch_bounds__(256) chart_match_loss_bwd_kernel(MatchArgs a, const float* __restrict__ cams,
        const float* __restrict__ depths) {
    const int j = (int)blockIdx.y, p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p >= a.N) return;
    Source src;
    cm_source(cams + (size_t)j * CM_CAM_FLOATS, (float)(p % a.W), (float)(p / a.W), depths[(size_t)j * a.N + p], src);
    float w = 1.0f;
    if (a.weights) w = fminf(fmaxf(a.weights[(size_t)j * a.N + p], -a.weight_max), a.weight_max);
    float g_src = 0.0f;
    for (int i = 0; i < a.n; i++) {
        const uint32_t word = a.words_in[((size_t)i * a.n + j) * a.nwords + (p >> 5)];
        Pair r;
        cm_pair<true>(a, cams + (size_t)i * CM_CAM_FLOATS, depths + (size_t)i * a.N, src, r);
        if (!(((word >> (p & 31)) & 1u) && r.fov) || !(r.e <= 3.4028234663852886e38f)) continue;  // nan_to_num passes no gradient where e is not finite
        const float df = r.z - r.s;
        const float G = w * (df > 0.0f ? 1.0f : (df < 0.0f ? -1.0f : 0.0f));  // sign(0) = 0
        if (G == 0.0f) continue;
        g_src += G * r.dsrc;
        unsigned long long* acc = a.acc + (size_t)i * a.N;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (r.tap[t] < 0) continue;
            const long long f = __double2ll_rn((double)(G * r.wt[t]) * CM_FIXED_ONE);  // |G wt| <= weight_max
            if (f != 0) atomicAdd(acc + r.tap[t], (unsigned long long)f);
        }
    }
    a.d_depths[(size_t)j * a.N + p] = g_src;
}

// dL_ddepths = k (source part - scattered tap sums),  k = cotangent / (n n N)
__global__ void __launch_bounds__(256) chart_match_finish_kernel(MatchArgs a) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= (long long)a.n * a.N) return;
    const float k = a.g1[0] / (float)((double)a.n * (double)a.n * (double)a.N);
    const float taps = (float)((double)(long long)a.acc[v] * (1.0 / CM_FIXED_ONE));
    a.d_depths[v] = k * a.d_depths[v] + k * (-taps);
}

}  // namespace g4s

using namespace g4s;

static inline bool cm_size_ok(int n, int height, int width) {
    return n > 0 && height > 0 && width > 0 && (long long)n * height * width <= CM_MAX_TERMS;
}

struct MatchLayout { size_t partials, acc, bytes; };
static MatchLayout cm_layout(int n, int height, int width) {
    WorkspaceCursor c;
    MatchLayout L;
    L.partials = c.take((size_t)n * chart_view_blocks(height, width) * 4);
    L.acc = c.take((size_t)n * height * width * 8);
    L.bytes = c.off;
    return L;
}

extern "C" size_t g4s_chart_match_workspace(int n, int height, int width) {
    if (!cm_size_ok(n, height, width)) return 0;
    return cm_layout(n, height, width).bytes + WORKSPACE_BASE_SLACK;
}

static int cm_check(int n, int height, int width, const float* cameras, const float* depths) {
    if (n <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "chart match: n must be positive (no views to match)");
    if (width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "chart match: width, height must be positive");
    if ((long long)n * height * width > CM_MAX_TERMS)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart match: n H W max(1, weight_max) must be at most 2^26 (fixed-point tap sums), got n H W = %lld",
                    (long long)n * height * width);
    if (!cameras || !depths) return null_pointer();
    return G4S_OK;
}

// weight_max: the caller's bound on |weights| (1 without weights); forward and backward both clamp the weights to it
static int cm_check_weights(int n, int height, int width, const float* weights, float& weight_max) {
    if (!weights) weight_max = 1.0f;
    if (!(weight_max >= 0.0f) || !(weight_max <= 3.0e38f))
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart match: weight_max must be a finite bound on |weights|, got %g", (double)weight_max);
    const double terms = (double)n * height * width * (weight_max > 1.0f ? (double)weight_max : 1.0);
    if (terms > (double)CM_MAX_TERMS)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart match: n H W max(1, weight_max) must be at most 2^26 (fixed-point tap sums), got %.6g",
                    terms);
    return G4S_OK;
}

static MatchArgs cm_args(int n, int height, int width, char* workspace) {
    MatchArgs a{};
    a.n = n; a.W = width; a.H = height; a.N = width * height; a.nwords = (a.N + 31) / 32;
    const double m = (double)(width < height ? width : height);
    a.fax = (float)(width / m); a.fay = (float)(height / m); a.fbx = (float)(-m / width); a.fby = (float)(-m / height);
    a.nblocks = n * (int)chart_view_blocks(height, width);
    if (workspace) {
        const MatchLayout L = cm_layout(n, height, width);
        a.partials = workspace_at<float>(workspace, L.partials);
        a.acc = workspace_at<unsigned long long>(workspace, L.acc);
    }
    return a;
}
static inline dim3 cm_grid(const MatchArgs& a) { return dim3(chart_view_blocks(a.H, a.W), (unsigned)a.n); }

extern "C" int g4s_chart_match(int n, int height, int width, const float* cameras, const float* depths, float thr,
                               unsigned int* words, float* errors, int raw_errors, unsigned char* fov_mask, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cm_check(n, height, width, cameras, depths)) return rc;
    if (n > 65535) return fail(G4S_ERR_INVALID_ARGUMENT, "chart match: at most 65535 views");
    MatchArgs a = cm_args(n, height, width, nullptr);
    a.thr = thr; a.words = words; a.errors = errors; a.raw_errors = raw_errors; a.fov_mask = fov_mask;
    hipLaunchKernelGGL(chart_match_kernel, cm_grid(a), dim3(256), 0, s, a, cameras, depths);
    return stage_done("chart_match", s);
}

extern "C" int g4s_chart_match_loss_forward(int n, int height, int width, const float* cameras, const float* depths,
                                            const unsigned int* words, const float* weights, float weight_max, float* out1,
                                            char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cm_check(n, height, width, cameras, depths)) return rc;
    if (n > 65535) return fail(G4S_ERR_INVALID_ARGUMENT, "chart match: at most 65535 views");
    if (int rc = cm_check_weights(n, height, width, weights, weight_max)) return rc;
    if (!words || !out1) return null_pointer();
    if (int rc = check_workspace(workspace, workspace_bytes, g4s_chart_match_workspace(n, height, width))) return rc;
    MatchArgs a = cm_args(n, height, width, workspace);
    a.words_in = words; a.weights = weights; a.weight_max = weight_max; a.out1 = out1;
    hipLaunchKernelGGL(chart_match_loss_fwd_kernel, cm_grid(a), dim3(256), 0, s, a, cameras, depths);
    hipLaunchKernelGGL(chart_match_reduce_kernel, dim3(1), dim3(1024), 0, s, a);
    return stage_done("chart_match_loss_forward", s);
}

extern "C" int g4s_chart_match_loss_backward(int n, int height, int width, const float* cameras, const float* depths,
                                             const unsigned int* words, const float* weights, float weight_max,
                                             const float* grad_out1, float* dL_ddepths, char* workspace,
                                             size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = cm_check(n, height, width, cameras, depths)) return rc;
    if (n > 65535) return fail(G4S_ERR_INVALID_ARGUMENT, "chart match: at most 65535 views");
    if (int rc = cm_check_weights(n, height, width, weights, weight_max)) return rc;
    if (!words || !grad_out1 || !dL_ddepths) return null_pointer();
    if (int rc = check_workspace(workspace, workspace_bytes, g4s_chart_match_workspace(n, height, width))) return rc;
    MatchArgs a = cm_args(n, height, width, workspace);
    a.words_in = words; a.weights = weights; a.weight_max = weight_max; a.g1 = grad_out1; a.d_depths = dL_ddepths;
    const size_t total = (size_t)n * a.N;
    hipError_t e = hipMemsetAsync(a.acc, 0, total * 8, s);
    if (e != hipSuccess) return finish(e, "chart_match_loss_backward");
    hipLaunchKernelGGL(chart_match_loss_bwd_kernel, cm_grid(a), dim3(256), 0, s, a, cameras, depths);
    hipLaunchKernelGGL(chart_match_finish_kernel, dim3(blocks256((long long)total)), dim3(256), 0, s, a);
    return stage_done("chart_match_loss_backward", s);
}
