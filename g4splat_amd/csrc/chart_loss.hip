// The chart-prior half of the training step's loss (include/g4s_losses.h: g4s_chart_prior_*, g4s_anisotropy_*),
// kernels and entry points.
//
// Reference semantics: train_with_refine_depth.py:403-492 -- the log-depth prior, the two normal priors, the curvature
// prior (matcha/dm_utils/rendering.py:392-406, normal2curv with an all-ones mask), MAtCha's random-pair depth-order
// loss (matcha/dm_regularization/depth.py:142-214) and the anisotropy penalty on the Gaussians' scales.
//
// MI355X design: 32x8-pixel tiles.  The forward stages rend_normal with a one-pixel halo in LDS (replicate padding =
// clamped coordinates), evaluates the five per-pixel terms and reduces them per block; a one-block kernel folds the
// block partials in double, in a fixed order.  The backward stages rend_normal with a TWO-pixel halo: the curvature
// stencil is a graph Laplacian, so its adjoint is the same stencil applied to the sign weights of the pixel and its
// four neighbours, which need the Laplacian there.  The depth-order term scatters (pixel p also feeds its partner q,
// and the clamp to the image piles hundreds of partners onto a border pixel): the unit-less factor of every pair is
// added as a 2^40 fixed-point integer with 64-bit integer atomics -- integer addition is associative, so the sum does not
// depend on the arrival order and the gradient is bit-identical from run to run -- and a finishing pass scales the sums
// into dL_dsurf_depth.
#include "g4s_internal.h"
#include "fixed_sums.h"
#include "chart_common.h"
#include "../../include/g4s_losses.h"

namespace g4s {

constexpr int CP_TW = 32, CP_TH = 8;                  // tile of one 256-thread block
constexpr long long CP_MAX_PIXELS = 1ll << 22;        // 2^22 factors of at most 2^40 each stay below 2^62
constexpr double CP_FIXED_ONE = 1099511627776.0;      // 2^40

struct ChartArgs {
    int W, H, bx;  // bx: tiles across
    long long N;
    const float *rn, *sn, *pn, *sd, *pd, *pc;
    const long long* shifts;  // [N,2] (row shift, column shift) or NULL
    float depth_scale, extent, log_scale;
    float* partials;  // [blocks][5]
    int nblocks;
    float* out5;
    const float* g5;
    float *d_rn, *d_sn, *d_sd;
    unsigned long long* acc;  // [N] fixed-point sums of the depth-order scatter
};

// The partner q = clamp(p + shift_p) of pixel (px, py).
__device__ __forceinline__ long long shifted_pixel(const ChartArgs& a, long long p, int px, int py) {
    long long qy = (long long)py + a.shifts[2 * p], qx = (long long)px + a.shifts[2 * p + 1];
    qy = qy < 0 ? 0 : (qy > a.H - 1 ? a.H - 1 : qy);
    qx = qx < 0 ? 0 : (qx > a.W - 1 ? a.W - 1 : qx);
    return qy * a.W + qx;
}
// diff * pd of the pair (p, q) and the normalised prior difference pd itself (depth.py:197-201).
__device__ __forceinline__ float order_product(const ChartArgs& a, long long p, long long q, float& pdn) {
    const float diff = (a.sd[p] - a.sd[q]) / a.extent;
    const float pdiff = (a.pd[p] - a.pd[q]) / a.extent;
    pdn = pdiff / fmaxf(fabsf(pdiff), 1e-8f);
    return diff * pdn;
}
// Laplacian of one channel at an LDS position, in the reference's order (u, l, b, r).
template <int LD>
__device__ __forceinline__ float lap4(const float* s, int r, int c) {
    const float ctr = s[r * LD + c];
    return (((s[(r - 1) * LD + c] - ctr) + (s[r * LD + c - 1] - ctr)) + (s[(r + 1) * LD + c] - ctr)) + (s[r * LD + c + 1] - ctr);
}

__global__ void __launch_bounds__(256) chart_fwd_kernel(ChartArgs a) {
    constexpr int LD = CP_TW + 2, ROWS = CP_TH + 2;
    __shared__ float s_n[3][ROWS * LD];
    __shared__ float s_red[5][4];
    const int tx0 = (int)(blockIdx.x % a.bx) * CP_TW, ty0 = (int)(blockIdx.x / a.bx) * CP_TH;
    for (int i = (int)threadIdx.x; i < ROWS * LD; i += 256) {
        const int r = i / LD, c = i % LD;
        const size_t g = (size_t)clampi(ty0 - 1 + r, a.H - 1) * a.W + clampi(tx0 - 1 + c, a.W - 1);  // replicate padding
#pragma unroll
        for (int ch = 0; ch < 3; ch++) s_n[ch][i] = a.rn[ch * a.N + g];
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % CP_TW, ty = (int)threadIdx.x / CP_TW, px = tx0 + tx, py = ty0 + ty;
    float t[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (px < a.W && py < a.H) {
        const long long p = (long long)py * a.W + px;
        const float sd = a.sd[p], pd = a.pd[p];
        t[0] = logf(1.0f + a.depth_scale * fabsf(pd - sd));
        const float p0 = a.pn[p], p1 = a.pn[a.N + p], p2 = a.pn[2 * a.N + p];
        t[1] = 1.0f - ((a.sn[p] * p0 + a.sn[a.N + p] * p1) + a.sn[2 * a.N + p] * p2);
        const int c = (ty + 1) * LD + tx + 1;
        t[2] = 1.0f - ((s_n[0][c] * p0 + s_n[1][c] * p1) + s_n[2][c] * p2);
        const float curv = (fabsf(lap4<LD>(s_n[0], ty + 1, tx + 1)) + fabsf(lap4<LD>(s_n[1], ty + 1, tx + 1))) +
                           fabsf(lap4<LD>(s_n[2], ty + 1, tx + 1));
        t[3] = fabsf(a.pc[p] - curv);
        if (a.shifts) {
            const long long q = shifted_pixel(a, p, px, py);
            float pdn;
            const float x = -fminf(order_product(a, p, q, pdn), 0.0f);
            t[4] = logf(1.0f + a.log_scale * x);
        }
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const float b = block_sum(t[k], s_red[k]);
        if (threadIdx.x == 0) a.partials[5 * (size_t)blockIdx.x + k] = b;
    }
}

// one block of 1024 threads folds the block partials in double; fixed association => bit-reproducible
__global__ void __launch_bounds__(1024) chart_reduce_kernel(ChartArgs a) {
    __shared__ double s_v[5][1024];
    fold_partials<5>(a.partials, a.nblocks, s_v);
    if (threadIdx.x < 5) a.out5[threadIdx.x] = (float)(s_v[threadIdx.x][0] / (double)a.N);
}

__global__ void __launch_bounds__(256) chart_bwd_kernel(ChartArgs a) {
    constexpr int LD = CP_TW + 4, ROWS = CP_TH + 4;    // rend_normal, two-pixel halo
    constexpr int WLD = CP_TW + 2, WROWS = CP_TH + 2;  // sign weights, one-pixel halo
    __shared__ float s_n[3][ROWS * LD];
    __shared__ float s_w[3][WROWS * WLD];
    const int tx0 = (int)(blockIdx.x % a.bx) * CP_TW, ty0 = (int)(blockIdx.x / a.bx) * CP_TH;
    for (int i = (int)threadIdx.x; i < ROWS * LD; i += 256) {
        const int r = i / LD, c = i % LD;
        const size_t g = (size_t)clampi(ty0 - 2 + r, a.H - 1) * a.W + clampi(tx0 - 2 + c, a.W - 1);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) s_n[ch][i] = a.rn[ch * a.N + g];
    }
    __syncthreads();
    // sign(curv - prior_curv) * sign(lap_c) at every pixel of the tile and of its one-pixel ring that lies inside the
    // image (a position outside is no neighbour of anything: it is never read below)
    for (int i = (int)threadIdx.x; i < WROWS * WLD; i += 256) {
        const int r = i / WLD, c = i % WLD, gy = ty0 - 1 + r, gx = tx0 - 1 + c;
        float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
            const float l0 = lap4<LD>(s_n[0], r + 1, c + 1), l1 = lap4<LD>(s_n[1], r + 1, c + 1), l2 = lap4<LD>(s_n[2], r + 1, c + 1);
            const float curv = (fabsf(l0) + fabsf(l1)) + fabsf(l2);
            const float sc = signf(curv - a.pc[(size_t)gy * a.W + gx]);
            w0 = sc * signf(l0); w1 = sc * signf(l1); w2 = sc * signf(l2);
        }
        s_w[0][i] = w0; s_w[1][i] = w1; s_w[2][i] = w2;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % CP_TW, ty = (int)threadIdx.x / CP_TW, px = tx0 + tx, py = ty0 + ty;
    if (px >= a.W || py >= a.H) return;
    const long long p = (long long)py * a.W + px;
    const float inv = 1.0f / (float)a.N;  // d mean / d element, as autograd's mean backward
    const float k0 = a.g5[0] * inv, k1 = a.g5[1] * inv, k2 = a.g5[2] * inv, k3 = a.g5[3] * inv;
    const int wc = (ty + 1) * WLD + tx + 1;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const float w = s_w[ch][wc];
        float s = 0.0f;  // small integers: exact
        if (py > 0) s += s_w[ch][wc - WLD] - w;
        if (px > 0) s += s_w[ch][wc - 1] - w;
        if (py < a.H - 1) s += s_w[ch][wc + WLD] - w;
        if (px < a.W - 1) s += s_w[ch][wc + 1] - w;
        const float pn = a.pn[ch * a.N + p];
        a.d_rn[ch * a.N + p] = k3 * s - k2 * pn;
        a.d_sn[ch * a.N + p] = -(k1 * pn);
    }
    const float e = a.pd[p] - a.sd[p];
    float gd = -(((k0 / (1.0f + a.depth_scale * fabsf(e))) * a.depth_scale) * signf(e));
    if (a.shifts) {
        const long long q = shifted_pixel(a, p, px, py);
        if (q != p) {  // a pixel paired with itself: diff = 0 and its two contributions cancel
            float pdn;
            const float prod = order_product(a, p, q, pdn);
            if (prod <= 0.0f) {  // torch.clamp(max=0) passes the gradient at equality
                const float f = pdn / (1.0f + a.log_scale * (-prod));  // in [-1, 1]
                if (f != 0.0f) {
                    const float kf = ((a.g5[4] * inv) * a.log_scale) / a.extent;
                    gd -= kf * f;
                    atomicAdd(a.acc + q, (unsigned long long)__double2ll_rn((double)f * CP_FIXED_ONE));
                }
            }
        }
    }
    a.d_sd[p] = gd;
}

// dL_dsurf_depth[q] += kf * (sum of the factors scattered to q)
__global__ void __launch_bounds__(256) chart_order_finish_kernel(ChartArgs a) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.N) return;
    const long long v = (long long)a.acc[p];
    if (v == 0) return;
    const float kf = ((a.g5[4] * (1.0f / (float)a.N)) * a.log_scale) / a.extent;
    a.d_sd[p] += kf * (float)((double)v * (1.0 / CP_FIXED_ONE));
}

// ---- anisotropy penalty on the activated scales (train_with_refine_depth.py:484-489) ----
struct AnisoArgs {
    int P;
    const float2* scaling;
    float max_ratio;
    float* partials;
    int nblocks;
    float* out1;
    const float* g1;
    float2* d_scaling;
};

__global__ void __launch_bounds__(256) aniso_fwd_kernel(AnisoArgs a) {
    __shared__ float s_red[4];
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    float v = 0.0f;
    if (i < a.P) {
        const float2 s = a.scaling[i];
        v = fmaxf(fmaxf(s.x, s.y) / fminf(s.x, s.y), a.max_ratio) - a.max_ratio;
    }
    const float b = block_sum(v, s_red);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = b;
}

__global__ void __launch_bounds__(1024) aniso_reduce_kernel(AnisoArgs a) {
    __shared__ double s_v[1][1024];
    fold_partials<1>(a.partials, a.nblocks, s_v);
    if (threadIdx.x == 0) a.out1[0] = (float)(s_v[0][0] / (double)a.P);
}

__global__ void __launch_bounds__(256) aniso_bwd_kernel(AnisoArgs a) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= a.P) return;
    const float2 s = a.scaling[i];
    const float k = a.g1[0] * (1.0f / (float)a.P);
    // max(dim=1) / min(dim=1) hand a tie to the first column: there both derivatives land on s.x
    const bool x_is_max = s.x >= s.y, x_is_min = s.x <= s.y;
    const float smax = x_is_max ? s.x : s.y, smin = x_is_min ? s.x : s.y;
    const float ratio = smax / smin;
    float2 d = make_float2(0.0f, 0.0f);
    if (ratio >= a.max_ratio) {  // clamp_min passes the gradient at equality
        const float dmax = k / smin, dmin = -((k * ratio) / smin);
        if (x_is_max) d.x += dmax; else d.y += dmax;
        if (x_is_min) d.x += dmin; else d.y += dmin;
    }
    a.d_scaling[i] = d;
}

}  // namespace g4s

using namespace g4s;

static inline size_t chart_blocks(int width, int height) {
    return (size_t)((width + CP_TW - 1) / CP_TW) * (size_t)((height + CP_TH - 1) / CP_TH);
}
static inline bool chart_size_ok(int width, int height) {
    return width > 0 && height > 0 && (long long)width * height <= CP_MAX_PIXELS;
}

struct ChartLayout { size_t partials, acc, bytes; };
static ChartLayout chart_layout(int width, int height) {
    WorkspaceCursor c;
    ChartLayout L;
    L.partials = c.take(chart_blocks(width, height) * 5 * 4);
    L.acc = c.take((size_t)width * height * 8);
    L.bytes = c.off;
    return L;
}

extern "C" size_t g4s_chart_prior_workspace(int width, int height) {
    if (!chart_size_ok(width, height)) return 0;
    return chart_layout(width, height).bytes + WORKSPACE_BASE_SLACK;
}

static int chart_check(int width, int height, const char* workspace, size_t workspace_bytes) {
    if (width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive");
    if ((long long)width * height > CP_MAX_PIXELS)
        return fail(G4S_ERR_INVALID_ARGUMENT, "chart prior: at most 2^22 pixels (fixed-point depth-order sums), got %lld",
                    (long long)width * height);
    return check_workspace(workspace, workspace_bytes, g4s_chart_prior_workspace(width, height));
}

static ChartArgs chart_args(int width, int height, const float* rn, const float* sn, const float* sd, const float* pd,
                            const float* pn, const float* pc, float depth_scale, float scene_extent, float log_scale,
                            const long long* shifts, char* workspace) {
    ChartArgs a{};
    a.W = width; a.H = height; a.bx = (width + CP_TW - 1) / CP_TW;
    a.N = (long long)width * height;
    a.rn = rn; a.sn = sn; a.sd = sd; a.pd = pd; a.pn = pn; a.pc = pc; a.shifts = shifts;
    a.depth_scale = depth_scale; a.extent = scene_extent; a.log_scale = log_scale;
    a.nblocks = (int)chart_blocks(width, height);
    const ChartLayout L = chart_layout(width, height);
    a.partials = workspace_at<float>(workspace, L.partials);
    a.acc = workspace_at<unsigned long long>(workspace, L.acc);
    return a;
}

extern "C" int g4s_chart_prior_forward(int width, int height, const float* rend_normal, const float* surf_normal,
                                       const float* surf_depth, const float* prior_depth, const float* prior_normal,
                                       const float* prior_curv, float depth_scale, float scene_extent, float log_scale,
                                       const long long* pixel_shifts, float* out5, char* workspace, size_t workspace_bytes,
                                       void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = chart_check(width, height, workspace, workspace_bytes)) return rc;
    if (!rend_normal || !surf_normal || !surf_depth || !prior_depth || !prior_normal || !prior_curv || !out5) return null_pointer();
    if (misaligned(pixel_shifts, 8)) return fail(G4S_ERR_INVALID_ARGUMENT, "pixel_shifts must be 8-byte aligned");
    ChartArgs a = chart_args(width, height, rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv,
                             depth_scale, scene_extent, log_scale, pixel_shifts, workspace);
    a.out5 = out5;
    {
        ProfScope ps(PF_CHART_PRIOR, s);
        hipLaunchKernelGGL(chart_fwd_kernel, dim3(a.nblocks), dim3(256), 0, s, a);
        hipLaunchKernelGGL(chart_reduce_kernel, dim3(1), dim3(1024), 0, s, a);
    }
    return stage_done("chart_prior_forward", s);
}

extern "C" int g4s_chart_prior_backward(int width, int height, const float* rend_normal, const float* surf_normal,
                                        const float* surf_depth, const float* prior_depth, const float* prior_normal,
                                        const float* prior_curv, float depth_scale, float scene_extent, float log_scale,
                                        const long long* pixel_shifts, const float* grad_out5, float* dL_drend_normal,
                                        float* dL_dsurf_normal, float* dL_dsurf_depth, char* workspace,
                                        size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = chart_check(width, height, workspace, workspace_bytes)) return rc;
    if (!rend_normal || !surf_normal || !surf_depth || !prior_depth || !prior_normal || !prior_curv || !grad_out5 ||
        !dL_drend_normal || !dL_dsurf_normal || !dL_dsurf_depth)
        return null_pointer();
    if (misaligned(pixel_shifts, 8)) return fail(G4S_ERR_INVALID_ARGUMENT, "pixel_shifts must be 8-byte aligned");
    ChartArgs a = chart_args(width, height, rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv,
                             depth_scale, scene_extent, log_scale, pixel_shifts, workspace);
    a.g5 = grad_out5; a.d_rn = dL_drend_normal; a.d_sn = dL_dsurf_normal; a.d_sd = dL_dsurf_depth;
    hipError_t e = hipSuccess;
    {
        ProfScope ps(PF_CHART_PRIOR, s);
        if (pixel_shifts) e = hipMemsetAsync(a.acc, 0, (size_t)a.N * 8, s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(chart_bwd_kernel, dim3(a.nblocks), dim3(256), 0, s, a);
            if (pixel_shifts)
                hipLaunchKernelGGL(chart_order_finish_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, s, a);
        }
    }
    if (e != hipSuccess) return finish(e, "chart_prior_backward");
    return stage_done("chart_prior_backward", s);
}

struct AnisoLayout { size_t partials, bytes; };
static AnisoLayout aniso_layout(int P) {
    WorkspaceCursor c;
    AnisoLayout L;
    L.partials = c.take((size_t)blocks256(P) * 4);
    L.bytes = c.off;
    return L;
}

extern "C" size_t g4s_anisotropy_workspace(int P) {
    if (P <= 0) return 0;
    return aniso_layout(P).bytes + WORKSPACE_BASE_SLACK;
}

static int aniso_check(int P, const float* scaling) {
    if (P <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "anisotropy: P must be positive (the mean of no ratios is undefined)");
    if (!scaling) return null_pointer();
    if (misaligned(scaling, 8)) return fail(G4S_ERR_INVALID_ARGUMENT, "scaling must be 8-byte aligned");
    return G4S_OK;
}

extern "C" int g4s_anisotropy_forward(int P, const float* scaling, float max_ratio, float* out1, char* workspace,
                                      size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = aniso_check(P, scaling)) return rc;
    if (!out1) return null_pointer();
    if (int rc = check_workspace(workspace, workspace_bytes, g4s_anisotropy_workspace(P))) return rc;
    AnisoArgs a{};
    a.P = P; a.scaling = (const float2*)scaling; a.max_ratio = max_ratio; a.out1 = out1;
    a.nblocks = (int)blocks256(P);
    a.partials = workspace_at<float>(workspace, aniso_layout(P).partials);
    {
        ProfScope ps(PF_CHART_PRIOR, s);
        hipLaunchKernelGGL(aniso_fwd_kernel, dim3(a.nblocks), dim3(256), 0, s, a);
        hipLaunchKernelGGL(aniso_reduce_kernel, dim3(1), dim3(1024), 0, s, a);
    }
    return stage_done("anisotropy_forward", s);
}

extern "C" int g4s_anisotropy_backward(int P, const float* scaling, float max_ratio, const float* grad_out1,
                                       float* dL_dscaling, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (int rc = aniso_check(P, scaling)) return rc;
    if (!grad_out1 || !dL_dscaling) return null_pointer();
    if (misaligned(dL_dscaling, 8)) return fail(G4S_ERR_INVALID_ARGUMENT, "dL_dscaling must be 8-byte aligned");
    AnisoArgs a{};
    a.P = P; a.scaling = (const float2*)scaling; a.max_ratio = max_ratio; a.g1 = grad_out1; a.d_scaling = (float2*)dL_dscaling;
    a.nblocks = (int)blocks256(P);
    {
        ProfScope ps(PF_CHART_PRIOR, s);
        hipLaunchKernelGGL(aniso_bwd_kernel, dim3(a.nblocks), dim3(256), 0, s, a);
    }
    return stage_done("anisotropy_backward", s);
}
