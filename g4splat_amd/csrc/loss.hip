// The losses of include/g4s_losses.h, kernels and entry points: the fused L1 + SSIM photometric loss with its gradient
//  and, further down, the geometry regularisers of the training step.
//
// Reference semantics: 2dgs/utils/loss_utils.py:17-18 (l1_loss), :31-33 (gaussian), :46-79 (ssim / _ssim:
// five depthwise 11x11 convolutions with zero padding), combined as train_with_refine_depth.py:382-383.
//
// MI355X design: 16x16-pixel tiles per (channel) block; the 26x26 halo tile of both images is staged in LDS
// once and the 11x11 Gaussian window is applied separably (11 + 11 taps instead of 121) to the five moments
// at the same time.  Kernel 1 turns the moments into the SSIM value and its three partial-derivative maps
// (d/dmu1 total, d/dE[x^2], d/dE[xy]) and reduces the SSIM / L1 sums per block; kernel 2 convolves the three
// maps (the adjoint of a zero-padded symmetric convolution is the same convolution) and adds the L1 sign
// term; a one-block kernel folds the block partials in double, in a fixed order.  HBM traffic ~ 130 B/pixel
// per channel-pixel against ~25 full-image passes of the eager formulation.
#include "g4s_internal.h"
#include "fixed_sums.h"
#include "../../include/g4s_losses.h"

namespace g4s {

constexpr int SS_T = 16, SS_R = 5, SS_IN = SS_T + 2 * SS_R;  // 26
constexpr int SS_LD = SS_IN + 1;                             // LDS row stride (odd: conflict-free columns)
// gaussian(11, 1.5) / sum, as float32 exactly like loss_utils.py:31-33 builds it
__device__ constexpr float kGauss[11] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f,
                                         0.10936068743467331f,  0.21300552785396576f,   0.26601171493530273f,
                                         0.21300552785396576f,  0.10936068743467331f,   0.036000773310661316f,
                                         0.0075987582094967365f, 0.001028380123898387f};
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;

struct PhotoArgs {
    int W, H;
    float lambda;
    const float* image;
    const float* gt;
    float* maps;      // [3 maps][3 channels][H][W]
    float* partials;  // [blocks][2]: ssim sum, l1 sum
    float* out3;
    float* dL_dimage;
    int nblocks;
};

__global__ void __launch_bounds__(256) ssim_fwd_kernel(PhotoArgs a) {
    __shared__ float s_x[SS_IN][SS_LD], s_y[SS_IN][SS_LD];
    __shared__ float s_h[5][SS_IN][SS_T + 1];
    __shared__ float s_red[2][4];
    const int ch = (int)blockIdx.z, tx0 = (int)blockIdx.x * SS_T, ty0 = (int)blockIdx.y * SS_T;
    const size_t N = (size_t)a.W * a.H;
    const float* img = a.image + ch * N;
    const float* gt = a.gt + ch * N;
    for (int i = (int)threadIdx.x; i < SS_IN * SS_IN; i += 256) {
        const int r = i / SS_IN, c = i % SS_IN, gx = tx0 - SS_R + c, gy = ty0 - SS_R + r;
        const bool in = gx >= 0 && gx < a.W && gy >= 0 && gy < a.H;  // zero padding (padding=window_size//2)
        s_x[r][c] = in ? img[(size_t)gy * a.W + gx] : 0.0f;
        s_y[r][c] = in ? gt[(size_t)gy * a.W + gx] : 0.0f;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < SS_IN * SS_T; i += 256) {  // rows of the halo tile, filtered along x
        const int r = i / SS_T, c = i % SS_T;
        float m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float g = kGauss[k], x = s_x[r][c + k], y = s_y[r][c + k];
            m1 = fmaf(g, x, m1); m2 = fmaf(g, y, m2);
            e11 = fmaf(g, x * x, e11); e22 = fmaf(g, y * y, e22); e12 = fmaf(g, x * y, e12);
        }
        s_h[0][r][c] = m1; s_h[1][r][c] = m2; s_h[2][r][c] = e11; s_h[3][r][c] = e22; s_h[4][r][c] = e12;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % SS_T, ty = (int)threadIdx.x / SS_T, px = tx0 + tx, py = ty0 + ty;
    float m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const float g = kGauss[k];
        m1 = fmaf(g, s_h[0][ty + k][tx], m1); m2 = fmaf(g, s_h[1][ty + k][tx], m2);
        e11 = fmaf(g, s_h[2][ty + k][tx], e11); e22 = fmaf(g, s_h[3][ty + k][tx], e22);
        e12 = fmaf(g, s_h[4][ty + k][tx], e12);
    }
    float ssim = 0, l1 = 0;
    if (px < a.W && py < a.H) {
        const float mu1sq = m1 * m1, mu2sq = m2 * m2, mu12 = m1 * m2;
        const float s1 = e11 - mu1sq, s2 = e22 - mu2sq, s12 = e12 - mu12;
        const float A1 = 2 * mu12 + SS_C1, A2 = 2 * s12 + SS_C2, B1 = mu1sq + mu2sq + SS_C1, B2 = s1 + s2 + SS_C2;
        const float rB1 = 1.0f / B1, rB2 = 1.0f / B2;
        ssim = (A1 * A2) * (rB1 * rB2);
        // partial derivatives of the map value with respect to E[x^2], E[xy] and (in total) mu1
        const float dS_de11 = -ssim * rB2;
        const float dS_de12 = 2 * A1 * (rB1 * rB2);
        const float dS_dm1 = 2 * m2 * A2 * (rB1 * rB2) - 2 * m1 * ssim * rB1 - 2 * m1 * dS_de11 - m2 * dS_de12;
        const size_t p = (size_t)py * a.W + px;
        a.maps[(0 * 3 + ch) * N + p] = dS_dm1;
        a.maps[(1 * 3 + ch) * N + p] = dS_de11;
        a.maps[(2 * 3 + ch) * N + p] = dS_de12;
        l1 = fabsf(s_x[ty + SS_R][tx + SS_R] - s_y[ty + SS_R][tx + SS_R]);
    }
    const float bs = block_sum(ssim, s_red[0]);
    const float bl = block_sum(l1, s_red[1]);
    if (threadIdx.x == 0) {
        const int b = (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
        a.partials[2 * b] = bs;
        a.partials[2 * b + 1] = bl;
    }
}

// one block of 1024 threads folds the block partials in double, in a fixed order => bit-reproducible
__global__ void __launch_bounds__(1024) photo_reduce_kernel(PhotoArgs a) {
    __shared__ double s_v[2][1024];
    fold_partials<2>(a.partials, a.nblocks, s_v);
    if (threadIdx.x == 0) {
        const double n = 3.0 * (double)a.W * (double)a.H;
        const double ssim = s_v[0][0] / n, l1 = s_v[1][0] / n;
        a.out3[0] = (float)((1.0 - (double)a.lambda) * l1 + (double)a.lambda * (1.0 - ssim));
        a.out3[1] = (float)l1;
        a.out3[2] = (float)ssim;
    }
}

__global__ void __launch_bounds__(256) ssim_bwd_kernel(PhotoArgs a) {
    __shared__ float s_m[3][SS_IN][SS_LD];
    __shared__ float s_h[3][SS_IN][SS_T + 1];
    const int ch = (int)blockIdx.z, tx0 = (int)blockIdx.x * SS_T, ty0 = (int)blockIdx.y * SS_T;
    const size_t N = (size_t)a.W * a.H;
    for (int i = (int)threadIdx.x; i < SS_IN * SS_IN; i += 256) {
        const int r = i / SS_IN, c = i % SS_IN, gx = tx0 - SS_R + c, gy = ty0 - SS_R + r;
        const bool in = gx >= 0 && gx < a.W && gy >= 0 && gy < a.H;
        const size_t p = (size_t)gy * a.W + gx;
#pragma unroll
        for (int m = 0; m < 3; m++) s_m[m][r][c] = in ? a.maps[(m * 3 + ch) * N + p] : 0.0f;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < SS_IN * SS_T; i += 256) {
        const int r = i / SS_T, c = i % SS_T;
        float v0 = 0, v1 = 0, v2 = 0;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float g = kGauss[k];
            v0 = fmaf(g, s_m[0][r][c + k], v0); v1 = fmaf(g, s_m[1][r][c + k], v1); v2 = fmaf(g, s_m[2][r][c + k], v2);
        }
        s_h[0][r][c] = v0; s_h[1][r][c] = v1; s_h[2][r][c] = v2;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % SS_T, ty = (int)threadIdx.x / SS_T, px = tx0 + tx, py = ty0 + ty;
    if (px >= a.W || py >= a.H) return;
    float cm = 0, c11 = 0, c12 = 0;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const float g = kGauss[k];
        cm = fmaf(g, s_h[0][ty + k][tx], cm); c11 = fmaf(g, s_h[1][ty + k][tx], c11); c12 = fmaf(g, s_h[2][ty + k][tx], c12);
    }
    const size_t p = (size_t)py * a.W + px;
    const float x = a.image[ch * N + p], y = a.gt[ch * N + p];
    const float inv_n = 1.0f / (3.0f * (float)a.W * (float)a.H);
    const float d = x - y;
    const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);  // torch.abs backward: sign(0) = 0
    const float dssim = cm + 2.0f * x * c11 + y * c12;               // d(sum of the SSIM map)/dx
    a.dL_dimage[ch * N + p] = ((1.0f - a.lambda) * sgn - a.lambda * dssim) * inv_n;
}

}  // namespace g4s

using namespace g4s;

extern "C" size_t g4s_photometric_workspace(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t N = (size_t)width * height;
    const size_t blocks = (size_t)((width + SS_T - 1) / SS_T) * ((height + SS_T - 1) / SS_T) * 3;
    return align_up(9 * N * 4) + align_up(blocks * 8) + 256;
}

extern "C" int g4s_photometric_loss(int width, int height, const float* image, const float* gt, float lambda_dssim,
                                    float* out3, float* dL_dimage, char* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive");
    if (!image || !gt || !out3) return null_pointer();
    if (int rc = check_workspace(workspace, workspace_bytes, g4s_photometric_workspace(width, height))) return rc;
    PhotoArgs a{};
    a.W = width; a.H = height; a.lambda = lambda_dssim; a.image = image; a.gt = gt; a.out3 = out3; a.dL_dimage = dL_dimage;
    const size_t N = (size_t)width * height;
    char* w = align_ptr(workspace);
    a.maps = (float*)w;
    a.partials = (float*)(w + align_up(9 * N * 4));
    const dim3 grid((width + SS_T - 1) / SS_T, (height + SS_T - 1) / SS_T, 3);
    a.nblocks = (int)(grid.x * grid.y * grid.z);
    {
        ProfScope ps(PF_PHOTO_LOSS, s);
        hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(photo_reduce_kernel, dim3(1), dim3(1024), 0, s, a);
        if (dL_dimage) hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(256), 0, s, a);
    }
    return stage_done("photometric_loss", s);
}

// ---- geometry regularisers of the training step (include/g4s_losses.h) ------------------------------
// normal_error.mean() = mean(1 - sum_c rend_normal_c surf_normal_c) and rend_dist.mean()
// (train_with_refine_depth.py:391-396): one pass over the seven planes + a fixed-order reduction forward, one pass
// backward, instead of ~8 element-wise / reduction launches each way.
namespace g4s {
struct GeoRegArgs {
    long long N;  // pixels
    int vec;      // N % 4 == 0 and every base 16-byte aligned
    const float *rn, *sn, *dist;
    float* partials;  // [blocks][2]
    int nblocks;
    float* out2;
    const float* g2;
    float *d_rn, *d_sn, *d_dist;
};

__global__ void __launch_bounds__(256) georeg_fwd_kernel(GeoRegArgs a) {
    __shared__ float s_red[2][4];
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    float e = 0.0f, d = 0.0f;
    if (p0 < a.N) {
        float r[3][4], n[3][4], t[4];
        const int cnt = (int)((a.N - p0) < 4 ? (a.N - p0) : 4);
        if (a.vec) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                *reinterpret_cast<float4*>(r[c]) = *reinterpret_cast<const float4*>(a.rn + c * a.N + p0);
                *reinterpret_cast<float4*>(n[c]) = *reinterpret_cast<const float4*>(a.sn + c * a.N + p0);
            }
            *reinterpret_cast<float4*>(t) = *reinterpret_cast<const float4*>(a.dist + p0);
        } else {
            for (int i = 0; i < 4; i++) {
                const long long p = p0 + (i < cnt ? i : 0);
                for (int c = 0; c < 3; c++) { r[c][i] = a.rn[c * a.N + p]; n[c][i] = a.sn[c * a.N + p]; }
                t[i] = a.dist[p];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i < cnt) {
                e += 1.0f - ((r[0][i] * n[0][i] + r[1][i] * n[1][i]) + r[2][i] * n[2][i]);
                d += t[i];
            }
        }
    }
    const float be = block_sum(e, s_red[0]);
    const float bd = block_sum(d, s_red[1]);
    if (threadIdx.x == 0) { a.partials[2 * blockIdx.x] = be; a.partials[2 * blockIdx.x + 1] = bd; }
}

__global__ void __launch_bounds__(1024) georeg_reduce_kernel(GeoRegArgs a) {
    __shared__ double s_v[2][1024];
    fold_partials<2>(a.partials, a.nblocks, s_v);
    if (threadIdx.x < 2) a.out2[threadIdx.x] = (float)(s_v[threadIdx.x][0] / (double)a.N);
}

__global__ void __launch_bounds__(256) georeg_bwd_kernel(GeoRegArgs a) {
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= a.N) return;
    const float inv = 1.0f / (float)a.N;
    const float gn = -(a.g2[0] * inv), gd = a.g2[1] * inv;  // d mean / d element = 1/N, as autograd's mean backward
    const int cnt = (int)((a.N - p0) < 4 ? (a.N - p0) : 4);
    if (a.vec) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float4 r = *reinterpret_cast<const float4*>(a.rn + c * a.N + p0);
            const float4 n = *reinterpret_cast<const float4*>(a.sn + c * a.N + p0);
            *reinterpret_cast<float4*>(a.d_rn + c * a.N + p0) = make_float4(gn * n.x, gn * n.y, gn * n.z, gn * n.w);
            *reinterpret_cast<float4*>(a.d_sn + c * a.N + p0) = make_float4(gn * r.x, gn * r.y, gn * r.z, gn * r.w);
        }
        *reinterpret_cast<float4*>(a.d_dist + p0) = make_float4(gd, gd, gd, gd);
    } else {
        for (int i = 0; i < cnt; i++) {
            for (int c = 0; c < 3; c++) {
                a.d_rn[c * a.N + p0 + i] = gn * a.sn[c * a.N + p0 + i];
                a.d_sn[c * a.N + p0 + i] = gn * a.rn[c * a.N + p0 + i];
            }
            a.d_dist[p0 + i] = gd;
        }
    }
}
}  // namespace g4s

extern "C" size_t g4s_geometry_regularizers_workspace(int width, int height) {
    const size_t blocks = ((size_t)width * height + 1023) / 1024;
    return g4s::align_up(blocks * 8) + 256;
}

// what both directions share; vec = float4 accesses: N % 4 == 0 and every plane of the direction on a 16-byte aligned base
static GeoRegArgs georeg_args(int width, int height, const float* rn, const float* sn) {
    GeoRegArgs a{};
    a.N = (long long)width * height;
    a.rn = rn; a.sn = sn;
    a.nblocks = (int)((a.N + 1023) / 1024);
    a.vec = (a.N % 4 == 0) && !misaligned(rn, 16) && !misaligned(sn, 16);
    return a;
}

extern "C" int g4s_geometry_regularizers_forward(int width, int height, const float* rend_normal, const float* surf_normal,
                                                 const float* rend_dist, float* out2, char* workspace, size_t workspace_bytes,
                                                 void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive");
    if (!rend_normal || !surf_normal || !rend_dist || !out2) return null_pointer();
    if (int rc = check_workspace(workspace, workspace_bytes, g4s_geometry_regularizers_workspace(width, height))) return rc;
    GeoRegArgs a = georeg_args(width, height, rend_normal, surf_normal);
    a.dist = rend_dist; a.out2 = out2;
    a.vec = a.vec && !misaligned(rend_dist, 16);
    a.partials = (float*)align_ptr(workspace);
    {
        ProfScope ps(PF_GEO_REG, s);
        hipLaunchKernelGGL(georeg_fwd_kernel, dim3(a.nblocks), dim3(256), 0, s, a);
        hipLaunchKernelGGL(georeg_reduce_kernel, dim3(1), dim3(1024), 0, s, a);
    }
    return stage_done("geometry_regularizers_forward", s);
}

extern "C" int g4s_geometry_regularizers_backward(int width, int height, const float* rend_normal, const float* surf_normal,
                                                  const float* grad_out2, float* dL_drend_normal, float* dL_dsurf_normal,
                                                  float* dL_drend_dist, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (width <= 0 || height <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "width, height must be positive");
    if (!rend_normal || !surf_normal || !grad_out2 || !dL_drend_normal || !dL_dsurf_normal || !dL_drend_dist)
        return null_pointer();
    GeoRegArgs a = georeg_args(width, height, rend_normal, surf_normal);
    a.g2 = grad_out2; a.d_rn = dL_drend_normal; a.d_sn = dL_dsurf_normal; a.d_dist = dL_drend_dist;
    a.vec = a.vec && !misaligned(dL_drend_normal, 16) && !misaligned(dL_dsurf_normal, 16) && !misaligned(dL_drend_dist, 16);
    {
        ProfScope ps(PF_GEO_REG, s);
        hipLaunchKernelGGL(georeg_bwd_kernel, dim3(a.nblocks), dim3(256), 0, s, a);
    }
    return stage_done("geometry_regularizers_backward", s);
}
