// What include/g4s_optim.h declares, kernels and entry points: the fused Adam step, the activations of the Gaussian
// parameters (with and without the mip filter), the densification statistics, the mip filter sizes and, last, the
// stream compaction of Gaussian rows.
#include "g4s_internal.h"
#include "g4s_device.h"
#include "../../include/g4s_optim.h"

// ---- fused Adam over up to eight parameter segments (include/g4s_optim.h) ------------------------------
namespace g4s {
struct AdamSegs {
    float* p[8];
    const float* g[8];
    float* m[8];
    float* v[8];
    long long n[8];        // elements
    long long first[9];    // first float4-block of each segment in the launch's block space (prefix sums)
    float step_size[8];    // lr / (1 - beta1^t)
    float inv_sqrt_bc2[8]; // 1 / sqrt(1 - beta2^t)
    int nseg;
    float w1, w2, beta2, eps;  // 1 - beta1, 1 - beta2 (formed in double on the host), beta2, eps
    const float* coef;     // g4s_adam_step_device: step_size[s] = coef[s], inv_sqrt_bc2[s] = coef[8 + s] (device memory,
                           // written by adam_prep_kernel in front of this launch); NULL: the two arrays above
};

// g4s_adam_step_device: the step counts and learning rates live on the device, so that a captured launch (hipGraph) does
// the right update at every replay.  One thread per segment: t <- t + 1, then the two bias-correction factors in double,
// exactly as the host does for g4s_adam_step.
struct AdamPrep {
    float* step[8];   // per segment: torch's capturable state["step"] (a float32 scalar on the device), incremented here
    const double* lr; // [nseg] on the device (double, like the Python floats the host path divides)
    float* coef;      // [16] scratch on the device
    int nseg;
    double beta1, beta2;
};
__global__ void adam_prep_kernel(AdamPrep a) {
    const int i = (int)threadIdx.x;
    if (i >= a.nseg) return;
    const float t = *a.step[i] + 1.0f;
    *a.step[i] = t;
    const double bc1 = 1.0 - pow(a.beta1, (double)t), bc2 = 1.0 - pow(a.beta2, (double)t);
    a.coef[i] = (float)(a.lr[i] / bc1);
    a.coef[8 + i] = (float)(1.0 / sqrt(bc2));
}

// One thread per 4 consecutive floats (16-byte accesses when the segment base is 16-byte aligned, which torch
// allocations are; the tail and misaligned bases fall back to scalar accesses).
__global__ void __launch_bounds__(256) adam_kernel(AdamSegs a) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;  // float4-block index over all segments
    int s = 0;
#pragma unroll
    for (int i = 1; i < 8; i++) s += (i < a.nseg && q >= a.first[i]) ? 1 : 0;
    const long long e0 = (q - a.first[s]) * 4;
    if (q >= a.first[a.nseg] || e0 >= a.n[s]) return;
    float* p = a.p[s] + e0;
    const float* g = a.g[s] + e0;
    float* m = a.m[s] + e0;
    float* v = a.v[s] + e0;
    const float w1 = a.w1, w2 = a.w2;
    const float ss = a.coef ? a.coef[s] : a.step_size[s], ib = a.coef ? a.coef[8 + s] : a.inv_sqrt_bc2[s];
    const bool vec = e0 + 4 <= a.n[s] && (((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15) == 0;
    float pv[4], gv[4], mv[4], vv[4];
    const int cnt = vec ? 4 : (int)((a.n[s] - e0) < 4 ? (a.n[s] - e0) : 4);
    if (vec) {
        *reinterpret_cast<float4*>(pv) = *reinterpret_cast<const float4*>(p);
        *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(g);
        *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(m);
        *reinterpret_cast<float4*>(vv) = *reinterpret_cast<const float4*>(v);
    } else {
        for (int i = 0; i < cnt; i++) { pv[i] = p[i]; gv[i] = g[i]; mv[i] = m[i]; vv[i] = v[i]; }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i >= cnt) break;
        mv[i] = mv[i] + w1 * (gv[i] - mv[i]);              // exp_avg.lerp_(grad, 1 - beta1)
        vv[i] = a.beta2 * vv[i] + w2 * gv[i] * gv[i];      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float denom = sqrtf(vv[i]) * ib + a.eps;     // (exp_avg_sq.sqrt() / sqrt(bias_correction2)).add_(eps)
        pv[i] = pv[i] - ss * (mv[i] / denom);              // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
    if (vec) {
        *reinterpret_cast<float4*>(p) = *reinterpret_cast<const float4*>(pv);
        *reinterpret_cast<float4*>(m) = *reinterpret_cast<const float4*>(mv);
        *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(vv);
    } else {
        for (int i = 0; i < cnt; i++) { p[i] = pv[i]; m[i] = mv[i]; v[i] = vv[i]; }
    }
}
}  // namespace g4s

using namespace g4s;

// The part of a launch's arguments that g4s_adam_step and g4s_adam_step_device fill alike: the constants, the segments'
// pointers and sizes and their first float4-blocks.  Returns the number of float4-blocks over all segments.
static long long adam_segments(AdamSegs& a, int nseg, float* const* params, const float* const* grads, float* const* exp_avg,
                               float* const* exp_avg_sq, const long long* numel, double beta1, double beta2, double eps) {
    a.nseg = nseg; a.w1 = (float)(1.0 - beta1); a.w2 = (float)(1.0 - beta2); a.beta2 = (float)beta2; a.eps = (float)eps;
    long long blocks4 = 0;
    for (int i = 0; i < nseg; i++) {
        a.p[i] = params[i]; a.g[i] = grads[i]; a.m[i] = exp_avg[i]; a.v[i] = exp_avg_sq[i]; a.n[i] = numel[i];
        a.first[i] = blocks4;
        blocks4 += (numel[i] + 3) / 4;
    }
    for (int i = nseg; i <= 8; i++) a.first[i] = blocks4;
    return blocks4;
}

extern "C" int g4s_adam_step(int nseg, float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, const long long* numel, const double* lr, const int* step, double beta1,
                             double beta2, double eps, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (nseg < 1 || nseg > 8) return fail(G4S_ERR_INVALID_ARGUMENT, "1..8 segments");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !numel || !lr || !step) return fail(G4S_ERR_INVALID_ARGUMENT, "NULL array");
    for (int i = 0; i < nseg; i++) {
        if (numel[i] < 0 || step[i] < 1) return fail(G4S_ERR_INVALID_ARGUMENT, "segment %d: numel < 0 or step < 1", i);
        if (numel[i] > 0 && (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]))
            return fail(G4S_ERR_INVALID_ARGUMENT, "segment %d: NULL pointer", i);
    }
    AdamSegs a{};
    const long long blocks4 = adam_segments(a, nseg, params, grads, exp_avg, exp_avg_sq, numel, beta1, beta2, eps);
    for (int i = 0; i < nseg; i++) {
        const double bc1 = 1.0 - pow(beta1, (double)step[i]), bc2 = 1.0 - pow(beta2, (double)step[i]);
        a.step_size[i] = (float)(lr[i] / bc1);
        a.inv_sqrt_bc2[i] = (float)(1.0 / sqrt(bc2));
    }
    {
        ProfScope ps(PF_ADAM, s);
        if (blocks4 > 0) hipLaunchKernelGGL(adam_kernel, dim3(blocks256(blocks4)), dim3(256), 0, s, a);
    }
    return stage_done("adam_step", s);
}

extern "C" int g4s_adam_step_device(int nseg, float* const* params, const float* const* grads, float* const* exp_avg,
                                    float* const* exp_avg_sq, const long long* numel, const double* lr_dev,
                                    float* const* step_dev, float* coef_dev, double beta1, double beta2, double eps,
                                    void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (nseg < 1 || nseg > 8) return fail(G4S_ERR_INVALID_ARGUMENT, "1..8 segments");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !numel || !lr_dev || !step_dev || !coef_dev)
        return fail(G4S_ERR_INVALID_ARGUMENT, "NULL array");
    for (int i = 0; i < nseg; i++) {
        if (numel[i] < 0 || !step_dev[i]) return fail(G4S_ERR_INVALID_ARGUMENT, "segment %d: numel < 0 or NULL step", i);
        if (numel[i] > 0 && (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]))
            return fail(G4S_ERR_INVALID_ARGUMENT, "segment %d: NULL pointer", i);
    }
    AdamPrep pr{};
    pr.nseg = nseg; pr.lr = lr_dev; pr.coef = coef_dev; pr.beta1 = beta1; pr.beta2 = beta2;
    for (int i = 0; i < nseg; i++) pr.step[i] = step_dev[i];
    AdamSegs a{};
    a.coef = coef_dev;
    const long long blocks4 = adam_segments(a, nseg, params, grads, exp_avg, exp_avg_sq, numel, beta1, beta2, eps);
    {
        ProfScope ps(PF_ADAM, s);
        hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(8), 0, s, pr);  // (the counts advance even when all segments are empty)
        if (blocks4 > 0) hipLaunchKernelGGL(adam_kernel, dim3(blocks256(blocks4)), dim3(256), 0, s, a);
    }
    return stage_done("adam_step_device", s);
}

namespace g4s {
// Densification statistics of one view (2dgs/scene/gaussian_model.py:649-651 and the max_radii2D update of the
// training loop, train_with_refine_depth.py): for the Gaussians selected by `filter`
//   xyz_gradient_accum += |dL/dmean2D|_2,  denom += 1,  max_radii2D = max(max_radii2D, radii)
// in one pass (28 B per Gaussian) instead of boolean-mask gathers, a norm and scatters (about twenty launches).
__global__ void __launch_bounds__(256) densify_stats_kernel(int P, const float* __restrict__ grad, const uint8_t* __restrict__ filter,
                                                            const int* __restrict__ radii, float* __restrict__ accum,
                                                            float* __restrict__ denom, float* __restrict__ max_radii) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P || !filter[i]) return;
    const float gx = grad[3 * i], gy = grad[3 * i + 1], gz = grad[3 * i + 2];
    accum[i] += sqrtf((gx * gx + gy * gy) + gz * gz);
    denom[i] += 1.0f;
    if (max_radii != nullptr) max_radii[i] = fmaxf(max_radii[i], (float)radii[i]);
}
}  // namespace g4s

extern "C" int g4s_densify_stats(int P, const float* grad_mean2D, const unsigned char* update_filter, const int* radii,
                                 float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P must not be negative");
    if (P == 0) return G4S_OK;
    if (!grad_mean2D || !update_filter || !xyz_gradient_accum || !denom || (max_radii2D && !radii))
        return null_pointer();
    hipLaunchKernelGGL(densify_stats_kernel, dim3(blocks256(P)), dim3(256), 0, s, P, grad_mean2D, update_filter,
                       radii, xyz_gradient_accum, denom, max_radii2D);
    return stage_done("densify_stats launch", s);
}

// Activations of the Gaussian parameters as render() reads them (2dgs/scene/gaussian_model.py:157-192, without the
// optional mip filter): scales = exp(_scaling), rotations = _rotation / max(|_rotation|, 1e-12), opacity =
// sigmoid(_opacity) -- one pass instead of ~5 element-wise / reduction launches, and one pass for their backward
// instead of ~9.
namespace g4s {
__global__ void __launch_bounds__(256) activations_fwd_kernel(int P, const float2* __restrict__ scaling,
                                                              const float4* __restrict__ rotation,
                                                              const float* __restrict__ opacity, float2* __restrict__ scales,
                                                              float4* __restrict__ rots, float* __restrict__ opac) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P) return;
    const float2 s = scaling[i];
    scales[i] = make_float2(expf(s.x), expf(s.y));
    const float4 q = rotation[i];
    const float n = fmaxf(sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w), 1e-12f);
    rots[i] = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
    opac[i] = 1.0f / (1.0f + expf(-opacity[i]));
}

__global__ void __launch_bounds__(256) activations_bwd_kernel(int P, const float2* __restrict__ scales,
                                                              const float4* __restrict__ rotation,
                                                              const float* __restrict__ opac, const float2* __restrict__ g_scales,
                                                              const float4* __restrict__ g_rots, const float* __restrict__ g_opac,
                                                              float2* __restrict__ d_scaling, float4* __restrict__ d_rotation,
                                                              float* __restrict__ d_opacity) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P) return;
    const float2 y = scales[i], gs = g_scales[i];
    d_scaling[i] = make_float2(gs.x * y.x, gs.y * y.y);  // exp' = exp
    const float4 q = rotation[i], g = g_rots[i];
    const float norm = sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    if (norm > 1e-12f) {  // y = q / |q|:  dq = (g - y <y, g>) / |q|
        const float inv = 1.0f / norm;
        const float4 u = make_float4(q.x * inv, q.y * inv, q.z * inv, q.w * inv);
        const float d = ((u.x * g.x + u.y * g.y) + u.z * g.z) + u.w * g.w;
        d_rotation[i] = make_float4((g.x - u.x * d) * inv, (g.y - u.y * d) * inv, (g.z - u.z * d) * inv, (g.w - u.w * d) * inv);
    } else {              // clamped denominator: y = q / 1e-12
        d_rotation[i] = make_float4(g.x * 1e12f, g.y * 1e12f, g.z * 1e12f, g.w * 1e12f);
    }
    const float o = opac[i];
    d_opacity[i] = g_opac[i] * o * (1.0f - o);  // sigmoid' = y (1 - y)
}
}  // namespace g4s

extern "C" int g4s_activations_forward(int P, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                                       float* scales, float* rotations, float* opacities, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P must not be negative");
    if (P == 0) return G4S_OK;
    if (!scaling_raw || !rotation_raw || !opacity_raw || !scales || !rotations || !opacities)
        return null_pointer();
    if (misaligned(scaling_raw, 8) || misaligned(scales, 8) || misaligned(rotation_raw, 16) || misaligned(rotations, 16))
        return fail(G4S_ERR_INVALID_ARGUMENT, "scaling / scales must be 8-byte, rotations 16-byte aligned");
    hipLaunchKernelGGL(activations_fwd_kernel, dim3(blocks256(P)), dim3(256), 0, s, P, (const float2*)scaling_raw,
                       (const float4*)rotation_raw, opacity_raw, (float2*)scales, (float4*)rotations, opacities);
    return stage_done("activations launch", s);
}

extern "C" int g4s_activations_backward(int P, const float* scales, const float* rotation_raw, const float* opacities,
                                        const float* dL_dscales, const float* dL_drotations, const float* dL_dopacities,
                                        float* dL_dscaling_raw, float* dL_drotation_raw, float* dL_dopacity_raw, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P must not be negative");
    if (P == 0) return G4S_OK;
    if (!scales || !rotation_raw || !opacities || !dL_dscales || !dL_drotations || !dL_dopacities || !dL_dscaling_raw ||
        !dL_drotation_raw || !dL_dopacity_raw)
        return null_pointer();
    if (misaligned(scales, 8) || misaligned(dL_dscales, 8) || misaligned(dL_dscaling_raw, 8) || misaligned(rotation_raw, 16) ||
        misaligned(dL_drotations, 16) || misaligned(dL_drotation_raw, 16))
        return fail(G4S_ERR_INVALID_ARGUMENT, "scale tensors must be 8-byte, rotation tensors 16-byte aligned");
    hipLaunchKernelGGL(activations_bwd_kernel, dim3(blocks256(P)), dim3(256), 0, s, P, (const float2*)scales,
                       (const float4*)rotation_raw, opacities, (const float2*)dL_dscales, (const float4*)dL_drotations,
                       dL_dopacities, (float2*)dL_dscaling_raw, (float4*)dL_drotation_raw, dL_dopacity_raw);
    return stage_done("activations backward launch", s);
}

// ---- activations with the mip filter on (2dgs/scene/gaussian_model.py:157-192, use_mip_filter) and the filter sizes
// themselves (compute_mip_filter, :388-434); the contract and the order of operations are in include/g4s_optim.h.
namespace g4s {
__global__ void __launch_bounds__(256) activations_mip_fwd_kernel(int P, const float2* __restrict__ scaling,
                                                                  const float4* __restrict__ rotation,
                                                                  const float* __restrict__ opacity,
                                                                  const float* __restrict__ mip, float2* __restrict__ scales,
                                                                  float4* __restrict__ rots, float* __restrict__ opac) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P) return;
    const float2 s = scaling[i];
    const float f = mip[i], f2 = f * f;
    const float ex = expf(s.x), ey = expf(s.y);
    const float ex2 = ex * ex, ey2 = ey * ey;
    const float ax = ex2 + f2, ay = ey2 + f2;
    scales[i] = make_float2(sqrtf(ax), sqrtf(ay));
    const float4 q = rotation[i];
    const float n = fmaxf(sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w), 1e-12f);
    rots[i] = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
    const float coef = sqrtf((ex2 * ey2) / (ax * ay));
    opac[i] = (1.0f / (1.0f + expf(-opacity[i]))) * coef;
}

// Recomputes the forward's intermediates from the raw parameters (4 floats per Gaussian re-read) instead of reading
// saved activations (3 floats saved and read); the filter carries no gradient.
__global__ void __launch_bounds__(256) activations_mip_bwd_kernel(int P, const float2* __restrict__ scaling,
                                                                  const float4* __restrict__ rotation,
                                                                  const float* __restrict__ opacity,
                                                                  const float* __restrict__ mip,
                                                                  const float2* __restrict__ g_scales,
                                                                  const float4* __restrict__ g_rots,
                                                                  const float* __restrict__ g_opac,
                                                                  float2* __restrict__ d_scaling,
                                                                  float4* __restrict__ d_rotation,
                                                                  float* __restrict__ d_opacity) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P) return;
    const float2 s = scaling[i], gs = g_scales[i];
    const float f = mip[i], f2 = f * f;
    const float ex = expf(s.x), ey = expf(s.y);
    const float ex2 = ex * ex, ey2 = ey * ey;
    const float ax = ex2 + f2, ay = ey2 + f2;
    const float coef = sqrtf((ex2 * ey2) / (ax * ay));
    const float sg = 1.0f / (1.0f + expf(-opacity[i]));
    const float go = g_opac[i];
    const float t = (go * sg) * coef;  // g_op * opacity:  d ln(coef) / d s_k = f^2 / a_k
    d_scaling[i] = make_float2(gs.x * (ex2 / sqrtf(ax)) + t * (f2 / ax), gs.y * (ey2 / sqrtf(ay)) + t * (f2 / ay));
    d_opacity[i] = (go * coef) * (sg * (1.0f - sg));
    const float4 q = rotation[i], g = g_rots[i];
    const float norm = sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    if (norm > 1e-12f) {  // y = q / |q|:  dq = (g - y <y, g>) / |q|
        const float inv = 1.0f / norm;
        const float4 u = make_float4(q.x * inv, q.y * inv, q.z * inv, q.w * inv);
        const float d = ((u.x * g.x + u.y * g.y) + u.z * g.z) + u.w * g.w;
        d_rotation[i] = make_float4((g.x - u.x * d) * inv, (g.y - u.y * d) * inv, (g.z - u.z * d) * inv, (g.w - u.w * d) * inv);
    } else {              // clamped denominator: y = q / 1e-12
        d_rotation[i] = make_float4(g.x * 1e12f, g.y * 1e12f, g.z * 1e12f, g.w * 1e12f);
    }
}

constexpr float MIP_UNSEEN = 100000.0f;  // the reference's initial distance (:395)

// Launch 1 of g4s_mip_filter: the smallest clamped depth over the views that see the point, or MIP_UNSEEN.  The view
// index is the same in every lane, so the sixteen table reads of a view are scalar loads.  The largest value a seen
// point keeps is folded per wave and goes to *seen_max by an integer max on the float's bits (the values are positive:
// the bits order like the values, and a maximum does not depend on the order of its operands).
__global__ void __launch_bounds__(256) mip_filter_depth_kernel(int P, const float* __restrict__ xyz, int V,
                                                               const float* __restrict__ cam, float znear,
                                                               float* __restrict__ out, uint32_t* __restrict__ seen_max) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < P;
    const size_t i3 = 3 * (size_t)(live ? i : 0);
    const float x = xyz[i3], y = xyz[i3 + 1], z = xyz[i3 + 2];
    float d = MIP_UNSEEN;
    bool seen = false;
    for (int v = 0; v < V; v++) {
        const float* __restrict__ c = cam + 16 * (size_t)v;
        const float xc = ((x * c[0] + y * c[3]) + z * c[6]) + c[9];
        const float yc = ((x * c[1] + y * c[4]) + z * c[7]) + c[10];
        const float zc = ((x * c[2] + y * c[5]) + z * c[8]) + c[11];
        const float zp = fmaxf(zc, 0.001f);
        const float w = c[14], h = c[15];
        const float pu = (xc / zp) * c[12] + 0.5f * w;
        const float pv = (yc / zp) * c[13] + 0.5f * h;
        const bool ok = zc > znear && pu >= -0.15f * w && pu <= 1.15f * w && pv >= -0.15f * h && pv <= 1.15f * h;
        if (ok) d = fminf(d, zp);
        seen = seen || ok;
    }
    if (live) out[i] = d;
    const uint32_t m = wave_max_u32(live && seen ? __float_as_uint(d) : 0u);
    if (lane_id() == 0 && m != 0u) atomicMax(seen_max, m);
}

// Launch 2: points that no view sees take the largest depth of the seen ones (:431; MIP_UNSEEN when there is none),
// then the scale.  A seen point further than MIP_UNSEEN holds MIP_UNSEEN too, and then so does the maximum.
__global__ void __launch_bounds__(256) mip_filter_scale_kernel(int P, float* __restrict__ out,
                                                               const uint32_t* __restrict__ seen_max, float scale) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P) return;
    const uint32_t m = *seen_max;
    const float far = m != 0u ? __uint_as_float(m) : MIP_UNSEEN;
    const float d = out[i];
    out[i] = (d == MIP_UNSEEN ? far : d) * scale;
}
}  // namespace g4s

extern "C" int g4s_activations_mip_forward(int P, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                                           const float* mip_filter, float* scales, float* rotations, float* opacities,
                                           void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P must not be negative");
    if (P == 0) return G4S_OK;
    if (!scaling_raw || !rotation_raw || !opacity_raw || !mip_filter || !scales || !rotations || !opacities)
        return null_pointer();
    if (misaligned(scaling_raw, 8) || misaligned(scales, 8) || misaligned(rotation_raw, 16) || misaligned(rotations, 16))
        return fail(G4S_ERR_INVALID_ARGUMENT, "scaling / scales must be 8-byte, rotations 16-byte aligned");
    hipLaunchKernelGGL(activations_mip_fwd_kernel, dim3(blocks256(P)), dim3(256), 0, s, P,
                       (const float2*)scaling_raw, (const float4*)rotation_raw, opacity_raw, mip_filter, (float2*)scales,
                       (float4*)rotations, opacities);
    return stage_done("activations (mip filter) launch", s);
}

extern "C" int g4s_activations_mip_backward(int P, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                                            const float* mip_filter, const float* dL_dscales, const float* dL_drotations,
                                            const float* dL_dopacities, float* dL_dscaling_raw, float* dL_drotation_raw,
                                            float* dL_dopacity_raw, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P must not be negative");
    if (P == 0) return G4S_OK;
    if (!scaling_raw || !rotation_raw || !opacity_raw || !mip_filter || !dL_dscales || !dL_drotations || !dL_dopacities ||
        !dL_dscaling_raw || !dL_drotation_raw || !dL_dopacity_raw)
        return null_pointer();
    if (misaligned(scaling_raw, 8) || misaligned(dL_dscales, 8) || misaligned(dL_dscaling_raw, 8) ||
        misaligned(rotation_raw, 16) || misaligned(dL_drotations, 16) || misaligned(dL_drotation_raw, 16))
        return fail(G4S_ERR_INVALID_ARGUMENT, "scale tensors must be 8-byte, rotation tensors 16-byte aligned");
    hipLaunchKernelGGL(activations_mip_bwd_kernel, dim3(blocks256(P)), dim3(256), 0, s, P,
                       (const float2*)scaling_raw, (const float4*)rotation_raw, opacity_raw, mip_filter,
                       (const float2*)dL_dscales, (const float4*)dL_drotations, dL_dopacities, (float2*)dL_dscaling_raw,
                       (float4*)dL_drotation_raw, dL_dopacity_raw);
    return stage_done("activations (mip filter) backward launch", s);
}

extern "C" size_t g4s_mip_filter_workspace(void) { return align_up(sizeof(uint32_t)) + 256; }  // one word, aligned here

extern "C" int g4s_mip_filter(int P, const float* xyz, int V, const float* cameras, float znear, float scale,
                              float* mip_filter_out, char* workspace, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P must not be negative");
    if (V < 1) return fail(G4S_ERR_INVALID_ARGUMENT, "at least one view");
    if (P == 0) return G4S_OK;
    if (!xyz || !cameras || !mip_filter_out || !workspace) return null_pointer();
    if (misaligned(xyz, 4) || misaligned(cameras, 4) || misaligned(mip_filter_out, 4))
        return fail(G4S_ERR_INVALID_ARGUMENT, "float tensors must be 4-byte aligned");
    uint32_t* seen_max = (uint32_t*)align_ptr(workspace);
    if (hipMemsetAsync(seen_max, 0, sizeof(uint32_t), s) != hipSuccess) return fail(G4S_ERR_HIP, "memset failed");
    const dim3 grid(blocks256(P));
    hipLaunchKernelGGL(mip_filter_depth_kernel, grid, dim3(256), 0, s, P, xyz, V, cameras, znear, mip_filter_out, seen_max);
    hipLaunchKernelGGL(mip_filter_scale_kernel, grid, dim3(256), 0, s, P, mip_filter_out, seen_max, scale);
    return stage_done("mip_filter launch", s);
}

// ---- stream compaction of Gaussian rows: the device side of prune_points / densify_and_clone /
// densify_and_split (2dgs/scene/gaussian_model.py:510-541, 583-626).  The reference edits its six parameter tensors,
// their twelve Adam moments and three statistics with one boolean-mask indexing each (~20 gather launches plus the
// mask -> index conversions); here the mask is scanned ONCE (wave ballot + popcount per 256 rows, one single-block
// scan of the block counts) and any number of row-major [P, w] float tensors are gathered against that scan, up to
// eight per launch, with coalesced reads and writes.  Stable: kept rows stay in index order (the order the
// reference's mask indexing produces).
namespace g4s {

// block_count[b] = number of kept rows among rows [256 b, 256 b + 256)
__global__ void __launch_bounds__(256) compact_count_kernel(int P, const uint8_t* __restrict__ keep,
                                                            uint32_t* __restrict__ block_count) {
    __shared__ uint32_t s_w[4];
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool k = i < P && keep[i] != 0;
    const uint32_t c = (uint32_t)__popcll(__ballot(k));
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// single block: exclusive scan of the block counts in place; total -> *out_count
__global__ void __launch_bounds__(1024) compact_scan_kernel(int nblocks, uint32_t* __restrict__ block_count,
                                                            int* __restrict__ out_count) {
    __shared__ uint32_t wsum[16];
    const int t = (int)threadIdx.x;
    const int seg = (nblocks + 1023) / 1024;
    const int b = imin_(nblocks, t * seg), e = imin_(nblocks, b + seg);
    uint32_t sum = 0;
    for (int i = b; i < e; i++) sum += block_count[i];
    const uint32_t inc = wave_incl_scan_u32(sum);
    if ((t & 63) == 63) wsum[t >> 6] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int w = 0; w < 16; w++) {
        if (w < (t >> 6)) base += wsum[w];
        all += wsum[w];
    }
    uint32_t run = base + inc - sum;
    for (int i = b; i < e; i++) {
        const uint32_t v = block_count[i];
        block_count[i] = run;
        run += v;
    }
    if (t == 0) *out_count = (int)all;
}

struct GatherArgs {
    int nseg;
    const float* src[8];
    float* dst[8];
    int width[8];
};

// rows [256 b, 256 b + 256): kept rows are listed in LDS in index order (ballot + popcount of the lower lanes +
// the wave's base), then every tensor's kept rows are copied element by element with consecutive threads on
// consecutive floats
__global__ void __launch_bounds__(256) compact_gather_kernel(int P, const uint8_t* __restrict__ keep,
                                                             const uint32_t* __restrict__ block_off, GatherArgs a,
                                                             long long dst_row0) {
    __shared__ uint32_t s_row[256];
    __shared__ uint32_t s_w[4];
    const int t = (int)threadIdx.x, w = t >> 6;
    const int i = (int)(blockIdx.x * 256 + t);
    const bool k = i < P && keep[i] != 0;
    const uint64_t m = __ballot(k);
    if (lane_id() == 0) s_w[w] = (uint32_t)__popcll(m);
    __syncthreads();
    const uint32_t wbase = (w > 0 ? s_w[0] : 0u) + (w > 1 ? s_w[1] : 0u) + (w > 2 ? s_w[2] : 0u);
    const uint32_t nkept = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    if (k) s_row[wbase + (uint32_t)__popcll(m & lanes_below_mask())] = (uint32_t)i;
    __syncthreads();
    const size_t out0 = (size_t)dst_row0 + block_off[blockIdx.x];
    for (int s = 0; s < a.nseg; s++) {
        const int wd = a.width[s];
        const float* __restrict__ src = a.src[s];
        float* __restrict__ dst = a.dst[s] + out0 * (size_t)wd;
        const uint32_t total = nkept * (uint32_t)wd;
        for (uint32_t e = (uint32_t)t; e < total; e += 256) {
            const uint32_t r = e / (uint32_t)wd, c = e - r * (uint32_t)wd;
            dst[e] = src[(size_t)s_row[r] * wd + c];
        }
    }
}

}  // namespace g4s

extern "C" size_t g4s_compact_workspace(int P) { return align_up((size_t)((P > 0 ? P : 0) / 256 + 2) * 4) + 256; }

extern "C" int g4s_compact_scan(int P, const unsigned char* keep, int* out_count, char* workspace, size_t workspace_bytes,
                                void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P must not be negative");
    if (!out_count || !workspace || (P > 0 && !keep)) return null_pointer();
    if (int rc = check_workspace(workspace, workspace_bytes, g4s_compact_workspace(P))) return rc;
    if (P == 0) {
        if (hipMemsetAsync(out_count, 0, sizeof(int), s) != hipSuccess) return fail(G4S_ERR_HIP, "memset failed");
        return G4S_OK;
    }
    uint32_t* block_off = (uint32_t*)align_ptr(workspace);
    const int nblocks = (P + 255) / 256;
    hipLaunchKernelGGL(compact_count_kernel, dim3(nblocks), dim3(256), 0, s, P, keep, block_off);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, nblocks, block_off, out_count);
    return stage_done("compact_scan launch", s);
}

extern "C" int g4s_compact_gather(int P, const unsigned char* keep, const char* workspace, int nseg, const float* const* src,
                                  float* const* dst, const int* widths, long long dst_row0, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    clear_error();
    if (P < 0 || nseg < 0 || dst_row0 < 0) return fail(G4S_ERR_INVALID_ARGUMENT, "P, nseg, dst_row0 must not be negative");
    if (P == 0 || nseg == 0) return G4S_OK;
    if (!keep || !workspace || !src || !dst || !widths) return null_pointer();
    for (int i = 0; i < nseg; i++)
        if (!src[i] || !dst[i] || widths[i] <= 0) return fail(G4S_ERR_INVALID_ARGUMENT, "tensor %d: NULL pointer or width <= 0", i);
    const uint32_t* block_off = (const uint32_t*)align_ptr((char*)workspace);
    const int nblocks = (P + 255) / 256;
    for (int s0 = 0; s0 < nseg; s0 += 8) {
        GatherArgs a{};
        a.nseg = nseg - s0 < 8 ? nseg - s0 : 8;
        for (int i = 0; i < a.nseg; i++) { a.src[i] = src[s0 + i]; a.dst[i] = dst[s0 + i]; a.width[i] = widths[s0 + i]; }
        hipLaunchKernelGGL(compact_gather_kernel, dim3(nblocks), dim3(256), 0, s, P, keep, block_off, a, dst_row0);
    }
    return stage_done("compact_gather launch", s);
}
