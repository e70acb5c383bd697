/*
 * g4s_losses.h -- C ABI of the fused photometric loss of G4Splat's training step
 * (SURVEY.md 8(f) f2), libg4s_hip.so.
 *
 * Replaces, for one [3,H,W] render and its ground-truth image,
 *   Ll1  = l1_loss(image, gt)                                   2d-gaussian-splatting/utils/loss_utils.py:17-18
 *   ssim = ssim(image, gt)      (11x11 Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2)
 *                                                               utils/loss_utils.py:31-33, 46-79
 *   loss = (1 - lambda_dssim) Ll1 + lambda_dssim (1 - ssim)     train_with_refine_depth.py:382-383
 * and their autograd backward (five grouped 11x11 convolutions forward, their transposes backward, ~25
 * element-wise kernels) by two tiled kernels + one reduction.  The value AND dloss/dimage are produced by the
 * same call -- the training step always needs both -- so the autograd binding
 * (g4splat_amd/losses.py) only scales the stored gradient in its backward.
 */
#ifndef G4S_LOSSES_H_INCLUDED
#define G4S_LOSSES_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Device scratch needed for a width x height image (three derivative maps per channel + block partials). */
size_t g4s_photometric_workspace(int width, int height);

/*
 *   image, gt   [3,H,W] float32 (device)
 *   out3        device float[3]: loss, Ll1, ssim
 *   dL_dimage   [3,H,W]: d loss / d image (every element written); may be NULL (value only)
 * Sums are reduced in a fixed order (no atomics): bit-reproducible.
 */
int g4s_photometric_loss(int width, int height, const float* image, const float* gt, float lambda_dssim, float* out3,
                         float* dL_dimage, char* workspace, size_t workspace_bytes, void* stream);

/*
 * Geometry regularisers of the training step, fused (train_with_refine_depth.py:391-396):
 *   out2[0] = mean over pixels of  1 - sum_c rend_normal[c] * surf_normal[c]     ("normal_error.mean()")
 *   out2[1] = mean over pixels of  rend_dist                                      ("rend_dist.mean()")
 * rend_normal, surf_normal [3,H,W], rend_dist [1,H,W] float32 (device), out2 device float[2]; the caller applies
 * lambda_normal / lambda_dist.  Fixed-order reduction (bit-reproducible).  The backward takes the cotangents of the
 * two means (device float[2]) and writes every element of the three gradients:
 *   dL_drend_normal = -(g0/N) surf_normal,  dL_dsurf_normal = -(g0/N) rend_normal,  dL_drend_dist = g1/N.
 */
size_t g4s_geometry_regularizers_workspace(int width, int height);
int g4s_geometry_regularizers_forward(int width, int height, const float* rend_normal, const float* surf_normal,
                                      const float* rend_dist, float* out2, char* workspace, size_t workspace_bytes,
                                      void* stream);
int g4s_geometry_regularizers_backward(int width, int height, const float* rend_normal, const float* surf_normal,
                                       const float* grad_out2, float* dL_drend_normal, float* dL_dsurf_normal,
                                       float* dL_drend_dist, void* stream);

/*
 * Chart-prior losses of the training step, fused (train_with_refine_depth.py:403-481; MAtCha's normal2curv,
 * matcha/dm_utils/rendering.py:392-406, and compute_depth_order_loss, matcha/dm_regularization/depth.py:142-214).
 * With N = H W, p a pixel and every map float32 on the device:
 *   rend_normal, surf_normal, prior_normal   [3,H,W]
 *   surf_depth, prior_depth, prior_curv      [1,H,W]
 *   depth_scale                              the reference's charts_scale_factor
 *   pixel_shifts                             int64 [N,2] = (row shift, column shift) per pixel, exactly the tensor
 *                                            torch.randint returns (read as it is); NULL: no depth-order term
 * out5 (device float[5]) receives five UNWEIGHTED means over the N pixels; the caller applies the lambdas:
 *   out5[0] = mean log(1 + depth_scale |prior_depth - surf_depth|)                                       l.428-430
 *   out5[1] = mean (1 - sum_c surf_normal_c prior_normal_c)                                              l.431-434
 *   out5[2] = mean (1 - sum_c rend_normal_c prior_normal_c)                                              l.437
 *   out5[3] = mean |prior_curv - curv|,  curv_p = sum_c |lap_p,c|,                                       l.415, 440
 *             lap_p,c = (((n_u - n_p) + (n_l - n_p)) + (n_b - n_p)) + (n_r - n_p)  over rend_normal_c, the neighbours
 *             above, left, below, right in this order; replicate padding: a neighbour outside the image is p itself
 *   out5[4] = mean log(1 + log_scale x_p),  x_p = -min(diff_p pd_p, 0),                                  l.465-475
 *             q = clamp(p + shift_p) to the image,  diff_p = (surf_depth_p - surf_depth_q) / scene_extent,
 *             pd_p = (prior_depth_p - prior_depth_q) / scene_extent, then pd_p <- pd_p / max(|pd_p|, 1e-8);
 *             exactly 0 when pixel_shifts is NULL
 * Sums are reduced in a fixed order (per-block partials, one block finishes in double): bit-reproducible.
 *
 * The backward takes the cotangents of the five means (device float[5]) and writes EVERY element of dL_drend_normal,
 * dL_dsurf_normal [3,H,W] and dL_dsurf_depth [1,H,W]; the priors get no gradient.  It reproduces autograd at the kinks:
 * sign(0) = 0 for |prior_depth - surf_depth|, for |prior_curv - curv| and for each |lap_p,c|; the clamp of the
 * depth-order term passes the gradient where diff_p pd_p <= 0, equality included.
 *   dL_dsurf_normal_c = -(g1/N) prior_normal_c
 *   dL_drend_normal_c = -(g2/N) prior_normal_c + sum over the neighbours nb of p inside the image of (w_nb,c - w_p,c),
 *                       w_p,c = (g3/N) sign(curv_p - prior_curv_p) sign(lap_p,c)   (the stencil is a graph Laplacian:
 *                       its adjoint is the same stencil)
 *   dL_dsurf_depth_p  = -(g0/N) depth_scale sign(prior_depth_p - surf_depth_p) / (1 + depth_scale |prior_depth_p - surf_depth_p|)
 *                       - k f_p + k sum over {p' : q(p') = p} of f_p',
 *                       f_p = pd_p / (1 + log_scale x_p) where diff_p pd_p <= 0, else 0;  k = g4 log_scale / (scene_extent N)
 * The last sum is a scatter (the clamp piles hundreds of partners onto a border pixel).  Each f, a number in [-1, 1], is
 * added at scale 2^40 with 64-bit INTEGER atomics into a zeroed [N] buffer of the workspace, and a finishing pass scales
 * the sums: integer addition is associative, so the gradient is bit-identical from run to run.  2^22 terms of at most
 * 2^40 stay below 2^62: an image of more than 2^22 pixels is refused (G4S_ERR_INVALID_ARGUMENT), as is a workspace
 * smaller than g4s_chart_prior_workspace (0 for a size that is refused).  No allocation, no host synchronisation:
 * both calls can be captured in a HIP graph.
 */
size_t g4s_chart_prior_workspace(int width, int height);
int g4s_chart_prior_forward(int width, int height, const float* rend_normal, const float* surf_normal,
                            const float* surf_depth, const float* prior_depth, const float* prior_normal,
                            const float* prior_curv, float depth_scale, float scene_extent, float log_scale,
                            const long long* pixel_shifts, float* out5, char* workspace, size_t workspace_bytes,
                            void* stream);
int g4s_chart_prior_backward(int width, int height, const float* rend_normal, const float* surf_normal,
                             const float* surf_depth, const float* prior_depth, const float* prior_normal,
                             const float* prior_curv, float depth_scale, float scene_extent, float log_scale,
                             const long long* pixel_shifts, const float* grad_out5, float* dL_drend_normal,
                             float* dL_dsurf_normal, float* dL_dsurf_depth, char* workspace, size_t workspace_bytes,
                             void* stream);

/*
 * Anisotropy penalty on the Gaussians' scales (train_with_refine_depth.py:484-489):
 *   out1[0] = mean over the P Gaussians of  max(s_max / s_min, max_ratio) - max_ratio
 * scaling [P,2] float32 (device, 8-byte aligned): the ACTIVATED scales, whatever get_scaling returned; s_max, s_min
 * its row-wise maximum and minimum.  Fixed-order reduction (bit-reproducible).  The backward takes the cotangent of the
 * mean (device float[1]) and writes every element of dL_dscaling [P,2]: where s_max / s_min >= max_ratio (equality
 * included, as clamp_min's backward), d/ds_max = (g/P) / s_min and d/ds_min = -(g/P) s_max / s_min^2; zero elsewhere.
 * On a tie both land on the first column, as torch.max / torch.min pick it.  P <= 0 is refused.
 */
size_t g4s_anisotropy_workspace(int P);
int g4s_anisotropy_forward(int P, const float* scaling, float max_ratio, float* out1, char* workspace,
                           size_t workspace_bytes, void* stream);
int g4s_anisotropy_backward(int P, const float* scaling, float max_ratio, const float* grad_out1, float* dL_dscaling,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
