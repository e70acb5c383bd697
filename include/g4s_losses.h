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

/*
 * Chart matcher: the cross-view matches and the matching loss of MAtCha's chart alignment
 * (matcha/dm_modules/matcher_3d.py:6-187 with matcha/dm_scene/cameras.py:905-956 and matcha/dm_utils/rendering.py:249-288;
 * used by ParallelAligner.optimize, matcha/dm_scene/parallel_aligner.py:694-701, 790-797, 829-832).
 *
 * n views of one size H x W.  i is the TARGET view (its camera projects, its depth map is tapped), j the SOURCE view,
 * p = y W + x a source pixel, N = H W.  Every operation below is one float32 operation, in this order, with no fused
 * multiply-add (the unit is compiled with -ffp-contract=off); divisions are IEEE.
 *   cameras   device float [n][44], made on the host in double and rounded once: the ray record o[3], D[3][3] of the
 *             view (include/g4s_render_maps.h, "Visibility grid": c2w = inverse(world_view_transform^T), the pixel
 *             intrinsics from full_proj_transform and the map's size as depths_to_points_parallel derives them,
 *             D = c2w[:3,:3] inverse(intrinsics)), then world_view_transform V[4][4] and projection_matrix P[4][4],
 *             row-major, in the reference's row-vector convention
 *   depths    device float [n,H,W]
 * Back-projection (pixel centres at integer x, y):
 *   dir_k = (D[k][0] x + D[k][1] y) + D[k][2],   q_k = d dir_k + o_k,   d = depths[j][p]
 * True depth and projection in target i (the reference negates view-space x and y, projects with projection_matrix,
 * divides by w.clamp_min(1e-6) and undoes the sign and aspect factors; the general form it computes is restated, not
 * plain NDC: with an off-centre principal point, or P[3][3] != 0, it differs from the back-projection's camera):
 *   v_c = ((q_0 V[0][c] + q_1 V[1][c]) + q_2 V[2][c]) + V[3][c]  (c = 0, 1, 2),   z = v_2
 *   r_c = (((-v_0) P[0][c] + (-v_1) P[1][c]) + z P[2][c]) + P[3][c]  (c = 0, 1, 3)
 *   wc = r_3 < 1e-6 ? 1e-6 : r_3  (a NaN stays),   u_x = r_0 / wc,  u_y = r_1 / wc
 *   finite = isfinite(u_x) and isfinite(u_y);  a non-finite u is replaced by 0 (each alone)
 *   g_x = (u_x float(W/m)) float(-m/W),  g_y = (u_y float(H/m)) float(-m/H),   m = min(H, W), the quotients formed in double
 *   (matcher_3d.py:27 calls .clamp() and drops the result: it has no effect, and none here)
 * Sampling (grid_sample, bilinear, zero padding, align_corners=False):
 *   ix = ((g_x + 1) W - 1) / 2,  iy = ((g_y + 1) H - 1) / 2,   x0 = floor(ix), y0 = floor(iy)
 *   wx1 = ix - x0,  wx0 = (x0 + 1) - ix,  wy1 = iy - y0,  wy0 = (y0 + 1) - iy
 *   s = 0, then s += (wx0 wy0) D_i[y0][x0], s += (wx1 wy0) D_i[y0][x0+1], s += (wx0 wy1) D_i[y0+1][x0],
 *   s += (wx1 wy1) D_i[y0+1][x0+1], a tap outside the map skipped: it adds 0 to the value and nothing to a gradient
 *   fov = (z > 0) and finite and (s > 0),   e = |z - s fov|  (fov as 1.0 / 0.0)
 * match:  match[i][j][p] = (fov ? e : 1e8) < thr at the REFERENCE depths, the self pairs i == j included.
 * loss:   L = (1 / (n n N)) sum over i, j, p of  w_j[p] match[i][j][p] fov nan_to_num(e)  at the CURRENT depths with the
 *         matches frozen; w [n,H,W] is indexed by the SOURCE view (NULL: 1) and clamped to +-weight_max (below).  Each thread adds its n terms in index
 *         order, waves and blocks reduce in a fixed tree, one block adds the block partials in double in a fixed order.
 * dL/dD, for every pair with match and fov (and a finite e), sg = sign(z - s) with sign(0) = 0 as autograd's abs,
 *         G = w_j[p] sg and k = cotangent / (n n N):
 *   through the source point, into D_j[p]:   k G (dz - (s_x dix + s_y diy)),  where
 *     dv_c = (dir_0 V[0][c] + dir_1 V[1][c]) + dir_2 V[2][c],  dz = dv_2,
 *     dr_c = ((-dv_0) P[0][c] + (-dv_1) P[1][c]) + dv_2 P[2][c],  dwc = r_3 >= 1e-6 ? dr_3 : 0  (clamp_min's backward:
 *     zero below the clamp, the gradient at equality),  du_x = dr_0 / wc - (u_x / wc) dwc,
 *     dix = ((du_x float(W/m)) float(-m/W)) (W / 2)  (and the same in y),
 *     s_x = sum over the taps inside of D_tap (-wy0, +wy0, -wy1, +wy1),  s_y = ... (-wx0, -wx1, +wx0, +wx1): what
 *     grid_sample's backward returns, also on a pixel-centre line (x0 = ix: the derivative to the right) and with taps
 *     off the edge (they drop out of s_x, s_y);
 *   through the taps, into D_i[tap]:   -k G (tap weight)  for each tap inside.
 *   The per-thread sum over i of the first part is held in a register in index order.  The second part is a scatter:
 *   each term G (tap weight) is added at scale 2^36 with 64-bit INTEGER atomics into a zeroed [n,N] buffer of the
 *   workspace and a finishing pass scales the sums, so the gradient is bit-identical from run to run.  A target pixel
 *   receives at most one tap of each of the n N source pixels, each term at most weight_max in magnitude:
 *   n N max(1, weight_max) 2^36 <= 2^62.  RANGE LIMIT: n H W max(1, weight_max) <= 2^26, refused beyond it
 *   (G4S_ERR_INVALID_ARGUMENT); weight_max is the caller's bound on |w| (1 without weights), and BOTH loss calls use the
 *   weights clamped to [-weight_max, weight_max]: a weight beyond the declared bound cannot overflow the sum, and the
 *   gradient stays the gradient of the value that the forward returned.
 * Decision edges: z > 0, s > 0, e < thr, r_3 < 1e-6, the floors and the four edge tests of each tap are evaluated in
 * the order above.  A pair within rounding of an edge may be decided the other way than the reference's matmuls decide it.
 *
 * g4s_chart_match        words [n][n][ceil(N/32)] uint32, bit p mod 32 of word p / 32, whole words written from wave
 *                        ballots, the tail word's unused bits 0.  Optional (NULL: not written): errors float [n,n,H,W],
 *                        fov ? e : 1e8 (the reference's reference_errors) or, with raw_errors != 0, nan_to_num(e) (what
 *                        compute_reprojection_errors returns); fov_mask uint8 [n,n,H,W].  words may be NULL too.
 * g4s_chart_match_loss_forward   out1: device float[1], no host read.
 * g4s_chart_match_loss_backward  grad_out1: device float[1], the cotangent; dL_ddepths [n,H,W], every element written.
 *                        Nothing of size n n N is stored.  No allocation, no host synchronisation: forward and backward
 *                        can be captured in a HIP graph.
 * All three refuse n <= 0, H <= 0, W <= 0 and n H W > 2^26; the two loss calls the range limit and a workspace smaller than
 * g4s_chart_match_workspace (0 for a size that is refused).
 */
size_t g4s_chart_match_workspace(int n, int height, int width);
int g4s_chart_match(int n, int height, int width, const float* cameras, const float* depths, float thr,
                    unsigned int* words, float* errors, int raw_errors, unsigned char* fov_mask, void* stream);
int g4s_chart_match_loss_forward(int n, int height, int width, const float* cameras, const float* depths,
                                 const unsigned int* words, const float* weights, float weight_max, float* out1,
                                 char* workspace, size_t workspace_bytes, void* stream);
int g4s_chart_match_loss_backward(int n, int height, int width, const float* cameras, const float* depths,
                                  const unsigned int* words, const float* weights, float weight_max,
                                  const float* grad_out1, float* dL_ddepths, char* workspace, size_t workspace_bytes,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
