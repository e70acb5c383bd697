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

/*
 * Chart alignment losses: the depth, gradient, normal and curvature terms of MAtCha's chart alignment, fused
 * (ParallelAligner.loss and .optimize, matcha/dm_scene/parallel_aligner.py:422-458, 713-722, 757-788, with
 * depths_to_points_parallel, depth2normal_parallel and normal2curv_parallel, matcha/dm_utils/rendering.py:249-322, 409-436,
 * and img_grad, matcha/dm_utils/image.py:4-9).
 *
 * n charts of one size H x W, N = H W, p = (y, x).  Every operation below is one float32 operation, in this order, with no
 * fused multiply-add (the unit is compiled with -ffp-contract=off); divisions and square roots are IEEE.
 *   cameras   device float [n][12]: the ray record o[3], D[3][3] of each view, the first 12 floats of the matcher's record
 *   depths and every other map: float32 on the device
 * Points:     dir_k = (D[k][0] x + D[k][1] y) + D[k][2],   q_k = d dir_k + o_k                    (as for the matcher)
 * Normals nu [n,H,W,3]: for an interior pixel (1 <= y <= H-2, 1 <= x <= W-2)
 *               a = q(y+1,x) - q(y-1,x)  (the reference's "dx", a ROW difference),   b = q(y,x+1) - q(y,x-1),   formed as
 *               a_k = (d(y+1,x) - d(y-1,x)) dir_k(y+1,x) + d(y-1,x) (D[k][1] + D[k][1]),
 *               b_k = (d(y,x+1) - d(y,x-1)) dir_k(y,x+1) + d(y,x-1) (D[k][0] + D[k][0])
 *               (the two rays differ by exactly 2 D[k][1], 2 D[k][0]: the same differences, but with the rounding of
 *               their own size, not of the points'; subtracting the float32 points loses four to five bits, which on
 *               noisy depths puts the float32 curvature mean a float32 ulp from its float64 value),
 *               c = a x b = (a_1 b_2 - a_2 b_1, a_2 b_0 - a_0 b_2, a_0 b_1 - a_1 b_0),  L = sqrt((c_0 c_0 + c_1 c_1) + c_2 c_2),
 *               nu = c / (L < 1e-12 ? 1e-12 : L)      (F.normalize; a NaN stays)
 *             every border pixel is exactly 0; a map with H < 3 or W < 3 has no interior.
 * Curvature kappa [n,H,W]:  lap_c = (((nu_u - nu_p) + (nu_l - nu_p)) + (nu_b - nu_p)) + (nu_r - nu_p), the neighbours above,
 *             left, below, right in this order, replicate padding (a neighbour outside the map is p itself): the stencil
 *             and order of the chart-prior section;  kappa = (|lap_0| + |lap_1|) + |lap_2|.  (optimize passes a mask of ones
 *             shaped like the normals, so the reference's curvature has three equal channels; the mean is the same.)
 * out4 (device float[4]) receives four UNWEIGHTED means; the caller applies the weights:
 *   out4[0] = mean over n N of            m_p (c_p |d_p - r_p| - lambda log c_p)                            l.435-458
 *             r: reference_depths (the target); c: confidence, the ACTIVATED 1 + exp(_confidence) (NULL: the term is
 *             |d - r|); lambda: confidence_weighting (0.2 in the reference); m: masks (NULL: 1)
 *   out4[1] = mean over 2 n (H-1)(W-1) of |gm (D_k d - D_k d0)|,  k = row, column                           l.760-766
 *             D_row d = d(y+1,x) - d(y,x),  D_col d = d(y,x+1) - d(y,x), both for y < H-1 and x < W-1; each pixel adds its
 *             row term and its column term; d0: initial_depths (the aligner's _depths, NOT r); gm: gradient_masks
 *             [n,H-1,W-1] (NULL: 1), applied per view (for gm >= 0 this is gm |D_k d - D_k d0|)
 *   out4[2] = mean over n N of            1 - ((nu0_0 nu_0 + nu0_1 nu_1) + nu0_2 nu_2)                      l.776-780
 *             a border pixel contributes exactly 1
 *   out4[3] = mean over n N of            |kappa0 - kappa|                                                  l.782-788
 *   nu0 = initial_normals [n,H,W,3] and kappa0 = initial_curvatures [n,H,W]: what g4s_chart_align_normals makes of the
 *   initial depths, computed once by the caller.
 *   flags: G4S_CHART_ALIGN_GRADIENT | _NORMAL | _CURVATURE switch terms 1, 2, 3 on; a term that is off leaves exactly 0
 *   in its slot, reads none of its inputs (they may be NULL) and does no work.
 *   Sums are reduced in a fixed order and in double (the float32 terms of 256 consecutive pixels of one view in a tree
 *   per block, one block finishes over the block partials): bit-reproducible, and a mean is as good as its terms.
 * The backward takes the cotangents of the four means (device float[4]) and writes EVERY element of dL_ddepths [n,H,W]
 * and, if confidence is given, of dL_dconfidence [n,H,W].  It reproduces autograd at the kinks: sign(0) = 0 for d - r, for
 * gm (D_k d - D_k d0), for each lap_c and for kappa0 - kappa; the clamp at 1e-12 passes the gradient at equality and gives
 * G / 1e-12 below it.  With k0 = g0 / float(n N), k2, k3 alike and k1 = g1 / float(2 n (H-1)(W-1)), dL/dd_p is the sum, in
 * this order, of
 *   depth:     ((k0 m_p) c_p) sign(d_p - r_p),     and dL/dc_p = (k0 m_p) (|d_p - r_p| - lambda / c_p)
 *   gradient:  k1 s,  s = 0 - s_row(y,x) - s_col(y,x) + s_row(y-1,x) + s_col(y,x-1) over the stencils that exist (at most
 *              four memberships), s_k = gm sign(gm (D_k d - D_k d0))
 *   normal and curvature:  dir(p) . dL/dq(p) = (dir_0 dq_0 + dir_1 dq_1) + dir_2 dq_2, where
 *              w_p,c = sign(kappa_p - kappa0_p) sign(lap_p,c),   G_p = k3 (sum over the four neighbours nb, in the order
 *              above, of (w_nb - w_p)) - k2 nu0_p   for an interior p (all its neighbours lie inside; border normals are
 *              constants; the stencil is a graph Laplacian: its adjoint is the same stencil),
 *              dL/dc = G / L - c (((c_0 G_0 + c_1 G_1) + c_2 G_2) / ((L L) L))    (G / 1e-12 where L < 1e-12),
 *              A = b x dL/dc,  B = dL/dc x a  (0 off the interior),
 *              dq(p') = 0 + A(y'-1,x') - A(y'+1,x') + B(y',x'-1) - B(y',x'+1), a neighbour outside the map skipped.
 * Every step is a gather from a fixed neighbourhood: no atomics, no fixed-point sums, no range limit on the values.
 *
 * Launches per call: g4s_chart_align_normals 1 or 2; forward 3 (normals, terms, reduce; 2 with the normal and curvature
 * terms off); backward 3 (normals, A and B, gather; 2 with the curvature term off, 1 with the normal term off as well).
 * The normals, A and B pass through three [n,H,W,3] maps of the workspace.  No allocation, no host synchronisation:
 * forward and backward can be captured in a HIP graph.
 *
 * g4s_chart_align_normals   normals [n,H,W,3] and curv_out [n,H,W] of `depths`; either may be NULL.  With depths NULL,
 *                           `normals` is READ and only curv_out is written (the curvature of any normal map).
 * All refuse (G4S_ERR_INVALID_ARGUMENT, with a message) n, H or W <= 0 and sizes whose [n,H,W,3] maps have 2^31 elements
 * or more (g4s_chart_align_workspace is 0 for them); the two loss calls also a workspace smaller than
 * g4s_chart_align_workspace, and the gradient term with H < 2 or W < 2 -- the reference's mean over an empty tensor is NaN
 * there.
 */
#define G4S_CHART_ALIGN_GRADIENT 1
#define G4S_CHART_ALIGN_NORMAL 2
#define G4S_CHART_ALIGN_CURVATURE 4
size_t g4s_chart_align_workspace(int n, int height, int width);
int g4s_chart_align_normals(int n, int height, int width, const float* cameras, const float* depths, float* normals,
                            float* curv_out, void* stream);
int g4s_chart_align_forward(int n, int height, int width, const float* cameras, const float* depths,
                            const float* reference_depths, const float* confidence, const float* masks,
                            const float* initial_depths, const float* gradient_masks, const float* initial_normals,
                            const float* initial_curvatures, float confidence_weighting, int flags, float* out4,
                            char* workspace, size_t workspace_bytes, void* stream);
int g4s_chart_align_backward(int n, int height, int width, const float* cameras, const float* depths,
                             const float* reference_depths, const float* confidence, const float* masks,
                             const float* initial_depths, const float* gradient_masks, const float* initial_normals,
                             const float* initial_curvatures, float confidence_weighting, int flags,
                             const float* grad_out4, float* dL_ddepths, float* dL_dconfidence, char* workspace,
                             size_t workspace_bytes, void* stream);

/*
 * Chart deformation: the trainable half of MAtCha's chart alignment, fused -- the chart encodings, the depth encoding, the
 * per-chart MLP and the deformed depths (ParallelAligner.verts_deformations, .verts, .deformed_depths,
 * matcha/dm_scene/parallel_aligner.py:341-413; MultiResChartsEncoding, ChartsEncoding, DepthEncoding,
 * matcha/dm_deformation/encodings.py:49-179; DeformationMultiMLP, MultiLinear, matcha/dm_deformation/multi_mlp.py:33-242) in the
 * configuration charts_alignment.py runs: depth encoding mode 'add' (or none), plain DeformationMultiMLP, output dimension 1
 * along the rays, not in disparity space, no final non-linearity.
 *
 * n charts of one size H x W, N = H W, pixel p = (r, c) = (p / W, p % W).  Every operation below is one float32 operation, in
 * this order; a product-sum written fma(a, b, s) is ONE fused operation, everything else is unfused (-ffp-contract=off).
 *   levels[l]       device float [n][C][h_l][w_l], l < L: the reference's parameter layout.  E = L C.
 *   depth_encoding  device float [n][E][B] (bins = 0: absent, and depth_coords is not read)
 *   weights[j], biases[j], j < layers: device float [n][out_j][in_j], [n][out_j]; in_0 = E, out_j = layer_size = S for
 *                   j < layers - 1, out of the last layer 1
 *   depth_coords    device float [n][N] in [0, 1];  cameras  device float [n][12], the ray record o[3], D[3][3] of each view;
 *   initial_depths  device float [n][N]
 * Positions.  lin_K[i] = float(2 i - (K - 1)) / float(K - 1) (-1 for K = 1): the correctly rounded torch.linspace(-1, 1, K)[i];
 *             torch's own float32 linspace is off it by an ulp or two at some i.  Pixel (r, c) samples at u_x = lin_H[r],
 *             u_y = lin_W[c]: the reference builds _pts_uv as (lin_H[r], lin_W[c]) and grid_sample reads component 0 as x, the
 *             WIDTH axis, so the pixel's ROW runs along a level's width.  Kept.
 * Taps(u, size):  t = ((u + 1) size - 1) / 2, clamped to [0, size - 1] (padding_mode='border', align_corners=False),
 *             i0 = floor(t), i1 = min(i0 + 1, size - 1), w0 = (floor(t) + 1) - t, w1 = t - floor(t).  Where i1 is clamped w1 is
 *             exactly 0 (grid_sample skips that tap; here it adds v 0, which differs only for a non-finite v).
 * Chart encoding of channel e = l C + ch:  (x0, x1, wx0, wx1) = Taps(u_x, w_l), (y0, y1, wy0, wy1) = Taps(u_y, h_l), v = levels[l][i][ch],
 *             enc_e = ((v[y0][x0] (wx0 wy0) + v[y0][x1] (wx1 wy0)) + v[y1][x0] (wx0 wy1)) + v[y1][x1] (wx1 wy1)
 * Depth encoding (an image of height B and width 1 sampled at x = 0):  (b0, b1, w0, w1) = Taps(-1 + 2 depth_coords[i][p], B),
 *             x_e = enc_e + (q[b0] w0 + q[b1] w1),  q = depth_encoding[i][e]         (mode 'add'; x_e = enc_e without)
 * MLP.        a_0 = x / scene_radius  (the reference's centre terms are exactly 0 and its input scale exactly 1);
 *             layer j < layers - 1:  z_o = b_o, then z_o = fma(W[o][k], a[k], z_o) over k in the order
 *                 k = 16 t + 4 g + s  for t = 0 .. in/16 - 1, s = 0..3, g = 0..3 (g fastest)
 *             -- the order in which the accumulator registers of one 16x16x4 MFMA tile feed the next product (an MFMA is a
 *             k-ordered fma chain) --, a = z > 0 ? z : 0;
 *             last layer:  p_g = fma chain from 0 over k = 16 t + 4 g + s (t, then s) for g = 0..3,
 *                 out = ((p_0 + p_1) + (p_2 + p_3)) + b;       delta = out deformation_radius
 * Deformed depth.  The reference forms verts = _verts + delta normalize(_rays), rays = verts - centre, and takes the view-space
 *             z.  Here, from the initial depth d0 and the ray record: dir_k = (D[k][0] c + D[k][1] r) + D[k][2],
 *                 depth = d0 + delta (sign(d0) / sqrt((dir_0 dir_0 + dir_1 dir_1) + dir_2 dir_2)),   exactly d0 where d0 = 0
 *             (the view-space z of dir is 1, so ray_hat . z = sign(d0) / |dir|).  No float32 points are subtracted: as for the
 *             normals above, that keeps the four to five bits the points' rounding would take.  normalize's clamp at 1e-12
 *             is not modelled for 0 < |d0| |dir| < 1e-12.
 * Supported envelope (anything else is refused with a message that names the limit): L <= G4S_CHART_DEFORM_MAX_LEVELS, C a
 *   multiple of 4, E in {16, 32, 64}, S in {32, 64}, 2 <= layers <= 4, 0 <= B <= 4096, every level 1 x 1 to 2^24 texels,
 *   n H W < 2^31, scene_radius > 0.
 * The backward takes dL/ddepths [n][N] on the device and writes EVERY element of the gradients, in the parameters' layouts.
 *   It recomputes the activations (the forward saves nothing).  With gz = (g s) deformation_radius, s the factor of delta
 *   above (gz = 0 where d0 = 0), ReLU passes the cotangent where z > 0, and da = W^T dz is the same fma chain over the output
 *   index (from 0).  A workgroup serves G4S_CHART_DEFORM_WG_PIXELS consecutive pixels of one chart in tiles of
 *   G4S_CHART_DEFORM_TILE.  Sums over pixels have three levels, each in index order: a tile's dW[o][k] is the fma chain, from
 *   0, of dz_o(p) a_k(p) over its pixels (pixels past the end add exact zeros) and its db_o the plain sum of dz_o(p); the tile
 *   sums are added to the workgroup's running sum in tile order; a chart's workgroup sums are added in workgroup order.
 *   dL/dx = da_0 / scene_radius [n][N][E] passes through the workspace.  The encodings GATHER from it: a texel sums, over
 *   the pixels whose taps reach it (rows, then columns, in index order; a pixel's taps in the order above), dL/dx_e times the
 *   tap's weight; a depth bin likewise over a workgroup's pixels in index order (tap b0, then b1), the workgroups' sums added
 *   in order.  No atomics, no fixed-point sums, no range limit: outputs and gradients are bit-identical from run to run.
 * Launches: forward 1; backward 3 + L (+1 with a depth encoding).  No allocation, no host synchronisation, nothing read
 * back: both can be captured in a HIP graph.  Workspace (backward only; the forward ignores it): n N E floats for dL/dx and
 * n ceil(N / G4S_CHART_DEFORM_WG_PIXELS) partials of (all weights + biases + E B) floats.
 */
#define G4S_CHART_DEFORM_TILE 64
#define G4S_CHART_DEFORM_WG_PIXELS 4096
#define G4S_CHART_DEFORM_MAX_LEVELS 8
typedef struct g4s_chart_deform_shape {
    int n, height, width;
    int levels, channels; /* L, C */
    int level_height[G4S_CHART_DEFORM_MAX_LEVELS], level_width[G4S_CHART_DEFORM_MAX_LEVELS];
    int bins;             /* B; 0: no depth encoding */
    int layers, layer_size;
    float scene_radius, deformation_radius;
} g4s_chart_deform_shape;
size_t g4s_chart_deform_workspace(const g4s_chart_deform_shape* shape); /* 0 for a shape outside the envelope */
int g4s_chart_deform_forward(const g4s_chart_deform_shape* shape, const float* const* levels, const float* depth_encoding,
                             const float* const* weights, const float* const* biases, const float* depth_coords,
                             const float* cameras, const float* initial_depths, float* depths, float* delta,
                             char* workspace, size_t workspace_bytes, void* stream);
int g4s_chart_deform_backward(const g4s_chart_deform_shape* shape, const float* const* levels, const float* depth_encoding,
                              const float* const* weights, const float* const* biases, const float* depth_coords,
                              const float* cameras, const float* initial_depths, const float* dL_ddepths,
                              float* const* dL_dlevels, float* dL_ddepth_encoding, float* const* dL_dweights,
                              float* const* dL_dbiases, char* workspace, size_t workspace_bytes, void* stream);

/*
 * Chart alignment: confidence, weighted encodings, encoding regularisers -- what the reference's `strong` alignment
 * configuration adds to the deformation above (weight_encodings_with_confidence, regularize_chart_encodings_norms,
 * use_total_variation_on_depth_encodings; matcha/dm_scene/parallel_aligner.py:341-363, 806-822), and the activation of the
 * learnable confidence.  Everything of "Chart deformation" holds unless stated otherwise; every operation is one float32
 * operation in the order written, unless it says double.
 *
 * Confidence (g4s_chart_confidence_*), element-wise over count = n H W elements, one launch each:
 *   forward:   conf = 1 + expf(raw);   optionally (encoding_weights != NULL)  cw = conf - 1,  w = 1 - expf(-(cw cw) / 2)
 *              -- cw is taken from the ROUNDED 1 + exp, as the reference takes it (lines 350-351): raw <= -17 gives conf = 1,
 *              cw = 0 and w = 0 exactly; raw >= 3 gives w = 1 exactly.
 *   backward:  dL/draw = dL/dconf expf(raw).  The reference detaches w: it has no gradient.
 *   Refused: count outside 1 .. 2^31 - 1, a NULL raw, confidence, dL_dconfidence or dL_draw.
 *
 * Deformation with weights and regularisers (g4s_chart_deform_reg_*): the arguments of the plain pair, and
 *   encoding_weights  device float [n][N] or NULL;  reg_flags: G4S_CHART_DEFORM_REG_NORM | G4S_CHART_DEFORM_REG_TV
 *   reg_out   (forward)  device float [2]: the norm term, the total variation; 0 for a term not asked for.  Required when
 *             reg_flags != 0; with reg_flags = 0 it may be NULL (then the forward is 1 launch) or is written with zeros.
 *   dL_dreg   (backward) device float [2], read on the device only; required when reg_flags != 0.
 * Weighted input.  With w = encoding_weights[i][p]:  x_e = (enc_e w) + (q[b0] w0 + q[b1] w1); only the chart encoding is
 *   weighted, the depth encoding is added afterwards (lines 355-363).  Without weights x_e is the plain pair's.
 * Norm term: the mean over all n N pixels of r(p) = sqrtf((s_0 + s_1) + (s_2 + s_3)), where s_g is the fma chain, from 0, of
 *   fma(enc_e, enc_e, s_g) over the channels e = 16 t + 4 g + s (t, then s) -- the channels lane group g holds, as in the last
 *   layer.  enc_e is the UNWEIGHTED chart encoding without the depth encoding (line 812).  Sum over the pixels in double:
 *   pixel slot j < 64 of a workgroup adds r of its pixels j, j + 64, ... in that order; the workgroup adds its 64 slots in
 *   index order; thread t < 256 of the final workgroup adds the workgroups' sums t, t + 256, ... of all charts (chart-major)
 *   and thread 0 adds the 256 results in thread order.  reg_out[0] = float(sum / double(n N)).
 *   Cotangent into enc_e:  enc_e coef(p),  coef(p) = (dL_dreg[0] / r(p)) / float(n N), and coef(p) = 0 exactly where
 *   r(p) = 0 (torch's subgradient).
 * Total variation: the mean over n E (B - 1) of fabsf(q[b + 1] - q[b]) (a float32 difference, then double): thread t < 256
 *   adds the entries t, t + 256, ... of the index ((i E + e) (B - 1) + b), thread 0 adds the 256 results in thread order.
 *   reg_out[1] = float(sum / double(n E (B - 1))).  Backward: dL/dq[b] of the depth path, then
 *   + (sign(q[b] - q[b-1]) - sign(q[b+1] - q[b])) (dL_dreg[1] / float(n E (B - 1))), sign(0) = 0, a missing neighbour 0.
 *   Refused: the TV bit with B < 2 (the reference's mean over an empty tensor is NaN).
 * Backward.  The depth encoding's gradient takes the unweighted dL/dx.  A level's texel gathers, over the same pixels in the
 *   same order as in the plain backward, the term  t_e(p)  times the tap weight, where t_e(p) = dL/dx_e(p), multiplied by w(p) if
 *   there are weights, then + enc_e(p) coef(p) if the norm is asked for; enc_e(p) is formed from the pixel's four texels by
 *   the forward's expression.  Every element of every gradient is written.  No atomics; bit-identical from run to run.
 * Bit-identity: with encoding_weights = NULL and reg_flags = 0, depths, delta and every gradient are bit-identical to the
 *   plain pair's (the same kernels instantiated with the additions compiled in and switched off).  A weight of exactly 1
 *   changes nothing either.
 * Workspace (g4s_chart_deform_reg_workspace; 0 for a refused shape or flags): one double per workgroup for the norm's partial
 *   sums, then the plain pair's -- dL/dx [n][N][E], UNCHANGED and unweighted, and the partials -- then coef [n][N] floats,
 *   written by the backward's first kernel and read by the level kernels.  No second [n][N][E] array.  The backward always
 *   needs all of it.  The forward touches the workspace only with the norm bit, and then only the partial sums at its head:
 *   it asks for g4s_chart_deform_reg_forward_workspace bytes (0 for a refused shape or flags), a few KB, and nothing the
 *   forward leaves there is read by the backward.
 * Launches: forward 1 (+1 when reg_out is given); backward as the plain one.  No allocation, no host synchronisation, nothing
 *   read back: capturable in a HIP graph.
 */
#define G4S_CHART_DEFORM_REG_NORM 1
#define G4S_CHART_DEFORM_REG_TV 2
int g4s_chart_confidence_forward(long long count, const float* raw, float* confidence, float* encoding_weights, void* stream);
int g4s_chart_confidence_backward(long long count, const float* raw, const float* dL_dconfidence, float* dL_draw, void* stream);
size_t g4s_chart_deform_reg_workspace(const g4s_chart_deform_shape* shape, int reg_flags);
size_t g4s_chart_deform_reg_forward_workspace(const g4s_chart_deform_shape* shape, int reg_flags);
int g4s_chart_deform_reg_forward(const g4s_chart_deform_shape* shape, const float* const* levels, const float* depth_encoding,
                                 const float* const* weights, const float* const* biases, const float* depth_coords,
                                 const float* cameras, const float* initial_depths, const float* encoding_weights, int reg_flags,
                                 float* depths, float* delta, float* reg_out, char* workspace, size_t workspace_bytes,
                                 void* stream);
int g4s_chart_deform_reg_backward(const g4s_chart_deform_shape* shape, const float* const* levels, const float* depth_encoding,
                                  const float* const* weights, const float* const* biases, const float* depth_coords,
                                  const float* cameras, const float* initial_depths, const float* encoding_weights,
                                  int reg_flags, const float* dL_ddepths, const float* dL_dreg, float* const* dL_dlevels,
                                  float* dL_ddepth_encoding, float* const* dL_dweights, float* const* dL_dbiases,
                                  char* workspace, size_t workspace_bytes, void* stream);

/*
 * Chart points: a packed list of 3D points per chart, projected into their chart and tapped in any [n,H,W] map -- the SfM fit
 * that makes the aligner's initial depths (matcha/pointmap/depthanythingv2.py:82-117 get_points_depth_in_depthmap, 156-253
 * fit_depth_to_point_cloud, looped by get_pointmap_from_sfm_data_with_depthanything, 634-697) and the point form of the
 * aligner's depth term (ParallelAligner.loss, matcha/dm_scene/parallel_aligner.py:423-453).
 *
 * n charts of one size H x W.  Every operation below is one float32 operation, in this order, with no fused multiply-add
 * (the unit is compiled with -ffp-contract=off), left to right as written, except where float64 is named; divisions are IEEE.
 *   points    device float [N,3], packed: chart c owns points offsets[c] .. offsets[c+1] - 1 (offsets: device int32 [n+1],
 *             offsets[0] = 0, ascending, offsets[n] = N).  An empty chart is legal.  N <= 2^29 - 1, n H W <= 2^31 - 2, n <= 65535.
 *   cameras   device float [n][32]: world_view_transform V[4][4], then full_proj_transform F[4][4], row-major, in the
 *             reference's row-vector convention.  (The matcher's [n,44] record carries projection_matrix, not the product the
 *             reference projects with here; chart_points.camera_records makes this record from the same cameras.)
 * Projection of point p of chart c:
 *   z_p = ((p_0 V[0][2] + p_1 V[1][2]) + p_2 V[2][2]) + V[3][2]
 *   q_k = ((p_0 F[0][k] + p_1 F[1][k]) + p_2 F[2][k]) + F[3][k]  (k = 0, 1, 3),   gx = q_0 / q_3,  gy = q_1 / q_3
 *   (the reference reaches gx, gy through pytorch3d's NDC times -min(H,W)/W: the two signs and aspect factors cancel, as its
 *   own CamerasWrapper.project_points(use_p3d_convention=True) shows)
 *   ix = ((gx + 1) W - 1) / 2,  iy = ((gy + 1) H - 1) / 2  (grid_sample, align_corners=False)
 *   clipped = not (q_3 > 0) or gx or gy not finite: then (ix, iy) = (-2, -2), whose taps all lie outside.  pytorch3d divides
 *   regardless; a difference, on purpose.
 * Tap of a map m of chart c at (ix, iy) (bilinear, zeros padding):  x0 = floor(ix), y0 = floor(iy), x1 = x0 + 1, y1 = y0 + 1,
 *   nw = (x1 - ix)(y1 - iy),  ne = (ix - x0)(y1 - iy),  sw = (x1 - ix)(iy - y0),  se = (ix - x0)(iy - y0)
 *   value = ((nw m(x0,y0) + ne m(x1,y0)) + sw m(x0,y1)) + se m(x1,y1), the term of a tap outside the map being +0;
 *   fov = value > 0.
 * Fit per chart (g4s_chart_points_fit), over all its points (a point outside the image contributes d = 0, the reference's
 *   quirk) or, with use_fov_mask, over the points with d > 0:  t = 1 / z_p, d = the value sampled from the disparity map.
 *   n, St, Sd, Std, Sdd and alpha, beta are those of "Depth cues" A (include/g4s_render_maps.h): float64 sums in a fixed order
 *   -- a workgroup owns G4S_CHART_POINTS_SPAN consecutive points of ONE chart, counted from the chart's first point, thread t
 *   adds points t, t + 256, ... of the span in ascending order, a fixed tree folds the threads, the partials are added by
 *   index --, no float atomics, coeffs [n,2] = {alpha, beta} and counts [n] (int32) on the device, no host read-back.  A
 *   degenerate chart (no point, one point, no variance) gives what IEEE gives: NaN or inf.  That is no error.
 * Apply:  depth = scale (1 / (alpha + beta d)) per pixel of chart c with coeffs[c].
 * View depths:  z of scale P:  (((scale p_0) V[0][2] + (scale p_1) V[1][2]) + (scale p_2) V[2][2]) + V[3][2], for the packed
 *   list (chart [N]) or for n runs of per_chart points (point maps [n,H,W,3], chart = NULL).
 * Point-reference term (g4s_chart_points_loss_*):  s_p, k_p = the values of depths, confidence at point p (k_p = 1 without a
 *   confidence),  e_p = |s_p - z_p|,  term_p = e_p, or k_p e_p - cw log k_p (float32, the device's logf).
 *   L = (sum of term_p) / N in float64, rounded once: spans of G4S_CHART_POINTS_SPAN consecutive points of the PACKED LIST,
 *   threads and tree as above, one workgroup adds the span sums by index.  N = 0 is refused.
 *   Gradient, with c = cotangent / float(N):  dL/ds_p = (c k_p) sign(s_p - z_p)  (c sign(.) without a confidence; sign(0) = 0),
 *   dL/dk_p = c (e_p - cw / k_p).  Pixel v receives, from each tap (p, corner) that lands on it, dL/ds_p w_corner
 *   (dL/dk_p w_corner); its gradient is their float32 sum in ascending (p, corner) order, the list cut into chunks of
 *   G4S_CHART_POINTS_CHUNK taps from its start: each chunk summed from 0, the chunk sums added from 0 in chunk order.  Every
 *   pixel is written.  No float atomics, no fixed-point range limit: two runs give the same bits.  No fov masking, no masks.
 * Inverted index (g4s_chart_points_index), built once per point set:  taps int32 [4 N]: the ids 4 p + corner of the taps inside
 *   a map, ordered by (chart pixel, p, corner); starts uint32 [n H W + 1]: pixel v owns taps[starts[v] .. starts[v+1] - 1].
 * g4s_chart_points_sample_backward spreads any dL/dvalue [N] to the map the same way.
 * Nothing allocates, synchronises or reads back: every call can be captured in a HIP graph.  The size queries are pure host
 * code and return 0 for a refused shape; g4s_chart_points_workspace serves fit and both loss calls.
 */
#define G4S_CHART_POINTS_SPAN 4096 /* points per workgroup of the float64 sums */
#define G4S_CHART_POINTS_CHUNK 64  /* taps per separately summed chunk of a pixel's list */
size_t g4s_chart_points_workspace(int n, int height, int width, int n_points);
size_t g4s_chart_points_index_workspace(int n, int height, int width, int n_points);
int g4s_chart_points_project(int n, int height, int width, const float* cameras, int n_points, const float* points,
                             const int* offsets, int* chart, float* z, float* ixy, unsigned char* clipped, void* stream);
int g4s_chart_points_sample(int n, int height, int width, int n_points, const int* chart, const float* ixy, const float* map,
                            float* values, unsigned char* fov, void* stream);
int g4s_chart_points_fit(int n, int n_points, const int* offsets, int max_count, const float* z, const float* values,
                         int use_fov_mask, float* coeffs, int* counts, char* workspace, size_t workspace_bytes, void* stream);
int g4s_chart_points_apply(int n, int height, int width, const float* disparities, const float* coeffs, float scale,
                           float* depths, void* stream);
int g4s_chart_points_view_depths(int n, const float* cameras, long long count, long long per_chart, const int* chart,
                                 const float* points, float scale, float* depths, void* stream);
int g4s_chart_points_index(int n, int height, int width, int n_points, const int* chart, const float* ixy, int* taps,
                           unsigned int* starts, char* workspace, size_t workspace_bytes, void* stream);
int g4s_chart_points_loss_forward(int n, int height, int width, int n_points, const int* chart, const float* ixy,
                                  const float* z, const float* depths, const float* confidence, float confidence_weighting,
                                  float* out1, char* workspace, size_t workspace_bytes, void* stream);
int g4s_chart_points_loss_backward(int n, int height, int width, int n_points, const int* chart, const float* ixy,
                                   const float* z, const float* depths, const float* confidence, float confidence_weighting,
                                   const int* taps, const unsigned int* starts, const float* grad_out1, float* dL_ddepths,
                                   float* dL_dconfidence, char* workspace, size_t workspace_bytes, void* stream);
int g4s_chart_points_sample_backward(int n, int height, int width, int n_points, const float* ixy, const int* taps,
                                     const unsigned int* starts, const float* grad_values, float* dL_dmap, void* stream);

#ifdef __cplusplus
}
#endif
#endif
