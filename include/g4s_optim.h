/*
 * g4s_optim.h -- C ABI of the fused Adam step over the Gaussian parameter groups,
 * libg4s_hip.so.
 *
 * Replaces torch.optim.Adam.step() as the reference configures it
 * (2d-gaussian-splatting/scene/gaussian_model.py:248-266: six parameter groups xyz / f_dc / f_rest / opacity /
 * scaling / rotation with their own learning rates, betas (0.9, 0.999), eps = 1e-15, no weight decay, no amsgrad)
 * -- ~10 full passes over 4 x 232 B per Gaussian in the foreach implementation -- by ONE kernel that reads
 * param / grad / exp_avg / exp_avg_sq once and writes param / exp_avg / exp_avg_sq once.  Same update rule:
 *
 *   m <- m + (1 - beta1) (g - m)              v <- beta2 v + (1 - beta2) g g
 *   p <- p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 */
#ifndef G4S_OPTIM_H_INCLUDED
#define G4S_OPTIM_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * nseg (1..8) segments; HOST arrays of device pointers params/grads/exp_avg/exp_avg_sq, element counts
 * numel, learning rates lr and step counts step (t >= 1, AFTER the increment, per segment like torch's
 * per-parameter state["step"]).  Tensors are float32, updated in place; the hyper-parameters are doubles like
 * the Python floats torch works from (1 - beta2 must be formed in double: in float32 it is off by 1.3e-5).
 */
int g4s_adam_step(int nseg, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const long long* numel, const double* lr, const int* step, double beta1,
                  double beta2, double eps, void* stream);

/*
 * The same update with the step counts and learning rates read from DEVICE memory, for launches captured in a hipGraph
 * (a replay must advance t and may see a new learning rate): lr_dev [nseg] float64 on the device (doubles, like `lr` above); step_dev = HOST array of
 * nseg device pointers to float32 scalars holding t BEFORE the call (torch's capturable state["step"]); each is
 * incremented by one on the device, then used.  coef_dev: 16 floats of device scratch owned by the caller for the
 * lifetime of the launch (the bias-correction factors, computed in double on the device like g4s_adam_step does on the
 * host).  Two launches.
 */
int g4s_adam_step_device(int nseg, float* const* params, const float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, const long long* numel, const double* lr_dev, float* const* step_dev,
                         float* coef_dev, double beta1, double beta2, double eps, void* stream);

/*
 * Densification statistics of one rendered view, fused.  Replaces GaussianModel.add_densification_stats
 * (2d-gaussian-splatting/scene/gaussian_model.py:649-651) and the max_radii2D update of the training loop
 * (train_with_refine_depth.py, "max_radii2D[visibility_filter] = max(max_radii2D[visibility_filter], radii[...])"):
 * for every i with update_filter[i] != 0
 *     xyz_gradient_accum[i] += || grad_mean2D[i, 0:3] ||_2      denom[i] += 1
 *     max_radii2D[i] = max(max_radii2D[i], radii[i])            (skipped when max_radii2D is NULL)
 * grad_mean2D [P,3] is the rasterizer's dL_dmean2D (the gradient of `viewspace_points`), update_filter one byte
 * per Gaussian (a torch bool tensor), radii int32 [P]; the three statistics are float32 [P], updated in place.
 */
int g4s_densify_stats(int P, const float* grad_mean2D, const unsigned char* update_filter, const int* radii,
                      float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream);

/*
 * Parameter activations as render() reads them (2d-gaussian-splatting/scene/gaussian_model.py:157-192, mip filter
 * off; with the filter on: g4s_activations_mip_* below): scales = exp(_scaling) [P,2], rotations = normalize(_rotation) [P,4] (x / max(|x|, 1e-12), as
 * torch.nn.functional.normalize), opacities = sigmoid(_opacity) [P].  One launch each way instead of ~5 / ~9.
 * The backward takes the activated scales / opacities the forward produced and the raw rotations.
 * Scale tensors 8-byte, rotation tensors 16-byte aligned.
 */
int g4s_activations_forward(int P, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                            float* scales, float* rotations, float* opacities, void* stream);
int g4s_activations_backward(int P, const float* scales, const float* rotation_raw, const float* opacities,
                             const float* dL_dscales, const float* dL_drotations, const float* dL_dopacities,
                             float* dL_dscaling_raw, float* dL_drotation_raw, float* dL_dopacity_raw, void* stream);

/*
 * The same activations with the mip filter ON (use_mip_filter, what G4Splat trains with), in the reference's order
 * of operations; mip_filter is the float32 [P] buffer compute_mip_filter fills (its [P,1] tensor, contiguous), f below:
 *
 *   e_k = exp(s_k)   a_k = e_k e_k + f f   scales_k = sqrt(a_k)            (k = x, y)
 *   coef = sqrt((e_x^2 e_y^2) / (a_x a_y))                                  opacity = sigmoid(o) coef
 *
 * and rotations exactly as above.  One launch each way, instead of ~18 element-wise launches forward and ~30 in
 * autograd's backward.  The backward RECOMPUTES from the raw parameters (4 floats per Gaussian re-read, against 3
 * activated floats saved and read); the filter is a no_grad buffer and receives no gradient.  With sg = sigmoid(o):
 *
 *   d o   = g_op coef sg (1 - sg)
 *   d s_k = g_sc,k e_k^2 / scales_k + g_op sg coef f^2 / a_k              (d ln coef / d s_k = f^2 / a_k: no 1 - x)
 *
 * Rotation backward as g4s_activations_backward, clamped branch included.  Same alignment rules.
 */
int g4s_activations_mip_forward(int P, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                                const float* mip_filter, float* scales, float* rotations, float* opacities, void* stream);
int g4s_activations_mip_backward(int P, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                                 const float* mip_filter, const float* dL_dscales, const float* dL_drotations,
                                 const float* dL_dopacities, float* dL_dscaling_raw, float* dL_drotation_raw,
                                 float* dL_dopacity_raw, void* stream);

/*
 * The mip filter sizes, GaussianModel.compute_mip_filter (2d-gaussian-splatting/scene/gaussian_model.py:388-434):
 * per Gaussian the depth of the closest view that sees it, times `scale`.  The reference loops over the cameras in
 * Python (~20 launches and several [P] / [P,3] temporaries per view); here the views are a device table and the
 * whole thing is two launches (and a 4-byte memset), without a host synchronisation or a per-view temporary.
 *
 *   cameras  [V,16] float32 on the device, per view: R row-major (9), T (3), focal_x, focal_y, image_width, image_height
 *            (R and T as the reference's cameras hold them: camera space = xyz @ R + T)
 *   scale    sqrt(filter_variance) / max focal_x, formed on the host in double and rounded once
 *   workspace  g4s_mip_filter_workspace() bytes of device scratch
 *
 * Per point (x, y, z) and view, in float32, every operation rounded on its own (no FMA; the library is built with
 * -ffp-contract=off and correctly rounded division), in exactly this order:
 *
 *   x_c = ((x R00 + y R10) + z R20) + T0     y_c = ((x R01 + y R11) + z R21) + T1     z_c = ((x R02 + y R12) + z R22) + T2
 *   z' = max(z_c, 0.001)       u = (x_c / z') focal_x + 0.5 W       v = (y_c / z') focal_y + 0.5 H
 *   seen by the view  <=>  z_c > znear  and  -0.15f W <= u <= 1.15f W  and  -0.15f H <= v <= 1.15f H
 *
 * (-0.15f, 1.15f: the float32 constants, multiplied in float32).  d = min(100000, z' of the views that see the point);
 * points seen by no view take the largest d of the seen ones; mip_filter_out[i] = d scale.  The largest d is folded by
 * an integer maximum on the floats' bits (they are positive), so the result does not depend on any order and two runs
 * give the same bits.  Against the reference: its xyz @ R is a GEMM whose summation order is the BLAS's, and it divides
 * by the focal length and multiplies by sqrt(filter_variance) in two steps -- a few ulp.  ONE documented difference:
 * when no view sees any point the reference raises (max() of an empty tensor); here every row gets 100000 scale, which
 * needs no synchronisation to find out.  V >= 1.
 */
size_t g4s_mip_filter_workspace(void);
int g4s_mip_filter(int P, const float* xyz, int V, const float* cameras, float znear, float scale, float* mip_filter_out,
                   char* workspace, void* stream);

/*
 * Stream compaction of Gaussian rows: the device side of prune_points / densify_and_clone / densify_and_split
 * (2d-gaussian-splatting/scene/gaussian_model.py:510-541, 583-626), which the reference expresses as one boolean-mask
 * indexing per tensor (six parameters, twelve Adam moments, three statistics).
 *
 *   g4s_compact_scan    scans `keep` (one byte per row, a torch bool tensor) ONCE: wave ballot + popcount per 256 rows,
 *                       a single-block scan of the block counts; the number of kept rows goes to *out_count (device int).
 *                       `workspace` (>= g4s_compact_workspace(P) bytes) holds the scan for the gathers that follow.
 *   g4s_compact_gather  copies the kept rows of `nseg` row-major float tensors src[s] = [P, widths[s]] to
 *                       dst[s] + dst_row0 * widths[s], in index order (stable, like mask indexing), eight tensors per
 *                       launch.  src / dst / widths are HOST arrays.  dst[s] must hold dst_row0 + count rows.
 */
size_t g4s_compact_workspace(int P);
int g4s_compact_scan(int P, const unsigned char* keep, int* out_count, char* workspace, size_t workspace_bytes, void* stream);
int g4s_compact_gather(int P, const unsigned char* keep, const char* workspace, int nseg, const float* const* src,
                       float* const* dst, const int* widths, long long dst_row0, void* stream);

#ifdef __cplusplus
}
#endif
#endif
