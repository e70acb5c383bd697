"""Fused photometric loss of the training step (include/g4s_losses.h):

    loss, Ll1, ssim = photometric_loss(image, gt_image, lambda_dssim)
    # == (1 - l) * l1_loss(image, gt) + l * (1 - ssim(image, gt)),  l1_loss(...), ssim(...)
    #    2dgs/utils/loss_utils.py:17-18, 46-79;  train_with_refine_depth.py:382-383

One call computes the three scalars AND d loss / d image (two tiled HIP kernels + a fixed-order reduction);
the autograd backward only scales the stored gradient.  `Ll1` and `ssim` are returned for logging (detached,
as the reference uses them).  No CPU path.

The chart-prior half of the same loss (train_with_refine_depth.py:403-492) is further down: `chart_prior_losses`
(log-depth, two normal priors, curvature, MAtCha's depth-order loss), `anisotropy_loss`, `draw_pixel_shifts` and
`chart_regularization`, which applies the reference's schedule and weights to them in one call."""
import torch

from . import _lib


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lambda_dssim):
        if not image.is_cuda or not gt.is_cuda:
            raise RuntimeError("image and gt must be CUDA tensors")
        if image.ndim != 3 or image.size(0) != 3 or image.shape != gt.shape:
            raise RuntimeError("image and gt must both have dimensions (3, H, W)")
        lib = _lib.load()
        dev = image.device
        H, W = int(image.size(1)), int(image.size(2))
        x, y = image.detach().float().contiguous(), gt.detach().float().contiguous()
        need_grad = ctx.needs_input_grad[0]
        with torch.cuda.device(dev):
            out3 = torch.empty(3, dtype=torch.float32, device=dev)
            grad = torch.empty_like(x) if need_grad else None
            nws = lib.g4s_photometric_workspace(W, H)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            _lib.call("g4s_photometric_loss", W, H, _lib.ptr(x), _lib.ptr(y), float(lambda_dssim), _lib.ptr(out3),
                      _lib.ptr(grad), _lib.ptr(ws), nws, _lib.stream(dev))
        ctx.grad = grad
        ctx.mark_non_differentiable(out3)
        return out3[0].clone(), out3

    @staticmethod
    def backward(ctx, g_loss, _g_out3):
        return (ctx.grad * g_loss if ctx.grad is not None else None), None, None


def photometric_loss(image, gt, lambda_dssim=0.2):
    """-> (loss, Ll1, ssim): `loss` carries the gradient to `image`; `Ll1`, `ssim` are detached scalars."""
    loss, out3 = _Photometric.apply(image, gt, float(lambda_dssim))
    return loss, out3[1], out3[2]


class _GeometryRegularizers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rend_normal, surf_normal, rend_dist):
        for t in (rend_normal, surf_normal, rend_dist):
            if not t.is_cuda:
                raise RuntimeError("geometry_regularizers: CUDA tensors only")
        if (rend_normal.ndim != 3 or rend_normal.size(0) != 3 or rend_normal.shape != surf_normal.shape
                or rend_dist.numel() != rend_normal.size(1) * rend_normal.size(2)):
            raise RuntimeError("expected rend_normal, surf_normal (3, H, W) and rend_dist (1, H, W)")
        lib = _lib.load()
        dev = rend_normal.device
        H, W = int(rend_normal.size(1)), int(rend_normal.size(2))
        rn, sn = rend_normal.detach().float().contiguous(), surf_normal.detach().float().contiguous()
        rd = rend_dist.detach().float().contiguous()
        with torch.cuda.device(dev):
            out2 = torch.empty(2, dtype=torch.float32, device=dev)
            nws = lib.g4s_geometry_regularizers_workspace(W, H)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            _lib.call("g4s_geometry_regularizers_forward", W, H, _lib.ptr(rn), _lib.ptr(sn), _lib.ptr(rd), _lib.ptr(out2),
                      _lib.ptr(ws), nws, _lib.stream(dev))
        ctx.save_for_backward(rn, sn)
        ctx.dist_shape = rend_dist.shape
        return out2

    @staticmethod
    def backward(ctx, g_out2):
        rn, sn = ctx.saved_tensors
        dev = rn.device
        H, W = int(rn.size(1)), int(rn.size(2))
        g2 = g_out2.detach().float().contiguous()
        with torch.cuda.device(dev):
            d_rn, d_sn = torch.empty_like(rn), torch.empty_like(sn)
            d_rd = torch.empty(ctx.dist_shape, dtype=torch.float32, device=dev)
            _lib.call("g4s_geometry_regularizers_backward", W, H, _lib.ptr(rn), _lib.ptr(sn), _lib.ptr(g2), _lib.ptr(d_rn),
                      _lib.ptr(d_sn), _lib.ptr(d_rd), _lib.stream(dev))
        return d_rn, d_sn, d_rd


def geometry_regularizers(rend_normal, surf_normal, rend_dist):
    """-> (normal_error.mean(), rend_dist.mean()) of train_with_refine_depth.py:391-396, i.e.
    (1 - (rend_normal * surf_normal).sum(dim=0)).mean() and rend_dist.mean(), as one fused HIP pass each way
    (include/g4s_losses.h).  The caller multiplies by lambda_normal / lambda_dist.  No CPU path."""
    out2 = _GeometryRegularizers.apply(rend_normal, surf_normal, rend_dist)
    return out2[0], out2[1]


# ---- chart-prior half of the loss (train_with_refine_depth.py:403-492; include/g4s_losses.h) ---------------------
class _ChartPrior(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv, pixel_shifts,
                depth_scale, scene_extent, log_scale):
        maps = (rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv)
        for t in maps + ((pixel_shifts,) if pixel_shifts is not None else ()):
            if not t.is_cuda or t.device != rend_normal.device:
                raise RuntimeError("chart_prior_losses: CUDA tensors on one device only")
        if rend_normal.ndim != 3 or rend_normal.size(0) != 3:
            raise RuntimeError("chart_prior_losses: rend_normal must have dimensions (3, H, W)")
        H, W = int(rend_normal.size(1)), int(rend_normal.size(2))
        if surf_normal.shape != rend_normal.shape or prior_normal.shape != rend_normal.shape:
            raise RuntimeError("chart_prior_losses: surf_normal and prior_normal must have rend_normal's dimensions (3, H, W)")
        for t in (surf_depth, prior_depth, prior_curv):
            if tuple(t.shape) not in ((1, H, W), (H, W)):
                raise RuntimeError("chart_prior_losses: surf_depth, prior_depth and prior_curv must have dimensions (1, H, W)")
        if pixel_shifts is not None and (pixel_shifts.dtype != torch.int64 or tuple(pixel_shifts.shape) != (H * W, 2)):
            raise RuntimeError("chart_prior_losses: pixel_shifts must be an int64 tensor with dimensions (H*W, 2)")
        lib = _lib.load()
        dev = rend_normal.device
        saved = [t.detach().float().contiguous() for t in maps]
        shifts = pixel_shifts.contiguous() if pixel_shifts is not None else None
        scalars = (float(depth_scale), float(scene_extent), float(log_scale))
        with torch.cuda.device(dev):
            out5 = torch.empty(5, dtype=torch.float32, device=dev)
            nws = lib.g4s_chart_prior_workspace(W, H)
            if nws == 0:
                raise RuntimeError(f"chart_prior_losses: a {H}x{W} map is empty or has more than 2^22 pixels")
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            _lib.call("g4s_chart_prior_forward", W, H, *[_lib.ptr(t) for t in saved], *scalars, _lib.ptr(shifts),
                      _lib.ptr(out5), _lib.ptr(ws), nws, _lib.stream(dev))
        ctx.save_for_backward(*saved)
        ctx.shifts, ctx.scalars, ctx.depth_shape = shifts, scalars, surf_depth.shape
        return out5

    @staticmethod
    def backward(ctx, g_out5):
        saved = ctx.saved_tensors
        rn = saved[0]
        dev = rn.device
        H, W = int(rn.size(1)), int(rn.size(2))
        g5 = g_out5.detach().float().contiguous()
        with torch.cuda.device(dev):
            d_rn, d_sn = torch.empty_like(rn), torch.empty_like(rn)
            d_sd = torch.empty(ctx.depth_shape, dtype=torch.float32, device=dev)
            nws = _lib.load().g4s_chart_prior_workspace(W, H)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            _lib.call("g4s_chart_prior_backward", W, H, *[_lib.ptr(t) for t in saved], *ctx.scalars, _lib.ptr(ctx.shifts),
                      _lib.ptr(g5), _lib.ptr(d_rn), _lib.ptr(d_sn), _lib.ptr(d_sd), _lib.ptr(ws), nws, _lib.stream(dev))
        return d_rn, d_sn, d_sd, None, None, None, None, None, None, None


def chart_prior_losses(rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv, depth_scale,
                       pixel_shifts=None, scene_extent=1.0, log_scale=20.0):
    """-> float[5], the UNWEIGHTED means of the chart-prior terms of train_with_refine_depth.py:415-475 (exact
    definitions: include/g4s_losses.h):
        [0] log(1 + depth_scale |prior_depth - surf_depth|)     [1] 1 - <surf_normal, prior_normal>
        [2] 1 - <rend_normal, prior_normal>                     [3] |prior_curv - normal2curv(rend_normal)|
        [4] MAtCha's depth-order loss over the pairs (p, clamp(p + pixel_shifts[p])), log space; 0 without shifts
    `pixel_shifts` is what draw_pixel_shifts returns.  Gradients reach rend_normal, surf_normal and surf_depth, bit for
    bit the same from run to run.  No CPU path."""
    return _ChartPrior.apply(rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv, pixel_shifts,
                             float(depth_scale), float(scene_extent), float(log_scale))


def draw_pixel_shifts(height, width, max_pixel_shift_ratio=0.05, device="cuda"):
    """The random partner offsets of the depth-order loss, int64 (H*W, 2) = (row shift, column shift): one
    torch.randint call with the reference's bounds and shape (matcha/dm_regularization/depth.py:177-178), so on the same
    device and seed it consumes the generator exactly as the reference does."""
    m = round(max_pixel_shift_ratio * max(height, width))  # Python's round: half to even
    return torch.randint(-m, m + 1, (height * width, 2), device=device)


class _Anisotropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, max_ratio):
        if not scaling.is_cuda:
            raise RuntimeError("anisotropy_loss: CUDA tensors only")
        if scaling.ndim != 2 or scaling.size(1) != 2 or scaling.size(0) == 0:
            raise RuntimeError("anisotropy_loss: scaling must have dimensions (P, 2) with P > 0")
        lib = _lib.load()
        dev = scaling.device
        s = scaling.detach().float().contiguous()
        P = int(s.size(0))
        with torch.cuda.device(dev):
            out1 = torch.empty(1, dtype=torch.float32, device=dev)
            nws = lib.g4s_anisotropy_workspace(P)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            _lib.call("g4s_anisotropy_forward", P, _lib.ptr(s), float(max_ratio), _lib.ptr(out1), _lib.ptr(ws), nws,
                      _lib.stream(dev))
        ctx.save_for_backward(s)
        ctx.max_ratio = float(max_ratio)
        return out1

    @staticmethod
    def backward(ctx, g_out1):
        (s,) = ctx.saved_tensors
        dev = s.device
        g1 = g_out1.detach().float().contiguous()
        with torch.cuda.device(dev):
            d_s = torch.empty_like(s)
            _lib.call("g4s_anisotropy_backward", int(s.size(0)), _lib.ptr(s), ctx.max_ratio, _lib.ptr(g1), _lib.ptr(d_s),
                      _lib.stream(dev))
        return d_s, None


def anisotropy_loss(scaling, max_ratio=5.0):
    """-> mean(clamp_min(s_max / s_min, max_ratio) - max_ratio) over the (P, 2) activated scales
    (train_with_refine_depth.py:484-489), unweighted; one fused HIP pass each way.  No CPU path."""
    return _Anisotropy.apply(scaling, float(max_ratio))[0]


def schedule_regularization_factor_2(iteration, initial_factor=0.5):
    """The reference's chart-regularisation schedule (matcha/dm_scene/charts.py:109-113): halved every thousand
    iterations, never below 0.015."""
    return max(initial_factor / 2 ** (iteration // 1000), 0.015)


def depth_order_weight(iteration):
    """lambda_depth_order of train_with_refine_depth.py:451-459."""
    weight = 0.0
    for start, value in ((1500, 1.0), (3000, 0.1), (4500, 0.01), (6000, 0.001)):
        if iteration > start:
            weight = value
    return weight


def chart_regularization(render_pkg, priors, gaussians_scaling, iteration, charts_scale_factor, scene_extent,
                         use_depth_order_regularization=True, initial_regularization_factor=0.5,
                         confidence_weighting=0.5, max_pixel_shift_ratio=0.05, log_scale=20.0, lambda_anisotropy=0.1,
                         anisotropy_max_ratio=5.0):
    """Lines 403-492 of train_with_refine_depth.py as one call -> (total_regularization_loss, terms).

    `render_pkg` is what render() returned (rend_normal, surf_normal, surf_depth are read); `priors` maps "depth",
    "normal" and "curv" to the view's chart maps; `gaussians_scaling` is gaussians.get_scaling; `scene_extent` is
    gaussians.spatial_lr_scale.  The weights are the reference's: schedule_regularization_factor_2 times 0.75 (depth,
    with the 0.5 confidence weighting), 0.5 (surf normal), 0.5 (rend normal), 0.25 (curvature), depth_order_weight and
    lambda_anisotropy.  `terms` holds the reference's named terms: depth_prior_loss (depth-order and surf-normal terms
    included, as there), normal_prior_loss, curv_prior_loss, anisotropy_loss.  While the depth-order weight is 0 no
    shifts are drawn -- the reference draws none either, so the generator stays in step with it."""
    factor = schedule_regularization_factor_2(iteration, initial_regularization_factor)
    surf_depth = render_pkg["surf_depth"]
    lambda_order = depth_order_weight(iteration) if use_depth_order_regularization else 0.0
    shifts = None
    if lambda_order > 0:
        shifts = draw_pixel_shifts(int(surf_depth.size(-2)), int(surf_depth.size(-1)), max_pixel_shift_ratio,
                                   device=surf_depth.device)
    m = chart_prior_losses(render_pkg["rend_normal"], render_pkg["surf_normal"], surf_depth, priors["depth"],
                           priors["normal"], priors["curv"], charts_scale_factor, shifts, scene_extent, log_scale)
    depth_prior_loss = (factor * 0.75 * confidence_weighting) * m[0] + (factor * 0.5) * m[1]
    if lambda_order > 0:
        depth_prior_loss = depth_prior_loss + lambda_order * m[4]
    terms = {"depth_prior_loss": depth_prior_loss, "normal_prior_loss": (factor * 0.5) * m[2],
             "curv_prior_loss": (factor * 0.25) * m[3]}
    total = terms["depth_prior_loss"] + terms["normal_prior_loss"] + terms["curv_prior_loss"]
    if lambda_anisotropy > 0.0:
        terms["anisotropy_loss"] = lambda_anisotropy * anisotropy_loss(gaussians_scaling, anisotropy_max_ratio)
        total = total + terms["anisotropy_loss"]
    return total, terms
