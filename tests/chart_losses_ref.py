"""Eager torch restatement of the chart-prior losses, written from the formulas in include/g4s_losses.h
(g4s_chart_prior_*, g4s_anisotropy_*).  It runs on whatever device its inputs live on and is differentiated by
autograd: the GPU tests compare the fused HIP op with it on the same GPU and time the two against each other, and
the golden generator checks it bit for bit against the reference's own depth-order loss on the CPU."""
import torch


def curvature(normal):
    """curv_p = sum_c |lap_p,c| of a (3, H, W) map; neighbours above, left, below, right; replicate padding."""
    p = torch.nn.functional.pad(normal[None], (1, 1, 1, 1), mode="replicate")[0]
    lap = (((p[:, :-2, 1:-1] - normal) + (p[:, 1:-1, :-2] - normal)) + (p[:, 2:, 1:-1] - normal)) + (p[:, 1:-1, 2:] - normal)
    return lap.abs().sum(dim=0, keepdim=True)


def depth_order(surf_depth, prior_depth, pixel_shifts, scene_extent, log_scale):
    """mean log(1 + log_scale x_p) over the pairs (p, q = clamp(p + shift_p))."""
    H, W = surf_depth.shape[-2:]
    dev = surf_depth.device
    rows = torch.arange(H, device=dev).view(H, 1).expand(H, W).reshape(-1)
    cols = torch.arange(W, device=dev).view(1, W).expand(H, W).reshape(-1)
    qy = (rows + pixel_shifts[:, 0]).clamp(0, H - 1)
    qx = (cols + pixel_shifts[:, 1]).clamp(0, W - 1)
    d, pr = surf_depth.reshape(H, W), prior_depth.reshape(H, W)
    diff = (d.reshape(-1) - d[qy, qx]) / scene_extent
    pd = (pr.reshape(-1) - pr[qy, qx]) / scene_extent
    pd = pd / pd.detach().abs().clamp(min=1e-8)
    x = -(diff * pd).clamp(max=0)
    return torch.log(1.0 + log_scale * x).mean()


def chart_prior_losses(rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv, depth_scale,
                       pixel_shifts=None, scene_extent=1.0, log_scale=20.0):
    """The five unweighted means, in the order of out5."""
    m0 = torch.log(1.0 + depth_scale * (prior_depth - surf_depth).abs()).mean()
    m1 = (1.0 - (surf_normal * prior_normal).sum(dim=0)).mean()
    m2 = (1.0 - (rend_normal * prior_normal).sum(dim=0)).mean()
    m3 = (prior_curv - curvature(rend_normal)).abs().mean()
    if pixel_shifts is None:
        m4 = torch.zeros_like(m0)
    else:
        m4 = depth_order(surf_depth, prior_depth, pixel_shifts, scene_extent, log_scale)
    return torch.stack([m0, m1, m2, m3, m4])


def anisotropy_loss(scaling, max_ratio=5.0):
    ratio = scaling.max(dim=1).values / scaling.min(dim=1).values
    return (ratio.clamp_min(max_ratio) - max_ratio).mean()


def lattice_inputs(H, W, seed, device="cpu"):
    """Inputs on a dyadic lattice (normals and curvature priors multiples of 2^-10 in [-1, 1], the curvature prior
    2^-11 off it, depths multiples of 2^-8 in [1, 4]): with a power-of-two scene extent every quantity that feeds a
    sign or a clamp is exact in float32, so the fused op and autograd take the same branch at every pixel."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda *s: (torch.randint(-1024, 1025, s, generator=g).float() / 1024.0)
    depth = lambda: (torch.randint(256, 1025, (1, H, W), generator=g).float() / 256.0)
    sn, pn = unit(3, H, W), unit(3, H, W)
    # rend_normal: a smooth field plus noise, so that its curvature straddles the priors in [-1, 1] (both signs occur)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    smooth = torch.stack([0.5 * torch.sin(xx / 5.0 + c) * torch.cos(yy / 7.0 - c) for c in range(3)])
    rn = (torch.round((smooth + 0.06 * unit(3, H, W)) * 1024.0) / 1024.0).clamp(-1.0, 1.0)
    pc = unit(1, H, W) + 2.0 ** -11
    sd, pd = depth(), depth()
    return [t.to(device) for t in (rn, sn, sd, pd, pn, pc)]


def chart_regularization(rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv, scaling, factor,
                         lambda_order, depth_scale, scene_extent, max_pixel_shift_ratio=0.05, log_scale=20.0,
                         lambda_anisotropy=0.1, max_ratio=5.0):
    """total_regularization_loss for a given schedule factor and depth-order weight; draws the shifts itself (one
    randint, only while the depth-order weight is positive), as an eager training loop would."""
    shifts = None
    if lambda_order > 0:
        H, W = surf_depth.shape[-2:]
        m = round(max_pixel_shift_ratio * max(H, W))
        shifts = torch.randint(-m, m + 1, (H * W, 2), device=surf_depth.device)
    t = chart_prior_losses(rend_normal, surf_normal, surf_depth, prior_depth, prior_normal, prior_curv, depth_scale, shifts,
                           scene_extent, log_scale)
    total = factor * 0.75 * 0.5 * t[0] + factor * 0.5 * t[1] + lambda_order * t[4] + factor * 0.5 * t[2] + factor * 0.25 * t[3]
    return total + lambda_anisotropy * anisotropy_loss(scaling, max_ratio)
