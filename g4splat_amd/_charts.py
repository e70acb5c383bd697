"""What the chart modules (chart_match, chart_align, chart_deform, chart_points, chart_aligner) share on the Python side: the
camera list and its spatial extent, the [n,H,W] stack of one size with its shape check, and the two ends of an autograd
function in depths and an optional confidence.  Private: the public names stay where they were (chart_match.spatial_extent).
"""
import numpy as np
import torch

from ._device import check_dtype, drop_leading_one, same_device, to_np


def camera_list(cameras):
    cams = list(getattr(cameras, "gs_cameras", cameras))
    if len(cams) == 0:
        raise ValueError("chart matcher: no views (n = 0)")
    return cams


def spatial_extent(cameras):
    """CamerasWrapper.get_spatial_extent: 1.1 x the largest distance of a camera centre from the mean centre (a float,
    computed in double on the host from world_view_transform)."""
    cams = camera_list(cameras)
    c = np.stack([np.linalg.inv(np.asarray(to_np(cam.world_view_transform), np.float64).reshape(4, 4).T)[:3, 3] for cam in cams])
    return 1.1 * float(np.linalg.norm(c - c.mean(axis=0, keepdims=True), axis=1).max())


def stack(depths, name, dev=None):
    """[n,H,W] on one HIP device (any float dtype, attached to its graph) from a stacked tensor or a list of maps of ONE size."""
    if isinstance(depths, torch.Tensor):
        if depths.dim() == 4 and depths.size(1) == 1:
            depths = depths[:, 0]
        if depths.dim() != 3:
            raise ValueError(f"{name}: a stacked tensor must be [n,H,W] (got {tuple(depths.shape)})")
        maps = None
    else:
        maps = [drop_leading_one(d) for d in depths]
        if len(maps) == 0:
            raise ValueError("chart matcher: no views (n = 0)")
        for v, d in enumerate(maps):
            dev = same_device(d, dev, f"{name}[{v}]")
            if d.dim() != 2:
                raise ValueError(f"{name}[{v}] must be [H,W] or [1,H,W] (got {tuple(d.shape)})")
            if d.shape != maps[0].shape:
                raise ValueError(f"{name}: the views must all have one size (view 0 is {tuple(maps[0].shape)}, view {v} is "
                                 f"{tuple(d.shape)})")
        depths = torch.stack(maps)
    dev = same_device(depths, dev, name)
    check_dtype(depths, (torch.float32, torch.float64, torch.float16, torch.bfloat16), name)
    if depths.size(0) == 0:
        raise ValueError("chart matcher: no views (n = 0)")
    return dev, depths


def f32(t):
    """What a library call reads: detached, float32, contiguous."""
    return t.detach().float().contiguous()


def maps_of_shape(t, name, shape, dev, whose="the shape"):
    """stack(t) on `dev`, refused unless it is [n,H,W] = `shape` (`whose`: how the message calls that shape)."""
    _dev, m = stack(t, name, dev)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"{name} must have {whose} {tuple(shape)} (got {tuple(m.shape)})")
    return m


# ---- the two ends of an autograd function in `depths` and an optional `confidence` (chart_align._Terms, chart_points._PointLoss)
def depths_and_confidence(depths, confidence):
    """(d, c, meta): what the library reads (c None without a confidence) and what grads_like() needs."""
    c = None if confidence is None else f32(confidence)
    meta = (depths.shape, depths.dtype, None if confidence is None else (confidence.shape, confidence.dtype))
    return f32(depths), c, meta


def grads_like(dd, dc, meta):
    """The two gradients in the inputs' shapes and dtypes."""
    dshape, ddtype, cmeta = meta
    dd = dd.reshape(dshape).to(ddtype)
    if dc is not None:
        dc = dc.reshape(cmeta[0]).to(cmeta[1])
    return dd, dc
