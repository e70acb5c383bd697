"""The warp initialiser (include/g4s_render_maps.h, "Warp surfels"; csrc/tsdf/warp_init.hip).

The trainer's default first act with --use_downsample_gaussians (2d-gaussian-splatting/train_with_refine_depth.py,
downsample_gaussians_type "warp"; scene/gaussian_model.py get_gaussian_parameters_by_warp_from_depths): one surfel per pixel
that no earlier view already explains under depth-consistent warping.

  warp_keep_masks                               the keep decision of every pixel of every view.
  warp_surfels                                  the surfels (and, on request, the masks).
  get_gaussian_parameters_by_warp_from_depths   scene/gaussian_model.py, by name and argument list.

One launch over (view, pixel) with the loop over the earlier views inside, a scan, and an emit; there is no torch path.
Tensors must be on a HIP device: anything else is a ValueError.  A camera is anything with world_view_transform,
full_proj_transform, FoVx and FoVy.  INTEGRATION.md section T lists the differences from the reference.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._device import ViewStack, check_dtype, check_view_count, drop_leading_one, host_f32, launch, same_device, view_list
from .visibility import ray_record


def _maps(maps, name, lead, n, dev):
    """`maps` -- a list, or one stacked tensor -- as float32 [H,W] (lead 0) or [3,H,W] (lead 3) tensors on one HIP device."""
    if lead and isinstance(maps, torch.Tensor):
        if maps.dim() != 4:
            raise ValueError(f"{name}: a stacked tensor must be [V,3,H,W] (got {tuple(maps.shape)})")
        maps = list(maps.unbind(0))
    maps = view_list(maps, name)
    check_view_count(maps, name, n)
    out = []
    for v, t in enumerate(maps):
        dev = same_device(t, dev, f"{name}[{v}]")
        check_dtype(t, (torch.float32,), f"{name}[{v}]")
        if not lead:
            t = drop_leading_one(t)
        if t.dim() != (3 if lead else 2) or t.numel() == 0 or (lead and t.size(0) != lead):
            raise ValueError(f"{name}[{v}] must be a non-empty {'[3,H,W]' if lead else '[H,W] or [1,H,W]'} map (got {tuple(t.shape)})")
        out.append(t.detach())
    return dev, out


def _stack(depths, cameras, images):
    """(device, ViewStack, ray records) of checked views; device None without views."""
    cameras = list(cameras)
    dev, depths = _maps(depths, "depths", 0, len(cameras), None)
    if images is not None:
        dev, images = _maps(images, "images", 3, len(cameras), dev)
        for v, (d, im) in enumerate(zip(depths, images)):
            if tuple(im.shape[1:]) != tuple(d.shape):
                raise ValueError(f"images[{v}] must be [3,{d.size(0)},{d.size(1)}] like its depth map (got {tuple(im.shape)})")
    if not cameras:
        return None, None, None
    views = ViewStack([(c, d, None if images is None else images[v]) for v, (c, d) in enumerate(zip(cameras, depths))], dev,
                      images is not None, 1, lambda cam: [cam.world_view_transform], focal=True)
    rays = np.concatenate([ray_record(c, views.size(v)[1], views.size(v)[0]) for v, c in enumerate(cameras)])
    return dev, views, host_f32(rays)


def _count(dev, views, rays, g, depth_error_thresh, max_scale, sync=False):
    """The count phase: (workspace, lattice keep maps uint8 [ceil(H/g), ceil(W/g)], number of rows)."""
    nbytes = _lib.load().g4s_warp_init_workspace(views.n, views.sizes, g)
    if nbytes == 0:
        raise ValueError(f"{views.n} views: the lattice cells of all views must stay below 2^31")
    step = g if g > 0 else 1
    keep = [torch.empty((-(-views.size(v)[0] // step), -(-views.size(v)[1] // step)), dtype=torch.uint8, device=dev)
            for v in range(views.n)]
    rows = ctypes.c_int(0)
    ws = launch(dev, "g4s_warp_init_count", *views.head, rays, g, float(depth_error_thresh), float(max_scale), _lib.ptrs(keep),
                ctypes.byref(rows), workspace=nbytes, sync=sync)
    return ws, keep, rows.value


def _full_masks(views, keep, g):
    """The lattice bytes as bool [H,W] maps: false off the lattice."""
    if g <= 1:
        return [k.view(torch.bool) for k in keep]
    out = []
    for v, k in enumerate(keep):
        m = torch.zeros(views.size(v), dtype=torch.bool, device=k.device)
        m[::g, ::g] = k.view(torch.bool)
        out.append(m)
    return out


def warp_keep_masks(depths, cameras, depth_error_thresh=0.01, max_scale=0.05, downsample_pixel_grid_size=-1):
    """A list of bool [H_v,W_v] device tensors: the keep decision of every pixel -- on the lattice of
    downsample_pixel_grid_size, with a positive depth, explained by no earlier view, scale below max_scale.  depths: a list
    of float32 [H,W] / [1,H,W] maps whose sizes may differ, or one stacked [V,H,W] tensor."""
    g = int(downsample_pixel_grid_size)
    dev, views, rays = _stack(depths, cameras, None)
    if views is None:
        return []
    _ws, keep, _rows = _count(dev, views, rays, g, depth_error_thresh, max_scale, sync=True)
    return _full_masks(views, keep, g)


def warp_surfels(depths, cameras, images, depth_error_thresh=0.01, min_scale=0.0005, max_scale=0.05,
                 downsample_pixel_grid_size=-1, return_masks=False):
    """(means [M,3], scales [M,2], quaternions [M,4] (w, x, y, z), colors [M,3]), float32 on the device: one row per kept
    pixel, views in order and the pixels of a view in row-major order.  images: float32 [3,H,W] per view, read unclamped.
    With return_masks the masks of warp_keep_masks come fifth.  No kept pixel gives empty tensors.  Two launches and a scan;
    one host synchronisation for M."""
    g = int(downsample_pixel_grid_size)
    dev, views, rays = _stack(depths, cameras, images)
    if views is None:
        z = lambda w: torch.empty((0, w), dtype=torch.float32)
        out = (z(3), z(2), z(4), z(3))
        return out + ([],) if return_masks else out
    ws, keep, M = _count(dev, views, rays, g, depth_error_thresh, max_scale)
    out = tuple(torch.empty((M, w), dtype=torch.float32, device=dev) for w in (3, 2, 4, 3))
    launch(dev, "g4s_warp_init_emit", *views.head, rays, views.rgb, g, float(min_scale), _lib.ptrs(keep), M,
           *[_lib.ptr(t) for t in out], workspace=ws, sync=True)
    return out + (_full_masks(views, keep, g),) if return_masks else out


def get_gaussian_parameters_by_warp_from_depths(depths, views, depth_error_thresh=0.01, min_scale=0.0005, max_scale=0.05,
                                                downsample_pixel_grid_size=-1):
    """scene/gaussian_model.py get_gaussian_parameters_by_warp_from_depths: (means, scales, quaternions, colors).  The images
    are the views' original_image; a depth may be [H,W] or [1,H,W].  Where the reference raises (no view keeps a pixel)
    this returns empty tensors."""
    views = list(views)
    return warp_surfels(list(depths), views, [v.original_image for v in views], depth_error_thresh, min_scale, max_scale,
                        downsample_pixel_grid_size)
