"""Gaussian initialisation from depth charts (include/g4s_render_maps.h, "Chart surfels"; csrc/tsdf/chart_init.hip).

The trainer's first act (2d-gaussian-splatting/train_with_refine_depth.py, "Initialize gaussians") on its chart path: one
surfel on every face of the triangulated pixel grids that is not elongated, and the voxel pick of surfel indices.  The
other path, the warp initialiser, is warp_init.py; initial_gaussians takes it on request.

  pointmap_surfels, depthmap_surfels     the surfels of point maps, or of depth maps whose points are formed in the kernel.
  get_gaussian_parameters_from_pa_data, get_gaussian_parameters_from_charts_data   matcha/dm_scene/charts.py, by name.
  voxel_downsample_gaussians             matcha/dm_scene/charts.py: one surfel index per voxel.
  initial_gaussians                      the trainer's lines from the depth maps to create_from_parameters' arguments.
  select_init_views                      the trainer's sub-selection of views (host lists).

Everything per face and per voxel runs in the library; there is no torch path and no pytorch3d or open3d.  Tensors must be
on a HIP device: anything else is a ValueError.  A camera is anything with world_view_transform and full_proj_transform.
INTEGRATION.md section Q lists the differences from the reference.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._device import (check_dtype, check_view_count, drop_leading_one, host_f32, launch, mask_bytes, same_device, view_list,
                      voxel_downsample_count)
from .visibility import ray_record


# ---- host side: argument checks ----------------------------------------------------------------------------------------
def _views(maps, name, trailing, dtypes=(torch.float32,), shape=None, n=None):
    """The views of `maps` -- one stacked tensor [V,H,W,*trailing] or a list of [H,W,*trailing] -- as a list of tensors of
    one shape and an accepted dtype (the device is _device's).  Returns (list, (H, W))."""
    tail = "".join(",%d" % t for t in trailing)
    maps = view_list(maps, name, tail)
    check_view_count(maps, name, n)
    out = []
    for v, t in enumerate(maps):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}[{v}] must be a tensor on a HIP device")
        check_dtype(t, dtypes, f"{name}[{v}]")
        if not trailing:
            t = drop_leading_one(t)
        if t.dim() != 2 + len(trailing) or tuple(t.shape[2:]) != tuple(trailing) or t.numel() == 0:
            raise ValueError(f"{name}[{v}] must be a non-empty [H,W{tail}] map (got {tuple(t.shape)})")
        if shape is None:
            shape = tuple(t.shape[:2])
        if tuple(t.shape[:2]) != shape:
            raise ValueError(f"{name}[{v}] must be {shape[0]} x {shape[1]} like the other views (got {tuple(t.shape[:2])})")
        out.append(t)
    return out, shape


def _device(*groups):
    """The one HIP device of every tensor of the named groups (name, list or None), which come back contiguous."""
    dev, out = None, []
    for name, maps in groups:
        if maps is None:
            out.append(None)
            continue
        for v, t in enumerate(maps):
            dev = same_device(t, dev, f"{name}[{v}]")
        out.append([t.detach().contiguous() for t in maps])
    return dev, out


def _empty(dev):
    z = lambda w: torch.empty((0, w), dtype=torch.float32, device=dev)
    return {"means": z(3), "scales": z(3), "quaternions": z(4), "colors": z(3)}


def _surfels(dev, maps, rays, images, masks, shape, ratio_th, normalized_scales, normal_scale):
    """The two phases over checked views.  rays: None (point maps) or the float32 [V,12] ray records (depth maps)."""
    V = len(maps)
    if V == 0:
        return _empty(dev)
    H, W = shape
    lib = _lib.load()
    nbytes = lib.g4s_chart_surfels_workspace(V, H, W)
    if nbytes == 0:
        raise ValueError(f"{V} views of {H} x {W}: 2 V (H-1)(W-1) must be below 2^31")
    depth_form = 0 if rays is None else 1
    rays = None if rays is None else host_f32(rays)
    count = ctypes.c_int(0)
    ws = launch(dev, "g4s_chart_surfels_count", V, H, W, depth_form, _lib.ptrs(maps), rays,
                None if masks is None else _lib.ptrs([mask_bytes(m) for m in masks]), float(ratio_th), ctypes.byref(count),
                workspace=nbytes)
    M = count.value
    out = {"means": torch.empty((M, 3), dtype=torch.float32, device=dev), "scales": torch.empty((M, 3), dtype=torch.float32, device=dev),
           "quaternions": torch.empty((M, 4), dtype=torch.float32, device=dev),
           "colors": torch.empty((M, 3), dtype=torch.float32, device=dev)}
    launch(dev, "g4s_chart_surfels_emit", V, H, W, depth_form, _lib.ptrs(maps), rays, _lib.ptrs(images), float(normalized_scales),
           float(normal_scale), M, _lib.ptr(out["means"]), _lib.ptr(out["scales"]), _lib.ptr(out["quaternions"]),
           _lib.ptr(out["colors"]), workspace=ws, sync=True)
    return out


def _checked(maps, name, trailing, images, masks, n=None):
    """The maps, images and masks of one call, checked: (device, maps, images, masks, (H, W))."""
    maps, shape = _views(maps, name, trailing, n=n)
    images, _s = _views(images, "images", (3,), shape=shape, n=len(maps))
    if masks is not None:
        masks, _s = _views(masks, "masks", (), (torch.bool, torch.uint8), shape, len(maps))
    dev, (maps, images, masks) = _device((name, maps), ("images", images), ("masks", masks))
    return dev, maps, images, masks, shape


# ---- the surfels -----------------------------------------------------------------------------------------------------------
def pointmap_surfels(points, images, masks=None, ratio_th=5., normalized_scales=0.5, normal_scale=1e-10):
    """The surfels of V point maps: {"means" [M,3], "scales" [M,3], "quaternions" [M,4] (w, x, y, z), "colors" [M,3]}, float32
    on the device, row m the m-th surviving face in the reference's face order.  points: [V,H,W,3] or a list of [H,W,3] of
    one size; images alike (values are clamped to [0,1]); masks: None, or bool / uint8 [V,H,W] -- applied only if true
    somewhere, and then a face needs ONE masked-in vertex (the reference's quirks).  Two launches and a scan; one host
    synchronisation for M."""
    dev, points, images, masks, shape = _checked(points, "points", (3,), images, masks)
    return _surfels(dev, points, None, images, masks, shape, ratio_th, normalized_scales, normal_scale)


def depthmap_surfels(depths, cameras, images, masks=None, ratio_th=5., normalized_scales=0.5, normal_scale=1e-10):
    """pointmap_surfels over visibility.depths_to_points of each view, bit for bit, without the point maps: a vertex is
    formed in the kernel from the depth and the camera's ray record.  depths: [V,H,W] or a list of [H,W] / [1,H,W]."""
    cameras = list(cameras)
    dev, depths, images, masks, shape = _checked(depths, "depths", (), images, masks, len(cameras))
    rays = np.concatenate([ray_record(c, shape[1], shape[0]) for c in cameras]) if cameras else np.zeros(0, np.float32)
    return _surfels(dev, depths, rays, images, masks, shape, ratio_th, normalized_scales, normal_scale)


def get_gaussian_parameters_from_pa_data(pa_points, images, conf_th=-1., ratio_th=5., normal_scale=1e-4, normalized_scales=0.5,
                                         visibility_masks=None):
    """matcha/dm_scene/charts.py get_gaussian_parameters_from_pa_data.  conf_th and visibility_masks are accepted and have no
    effect, as in the reference (it builds the mesh with masks=None)."""
    return pointmap_surfels(pa_points, images, None, ratio_th, normalized_scales, normal_scale)


def get_gaussian_parameters_from_charts_data(charts_data, images, conf_th=-1., ratio_th=5., normal_scale=1e-4,
                                             normalized_scales=0.5, visibility_masks=None):
    """matcha/dm_scene/charts.py get_gaussian_parameters_from_charts_data: charts_data has 'pts' [V,H,W,3], 'confs' [V,H,W] and
    'scale_factor'.  Points and normal_scale are divided by scale_factor; with visibility_masks (a list whose concatenation
    along dim 0 is [V,H,W]) the confidences are multiplied by them and conf_th becomes 0.1; the mask is confs > conf_th."""
    scale = charts_data["scale_factor"]
    pts, confs = charts_data["pts"], charts_data["confs"]
    for name, t in (("charts_data['pts']", pts), ("charts_data['confs']", confs)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError(f"{name} must be a tensor on a HIP device")
    if visibility_masks is not None:
        confs = confs * torch.cat(list(visibility_masks), dim=0)
        conf_th = 0.1
    return pointmap_surfels(pts / scale, images, confs > conf_th, ratio_th, normalized_scales, float(normal_scale / scale))


# ---- the voxel pick --------------------------------------------------------------------------------------------------------
def voxel_downsample_gaussians(gaussian_params, voxel_size=0.01):
    """matcha/dm_scene/charts.py voxel_downsample_gaussians: (sample_idx int64 [n_voxels] on the device, downsample_factor).
    Per voxel the reference's rounded mean index of its surfels (which may name a surfel of another voxel), voxels in
    ascending (cz, cy, cx)."""
    means = gaussian_params["means"]
    if not isinstance(means, torch.Tensor) or means.device.type != "cuda":
        raise ValueError("gaussian_params['means'] must be a tensor on a HIP device")
    if means.dtype != torch.float32 or means.dim() != 2 or means.size(1) != 3 or means.size(0) == 0:
        raise ValueError(f"gaussian_params['means'] must be a non-empty float32 [N,3] (got {means.dtype} {tuple(means.shape)})")
    pts = means.detach().contiguous()
    n = pts.size(0)
    ws, count = voxel_downsample_count(pts, voxel_size, "voxel_downsample_gaussians")
    idx = torch.empty(count, dtype=torch.int64, device=pts.device)
    launch(pts.device, "g4s_voxel_downsample_emit_index", n, count, _lib.ptr(idx), workspace=ws, sync=True)
    return idx, n / count


# ---- the trainer's lines -----------------------------------------------------------------------------------------------------
MAX_INIT_INPUT_VIEWS = 50
MAX_INIT_EXTRA_VIEWS = 30


def select_init_views(n_input, n_extra, warp=False):
    """The trainer's view sub-selection as two index lists: with more than 50 input views, 50 of them by
    np.linspace(0, n_input - 1, 50, dtype=int); with more than 30 extra (inpainted) views, its hard-coded 0-9, 15-24 and
    30 .. n_extra - 1.  warp: the warp initialiser takes every input view (the trainer's warp_max_init_gs_input_view_num
    is None); the extra views are chosen as before."""
    n_input, n_extra = int(n_input), int(n_extra)
    if n_input < 0 or n_extra < 0:
        raise ValueError("view counts must not be negative")
    if n_input > MAX_INIT_INPUT_VIEWS and not warp:
        input_ids = [int(i) for i in np.linspace(0, n_input - 1, MAX_INIT_INPUT_VIEWS, dtype=int)]
    else:
        input_ids = list(range(n_input))
    if n_extra > MAX_INIT_EXTRA_VIEWS:
        extra_ids = list(range(10)) + list(range(15, 25)) + list(range(30, n_extra))
    else:
        extra_ids = list(range(n_extra))
    return input_ids, extra_ids


def initial_gaussians(input_depths, input_cameras, input_images, extra_depths=None, extra_cameras=None, extra_images=None,
                      max_gaussians_num=10_000_000, use_downsample_gaussians=False, downsample_gaussians_type="voxel",
                      warp_depth_error_thresh=0.01, warp_downsample_pixel_grid_size=-1):
    """The trainer's initial Gaussians from the plane-aware depths: (means [M,3], scales [M,2], quaternions [M,4], colors
    [M,3]), ready for GaussianModel.create_from_parameters.  The surfels of the input views, then those of the extra views
    (ratio_th 5, normalized_scales 0.5, normal_scale 1e-10); if there are more than max_gaussians_num and
    use_downsample_gaussians is set, the voxel pick at 1 cm; scales[:, :2] times the downsample factor.  The views are
    taken as given: select_init_views is the caller's.

    With use_downsample_gaussians and downsample_gaussians_type "warp" (the trainer's default type) the warp initialiser
    runs instead: warp_init.warp_surfels over the input views followed by the extra views, images [3,H,W]."""
    if downsample_gaussians_type not in ("voxel", "warp"):
        raise ValueError(f"downsample_gaussians_type must be 'voxel' or 'warp' (got {downsample_gaussians_type!r})")
    if use_downsample_gaussians and downsample_gaussians_type == "warp":
        from .warp_init import warp_surfels
        more = extra_depths is not None and len(extra_depths) > 0
        return warp_surfels(list(input_depths) + (list(extra_depths) if more else []),
                            list(input_cameras) + (list(extra_cameras) if more else []),
                            list(input_images) + (list(extra_images) if more else []),
                            depth_error_thresh=warp_depth_error_thresh, downsample_pixel_grid_size=warp_downsample_pixel_grid_size)
    params = depthmap_surfels(input_depths, input_cameras, input_images)
    if extra_depths is not None and len(extra_depths) > 0:
        extra = depthmap_surfels(extra_depths, extra_cameras, extra_images)
        params = {k: torch.cat([params[k], extra[k]], dim=0) for k in params}
    n = params["means"].size(0)
    if n > max_gaussians_num and use_downsample_gaussians:
        idx, factor = voxel_downsample_gaussians(params, voxel_size=0.01)
        return params["means"][idx], params["scales"][:, :2][idx] * factor, params["quaternions"][idx], params["colors"][idx]
    return params["means"], params["scales"][:, :2] * 1.0, params["quaternions"], params["colors"]
