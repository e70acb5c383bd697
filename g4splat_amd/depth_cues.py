"""Depth cues of the inpainted views (include/g4s_render_maps.h, "Depth cues"; csrc/tsdf/depth_cues.hip).

The code the reference runs per inpainted view between the inpainter and the global-plane merge (guidance/see3d_dn_util.py,
guidance/dense_dn_util.py) and between the merge and the inconsistency solvers (planes/refine_depth_with_planes.py):

  align_disparities, depth_linear_align, depth_linear_align_2   matcha/pointmap/depthanythingv2.py: the masked least-squares
                              scale and shift of a mono disparity (or depth) onto a rendered depth.
  view_geometry_cues          the loop body of the two *_dn_util scripts: visibility, aligned depth, its normals in world and
                              camera frame, the merged depth.
  plane_aligned_depth, apply_global_planes   compute_plane_aligned_depth and its paste per (plane, view) pair.
  refill_unseen_regions, refine_depths_with_planes   the second alignment, the refill, the refined clouds.

Everything per pixel runs in the library, all views in a number of launches that does not depend on the number of views or
planes; there is no torch path.  `planes` is an input: plane_fit.fit_global_planes produces it, or the caller does.

A camera is anything with world_view_transform, full_proj_transform, FoVx, FoVy (image_width and image_height are not
read: a view's size is its maps').  Maps are lists of [H_v, W_v] device tensors, or one stacked [V,H,W] tensor; views may
differ in size.  There is no file I/O.  INTEGRATION.md section P lists the differences from the reference.
"""
import numpy as np
import torch

from . import _lib
from ._device import (ViewStack, check_dtype, check_view_count, drop_leading_one, focal_lengths, hip_device, host_array, host_f32,
                      launch, mask_bytes, same_device, to_np, view_list)
from .visibility import depths_to_points, ray_record

_DOMAINS = {"disparity": 0, "depth": 1, "inverse_source": 2}
ALIGN_SPAN = 4096  # G4S_DEPTH_ALIGN_SPAN: pixels one workgroup of the sums kernel reduces


class GeometryCues:
    """What view_geometry_cues returns: per-view lists visibility (bool [H,W]), mono_depth, aligned_depth, depth (merged)
    (float32 [H,W]), normal_world, normal_cam (float32 [H,W,3]), and coeffs float32 [V,2] = (alpha, beta), counts int32 [V]."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


# ---- host side: argument checks and tables (no device code: tests/test_depth_cues_cpu.py runs them) -------------------------
def _check_maps(maps, name, dev, dtypes, shapes=None, n=None):
    """The maps as contiguous [H,W] tensors on one HIP device; ValueError for anything else.  Returns (device, list)."""
    maps = view_list(maps, name)
    check_view_count(maps, name, n)
    out = []
    for v, t in enumerate(maps):
        dev = same_device(t, dev, f"{name}[{v}]")
        check_dtype(t, dtypes, f"{name}[{v}]")
        t = drop_leading_one(t)
        if t.dim() != 2 or t.numel() == 0:
            raise ValueError(f"{name}[{v}] must be a non-empty [H,W] map (got {tuple(t.shape)})")
        if shapes is not None and tuple(t.shape) != shapes[v]:
            raise ValueError(f"{name}[{v}] must have shape {shapes[v]} (got {tuple(t.shape)})")
        out.append(t.detach().contiguous())
    return dev, out


def _shapes(maps):
    return [tuple(t.shape) for t in maps]


def _stack(maps, dev, cameras=None):
    """ViewStack over checked maps: sizes and the pointer array, and with cameras their world_view_transform."""
    if cameras is None:
        return ViewStack([(None, m, None) for m in maps], dev)
    return ViewStack([(c, m, None) for c, m in zip(cameras, maps)], dev, False, 1, lambda cam: [cam.world_view_transform])


def plane_camera_record(camera, width, height):
    """The fourteen floats of the contract's plane camera: centre o[3], camera -> world rotation R[3][3] row-major (from the
    inverse of world_view_transform, in double), fx = W / (2 tan(FoVx / 2)), fy alike."""
    wvt = np.asarray(to_np(camera.world_view_transform), np.float64).reshape(4, 4)
    c2w = np.linalg.inv(wvt).T
    fx, fy = focal_lengths(camera, width, height)
    return np.concatenate([c2w[:3, 3], c2w[:3, :3].reshape(9), [fx, fy]]).astype(np.float32)


def plane_table(global_3Dplane_ID_dict, planes, n_views):
    """The library's table of fitted (view, id) pairs: (view_offset [V+1], ids [E], entry_plane [E], plane_rows [P,6] float32,
    keys [P]).  Plane p is the p-th key of the dict that `planes` holds, (normal, centre) as six floats; a key missing
    from `planes` is skipped (the reference's `continue`); a pair listed under several fitted keys keeps the last in dict
    order (the reference pastes sequentially).  ValueError: a view outside 0 .. n_views - 1, an id that is not positive, a
    plane that is not six finite numbers."""
    keys, rows = [], []
    per_view = [dict() for _ in range(n_views)]
    for key, pairs in global_3Dplane_ID_dict.items():
        pairs = [(int(v), int(p)) for v, p in pairs]
        for v, p in pairs:
            if not 0 <= v < n_views:
                raise ValueError(f"global_3Dplane_ID_dict names view {v} but there are {n_views} views")
            if p <= 0:
                raise ValueError(f"global_3Dplane_ID_dict: plane id {p} of view {v} must be positive")
        if key not in planes:
            continue
        normal, centre = planes[key]
        row = np.concatenate([np.asarray(to_np(normal), np.float64).reshape(-1), np.asarray(to_np(centre), np.float64).reshape(-1)])
        with np.errstate(over="ignore"):
            finite = row.shape == (6,) and np.isfinite(row.astype(np.float32)).all()
        if not finite:
            raise ValueError(f"planes[{key!r}] must be a finite (normal[3], center[3])")
        for v, p in pairs:
            per_view[v][p] = len(rows)
        keys.append(key)
        rows.append(row.astype(np.float32))
    view_offset, ids, entry_plane = [0], [], []
    for table in per_view:
        for p in sorted(table):
            ids.append(p)
            entry_plane.append(table[p])
        view_offset.append(len(ids))
    plane_rows = np.stack(rows) if rows else np.zeros((0, 6), np.float32)
    return view_offset, ids, entry_plane, plane_rows, keys


# ---- A. alignment ----------------------------------------------------------------------------------------------------------
def _align_coeffs(dev, sources, targets, masks, domain, threshold=None, coeffs=None, counts=None):
    """g4s_depth_align over the views: (coeffs [V,2], counts [V]) on the device.  threshold: `masks` are float maps."""
    V = len(sources)
    if coeffs is None:
        coeffs = torch.empty((max(V, 1), 2), dtype=torch.float32, device=dev)
        counts = torch.empty(max(V, 1), dtype=torch.int32, device=dev)
    if V:
        stack = _stack(sources, dev)
        launch(dev, "g4s_depth_align", _DOMAINS[domain], 0 if threshold is None else 1,
               0.0 if threshold is None else float(threshold), V, stack.sizes, stack.depth, _lib.ptrs(targets), _lib.ptrs(masks),
               _lib.ptr(coeffs), _lib.ptr(counts), workspace=_lib.load().g4s_depth_align_workspace(V, stack.sizes), sync=True)
    return coeffs[:V], counts[:V]


def align_disparities(disps, targets, masks, domain="disparity"):
    """(aligned, coeffs, counts): per view the least-squares alpha, beta over the masked pixels with 1 / target ~ alpha +
    beta disp (domain "disparity": aligned = 1 / (alpha + beta disp)) or target ~ alpha + beta disp (domain "depth": aligned
    = alpha + beta disp).  aligned is a list of float32 [H,W]; coeffs float32 [V,2] = (alpha, beta) and counts int32 [V] (the
    masked pixels) stay on the device.  A view without two distinct masked values gives NaN or inf, as in the reference."""
    if domain not in ("disparity", "depth"):
        raise ValueError(f"domain must be 'disparity' or 'depth' (got {domain!r})")
    dev, disps = _check_maps(disps, "disps", None, (torch.float32,))
    V = len(disps)
    _d, targets = _check_maps(targets, "targets", dev, (torch.float32,), _shapes(disps), V)
    _d, masks = _check_maps(masks, "masks", dev, (torch.bool, torch.uint8), _shapes(disps), V)
    if V == 0:
        return [], torch.zeros((0, 2)), torch.zeros(0, dtype=torch.int32)
    coeffs, counts = _align_coeffs(dev, disps, targets, [mask_bytes(m) for m in masks], domain)
    aligned = [torch.empty_like(d) for d in disps]
    stack = _stack(disps, dev)
    launch(dev, "g4s_depth_align_apply", _DOMAINS[domain], V, stack.sizes, stack.depth, _lib.ptr(coeffs), _lib.ptrs(aligned),
           workspace=_lib.load().g4s_depth_align_apply_workspace(V), sync=True)
    return aligned, coeffs, counts


def _single(disp, render_depth, visible_mask, return_alpha_beta, domain):
    aligned, coeffs, _counts = align_disparities([disp], [render_depth], [visible_mask], domain)
    if not return_alpha_beta:
        return aligned[0]
    alpha, beta = coeffs[0].tolist()  # the one read-back
    return aligned[0], alpha, beta


def depth_linear_align(disp, render_depth, visible_mask, return_alpha_beta=False):
    """matcha/pointmap/depthanythingv2.py depth_linear_align for one view: 1 / (alpha + beta disp), and with
    return_alpha_beta also alpha and beta as Python floats (one read-back)."""
    return _single(disp, render_depth, visible_mask, return_alpha_beta, "disparity")


def depth_linear_align_2(depth, render_depth, visible_mask, return_alpha_beta=False):
    """depth_linear_align_2 for one view: alpha + beta depth."""
    return _single(depth, render_depth, visible_mask, return_alpha_beta, "depth")


# ---- B. cue maps -----------------------------------------------------------------------------------------------------------
def view_geometry_cues(cameras, mono_disps, warp_depths, alphas, visible_threshold=0.9):
    """The loop body of guidance/see3d_dn_util.py / dense_dn_util.py for all views at once (three launches): a GeometryCues.
    mono_disps, warp_depths and alphas are float32 maps of the view's size."""
    cameras = list(cameras)
    V = len(cameras)
    dev, disps = _check_maps(mono_disps, "mono_disps", None, (torch.float32,), None, V)
    _d, warps = _check_maps(warp_depths, "warp_depths", dev, (torch.float32,), _shapes(disps), V)
    _d, alphas = _check_maps(alphas, "alphas", dev, (torch.float32,), _shapes(disps), V)
    threshold = float(visible_threshold)
    if threshold != threshold:
        raise ValueError("visible_threshold must not be NaN")
    if V == 0:
        return GeometryCues(visibility=[], mono_depth=[], aligned_depth=[], depth=[], normal_world=[], normal_cam=[],
                            coeffs=torch.zeros((0, 2)), counts=torch.zeros(0, dtype=torch.int32))
    coeffs, counts = _align_coeffs(dev, disps, warps, alphas, "disparity", threshold)
    vis = [torch.empty(d.shape, dtype=torch.bool, device=dev) for d in disps]
    mono, aligned, merged = ([torch.empty_like(d) for d in disps] for _ in range(3))
    nw, nc = ([torch.empty((*d.shape, 3), dtype=torch.float32, device=dev) for d in disps] for _ in range(2))
    stack = _stack(disps, dev, cameras)
    rays = np.concatenate([ray_record(c, d.shape[1], d.shape[0]) for c, d in zip(cameras, disps)])
    n, world_view, sizes, dptr = stack.head
    launch(dev, "g4s_depth_cue_maps", n, world_view, host_f32(rays), sizes, dptr, _lib.ptrs(warps), _lib.ptrs(alphas), threshold,
           _lib.ptr(coeffs), _lib.ptrs([mask_bytes(m) for m in vis]), _lib.ptrs(mono), _lib.ptrs(aligned), _lib.ptrs(merged),
           _lib.ptrs(nw), _lib.ptrs(nc), workspace=_lib.load().g4s_depth_cue_maps_workspace(n), sync=True)
    return GeometryCues(visibility=vis, mono_depth=mono, aligned_depth=aligned, depth=merged, normal_world=nw, normal_cam=nc,
                        coeffs=coeffs, counts=counts)


# ---- C. plane depths -------------------------------------------------------------------------------------------------------
def apply_global_planes(cameras, depths, plane_masks, global_3Dplane_ID_dict, planes):
    """The paste loop of planes/refine_depth_with_planes.py in one launch: (new depth maps, replaced int32 [V], zeroed int32
    [V]).  A pixel whose (view, mask id) is listed under a global plane that `planes` = {global id: (normal[3], center[3])}
    holds takes the depth of its ray's intersection with that plane, or 0 where the intersection is behind the camera;
    `replaced` and `zeroed` count the two.  plane_masks are int32 [H,W] with arbitrary positive ids, 0 = none.  The inputs are
    only read."""
    cameras = list(cameras)
    V = len(cameras)
    dev, depths = _check_maps(depths, "depths", None, (torch.float32,), None, V)
    _d, masks = _check_maps(plane_masks, "plane_masks", dev, (torch.int32,), _shapes(depths), V)
    view_offset, ids, entry_plane, rows, _keys = plane_table(global_3Dplane_ID_dict, planes, V)
    if V == 0:
        return [], torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    records = np.concatenate([plane_camera_record(c, d.shape[1], d.shape[0]) for c, d in zip(cameras, depths)])
    if not np.isfinite(records).all():
        raise ValueError("a camera's world_view_transform or field of view is not finite")
    out = [torch.empty_like(d) for d in depths]
    counts = torch.empty((2, V), dtype=torch.int32, device=dev)
    stack = _stack(depths, dev)
    launch(dev, "g4s_plane_depths", V, host_f32(records), stack.sizes, stack.depth, _lib.ptrs(out), _lib.ptrs(masks),
           host_array(_lib.c_i, view_offset), host_array(_lib.c_i, ids), host_array(_lib.c_i, entry_plane), len(rows),
           host_array(_lib.c_f, rows.reshape(-1).tolist()), _lib.ptr(counts),
           workspace=_lib.load().g4s_plane_depths_workspace(V, len(ids), len(rows)), sync=True)
    return out, counts[0], counts[1]


def plane_aligned_depth(plane_normal, plane_center, camera, img_shape):
    """planes/refine_depth_with_planes.py compute_plane_aligned_depth: (aligned_depth float32 [H,W], valid bool [H,W]) of the
    whole image against one plane.  The reference's second result, the list of valid intersection points, is replaced by
    the mask (nobody uses the list)."""
    H, W = (int(s) for s in img_shape)
    if H <= 0 or W <= 0:
        raise ValueError(f"img_shape must be positive (got {tuple(img_shape)})")
    dev = hip_device(plane_normal.device if isinstance(plane_normal, torch.Tensor) and plane_normal.is_cuda else "cuda")
    depth = torch.zeros((H, W), dtype=torch.float32, device=dev)
    mask = torch.ones((H, W), dtype=torch.int32, device=dev)
    out, _replaced, _zeroed = apply_global_planes([camera], [depth], [mask], {0: [(0, 1)]}, {0: (plane_normal, plane_center)})
    return out[0], out[0] > 0


# ---- D. refill, and the whole stage ------------------------------------------------------------------------------------------
def _refill(dev, depths, monos, masks, confs, n_input):
    """In place on `depths`: the second alignment (two launches) and the refill (one)."""
    V = len(depths)
    coeffs = torch.zeros((V, 2), dtype=torch.float32, device=dev)
    counts = torch.zeros(V, dtype=torch.int32, device=dev)
    if n_input == V:
        return coeffs, counts
    confs8 = [mask_bytes(c) for c in confs]
    _align_coeffs(dev, monos[n_input:], depths[n_input:], confs8[n_input:], "inverse_source", None, coeffs[n_input:],
                  counts[n_input:])
    stack = _stack(monos, dev)
    launch(dev, "g4s_depth_refill", V, n_input, stack.sizes, _lib.ptrs(depths), stack.depth, _lib.ptrs(masks), _lib.ptrs(confs8),
           _lib.ptr(coeffs), workspace=_lib.load().g4s_depth_refill_workspace(V), sync=True)
    return coeffs, counts


def _refill_args(depths, mono_depths, plane_masks, conf_maps, n_input_views):
    dev, depths = _check_maps(depths, "depths", None, (torch.float32,))
    V = len(depths)
    _d, monos = _check_maps(mono_depths, "mono_depths", dev, (torch.float32,), _shapes(depths), V)
    _d, masks = _check_maps(plane_masks, "plane_masks", dev, (torch.int32,), _shapes(depths), V)
    _d, confs = _check_maps(conf_maps, "conf_maps", dev, (torch.bool, torch.uint8), _shapes(depths), V)
    n_input = int(n_input_views)
    if not 0 <= n_input <= V:
        raise ValueError(f"n_input_views must be in 0 .. {V} (got {n_input})")
    return dev, depths, monos, masks, confs, n_input


def refill_unseen_regions(depths, mono_depths, plane_masks, conf_maps, n_input_views):
    """The "refine non-plane region" loop of planes/refine_depth_with_planes.py: (new depth maps, coeffs [V,2], counts [V]).
    For every view v >= n_input_views the mono depth is aligned to depths[v] over the confident pixels (1 / depth ~ alpha +
    beta / mono_depth) and written where the view has neither a plane (plane_mask == 0) nor confidence (conf false).  Input
    views come back unchanged (their coeffs are 0); mono_depths of input views are not read."""
    dev, depths, monos, masks, confs, n_input = _refill_args(depths, mono_depths, plane_masks, conf_maps, n_input_views)
    out = [d.clone() for d in depths]
    coeffs, counts = _refill(dev, out, monos, masks, confs, n_input) if out else (torch.zeros((0, 2)), torch.zeros(0))
    return out, coeffs, counts


def refine_depths_with_planes(cameras, depths, plane_masks, conf_maps, mono_depths, global_3Dplane_ID_dict, planes,
                              n_input_views, return_points=False):
    """Lines 605-652 of planes/refine_depth_with_planes.py after the fit: the plane depths of all (plane, view) pairs, the
    alignment of the inpainted views' mono depth to the result over their confident pixels, the refill of what is neither
    plane nor confident -- four launches for all views --, and with return_points the refined clouds [H*W,3] (one launch per
    view).  Returns the refined depth maps, or (depth maps, points)."""
    cameras = list(cameras)
    dev, depths, monos, masks, confs, n_input = _refill_args(depths, mono_depths, plane_masks, conf_maps, n_input_views)
    if len(cameras) != len(depths):
        raise ValueError(f"{len(cameras)} cameras but {len(depths)} depths")
    refined, _replaced, _zeroed = apply_global_planes(cameras, depths, masks, global_3Dplane_ID_dict, planes)
    if refined:
        _refill(dev, refined, monos, masks, confs, n_input)
    if not return_points:
        return refined
    return refined, [depths_to_points(d, c) for d, c in zip(refined, cameras)]
