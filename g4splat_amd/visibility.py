"""Visibility grid for novel-view selection (include/g4s_render_maps.h, "Visibility grid"; csrc/tsdf/visibility.hip).

The stage the reference runs between training and inpainting (render_novel_views.py, render_chart_views.py): which voxels
of the scene's box some input view sees in free space (guidance/vis_grid.py VisibilityGrid), the per-pixel visibility map
of a candidate camera, and the between-view masks of guidance/cam_utils.py and planes/get_global_3Dpnts.py.  Everything
consumes only render()'s surf_depth, stays on the device, and goes through the library: there is no torch path.

A camera is anything with world_view_transform, FoVx and FoVy (and full_proj_transform where a ray record is needed):
synthetic.PinholeCamera, the reference's Camera.  Depth maps are device tensors [H,W] or [1,H,W]; a view's width and
height are its map's.  INTEGRATION.md section L lists the differences from the reference.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, ply_io
from ._device import camera_views, default_device, depth_map, device_points, hip_device, host_f32, launch, to_np

_MODES = {"free": 0, "surface": 1}


# ---- host-side records -------------------------------------------------------------------------------------------------
def ray_record(camera, width, height):
    """The twelve floats (origin o[3], D[3][3] row-major) of the contract: dir = D @ (x, y, 1) for integer pixel
    coordinates, point = o + t * dir.  Computed in double the way matcha/dm_scene/charts.py depths_to_points_parallel
    derives its rays (c2w from world_view_transform, pixel intrinsics from full_proj_transform and the map's size)."""
    wvt = np.asarray(to_np(camera.world_view_transform), np.float64).reshape(4, 4)
    full = np.asarray(to_np(camera.full_proj_transform), np.float64).reshape(4, 4)
    c2w = np.linalg.inv(wvt.T)
    W, H = float(width), float(height)
    ndc2pix = np.array([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], np.float64).T
    intr = ((c2w.T @ full) @ ndc2pix)[:3, :3].T
    D = c2w[:3, :3] @ np.linalg.inv(intr)
    return np.concatenate([c2w[:3, 3], D.reshape(9)]).astype(np.float32)


def _view_table(views):
    return _lib.load().g4s_visgrid_workspace(views.n)


# ---- view counts ----------------------------------------------------------------------------------------------------------
def view_counts(points, cameras, depths, mode="free", depth_threshold=0.1, skip_view=None):
    """int32 [n]: for every point [n,3] (device tensor) the number of views that pass the FREE (in image, in front of
    the camera, nearer than the view's depth) or the SURFACE (relative depth difference below depth_threshold)
    predicate; skip_view names a view to leave out."""
    dev, pts = device_points(points)
    n = pts.size(0)
    views = camera_views(cameras, depths, dev)
    counts = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    launch(dev, "g4s_view_counts_points", n, _lib.ptr(pts), _MODES[mode], float(depth_threshold),
           -1 if skip_view is None else int(skip_view), *views.head, _lib.ptr(counts), workspace=_view_table(views), sync=True)
    return counts[:n]


def pixel_view_counts(camera, depth, cameras, depths, mode="surface", depth_threshold=0.1, skip_view=None):
    """int32 [H,W]: view_counts of the pixels of `depth` back-projected through `camera`, fused: the points are formed
    in the kernel and never stored.  Bit-identical to view_counts(depths_to_points(depth, camera), ...)."""
    dev, d = depth_map(depth)
    H, W = d.shape
    views = camera_views(cameras, depths, dev)
    counts = torch.empty((H, W), dtype=torch.int32, device=dev)
    launch(dev, "g4s_view_counts_pixels", W, H, _lib.ptr(d), host_f32(ray_record(camera, W, H)), _MODES[mode],
           float(depth_threshold), -1 if skip_view is None else int(skip_view), *views.head, _lib.ptr(counts),
           workspace=_view_table(views), sync=True)
    return counts


def depths_to_points(depth, camera):
    """float32 [H*W,3]: the world points of a depth map's pixels, origin + depth * direction."""
    dev, d = depth_map(depth)
    H, W = d.shape
    points = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
    launch(dev, "g4s_depth_to_points", W, H, _lib.ptr(d), host_f32(ray_record(camera, W, H)), _lib.ptr(points), sync=True)
    return points


def check_valid_camera_center_by_depth(cameras, depths, points):
    """guidance/cam_utils.py: bool [n], the point lies in some view's observed free space."""
    return view_counts(points, cameras, depths, "free") > 0


def get_visible_mask_for_input_views(cameras, depths, points, depth_threshold=0.1):
    """planes/get_global_3Dpnts.py: bool [n], some view sees the point on its surface."""
    return view_counts(points, cameras, depths, "surface", depth_threshold) > 0


def build_visibility_masks(cameras, depths, points=None, depth_threshold=0.1, least_num_views=1, return_origin_masks=False):
    """guidance/cam_utils.py: per view a float [1,H,W] mask of the pixels that at least least_num_views OTHER views see on
    their surface (return_origin_masks: the number of such views instead).  points[i] [H*W,3] are view i's world points;
    points=None back-projects view i's own depth map in the kernel."""
    cameras, depths = list(cameras), list(depths)
    masks = []
    for i, (cam, depth) in enumerate(zip(cameras, depths)):
        _dev, d = depth_map(depth)
        H, W = d.shape
        if points is None:
            n = pixel_view_counts(cam, d, cameras, depths, "surface", depth_threshold, skip_view=i)
        else:
            n = view_counts(points[i], cameras, depths, "surface", depth_threshold, skip_view=i)
            if n.numel() != H * W:
                raise ValueError(f"view {i}: {n.numel()} points for a {H} x {W} map")
        n = n.reshape(1, H, W)
        masks.append(n.float() if return_origin_masks else (n >= least_num_views).float())
    return masks


# ---- the grid ---------------------------------------------------------------------------------------------------------------
class VisibilityGrid:
    """guidance/vis_grid.py VisibilityGrid on the device: resolution^3 voxels over bbox_min .. bbox_max, a voxel visible
    iff its centre passes the FREE predicate in some input view.  Held as one bit per voxel (`words`, int64
    [ceil(R^3 / 64)], bit flat & 63 of word flat >> 6, flat = (ix R + iy) R + iz); `visibility_grid` is the reference's
    float [R,R,R] tensor, expanded on first use."""

    def __init__(self, bbox_min, bbox_max, resolution, input_cameras, input_depths, device=None):
        if device is None:
            device = bbox_min.device if isinstance(bbox_min, torch.Tensor) and bbox_min.is_cuda else default_device()
        self.device = hip_device(device)
        R = int(resolution)
        if R < 1 or R ** 3 >= 2 ** 31:
            raise ValueError("resolution must be at least 1 and resolution^3 below 2^31")
        self.resolution = R
        lo = np.asarray(to_np(bbox_min), np.float32).reshape(3)
        hi = np.asarray(to_np(bbox_max), np.float32).reshape(3)
        self._lo, self._hi = host_f32(lo), host_f32(hi)
        cell = (hi - lo) / np.float32(R)
        self.bbox_min = torch.as_tensor(lo, device=self.device)
        self.bbox_max = torch.as_tensor(hi, device=self.device)
        self.grid_size = torch.as_tensor(cell, device=self.device)
        self.min_grid_size = float(cell.min())
        self.input_cameras, self.input_depths = list(input_cameras), list(input_depths)
        self._grid = None
        dev = self.device
        views = camera_views(self.input_cameras, self.input_depths, dev)
        self.words = torch.empty((R ** 3 + 63) // 64, dtype=torch.int64, device=dev)
        launch(dev, "g4s_visgrid_build", R, self._lo, self._hi, *views.head, _lib.ptr(self.words), workspace=_view_table(views),
               sync=True)

    @property
    def visibility_grid(self):
        if self._grid is None:
            R, dev = self.resolution, self.device
            grid = torch.empty((R, R, R), dtype=torch.float32, device=dev)
            launch(dev, "g4s_visgrid_expand", R, _lib.ptr(self.words), _lib.ptr(grid))
            self._grid = grid
        return self._grid

    def check_valid_camera_center(self, points):
        """bool [...]: the voxel each point [...,3] falls into is visible (points outside the box count as their
        border voxel, as in the reference)."""
        shape = tuple(points.shape[:-1])
        _dev, pts = device_points(points.to(self.device))
        n = pts.size(0)
        out = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        launch(self.device, "g4s_visgrid_sample", self.resolution, self._lo, self._hi, _lib.ptr(self.words), n, _lib.ptr(pts),
               _lib.ptr(out), sync=True)
        return out[:n].bool().reshape(shape)

    def n_samples(self, depth):
        """The reference's sample count of a depth map [H,W]: int(largest depth / min_grid_size) + 1, invalid pixels
        (depth <= 1e-6) counting as 1e-3.  One read-back."""
        m = torch.where(depth <= 1e-6, torch.full_like(depth, 1e-3), depth).max().item()
        if not math.isfinite(m):
            raise ValueError("depth map holds a non-finite value")
        return int(m / self.min_grid_size) + 1

    def render_visibility_map(self, cameras, depths):
        """List of float [H,W] maps: 1 where every sample of the pixel's ray, from the camera up to ten samples before
        its depth, lies in a visible voxel; 0 otherwise and where depth <= 1e-6.  The depth maps are not modified."""
        maps = []
        dev = self.device
        for cam, depth in zip(cameras, depths):
            _d, d = depth_map(depth, dev)
            H, W = d.shape
            out = torch.empty((H, W), dtype=torch.float32, device=dev)
            S = self.n_samples(d)
            launch(dev, "g4s_visgrid_march", self.resolution, self._lo, self._hi, _lib.ptr(self.words), W, H, _lib.ptr(d),
                   host_f32(ray_record(cam, W, H)), S, _lib.ptr(out), sync=True)
            maps.append(out)
        return maps

    def _centres(self, invisible):
        lib, dev, R = _lib.load(), self.device, self.resolution
        n = ctypes.c_int(0)
        ws = launch(dev, "g4s_visgrid_compact_count", R, _lib.ptr(self.words), int(invisible), ctypes.byref(n),
                    workspace=lib.g4s_visgrid_compact_workspace(R))
        out = torch.empty((max(n.value, 1), 3), dtype=torch.float32, device=dev)
        launch(dev, "g4s_visgrid_compact_emit", R, self._lo, self._hi, _lib.ptr(self.words), int(invisible), n.value,
               _lib.ptr(out), workspace=ws, sync=True)
        return out[:n.value]

    def get_all_visible_pnts(self):
        """float [n,3]: the centres of the visible voxels in flat-index order (grid_centers[mask]'s); None if there is
        none, as in the reference."""
        pts = self._centres(False)
        return pts if pts.size(0) else None

    def invisible_points(self):
        """float [n,3]: the centres of the invisible voxels in flat-index order (possibly empty)."""
        return self._centres(True)

    def get_visible_boundary(self):
        """(x_min, y_min, z_min, x_max, y_max, z_max) of the visible voxel centres, 0-dim tensors; None without any."""
        pts = self.get_all_visible_pnts()
        if pts is None:
            return None
        lo, hi = pts.min(0).values, pts.max(0).values
        return lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]

    def vis_invisible_pnts(self, save_path):
        """Writes the invisible voxel centres as a vertex-only PLY; nothing is written when every voxel is visible."""
        pts = self.invisible_points()
        if pts.size(0) == 0:
            return
        ply_io.write_point_cloud(save_path, pts)
