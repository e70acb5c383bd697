"""Chart points (include/g4s_losses.h, "Chart points"; csrc/chart_points.hip): 3D points per chart, projected into their chart
and tapped in any [n,H,W] map.

Two stages of the reference use this one primitive.  Before the alignment, matcha/pointmap/depthanythingv2.py fits every
chart's mono disparity to its SfM points (get_points_depth_in_depthmap, fit_depth_to_point_cloud, looped per chart with
grid_sample and two .item() calls each); build_charts does that for all charts on the device and returns what align_charts
takes.  Inside the alignment, ParallelAligner.loss with 3D points as reference_data samples the predicted depths and the
confidence under the points in every iteration; point_reference_loss is that term with its gradient, bit-reproducible.
Everything goes through the library; there is no torch path.

A camera is anything with world_view_transform and full_proj_transform in the reference's row-vector convention; `cameras` is
a list of them or a wrapper with `.gs_cameras`.  INTEGRATION.md section Y lists the differences from the reference.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._device import check_dtype, launch, same_device, to_np
from ._charts import camera_list, depths_and_confidence, f32, grads_like, maps_of_shape, spatial_extent, stack

SPAN = 4096  # G4S_CHART_POINTS_SPAN: points per workgroup of the float64 sums
CHUNK = 64   # G4S_CHART_POINTS_CHUNK: taps per separately summed chunk of a pixel's list
MAX_POINTS = (1 << 29) - 1
_FLOATS = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


def camera_records(cameras):
    """float32 [n,32]: world_view_transform and full_proj_transform of each view, row-major -- the `cameras` argument of the
    library calls."""
    return np.stack([np.concatenate([np.asarray(to_np(c.world_view_transform), np.float32).reshape(16),
                                     np.asarray(to_np(c.full_proj_transform), np.float32).reshape(16)]) for c in cameras]).astype(np.float32)


def _point_lists(points, n):
    """The per-chart [N_c,3] tensors of a list or an [n,N,3] tensor, checked on the host: shapes, dtype and count."""
    if isinstance(points, torch.Tensor):
        if points.dim() != 3 or points.size(-1) != 3:
            raise ValueError(f"chart points: a stacked tensor must be [n,N,3] (got {tuple(points.shape)})")
        lists = list(points.unbind(0))
    else:
        lists = list(points)
    if len(lists) != n:
        raise ValueError(f"{n} views but {len(lists)} point lists")
    for c, p in enumerate(lists):
        if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.size(-1) != 3:
            raise ValueError(f"chart points: points[{c}] must be a [N,3] tensor (got {tuple(getattr(p, 'shape', ()))})")
        check_dtype(p, _FLOATS, f"points[{c}]")
    if sum(p.size(0) for p in lists) > MAX_POINTS:
        raise ValueError("chart points: at most 2^29 - 1 points")
    return lists


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, maps, cp):
        m = f32(maps)
        with torch.cuda.device(cp.device):
            values = torch.empty(cp.n_points, dtype=torch.float32, device=cp.device)
            fov = torch.empty(cp.n_points, dtype=torch.uint8, device=cp.device)
            _lib.call("g4s_chart_points_sample", cp.n, cp.height, cp.width, cp.n_points, _lib.ptr(cp.chart), _lib.ptr(cp.ixy),
                      _lib.ptr(m), _lib.ptr(values), _lib.ptr(fov), _lib.stream(cp.device))
        fov = fov.bool()
        ctx.cp, ctx.meta = cp, (maps.shape, maps.dtype)
        ctx.mark_non_differentiable(fov)
        return values, fov

    @staticmethod
    def backward(ctx, g, _unused):
        cp = ctx.cp
        cp.build_index()
        with torch.cuda.device(cp.device):
            g = f32(g)
            out = torch.empty((cp.n, cp.height, cp.width), dtype=torch.float32, device=cp.device)
            _lib.call("g4s_chart_points_sample_backward", cp.n, cp.height, cp.width, cp.n_points, _lib.ptr(cp.ixy),
                      _lib.ptr(cp._taps), _lib.ptr(cp._starts), _lib.ptr(g), _lib.ptr(out), _lib.stream(cp.device))
        shape, dtype = ctx.meta
        return out.reshape(shape).to(dtype), None


class ChartPoints:
    """The packed points of n charts of height x width with everything that depends on the points and cameras alone: offsets
    int32 [n+1], chart int32 [N], view_depths [N] (z in the point's chart), ixy [N,2] (pixel coordinates; a clipped point at
    (-2, -2)), clipped bool [N] and, built on first use by a backward, the inverted index (tap ids per pixel)."""

    def __init__(self, cameras, points, height, width):
        self.cameras = cameras
        cams = camera_list(cameras)
        lists = _point_lists(points, len(cams))
        height, width = int(height), int(width)
        if height <= 0 or width <= 0:
            raise ValueError(f"chart points: height, width must be positive (got {height} x {width})")
        dev = None
        for c, p in enumerate(lists):
            dev = same_device(p, dev, f"points[{c}]")
        self.device, self.n, self.height, self.width = dev, len(cams), height, width
        self.counts = [int(p.size(0)) for p in lists]
        self.n_points = sum(self.counts)
        N = self.n_points
        lib = _lib.load()
        self._workspace_bytes = lib.g4s_chart_points_workspace(self.n, height, width, N)
        if self._workspace_bytes == 0:
            raise ValueError(f"chart points: n = {self.n}, H W = {height} x {width}, N = {N} is beyond n <= 65535, n H W <= 2^31 - 2, N <= 2^29 - 1")
        with torch.cuda.device(dev):
            self.points = torch.cat([p.detach().float() for p in lists]).contiguous() if N else torch.zeros((0, 3), device=dev)
            self.offsets = torch.as_tensor(np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32), device=dev)
            self._cams = torch.as_tensor(camera_records(cams), device=dev)
            self.chart = torch.empty(N, dtype=torch.int32, device=dev)
            self.view_depths = torch.empty(N, dtype=torch.float32, device=dev)
            self.ixy = torch.empty((N, 2), dtype=torch.float32, device=dev)
            clipped = torch.empty(N, dtype=torch.uint8, device=dev)
            _lib.call("g4s_chart_points_project", self.n, height, width, _lib.ptr(self._cams), N, _lib.ptr(self.points),
                      _lib.ptr(self.offsets), _lib.ptr(self.chart), _lib.ptr(self.view_depths), _lib.ptr(self.ixy), _lib.ptr(clipped),
                      _lib.stream(dev))
        self.clipped = clipped.bool()
        self._taps = self._starts = None

    def build_index(self):
        """The inverted index of the backward, once: taps int32 [4N] ordered by (pixel, point, corner), starts int32 [nHW+1]."""
        if self._starts is not None:
            return
        dev = self.device
        nws = _lib.load().g4s_chart_points_index_workspace(self.n, self.height, self.width, self.n_points)
        with torch.cuda.device(dev):
            taps = torch.empty(4 * self.n_points, dtype=torch.int32, device=dev)
            starts = torch.empty(self.n * self.height * self.width + 1, dtype=torch.int32, device=dev)
            launch(dev, "g4s_chart_points_index", self.n, self.height, self.width, self.n_points, _lib.ptr(self.chart),
                   _lib.ptr(self.ixy), _lib.ptr(taps), _lib.ptr(starts), workspace=nws)
        self._taps, self._starts = taps, starts

    def _maps(self, maps, name):
        return maps_of_shape(maps, name, (self.n, self.height, self.width), self.device)

    def sample(self, maps):
        """(values float32 [N], fov bool [N]) of maps [n,H,W] under the points: bilinear, zeros padding, fov = value > 0.
        Differentiable in `maps`."""
        return _Sample.apply(self._maps(maps, "maps"), self)

    def split(self, values):
        """Per-chart views of a packed [N, ...] tensor."""
        return list(torch.split(values, self.counts))


@torch.no_grad()
def fit_disparities(disparities, chart_points, use_fov_mask=False, return_counts=False):
    """coeffs float32 [n,2] = (alpha, beta) per chart on the device, fitted so that 1 / (alpha + beta disparity) meets the view
    depths of the chart's points (float64 sums in a fixed order, no read-back).  A chart with fewer than two usable points
    gives NaN or inf, as IEEE does; that is no error."""
    cp = chart_points
    values, _fov = cp.sample(cp._maps(disparities, "disparities"))
    with torch.cuda.device(cp.device):
        coeffs = torch.empty((cp.n, 2), dtype=torch.float32, device=cp.device)
        counts = torch.empty(cp.n, dtype=torch.int32, device=cp.device)
        launch(cp.device, "g4s_chart_points_fit", cp.n, cp.n_points, _lib.ptr(cp.offsets), max(cp.counts), _lib.ptr(cp.view_depths),
               _lib.ptr(values), int(bool(use_fov_mask)), _lib.ptr(coeffs), _lib.ptr(counts), workspace=cp._workspace_bytes)
    return (coeffs, counts) if return_counts else coeffs


@torch.no_grad()
def aligned_depths(disparities, coeffs, scale=1.0):
    """scale * (1 / (alpha + beta disparity)) [n,H,W] with coeffs [n,2] on the device."""
    dev, d = stack(disparities, "disparities")
    d = f32(d)
    n, H, W = d.shape
    if not isinstance(coeffs, torch.Tensor) or tuple(coeffs.shape) != (n, 2):
        raise ValueError(f"coeffs must be a [{n},2] tensor (got {tuple(getattr(coeffs, 'shape', ()))})")
    same_device(coeffs, dev, "coeffs")
    c = f32(coeffs)
    with torch.cuda.device(dev):
        out = torch.empty_like(d)
        _lib.call("g4s_chart_points_apply", n, H, W, _lib.ptr(d), _lib.ptr(c), float(scale), _lib.ptr(out), _lib.stream(dev))
    return out


@torch.no_grad()
def view_depths_of_point_maps(cameras, point_maps, scale=1.0):
    """z of scale * P in each point map's own view: [n,H,W] from point maps [n,H,W,3] (a tensor or a list of [H,W,3])."""
    cams = camera_list(cameras)
    if not isinstance(point_maps, torch.Tensor):
        point_maps = torch.stack(list(point_maps))
    if point_maps.dim() != 4 or point_maps.size(-1) != 3:
        raise ValueError(f"point_maps must be [n,H,W,3] (got {tuple(point_maps.shape)})")
    if point_maps.size(0) != len(cams):
        raise ValueError(f"{len(cams)} views but {point_maps.size(0)} point maps")
    dev = same_device(point_maps, None, "point_maps")
    p = f32(point_maps)
    n, H, W = p.shape[:3]
    with torch.cuda.device(dev):
        rec = torch.as_tensor(camera_records(cams), device=dev)
        out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        _lib.call("g4s_chart_points_view_depths", n, _lib.ptr(rec), n * H * W, H * W, _lib.ptr(None), _lib.ptr(p), float(scale),
                  _lib.ptr(out), _lib.stream(dev))
    return out


class _PointLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depths, confidence, cp, cw):
        d, c, ctx.meta = depths_and_confidence(depths, confidence)
        with torch.cuda.device(cp.device):
            out = torch.empty(1, dtype=torch.float32, device=cp.device)
            launch(cp.device, "g4s_chart_points_loss_forward", cp.n, cp.height, cp.width, cp.n_points, _lib.ptr(cp.chart),
                   _lib.ptr(cp.ixy), _lib.ptr(cp.view_depths), _lib.ptr(d), _lib.ptr(c), float(cw), _lib.ptr(out),
                   workspace=cp._workspace_bytes)
        ctx.save_for_backward(d, c)
        ctx.cp, ctx.cw = cp, cw
        return out[0]

    @staticmethod
    def backward(ctx, g):
        d, c = ctx.saved_tensors
        cp = ctx.cp
        cp.build_index()
        with torch.cuda.device(cp.device):
            g1 = g.detach().float().reshape(1).contiguous()  # the cotangent stays on the device
            dd = torch.empty_like(d)
            dc = None if c is None else torch.empty_like(c)
            launch(cp.device, "g4s_chart_points_loss_backward", cp.n, cp.height, cp.width, cp.n_points, _lib.ptr(cp.chart),
                   _lib.ptr(cp.ixy), _lib.ptr(cp.view_depths), _lib.ptr(d), _lib.ptr(c), float(ctx.cw), _lib.ptr(cp._taps),
                   _lib.ptr(cp._starts), _lib.ptr(g1), _lib.ptr(dd), _lib.ptr(dc), workspace=cp._workspace_bytes)
        return (*grads_like(dd, dc, ctx.meta), None, None)


def point_reference_loss(depths, chart_points, confidence=None, confidence_weighting=0.2, masks=None):
    """The depth term of ParallelAligner.loss with 3D points as the reference, a 0-d tensor: the mean over all points of
    |s_p - z_p|, or of k_p |s_p - z_p| - confidence_weighting log k_p with a confidence, s_p and k_p being `depths` and
    `confidence` [n,H,W] sampled under point p and z_p its view depth.  Differentiable in both maps; value and gradients are
    bit-identical from run to run.  masks are refused: the reference's `masks * diff` cannot broadcast against points."""
    if masks is not None:
        raise ValueError("point reference loss: masks are not supported with points (the reference's masks * diff cannot broadcast)")
    cp = chart_points
    if not isinstance(cp, ChartPoints):
        raise ValueError("point reference loss: chart_points must be a ChartPoints")
    if cp.n_points == 0:
        raise ValueError("point reference loss: no points (a mean over none)")
    d = cp._maps(depths, "depths")
    c = None if confidence is None else cp._maps(confidence, "confidence")
    return _PointLoss.apply(d, c, cp, float(confidence_weighting))


# ---- the reference's names, one chart at a time ------------------------------------------------------------------------------
def get_points_depth_in_depthmap(pts, depthmap, camera, padding_mode="zeros"):
    """(map_z [N], fov_mask bool [N]) of one chart: depthmap [H,W] or [H,W,1] sampled under pts [N,3] seen by `camera`."""
    if padding_mode != "zeros":
        raise NotImplementedError(f"chart points: padding_mode {padding_mode!r} is not supported (zeros only)")
    if not isinstance(depthmap, torch.Tensor) or depthmap.dim() not in (2, 3) or (depthmap.dim() == 3 and depthmap.size(-1) != 1):
        raise ValueError(f"depthmap must be [H,W] or [H,W,1] (got {tuple(getattr(depthmap, 'shape', ()))})")
    H, W = depthmap.shape[:2]
    return ChartPoints([camera], [pts], H, W).sample(depthmap.reshape(1, H, W))


def fit_depth_to_point_cloud(disp, pts, cameras, camera_idx, return_alpha_beta=False, use_fov_mask=False, image=None,
                             pt_colors=None, use_rasterizer=False):
    """The reference's fit of one chart: 1 / (alpha + beta disp) [H,W], or (alpha, beta) as 0-d device tensors (the reference
    reads them back with .item())."""
    if use_rasterizer:
        raise NotImplementedError("Rasterizer implementation is not really satisfactory yet.")
    if image is not None and pt_colors is not None:
        raise NotImplementedError("Color weighting implementation is not satisfactory yet.")
    cams = camera_list(cameras)
    if not 0 <= int(camera_idx) < len(cams):
        raise ValueError(f"camera_idx {camera_idx} is not in range({len(cams)})")
    if not isinstance(disp, torch.Tensor) or disp.dim() != 2:
        raise ValueError(f"disp must be [H,W] (got {tuple(getattr(disp, 'shape', ()))})")
    H, W = disp.shape
    cp = ChartPoints([cams[int(camera_idx)]], [pts], H, W)
    coeffs = fit_disparities(disp[None], cp, use_fov_mask)
    if return_alpha_beta:
        return coeffs[0, 0], coeffs[0, 1]
    return aligned_depths(disp[None], coeffs)[0]


# ---- from SfM output and mono disparities to the aligner's inputs --------------------------------------------------------------
def rescale_cameras(cameras, factor):
    """rescale_cameras' rule on the matrices: the translation times the factor.  world_view_transform's last row is scaled in
    double, full_proj_transform is the product with the camera's projection_matrix (taken from full_proj_transform where the
    camera has none); the other attributes a chart unit reads are copied."""
    out = []
    for cam in camera_list(cameras):
        wvt = np.asarray(to_np(cam.world_view_transform), np.float64).reshape(4, 4)
        if hasattr(cam, "projection_matrix"):
            proj = np.asarray(to_np(cam.projection_matrix), np.float64).reshape(4, 4)
        else:
            proj = np.linalg.inv(wvt) @ np.asarray(to_np(cam.full_proj_transform), np.float64).reshape(4, 4)
        scaled = wvt.copy()
        scaled[3, :3] *= float(factor)
        new = SimpleNamespace(world_view_transform=scaled.astype(np.float32), projection_matrix=proj.astype(np.float32),
                              full_proj_transform=(scaled @ proj).astype(np.float32))
        for k in ("FoVx", "FoVy", "image_width", "image_height", "znear", "zfar", "image_name", "uid", "colmap_id"):
            if hasattr(cam, k):
                setattr(new, k, getattr(cam, k))
        out.append(new)
    return out


def build_charts(cameras, disparities, sfm_points, point_maps=None, target_scale=5.0, use_fov_mask=False):
    """get_pointmap_from_sfm_data_with_depthanything and the rescaling of scripts/align_charts.py, for all charts at once:
    returns (rescaled cameras, initial_depths [n,H,W], reference, scale_factor).  `reference` is reference_depths [n,H,W] when
    point maps [n,H,W,3] are given (the view depths of the scaled maps) and otherwise the ChartPoints of the scaled SfM points:
    chart_aligner.align_charts takes either as its third argument."""
    cams = camera_list(cameras)
    dev, disp = stack(disparities, "disparities")
    n, H, W = disp.shape
    if n != len(cams):
        raise ValueError(f"{len(cams)} views but {n} disparities")
    lists = _point_lists(sfm_points, n)
    factor = float(target_scale) / spatial_extent(cams)
    scaled_cams = rescale_cameras(cams, factor)
    cp = ChartPoints(cams, lists, H, W)
    coeffs = fit_disparities(disp, cp, use_fov_mask)
    initial = aligned_depths(disp, coeffs, factor)
    if point_maps is not None:
        reference = view_depths_of_point_maps(scaled_cams, point_maps, factor)
    else:
        reference = ChartPoints(scaled_cams, [p.detach().float() * factor for p in lists], H, W)
    return scaled_cams, initial, reference, factor
