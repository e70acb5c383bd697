"""The depth, gradient, normal and curvature terms of MAtCha's chart alignment (include/g4s_losses.h, "Chart alignment
losses"; csrc/chart_align.hip).

ParallelAligner.optimize (matcha/dm_scene/parallel_aligner.py) evaluates these terms in every one of its 1000 iterations over
all n charts: it back-projects them, slices, crosses and normalises [n,H,W,3] tensors, pads and differences them, and keeps
every intermediate for autograd.  Here the four means come from one library call and both gradients from a second; the
matching loss, the last default term, is chart_match.ChartMatcher.loss.  Everything goes through the library; there is no
torch path.

A camera is anything with world_view_transform and full_proj_transform in the reference's row-vector convention (the
reference's GSCamera); `cameras` is a list of them or a wrapper with `.gs_cameras`, as for the matcher.  Depth maps are
device tensors of one size: a stacked [n,H,W] tensor or a list of [H,W] / [1,H,W] maps.  INTEGRATION.md section V lists the
differences from the reference.
"""
import numpy as np
import torch

from . import _lib
from ._charts import camera_list, depths_and_confidence, f32, grads_like, maps_of_shape, stack
from ._device import launch
from .visibility import ray_record

GRADIENT, NORMAL, CURVATURE = 1, 2, 4  # G4S_CHART_ALIGN_*


def ray_records(cameras, width, height):
    """float32 [n,12]: the ray record (visibility.ray_record: o[3], D[3][3]) of each view -- the `cameras` argument of the
    library calls."""
    return np.stack([ray_record(cam, width, height) for cam in cameras]).astype(np.float32)


def _workspace_bytes(n, H, W):
    nws = _lib.load().g4s_chart_align_workspace(n, H, W)
    if nws == 0:
        raise ValueError(f"chart align: [n,H,W,3] = [{n},{H},{W},3] is empty or has 2^31 elements or more")
    return nws


def _normals_call(dev, n, H, W, cams, depths, normals, curv):
    with torch.cuda.device(dev):  # a stream and no workspace
        _lib.call("g4s_chart_align_normals", n, H, W, _lib.ptr(cams), _lib.ptr(depths), _lib.ptr(normals), _lib.ptr(curv),
                  _lib.stream(dev))


@torch.no_grad()
def depth2normal_parallel(depths, cameras):
    """The reference's depth2normal_parallel: [n,H,W,3] float32, the normalised cross product of the central point
    differences at the interior pixels, exactly 0 on the border."""
    dev, d = stack(depths, "depths")
    d = f32(d)
    n, H, W = d.shape
    cam_list = camera_list(cameras)
    if len(cam_list) != n:
        raise ValueError(f"{len(cam_list)} views but {n} depths")
    _workspace_bytes(n, H, W)  # the size check
    with torch.cuda.device(dev):
        cams = torch.as_tensor(ray_records(cam_list, W, H), device=dev)
        normals = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
    _normals_call(dev, n, H, W, cams, d, normals, None)
    return normals


@torch.no_grad()
def normal2curv_parallel(normals, mask=None):
    """The reference's normal2curv_parallel for normals [n,H,W,3] and a mask that leaves the stencil whole (all ones, as
    optimize passes it): [n,H,W,1], the L1 norm of the replicate-padded Laplacian of the normals, times `mask` where one is
    given (it broadcasts as the reference's final product does; a mask inside the stencil is not supported)."""
    if not isinstance(normals, torch.Tensor) or normals.dim() != 4 or normals.size(-1) != 3:
        raise ValueError(f"normals must be a [n,H,W,3] tensor (got {tuple(getattr(normals, 'shape', ()))})")
    dev, _ = stack(normals[..., 0], "normals")
    nu = f32(normals)
    n, H, W = nu.shape[:3]
    _workspace_bytes(n, H, W)
    with torch.cuda.device(dev):
        curv = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    _normals_call(dev, n, H, W, None, None, nu, curv)
    curv = curv[..., None]
    if mask is not None:
        if not bool(mask.all()):
            raise NotImplementedError("normal2curv_parallel: only a mask of ones (the stencil is not masked)")
        curv = curv * mask
    return curv


class _Terms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depths, confidence, losses, reference_depths, masks, gradient_masks, flags):
        a = losses
        d, c, ctx.meta = depths_and_confidence(depths, confidence)
        args = (a.n, a.height, a.width, _lib.ptr(a._cams), _lib.ptr(d), _lib.ptr(reference_depths), _lib.ptr(c), _lib.ptr(masks),
                _lib.ptr(a._initial_depths), _lib.ptr(gradient_masks), _lib.ptr(a.initial_normals), _lib.ptr(a._initial_curv),
                float(a.confidence_weighting), int(flags))
        with torch.cuda.device(a.device):
            out = torch.empty(4, dtype=torch.float32, device=a.device)
            launch(a.device, "g4s_chart_align_forward", *args, _lib.ptr(out), workspace=a._workspace_bytes)
        ctx.save_for_backward(d, c, reference_depths, masks, gradient_masks)
        ctx.losses, ctx.flags = a, flags
        return out

    @staticmethod
    def backward(ctx, g):
        d, c, reference_depths, masks, gradient_masks = ctx.saved_tensors
        a = ctx.losses
        with torch.cuda.device(a.device):
            g4 = g.detach().float().reshape(4).contiguous()  # the cotangent stays on the device
            dd = torch.empty_like(d)
            dc = None if c is None else torch.empty_like(c)
            launch(a.device, "g4s_chart_align_backward", a.n, a.height, a.width, _lib.ptr(a._cams), _lib.ptr(d),
                   _lib.ptr(reference_depths), _lib.ptr(c), _lib.ptr(masks), _lib.ptr(a._initial_depths), _lib.ptr(gradient_masks),
                   _lib.ptr(a.initial_normals), _lib.ptr(a._initial_curv), float(a.confidence_weighting), int(ctx.flags),
                   _lib.ptr(g4), _lib.ptr(dd), _lib.ptr(dc), workspace=a._workspace_bytes)
        return (*grads_like(dd, dc, ctx.meta), None, None, None, None, None)


class AlignmentLosses:
    """The loss terms of ParallelAligner.optimize that are O(n H W), on the device.  `initial_depths` are the aligner's
    `_depths`: the gradient term compares with them, and `initial_normals` [n,H,W,3] and `initial_curvatures` [n,H,W,1]
    (the reference's attribute names; its curvatures carry three equal channels) are made from them once, here."""

    def __init__(self, cameras, initial_depths, confidence_weighting=0.2):
        self.cameras = cameras
        cam_list = camera_list(cameras)
        dev, d0 = stack(initial_depths, "initial_depths")
        n, H, W = d0.shape
        if n != len(cam_list):
            raise ValueError(f"{len(cam_list)} views but {n} initial_depths")
        self._workspace_bytes = _workspace_bytes(n, H, W)
        self.device, self.n, self.height, self.width = dev, n, H, W
        self.confidence_weighting = float(confidence_weighting)
        self._initial_depths = f32(d0)
        with torch.cuda.device(dev):
            self._cams = torch.as_tensor(ray_records(cam_list, W, H), device=dev)
            self.initial_normals = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
            self._initial_curv = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        _normals_call(dev, n, H, W, self._cams, self._initial_depths, self.initial_normals, self._initial_curv)
        self.initial_curvatures = self._initial_curv[..., None]

    def _map(self, t, name, shape=None):
        """An optional [n,H,W] input (detached, float32, contiguous), or one of `shape`."""
        if t is None:
            return None
        if isinstance(t, torch.Tensor) and t.dtype in (torch.bool, torch.uint8):
            t = t.float()
        return f32(maps_of_shape(t, name, (self.n, self.height, self.width) if shape is None else shape, self.device))

    def terms(self, depths, reference_depths, confidence=None, masks=None, gradient_masks=None, use_gradient_loss=False,
              use_normal_loss=True, use_curvature_loss=True):
        """float32 [4]: the UNWEIGHTED means of the depth, gradient, normal and curvature terms at `depths`, differentiable in
        `depths` and `confidence` (the activated 1 + exp(_confidence); None: the depth term is |d - r|).  A term that is
        switched off is exactly 0.  reference_depths is the target, the depth-map form of optimize's reference_data; masks
        [n,H,W] and gradient_masks [n,H-1,W-1] (applied per view) are treated as detached.  Value and gradients are
        bit-identical from run to run."""
        shape = (self.n, self.height, self.width)
        d = maps_of_shape(depths, "depths", shape, self.device, "the initial depths' shape")
        if confidence is not None:
            confidence = maps_of_shape(confidence, "confidence", shape, self.device, "the depths' shape")
        flags = (GRADIENT if use_gradient_loss else 0) | (NORMAL if use_normal_loss else 0) | (CURVATURE if use_curvature_loss else 0)
        if use_gradient_loss and (self.height < 2 or self.width < 2):
            raise ValueError(f"chart align: the gradient term needs H >= 2 and W >= 2 (got {self.height} x {self.width}; the "
                             "reference's mean over no differences is NaN)")
        gm = self._map(gradient_masks, "gradient_masks", (self.n, self.height - 1, self.width - 1)) if use_gradient_loss else None
        return _Terms.apply(d, confidence, self, self._map(reference_depths, "reference_depths"), self._map(masks, "masks"), gm, flags)

    def loss(self, depths, reference_depths, confidence=None, masks=None, gradient_masks=None, use_gradient_loss=True,
             use_normal_loss=True, use_curvature_loss=False, gradient_loss_weight=10., normal_loss_weight=2.,
             curvature_loss_weight=1.):
        """The weighted sum of the four terms as a 0-d tensor, with optimize's keyword names and defaults."""
        t = self.terms(depths, reference_depths, confidence, masks, gradient_masks, use_gradient_loss, use_normal_loss,
                       use_curvature_loss)
        return ((t[0] + float(gradient_loss_weight) * t[1]) + float(normal_loss_weight) * t[2]) + float(curvature_loss_weight) * t[3]
