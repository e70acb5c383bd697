"""Chart matcher of MAtCha's chart alignment (include/g4s_losses.h, "Chart matcher"; csrc/chart_match.hip).

The stage the reference runs before everything else (scripts/align_charts.py -> ParallelAligner.optimize): which pixel of
which chart agrees in depth with which other chart (matcha/dm_modules/matcher_3d.py Matcher3D), and the matching loss that
every one of its 1000 iterations evaluates over all n^2 H W pairs.  Here the matches are one bit per pair and the loss and
its gradient are fused: nothing of size [n,n,H,W] exists unless it is asked for.  Everything goes through the library;
there is no torch path.

A camera is anything with world_view_transform, projection_matrix and full_proj_transform in the reference's row-vector
convention (the reference's GSCamera); `cameras` is a list of them or a wrapper with `.gs_cameras`.  Depth maps are device
tensors, all of one size: a stacked [n,H,W] tensor or a list of [H,W] / [1,H,W] maps.  INTEGRATION.md section U lists the
differences from the reference.
"""
import numpy as np
import torch

from . import _lib
from ._charts import camera_list, f32, maps_of_shape, spatial_extent, stack  # noqa: F401 (spatial_extent: public here)
from ._device import hip_device, launch, same_device, to_np
from .visibility import ray_record

MATCHING_THR_FACTOR = 1.0 / 20.0  # the reference's matching_thr_factor
MAX_TERMS = 1 << 26               # the range limit of the backward: n H W max(1, weight_max)


def camera_records(cameras, width, height):
    """float32 [n,44]: per view the ray record (visibility.ray_record: o[3], D[3][3]), world_view_transform and
    projection_matrix, row-major -- the `cameras` argument of the library calls."""
    rows = []
    for cam in cameras:
        wvt = np.asarray(to_np(cam.world_view_transform), np.float32).reshape(16)
        proj = np.asarray(to_np(cam.projection_matrix), np.float32).reshape(16)
        rows.append(np.concatenate([ray_record(cam, width, height), wvt, proj]))
    return np.stack(rows).astype(np.float32)


class _MatchLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depths, matcher, weights, weight_max):
        m = matcher
        d = f32(depths)
        with torch.cuda.device(m.device):
            out = torch.empty(1, dtype=torch.float32, device=m.device)
            launch(m.device, "g4s_chart_match_loss_forward", m.n, m.height, m.width, _lib.ptr(m._cams), _lib.ptr(d),
                   _lib.ptr(m.words), _lib.ptr(weights), float(weight_max), _lib.ptr(out), workspace=m._workspace_bytes)
        ctx.save_for_backward(d, m.words)  # the bits of THIS forward, whatever match() does before the backward
        ctx.matcher, ctx.weights, ctx.weight_max, ctx.shape, ctx.dtype = m, weights, weight_max, depths.shape, depths.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        d, words = ctx.saved_tensors
        m = ctx.matcher
        with torch.cuda.device(m.device):
            g1 = g.detach().float().reshape(1).contiguous()
            grad = torch.empty_like(d)
            launch(m.device, "g4s_chart_match_loss_backward", m.n, m.height, m.width, _lib.ptr(m._cams), _lib.ptr(d),
                   _lib.ptr(words), _lib.ptr(ctx.weights), float(ctx.weight_max), _lib.ptr(g1), _lib.ptr(grad),
                   workspace=m._workspace_bytes)
        return grad.reshape(ctx.shape).to(ctx.dtype), None, None, None


class ChartMatcher:
    """Matcher3D on the device.  `words` holds the matches as the library packs them: int32 [n,n,ceil(HW/32)] whose bits
    are the uint32 words of the contract (bit p mod 32 of word p // 32 for target i, source j, pixel p = y W + x)."""

    def __init__(self, cameras, reference_depths=None, reference_pts=None):
        self.cameras = cameras
        self._cam_list = camera_list(cameras)
        self.znear = 1e-6
        self.words = None
        self.matching_thr = None
        self.update_references(reference_pts=reference_pts, reference_depths=reference_depths)

    @torch.no_grad()
    def update_references(self, reference_pts=None, reference_depths=None):
        if reference_pts is None and reference_depths is None:
            raise ValueError("Either reference_pts or reference_depths should be provided.")
        if reference_depths is None:
            # the reference's transform_points(reference_pts)[..., 2]: O(n H W), stays torch
            dev, pts = _stack_points(reference_pts)
            wvt = torch.as_tensor(np.stack([np.asarray(to_np(c.world_view_transform), np.float32).reshape(4, 4) for c in self._cam_list]),
                                  device=dev)
            if pts.size(0) != wvt.size(0):
                raise ValueError(f"{wvt.size(0)} views but {pts.size(0)} reference_pts")
            reference_depths = (torch.cat([pts, torch.ones_like(pts[..., :1])], dim=-1).flatten(1, 2) @ wvt)[..., 2].reshape(pts.shape[:3])
        dev, depths = stack(reference_depths, "reference_depths")
        n, H, W = depths.shape
        if n != len(self._cam_list):
            raise ValueError(f"{len(self._cam_list)} views but {n} reference_depths")
        nws = _lib.load().g4s_chart_match_workspace(n, H, W)
        if nws == 0:
            raise ValueError(f"chart matcher: n H W = {n * H * W} is empty or beyond the range limit n H W max(1, weight_max) <= 2^26")
        self.device, self.n, self.height, self.width = dev, n, H, W
        self.n_charts = n
        self._workspace_bytes = nws
        self.reference_depths = f32(depths)
        self._cams = torch.as_tensor(camera_records(self._cam_list, W, H), device=dev)
        self.words, self._matches, self._errors = None, None, None

    @torch.no_grad()
    def match(self, matching_thr=None, normal_threshold=None):
        """The matches of the reference depths under `matching_thr` (None: spatial_extent(cameras) / 20)."""
        if normal_threshold is not None:
            raise NotImplementedError("Normal threshold not implemented yet.")
        if matching_thr is None:
            matching_thr = MATCHING_THR_FACTOR * spatial_extent(self._cam_list)
        self.matching_thr = float(matching_thr)
        nwords = (self.height * self.width + 31) // 32
        self.words = torch.empty((self.n, self.n, nwords), dtype=torch.int32, device=self.device)
        self._matches, self._errors = None, None
        self._run(self.reference_depths, self.words, None, 0, None)

    def _run(self, depths, words, errors, raw, fov):
        with torch.cuda.device(self.device):  # a stream and no workspace: called like the mesh filters, not through launch()
            _lib.call("g4s_chart_match", self.n, self.height, self.width, _lib.ptr(self._cams), _lib.ptr(depths),
                      float(self.matching_thr if self.matching_thr is not None else 0.0), _lib.ptr(words), _lib.ptr(errors),
                      int(raw), _lib.ptr(fov), _lib.stream(self.device))
            torch.cuda.current_stream(self.device).synchronize()

    def _need_match(self):
        if self.words is None:
            raise RuntimeError("chart matcher: call match() first")

    @property
    def reference_matches(self):
        """bool [n,n,H,W], expanded from `words` on first use."""
        self._need_match()
        if self._matches is None:
            shifts = torch.arange(32, dtype=torch.int32, device=self.device)
            bits = (self.words[..., None] >> shifts) & 1
            N = self.height * self.width
            self._matches = bits.reshape(self.n, self.n, -1)[:, :, :N].bool().reshape(self.n, self.n, self.height, self.width)
        return self._matches

    @property
    def reference_errors(self):
        """float [n,n,H,W]: |z - sampled| of the reference depths, 1e8 outside the fov; computed on request."""
        self._need_match()
        if self._errors is None:
            self._errors = torch.empty((self.n, self.n, self.height, self.width), dtype=torch.float32, device=self.device)
            self._run(self.reference_depths, None, self._errors, 0, None)
        return self._errors

    def _current(self, depths):
        return maps_of_shape(depths, "depths", (self.n, self.height, self.width), self.device, "the references' shape")

    @torch.no_grad()
    def compute_reprojection_errors(self, depths=None, points=None):
        """(errors float [n,n,H,W], fov_mask bool [n,n,H,W]) at `depths`, dense: for parity with the reference and for
        small inputs (the loss never forms them)."""
        if points is not None:
            raise NotImplementedError("chart matcher: compute_reprojection_errors takes depths, not points")
        if depths is None:
            raise ValueError("Either depths or points should be provided.")
        d = f32(self._current(depths))
        shape = (self.n, self.n, self.height, self.width)
        errors = torch.empty(shape, dtype=torch.float32, device=self.device)
        fov = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self._run(d, None, errors, 1, fov)
        return errors, fov.bool()

    def loss(self, depths, weights=None, weight_max=None):
        """The matching loss (errors * fov_mask * reference_matches [* weights[None]]).mean() at `depths` as a 0-d tensor,
        differentiable in `depths` only; the matches are those of the last match().  weights [n,H,W] (the source chart's
        confidence) are treated as detached.  weight_max bounds |weights| for the backward's fixed-point sums; None reads
        weights.abs().max() back once per call (pass it to stay capturable in a HIP graph).  Value and gradient both use
        the weights clamped to [-weight_max, weight_max], so a bound that is too small changes the loss, never the
        agreement of the two.  Bit-identical from run to
        run, value and gradient."""
        self._need_match()
        d = self._current(depths)
        if weights is not None:
            weights = f32(maps_of_shape(weights, "weights", d.shape, self.device, "the depths' shape"))
            if weight_max is None:
                weight_max = float(weights.abs().max())
        else:
            weight_max = 1.0
        terms = self.n * self.height * self.width * max(1.0, float(weight_max))
        if not terms <= MAX_TERMS:
            raise ValueError(f"chart matcher: n H W max(1, weight_max) = {terms:.6g} is beyond the range limit 2^26 of the "
                             "backward's fixed-point sums")
        return _MatchLoss.apply(d, self, weights, float(weight_max))


def _stack_points(pts):
    if not isinstance(pts, torch.Tensor):
        pts = torch.stack(list(pts))
    if pts.dim() != 4 or pts.size(-1) != 3:
        raise ValueError(f"reference_pts must be [n,H,W,3] (got {tuple(pts.shape)})")
    dev = same_device(pts, None, "reference_pts")
    return hip_device(dev), pts.detach().float()
