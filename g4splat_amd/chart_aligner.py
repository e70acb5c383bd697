"""MAtCha's chart alignment end to end: ParallelAligner.optimize (matcha/dm_scene/parallel_aligner.py:552-887) and
align_charts_in_parallel (matcha/dm_trainers/charts_alignment.py) on the device.

ChartAligner holds the reference's trainable parameters under the reference's names -- charts_encoding.*, depth_encoding.encodings,
_confidence, deformation.mlp.* -- and composes one iteration from the library's pieces:

    confidence kernel (g4s_chart_confidence_*)  ->  weighted deformation with both encoding regularisers
    (chart_deform.ChartDeformation.deformed_depths_and_regularizers)  ->  chart_align.AlignmentLosses.terms  ->
    chart_match.ChartMatcher.loss  ->  total_loss  ->  backward  ->  optim.FusedAdam.step  ->  zero grads

Nothing in an iteration allocates outside torch's caching allocator, synchronises or reads back, so with graph=True the iteration is
captured once in a HIP graph and replayed; learning rates change through FusedAdam.sync_lr(), and after a refresh of the
matches (matching_update_iters) the iteration is captured again.  INTEGRATION.md section X lists the differences from the reference."""
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .chart_align import AlignmentLosses
from .chart_deform import (ChartDeformation, ChartsEncodingParams, DepthEncodingParams, MLPParams,  # noqa: F401 (re-exported)
                           MultiResChartsEncodingParams)
from ._charts import camera_list, f32, maps_of_shape, spatial_extent
from .chart_match import MATCHING_THR_FACTOR, ChartMatcher
from .chart_points import ChartPoints, point_reference_loss
from .optim import FusedAdam

# the `alignment:` blocks of the reference's configs/charts_alignment/default.yaml and strong.yaml, as values
_COMMON = dict(
    use_learnable_depth_encoding=True, learnable_depth_encoding_mode="add", predict_in_disparity_space=False,
    use_learnable_confidence=True, use_meta_mlp=False, use_lora_mlp=False, lora_rank=4, n_lora_layers=2,
    use_multi_res_charts_encoding=True, n_iterations=1000, encodings_lr=0.01, mlp_lr=0.001, confidence_lr=0.001,
    lr_update_iters=[1000], lr_update_factor=0.1, use_gradient_loss=False, gradient_loss_weight=50., use_hessian_loss=False,
    hessian_loss_weight=100., use_normal_loss=True, normal_loss_weight=4., use_curvature_loss=True, curvature_loss_weight=1.,
    use_matching_loss=True, matching_update_iters=None, matching_loss_weight=5., matching_thr_factor=0.05,
    use_confidence_in_matching_loss=False, use_reprojection_loss=False, reprojection_loss_weight=2., reprojection_loss_power=0.5,
    chart_encodings_norm_loss_weight=2., total_variation_on_depth_encodings_weight=5.)
ALIGNMENT_CONFIGS = {
    "default": dict(_COMMON, regularize_chart_encodings_norms=False, use_total_variation_on_depth_encodings=False,
                    weight_encodings_with_confidence=False),
    "strong": dict(_COMMON, regularize_chart_encodings_norms=True, use_total_variation_on_depth_encodings=True,
                   weight_encodings_with_confidence=True),
}

# the architecture keywords of ParallelAligner among a configuration's entries
ARCHITECTURE_KEYS = ("use_learnable_depth_encoding", "learnable_depth_encoding_mode", "predict_in_disparity_space",
                     "use_learnable_confidence", "use_meta_mlp", "use_lora_mlp", "lora_rank", "n_lora_layers",
                     "use_multi_res_charts_encoding", "weight_encodings_with_confidence")
TERM_NAMES = ("loss", "depth_loss", "grad", "hess", "normal", "curv", "matching", "ce_norm", "de_tv")  # the reference's log keys
ADAM_STEP_BOUND = 3.2  # |one Adam update| <= lr (1 - beta1) / sqrt(1 - beta2) = 3.17 lr at the default betas


def total_loss(terms, reg, matching, weights, hessian=None):
    """The reference's weighted sum (parallel_aligner.py:757-819), in its order: the depth term, then each further term times
    its weight.  terms: the four means of AlignmentLosses.terms (depth, gradient, normal, curvature); reg: the two encoding
    regularisers (norm, total variation); matching, hessian: scalars or None.  weights: a mapping with the keys gradient,
    hessian, normal, curvature, matching, norm, tv; a missing key or a None switches the term off (it is not added, as in the
    reference).  Works on tensors, numpy scalars and floats alike; every product and sum is one operation of the inputs' type."""
    w = lambda k: weights.get(k)  # noqa: E731
    loss = terms[0]
    if w("gradient") is not None:
        loss = loss + w("gradient") * terms[1]
    if w("hessian") is not None:
        loss = loss + w("hessian") * hessian
    if w("normal") is not None:
        loss = loss + w("normal") * terms[2]
    if w("curvature") is not None:
        loss = loss + w("curvature") * terms[3]
    if w("matching") is not None:
        loss = loss + w("matching") * matching
    if w("norm") is not None:
        loss = loss + w("norm") * reg[0]
    if w("tv") is not None:
        loss = loss + w("tv") * reg[1]
    return loss


def updates_learning_rate(name):
    """The groups optimize multiplies by lr_update_factor (parallel_aligner.py:738-742): every one but _confidence."""
    return name.endswith("encodings") or name.startswith("deformation")


class _Confidence(torch.autograd.Function):
    """conf = 1 + exp(raw) and, detached, the encoding weight 1 - exp(-(conf - 1)^2 / 2): one launch each way."""

    @staticmethod
    def forward(ctx, raw, want_weights):
        r = raw.detach().float().contiguous()
        dev = r.device
        with torch.cuda.device(dev):
            conf = torch.empty_like(r)
            w = torch.empty_like(r) if want_weights else None
            _lib.call("g4s_chart_confidence_forward", r.numel(), _lib.ptr(r), _lib.ptr(conf), _lib.ptr(w), _lib.stream(dev))
        ctx.save_for_backward(r)
        ctx.meta = (raw.shape, raw.dtype)
        if want_weights:
            ctx.mark_non_differentiable(w)
            return conf, w
        return conf

    @staticmethod
    def backward(ctx, g, *_unused):
        (r,) = ctx.saved_tensors
        dev = r.device
        with torch.cuda.device(dev):
            g = g.detach().float().contiguous()
            out = torch.empty_like(r)
            _lib.call("g4s_chart_confidence_backward", r.numel(), _lib.ptr(r), _lib.ptr(g), _lib.ptr(out), _lib.stream(dev))
        shape, dtype = ctx.meta
        return out.reshape(shape).to(dtype), None


def confidence_and_weights(raw, want_weights=True):
    """(1 + exp(raw), 1 - exp(-(conf - 1)^2 / 2)) on a HIP device; the weights carry no gradient (the reference detaches)."""
    if not isinstance(raw, torch.Tensor) or raw.device.type != "cuda":
        raise RuntimeError("chart aligner: the confidence needs a tensor on a HIP device (there is no CPU path)")
    return _Confidence.apply(raw, bool(want_weights))


def _is_points(reference_data, shape):
    """Whether reference_data is the reference's other form, 3D points per chart ([P,3] or [H,W,3] each), and not depth maps.
    (The reference decides by a last dimension of 3 alone, which takes charts three pixels wide for points.)"""
    first = reference_data[0]
    if first.dim() == 3:  # [H,W,3] points; [1,H,W] is a depth map with a leading one
        return first.shape[-1] == 3 and first.shape[0] != 1
    return first.dim() == 2 and first.shape[-1] == 3 and tuple(first.shape) != tuple(shape[1:])


class ChartAligner(torch.nn.Module):
    """ParallelAligner on the device.  Takes its architecture keywords; parameters live on the depths' device, and everything
    but construction, prepare_for_optimization and the host-side checks needs a HIP device."""

    def __init__(self, cameras, depths, charts_encoding_params=None, depth_encoding_params=None, mlp_params=None,
                 use_learnable_depth_encoding=True, learnable_depth_encoding_mode="add", use_learnable_confidence=True,
                 predict_in_disparity_space=False, use_meta_mlp=False, use_lora_mlp=False, lora_rank=4, n_lora_layers=2,
                 use_multi_res_charts_encoding=True, multi_res_charts_encoding_params=None, weight_encodings_with_confidence=False,
                 spatial_extent_override=None):
        super().__init__()
        if weight_encodings_with_confidence and not use_learnable_confidence:
            raise ValueError("Encodings cannot be weighted with confidence if confidence is not learnable.")
        deform = ChartDeformation(cameras, depths, charts_encoding_params, depth_encoding_params, mlp_params,
                                  use_learnable_depth_encoding, use_multi_res_charts_encoding, multi_res_charts_encoding_params,
                                  learnable_depth_encoding_mode, predict_in_disparity_space, use_meta_mlp, use_lora_mlp,
                                  spatial_extent_override=spatial_extent_override)
        object.__setattr__(self, "_deform", deform)  # not a sub-module: its parameters are registered here, under the reference's names
        self.cameras = cameras
        self.device, self.n, self.height, self.width = deform.device, deform.n, deform.height, deform.width
        self.use_learnable_confidence = bool(use_learnable_confidence)
        self.weight_encodings_with_confidence = bool(weight_encodings_with_confidence)
        self.use_learnable_depth_encoding = deform.use_learnable_depth_encoding
        self.use_multi_res_charts_encoding = deform.use_multi_res_charts_encoding
        self.charts_encoding = deform.charts_encoding
        self.deformation = deform.deformation
        if deform.depth_encoding is not None:
            self.depth_encoding = deform.depth_encoding
        if use_learnable_confidence:
            self._confidence = torch.nn.Parameter(torch.zeros((self.n, self.height, self.width), device=self.device))
        self.confidence_weighting = 0.2
        self._depths = deform._d0
        self._spatial_extent = spatial_extent(camera_list(cameras)) if spatial_extent_override is None else float(spatial_extent_override)
        self.losses = None  # AlignmentLosses, built on first use (it launches)
        self.matcher = None
        self.optimizer = None
        self.train_losses, self.loss_terms = [], []
        self.graph_captures = 0

    # ---- what the reference exposes ------------------------------------------------------------------------------------------
    @property
    def deformation_module(self):
        return self._deform

    def _hip(self):
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("chart aligner: needs the charts on a HIP device (there is no CPU path)")

    @property
    def confidence(self):
        """1 + exp(_confidence) [n,H,W], differentiable in _confidence."""
        self._hip()
        if not self.use_learnable_confidence:
            raise AttributeError("chart aligner: built without use_learnable_confidence")
        return confidence_and_weights(self._confidence, False)

    def _forward(self, norm=False, tv=False):
        """(confidence or None, deformed depths, reg [2]) at the current parameters"""
        conf = w = None
        if self.use_learnable_confidence:
            if self.weight_encodings_with_confidence:
                conf, w = confidence_and_weights(self._confidence, True)
            else:
                conf = confidence_and_weights(self._confidence, False)
        depths, reg = self._deform.deformed_depths_and_regularizers(w, norm=norm, tv=tv)
        return conf, depths, reg

    @property
    def deformed_depths(self):
        """The view-space depths of the deformed charts [n,H,W] at the current parameters (the reference's property reads the
        vertices stored by the last optimize; here it is always current), differentiable in every parameter."""
        self._hip()
        return self._forward()[1]

    @property
    def verts(self):
        """o + depth dir [n,H,W,3]: the deformed charts' points, from the deformed depths and each view's ray record."""
        d = self.deformed_depths
        rec = self._deform._cams
        o, D = rec[:, 0:3], rec[:, 3:12].reshape(self.n, 3, 3)
        yy, xx = torch.meshgrid(torch.arange(self.height, dtype=torch.float32, device=d.device),
                                torch.arange(self.width, dtype=torch.float32, device=d.device), indexing="ij")
        pix = torch.stack([xx, yy, torch.ones_like(xx)], -1)  # [H,W,3]
        dirs = torch.einsum("hwj,nkj->nhwk", pix, D)
        return o[:, None, None, :] + d[..., None] * dirs

    def reset_encodings(self):
        self._deform.reset_encodings()

    def reset_mlp(self, std=None):
        self._deform.reset_mlp(std)

    # ---- the optimiser -----------------------------------------------------------------------------------------------------------
    def parameter_groups(self, encodings_lr=1e-2, mlp_lr=1e-3, confidence_lr=1e-3):
        """The reference's groups (parallel_aligner.py:567-590) in its order with its names and learning rates: the chart
        encodings, the depth encoding, _confidence, then the remaining trainable parameters in registration order.  (The
        reference also lists its constant buffers _verts, _depths, ... there, which never receive a gradient.)"""
        named = dict(self.named_parameters())
        names = [k for k in named if k.startswith("charts_encoding.")]
        groups = [{"params": [named[k]], "lr": encodings_lr, "name": k} for k in names]
        if self.use_learnable_depth_encoding:
            groups.append({"params": [named["depth_encoding.encodings"]], "lr": encodings_lr, "name": "depth_encoding.encodings"})
        if self.use_learnable_confidence:
            groups.append({"params": [named["_confidence"]], "lr": confidence_lr, "name": "_confidence"})
        done = {g["name"] for g in groups}
        groups += [{"params": [p], "lr": mlp_lr, "name": k} for k, p in named.items() if k not in done]
        return groups

    def prepare_for_optimization(self, encodings_lr=1e-2, mlp_lr=1e-3, lr_update_iters=(300,), lr_update_factor=0.1,
                                 confidence_lr=1e-3, verbose=False):
        """Resets as the reference does (reset_encodings, then reset_mlp; _confidence is kept) and builds
        FusedAdam(lr=0, eps=1e-15, capturable=True) over parameter_groups().  On the host the optimiser is torch.optim.Adam
        with the same groups (FusedAdam has no CPU path); optimize() needs a HIP device."""
        self.reset_encodings()
        self.reset_mlp()
        groups = self.parameter_groups(encodings_lr, mlp_lr, confidence_lr)
        if torch.device(self.device).type == "cuda":
            self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15, capturable=True)
        else:
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        if verbose:
            print("=== Optimizable parameters ===")
            for g in self.optimizer.param_groups:
                print(g["name"], g["lr"], tuple(g["params"][0].shape))
        self.lr_update_iters, self.lr_update_factor = list(lr_update_iters), lr_update_factor

    def update_learning_rates(self):
        """The reference's rule at an iteration in lr_update_iters, then sync_lr() for a captured step."""
        for g in self.optimizer.param_groups:
            if updates_learning_rate(g["name"]):
                g["lr"] = g["lr"] * self.lr_update_factor
        if hasattr(self.optimizer, "sync_lr"):
            self.optimizer.sync_lr()

    # ---- one iteration ---------------------------------------------------------------------------------------------------------
    def _iteration(self, o):
        """One iteration under the options `o`; returns (the detached term vector in TERM_NAMES' order, the detached depths)."""
        conf, depths, reg = self._forward(o.weights.get("norm") is not None, o.weights.get("tv") is not None)
        terms = self.losses.terms(depths, o.reference, conf, o.masks, o.gradient_masks, o.weights.get("gradient") is not None,
                                  o.weights.get("normal") is not None, o.weights.get("curvature") is not None)
        if o.points is not None:
            # the all-zero masks make the fused depth term exactly 0 (value and gradient); the points' term takes its place
            terms = torch.cat([point_reference_loss(depths, o.points, conf, self.confidence_weighting).reshape(1), terms[1:]])
        matching = hessian = None
        if o.weights.get("matching") is not None:
            if o.confidence_in_matching:
                matching = self.matcher.loss(depths, conf.detach(), o.weight_max)
            else:
                matching = self.matcher.loss(depths)
        if o.weights.get("hessian") is not None:
            hessian = hessian_term(depths, self._depths)
        loss = total_loss(terms, reg, matching, o.weights, hessian)
        loss.backward()
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)
        zero = torch.zeros((), dtype=torch.float32, device=depths.device)
        vec = torch.stack([loss.detach(), terms[0].detach(), terms[1].detach(), zero if hessian is None else hessian.detach(),
                           terms[2].detach(), terms[3].detach(), zero if matching is None else matching.detach(), reg[0].detach(),
                           reg[1].detach()])
        return vec, depths.detach()

    def _state_tensors(self):
        params = [p for g in self.optimizer.param_groups for p in g["params"]]
        fresh = [p for p in params if len(self.optimizer.state[p]) == 0]
        tensors = list(params)
        for p in params:
            tensors += [v for v in self.optimizer.state[p].values() if torch.is_tensor(v)]
        return tensors, fresh

    def _capture(self, o, warmup=2):
        """Warm-up iterations on a side stream (lazy optimiser state, allocator pools), undone afterwards as
        graphed.TrainStepGraph undoes them; then one iteration captured."""
        dev = self.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            tensors, fresh = self._state_tensors()
            with torch.no_grad():
                keep = [(t, t.detach().clone()) for t in tensors]
            for _ in range(max(int(warmup), 1)):
                self._iteration(o)
            with torch.no_grad():
                for t, c in keep:
                    t.copy_(c)
                for p in fresh:
                    for v in self.optimizer.state[p].values():
                        if torch.is_tensor(v):
                            v.zero_()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._iteration(o)
        self.graph_captures += 1
        return graph, out

    def _update_matches(self, depths, matching_thr):
        """matcher.update_references(deformed depths) + match(thr), as the reference does between two iterations.  The matcher
        binds new buffers for its matches, so a captured iteration is captured again afterwards."""
        self.matcher.update_references(reference_depths=depths)
        self.matcher.match(matching_thr)

    def optimize(self, reference_data=None, masks=None, gradient_masks=None, n_iterations=600, use_gradient_loss=True,
                 use_hessian_loss=False, use_normal_loss=True, use_curvature_loss=False, use_matching_loss=False,
                 use_reprojection_loss=False, matching_thr=None, use_confidence_in_matching_loss=False, matching_update_iters=None,
                 gradient_loss_weight=10., hessian_loss_weight=100., normal_loss_weight=2., curvature_loss_weight=1.,
                 matching_loss_weight=1., reprojection_loss_weight=2., encodings_lr=1e-2, mlp_lr=1e-3, confidence_lr=1e-3,
                 lr_update_iters=(300,), lr_update_factor=0.1, verbose=False, match_to_img=None, match_to_pix=None,
                 reprojection_loss_power=0.5, regularize_chart_encodings_norms=False, chart_encodings_norm_loss_weight=0.5,
                 use_total_variation_on_depth_encodings=False, total_variation_on_depth_encodings_weight=1.0, graph=None,
                 prepare=True, reference_points=None):
        """ParallelAligner.optimize with its keywords and defaults.  reference_points: the reference's other form of
        reference_data, 3D points per chart -- a list of [N_c,3] tensors or a chart_points.ChartPoints --, given INSTEAD of
        reference_data: the depth term becomes chart_points.point_reference_loss.  graph: capture the iteration in a HIP graph and replay it
        (None: yes on a HIP device); prepare=False keeps the current parameters and optimiser (the reference always resets).
        train_losses gets the total loss and loss_terms a dict of the named terms every max(1, n_iterations // 50) iterations
        (one read-back each); the reference divides by zero below 50 iterations."""
        shape = (self.n, self.height, self.width)
        if use_reprojection_loss:
            raise NotImplementedError("chart aligner: use_reprojection_loss is not supported (the reference's own script refuses it)")
        if reference_points is not None:
            if reference_data is not None:
                raise ValueError("chart aligner: give reference_data or reference_points, not both")
            if use_matching_loss:
                raise NotImplementedError("Matching loss is not implemented when using points as reference.")
            if masks is not None:
                raise ValueError("chart aligner: masks are not supported with reference_points (the reference's masks * diff "
                                 "cannot broadcast against points)")
            if not isinstance(reference_points, ChartPoints):
                reference_points = ChartPoints(self.cameras, reference_points, self.height, self.width)
            if (reference_points.n, reference_points.height, reference_points.width) != shape:
                raise ValueError(f"reference_points must belong to charts of shape {shape}")
            if reference_points.n_points == 0:
                raise ValueError("chart aligner: reference_points holds no point")
        elif reference_data is None:
            raise ValueError("chart aligner: reference_data (depth maps) or reference_points (3D points per chart) is needed")
        elif _is_points(reference_data, shape):
            raise NotImplementedError("chart aligner: 3D points as reference_data are not supported (depth maps [n,H,W] only); "
                                      "pass them as reference_points=")
        if use_confidence_in_matching_loss and not self.use_learnable_confidence:
            raise ValueError("chart aligner: use_confidence_in_matching_loss needs use_learnable_confidence")
        if use_hessian_loss and gradient_masks is not None:
            raise NotImplementedError("chart aligner: the hessian term with gradient_masks (the reference's broadcast fails there)")
        if use_total_variation_on_depth_encodings and self._deform._B < 2:
            raise ValueError(f"chart aligner: the total variation needs at least 2 depth bins (got {self._deform._B})")
        self._hip()
        graph = True if graph is None else bool(graph)
        n_iterations = int(n_iterations)
        lr_update_iters = list(lr_update_iters)
        if reference_points is not None:
            reference_points.build_index()  # before any capture: the index is built once, not per replay
            reference = torch.zeros(shape, dtype=torch.float32, device=self.device)
            masks = torch.zeros(shape, dtype=torch.float32, device=self.device)
        else:
            reference = f32(maps_of_shape(reference_data, "reference_data", shape, self.device, "the charts' shape"))
        if self.losses is None:
            self.losses = AlignmentLosses(self.cameras, self._depths, self.confidence_weighting)
        self.losses.confidence_weighting = float(self.confidence_weighting)
        if use_matching_loss:
            self.matcher = ChartMatcher(self.cameras, reference_depths=reference)
            if matching_thr is None:
                matching_thr = MATCHING_THR_FACTOR * self._spatial_extent
            self.matcher.match(matching_thr)
        if prepare or self.optimizer is None:
            self.prepare_for_optimization(encodings_lr, mlp_lr, lr_update_iters, lr_update_factor, confidence_lr, verbose)
        else:
            self.lr_update_iters, self.lr_update_factor = lr_update_iters, lr_update_factor

        o = SimpleNamespace()
        o.reference = reference
        o.points = reference_points
        o.masks = None if masks is None else self.losses._map(masks, "masks")
        o.gradient_masks = None if gradient_masks is None or not use_gradient_loss else \
            self.losses._map(gradient_masks, "gradient_masks", (self.n, self.height - 1, self.width - 1))
        o.weights = {"gradient": float(gradient_loss_weight) if use_gradient_loss else None,
                     "hessian": float(hessian_loss_weight) if use_hessian_loss else None,
                     "normal": float(normal_loss_weight) if use_normal_loss else None,
                     "curvature": float(curvature_loss_weight) if use_curvature_loss else None,
                     "matching": float(matching_loss_weight) if use_matching_loss else None,
                     "norm": float(chart_encodings_norm_loss_weight) if regularize_chart_encodings_norms else None,
                     "tv": float(total_variation_on_depth_encodings_weight) if use_total_variation_on_depth_encodings else None}
        o.confidence_in_matching = bool(use_matching_loss and use_confidence_in_matching_loss)
        o.weight_max = None
        if o.confidence_in_matching:
            # a bound on the confidence over the whole run, so that the matcher's fixed-point backward needs no read-back per
            # iteration: one Adam update moves _confidence by at most ADAM_STEP_BOUND lr
            top = float(self._confidence.detach().max())
            o.weight_max = 1.0 + math.exp(top + ADAM_STEP_BOUND * float(confidence_lr) * n_iterations)
        self._options = o  # (tools/bench_chart_aligner.py steps _iteration and _capture itself after n_iterations = 0)
        self.train_losses, self.loss_terms = [], []
        interval = max(1, n_iterations // 50)
        update_iters = set(matching_update_iters) if (use_matching_loss and matching_update_iters is not None) else set()
        captured = None
        for i in range(n_iterations):
            if i in lr_update_iters:
                self.update_learning_rates()
            if graph:
                if captured is None:
                    captured = self._capture(o)  # records the iteration; the replay below runs it
                    g, (vec, depths) = captured
                g.replay()
            else:
                vec, depths = self._iteration(o)
            if i in update_iters:
                self._update_matches(depths.clone(), matching_thr)
                captured = None  # the matches are in new buffers: capture again (two warm-up iterations, undone, and a capture)
            if i % interval == 0:
                values = vec.tolist()
                self.train_losses.append(values[0])
                self.loss_terms.append({k: v for k, v in zip(TERM_NAMES, values) if _logged(k, o.weights)})
        return self.train_losses

    # ---- results ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def outputs(self):
        """(verts [n,H,W,3], depths [n,H,W], confs [n,H,W]) at the current parameters; without a learnable confidence the
        confidences are the 4 that align_charts_in_parallel substitutes."""
        verts = self.verts
        depths = self.deformed_depths
        confs = self.confidence if self.use_learnable_confidence else 4.0 * torch.ones_like(depths)
        return verts, depths, confs

    @torch.no_grad()
    def save_charts_data(self, path, scale_factor=1.0):
        """charts_data.npz as align_charts_in_parallel writes it: prior_depths, depths, pts, confs, scale_factor.  `path` is the
        file, or a directory that gets charts_data.npz."""
        verts, depths, confs = self.outputs()
        if os.path.isdir(path):
            path = os.path.join(path, "charts_data.npz")
        np.savez(path, prior_depths=self._depths.cpu().numpy(), depths=depths.cpu().numpy(), pts=verts.cpu().numpy(),
                 confs=confs.cpu().numpy(), scale_factor=scale_factor)
        return path


def _logged(name, weights):
    key = {"grad": "gradient", "hess": "hessian", "normal": "normal", "curv": "curvature", "matching": "matching", "ce_norm": "norm",
           "de_tv": "tv"}.get(name)
    return key is None or weights.get(key) is not None


def hessian_term(depths, prior):
    """The reference's hessian term without masks: the mean over n, the four second differences and the (H-2) x (W-2) interior
    of |second difference of depths - second difference of prior|.  With the forward differences along a column,
    a(i,j) = d(i+1,j) - d(i,j), and along a row, b(i,j) = d(i,j+1) - d(i,j), the four are
        a(i+1,j) - a(i,j),   b(i+1,j) - b(i,j),   a(i,j+1) - a(i,j),   b(i,j+1) - b(i,j)      for i < H-2, j < W-2,
    each one float32 subtraction of two first differences (the two mixed ones agree in exact arithmetic and are both counted,
    as the reference counts them).  Plain torch ops on [n,H,W] maps; works on the host too."""
    if depths.dim() != 3 or depths.shape != prior.shape or depths.shape[1] < 3 or depths.shape[2] < 3:
        raise ValueError(f"hessian term: needs two [n,H,W] maps of one shape with H, W >= 3 (got {tuple(depths.shape)}, {tuple(prior.shape)})")
    H, W = depths.shape[1] - 2, depths.shape[2] - 2
    total = None
    for axis1 in (1, 2):
        first_d, first_p = depths.diff(dim=axis1), prior.diff(dim=axis1)
        for axis2 in (1, 2):
            second = (first_d.diff(dim=axis2) - first_p.diff(dim=axis2))[:, :H, :W]
            total = second.abs().sum() if total is None else total + second.abs().sum()
    return total / (4 * depths.shape[0] * H * W)


def align_charts(cameras, initial_depths, reference_depths=None, masks=None, scale_factor=1.0, charts_data_path=None,
                 return_training_losses=False, graph=None, reference_points=None, **align_config):
    """align_charts_in_parallel from the point where it has its cameras and initial depths: builds a ChartAligner from the
    configuration's architecture keywords, runs optimize with the rest (matching_thr_factor becomes matching_thr) and returns
    (verts, depths, confs[, train_losses]) -- (verts, depths[, train_losses]) without a learnable confidence, as the reference
    does.  charts_data_path: a directory (or file) that gets charts_data.npz.  align_config: e.g. ALIGNMENT_CONFIGS["strong"].
    reference_points (a list of [N_c,3] tensors or a ChartPoints, also accepted in reference_depths' place as
    chart_points.build_charts returns it) replaces reference_depths; the matching loss is then refused as the reference refuses it."""
    if isinstance(reference_depths, ChartPoints):
        if reference_points is not None:
            raise ValueError("align_charts: two sets of reference points")
        reference_points, reference_depths = reference_depths, None
    cfg = dict(ALIGNMENT_CONFIGS["default"], **align_config)  # align_charts_in_parallel's own defaults are default.yaml's
    arch = {k: cfg.pop(k) for k in ARCHITECTURE_KEYS if k in cfg}
    factor = cfg.pop("matching_thr_factor", MATCHING_THR_FACTOR)
    aligner = ChartAligner(cameras, initial_depths, **arch)
    cfg.setdefault("matching_thr", float(factor) * aligner._spatial_extent)
    aligner.optimize(reference_depths, masks=masks, graph=graph, reference_points=reference_points, **cfg)
    verts, depths, confs = aligner.outputs()
    if charts_data_path is not None:
        aligner.save_charts_data(charts_data_path, scale_factor)
    out = (verts, depths, confs) if aligner.use_learnable_confidence else (verts, depths)
    return out + (aligner.train_losses,) if return_training_losses else out
