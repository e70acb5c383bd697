"""The deformation of MAtCha's chart alignment: chart encodings, depth encoding, per-chart MLP and the deformed depths
(include/g4s_losses.h, "Chart deformation"; csrc/chart_deform.hip).

ParallelAligner (matcha/dm_scene/parallel_aligner.py) holds its trainable parameters in charts_encoding, depth_encoding and
deformation, and every one of its 1000 iterations runs five grid_sample calls, a cat, three bmm and a transform over all n
charts, with every [n, H W, 32] and [n, H W, 64] tensor kept for autograd.  ChartDeformation holds the same parameters under
the same names; deformed_depths() is one library call, its backward a second.  Everything goes through the library; there is
no torch path.  Cameras and depth maps are taken as chart_align.AlignmentLosses takes them.  INTEGRATION.md section W lists the
differences from the reference.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._device import launch
from .chart_align import ray_records
from ._charts import camera_list, f32, maps_of_shape, spatial_extent, stack

TILE_PIXELS, WORKGROUP_PIXELS, MAX_LEVELS = 64, 4096, 8  # G4S_CHART_DEFORM_TILE, _WG_PIXELS, _MAX_LEVELS
ENCODING_WIDTHS, LAYER_SIZES, MIN_LAYERS, MAX_LAYERS, MAX_BINS = (16, 32, 64), (32, 64), 2, 4, 4096


# ---- the reference's parameter objects (its defaults), duck-typed on their attribute names -----------------------------
class ChartsEncodingParams:
    def __init__(self, encoding_dim=32, resolution_factor=0.4, initialization_range=1e-4):
        self.encoding_dim, self.resolution_factor, self.initialization_range = encoding_dim, resolution_factor, initialization_range


class MultiResChartsEncodingParams:
    def __init__(self, encoding_dim_per_res=8, resolutions=(0.05, 0.1, 0.2, 0.4), initialization_range=1e-4):
        self.encoding_dim_per_res, self.resolutions = encoding_dim_per_res, list(resolutions)
        self.encoding_dim = encoding_dim_per_res * len(self.resolutions)
        self.initialization_range = initialization_range


class DepthEncodingParams:
    def __init__(self, encoding_dim=32, n_bins=30, initialization_range=1e-4):
        self.encoding_dim, self.n_bins, self.initialization_range = encoding_dim, n_bins, initialization_range


class MLPParams:
    def __init__(self, n_deformation_layers=3, deformation_layer_size=64, scene_radius_factor=2., deformation_radius_factor=1.,
                 no_final_linearity=True):
        self.n_deformation_layers, self.deformation_layer_size = n_deformation_layers, deformation_layer_size
        self.scene_radius_factor, self.deformation_radius_factor = scene_radius_factor, deformation_radius_factor
        self.no_final_linearity = no_final_linearity


@torch.no_grad()
def depth_coordinates(depths, n_bins):
    """The per-chart quantile coordinates of ParallelAligner.__init__ (lines 279-306): float32 [n, H W] in [0, 1].  A depth
    in quantile interval i (of n_bins, the last one open above) gets ((d - q_i) / (q_i+1 - q_i) + i) / (n_bins - 1), one in
    the last interval 1.  Runs once per alignment, in torch ON THE HOST (a device divides by a scalar through its reciprocal,
    an ulp off), and returns on the depths' device."""
    d = torch.stack(list(depths)) if not isinstance(depths, torch.Tensor) else depths
    device = d.device
    d = d.detach().float().reshape(d.shape[0], -1).cpu()
    nb = int(n_bins)
    qs = torch.tensor([i / nb for i in range(nb)], dtype=torch.float32, device=d.device)
    quant = torch.stack([torch.quantile(row, qs) for row in d])  # [n, nb], as torch.quantile(depth_i, i / nb).item()
    coords = torch.zeros_like(d)
    for i in range(nb):
        lo = quant[:, i:i + 1]
        if i < nb - 1:
            hi = quant[:, i + 1:i + 2]
            mask = (d >= lo) & (d < hi)
            val = ((d - lo) / (hi - lo) + i) / (nb - 1)
        else:
            mask, val = d >= lo, torch.ones_like(d)
        coords = torch.where(mask, val, coords)
    return coords.to(device)


# ---- parameter containers that give the reference's names --------------------------------------------------------------
class _Encoding(torch.nn.Module):  # ChartsEncoding, DepthEncoding: .encodings
    def __init__(self, shape, initialization_range, device):
        super().__init__()
        self.initialization_range = initialization_range
        self.encodings = torch.nn.Parameter(torch.empty(shape, device=device))
        self.reset()

    @torch.no_grad()
    def reset(self):
        """initialization_range * (-1 + 2 u), u drawn on the host as the reference draws it"""
        self.encodings.copy_(self.initialization_range * (-1. + 2. * torch.rand(tuple(self.encodings.shape))))


class _MultiRes(torch.nn.Module):  # MultiResChartsEncoding: .charts_encoding.{l}.encodings
    def __init__(self, levels):
        super().__init__()
        self.charts_encoding = torch.nn.ModuleList(levels)


class _MultiLinear(torch.nn.Module):  # MultiLinear: .weight [n,out,in], .bias [n,out]
    def __init__(self, n, fan_in, fan_out, device):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty((n, fan_out, fan_in), device=device))
        self.bias = torch.nn.Parameter(torch.empty((n, fan_out), device=device))


class _MLP(torch.nn.Module):  # DeformationMultiMLP: .mlp.{0,2,4,..}
    def __init__(self, n, n_layer, layer_size, input_dim, device):
        super().__init__()
        dims = [input_dim] + [layer_size] * (n_layer - 1) + [1]
        mods = []
        for j in range(n_layer):
            mods.append(_MultiLinear(n, dims[j], dims[j + 1], device))
            if j < n_layer - 1:
                mods.append(torch.nn.ReLU())
        self.mlp = torch.nn.Sequential(*mods)

    def layers(self):
        return [m for m in self.mlp if isinstance(m, _MultiLinear)]


class _Deform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, want_delta, *params):
        m = module
        p = [t.detach().float().contiguous() for t in params]
        with torch.cuda.device(m.device):
            depths = torch.empty((m.n, m.height, m.width), dtype=torch.float32, device=m.device)
            delta = torch.empty_like(depths) if want_delta else None
            launch(m.device, "g4s_chart_deform_forward", *m._call_head(p), _lib.ptr(depths), _lib.ptr(delta))
        ctx.save_for_backward(*p)
        ctx.module = m
        ctx.meta = [(t.shape, t.dtype) for t in params]
        if want_delta:
            ctx.mark_non_differentiable(delta)
            return depths, delta
        return depths

    @staticmethod
    def backward(ctx, g, *_unused):
        m, p = ctx.module, list(ctx.saved_tensors)
        with torch.cuda.device(m.device):
            g = g.detach().float().contiguous()  # the cotangent stays on the device
            grads = [torch.empty_like(t) for t in p]
            lv, de, ws, bs = m._split(grads)
            launch(m.device, "g4s_chart_deform_backward", *m._call_head(p), _lib.ptr(g), _lib.ptrs(lv), _lib.ptr(de), _lib.ptrs(ws),
                   _lib.ptrs(bs), workspace=m.workspace_bytes)
        return (None, None) + tuple(gr.reshape(s).to(dt) for gr, (s, dt) in zip(grads, ctx.meta))


REG_NORM, REG_TV = 1, 2  # G4S_CHART_DEFORM_REG_NORM, _TV


class _DeformReg(torch.autograd.Function):
    """The weighted deformation with the encoding regularisers (g4s_chart_deform_reg_*): (depths [n,H,W], reg [2])."""

    @staticmethod
    def forward(ctx, module, flags, encoding_weights, *params):
        m = module
        p = [t.detach().float().contiguous() for t in params]
        with torch.cuda.device(m.device):
            depths = torch.empty((m.n, m.height, m.width), dtype=torch.float32, device=m.device)
            reg = torch.empty(2, dtype=torch.float32, device=m.device)
            launch(m.device, "g4s_chart_deform_reg_forward", *m._call_head(p), _lib.ptr(encoding_weights), int(flags), _lib.ptr(depths),
                   _lib.ptr(None), _lib.ptr(reg), workspace=m.reg_workspace_bytes(flags, forward=True) if flags & REG_NORM else None)
        ctx.weighted = encoding_weights is not None
        ctx.save_for_backward(*([encoding_weights] if ctx.weighted else []), *p)
        ctx.module, ctx.flags = m, int(flags)
        ctx.meta = [(t.shape, t.dtype) for t in params]
        return depths, reg

    @staticmethod
    def backward(ctx, g, greg):
        m, p = ctx.module, list(ctx.saved_tensors)
        w = p.pop(0) if ctx.weighted else None
        with torch.cuda.device(m.device):
            g = g.detach().float().contiguous()  # the cotangents stay on the device
            greg = greg.detach().float().contiguous()
            grads = [torch.empty_like(t) for t in p]
            lv, de, ws, bs = m._split(grads)
            launch(m.device, "g4s_chart_deform_reg_backward", *m._call_head(p), _lib.ptr(w), ctx.flags, _lib.ptr(g), _lib.ptr(greg),
                   _lib.ptrs(lv), _lib.ptr(de), _lib.ptrs(ws), _lib.ptrs(bs), workspace=m.reg_workspace_bytes(ctx.flags))
        return (None, None, None) + tuple(gr.reshape(s).to(dt) for gr, (s, dt) in zip(grads, ctx.meta))


class ChartDeformation(torch.nn.Module):
    """The trainable half of ParallelAligner: charts_encoding, depth_encoding and deformation under the reference's parameter
    names, and deformed_depths() [n,H,W] with gradients to every one of them.  `depths` are the aligner's `_depths` (constants,
    as the rays and depth_coords are).  Parameters live on the depths' device; deformed_depths() needs a HIP device."""

    def __init__(self, cameras, depths, charts_encoding_params=None, depth_encoding_params=None, mlp_params=None,
                 use_learnable_depth_encoding=True, use_multi_res_charts_encoding=True, multi_res_charts_encoding_params=None,
                 learnable_depth_encoding_mode="add", predict_in_disparity_space=False, use_meta_mlp=False, use_lora_mlp=False,
                 weight_encodings_with_confidence=False, output_dim=1, spatial_extent_override=None):
        super().__init__()
        cep = ChartsEncodingParams() if charts_encoding_params is None else charts_encoding_params
        dep = DepthEncodingParams() if depth_encoding_params is None else depth_encoding_params
        mlp = MLPParams() if mlp_params is None else mlp_params
        mrp = MultiResChartsEncodingParams() if multi_res_charts_encoding_params is None else multi_res_charts_encoding_params
        if use_learnable_depth_encoding and learnable_depth_encoding_mode != "add":
            if learnable_depth_encoding_mode in ("multiply", "replace", "concatenate", "adaln"):
                raise NotImplementedError(f"chart deform: learnable_depth_encoding_mode '{learnable_depth_encoding_mode}' (only 'add')")
            raise ValueError(f"learnable_depth_encoding_mode must be 'add' (got {learnable_depth_encoding_mode!r})")
        for flag, what in ((use_meta_mlp, "the meta MLP"), (use_lora_mlp, "the LoRA MLP"),
                           (weight_encodings_with_confidence, "weight_encodings_with_confidence"),
                           (predict_in_disparity_space, "predict_in_disparity_space"),
                           (not getattr(mlp, "no_final_linearity", True), "a sigmoid final layer"),
                           (output_dim != 1, f"output dimension {output_dim} (deformations along the rays only)")):
            if flag:
                raise NotImplementedError(f"chart deform: {what} is not supported")
        self.cameras = cameras
        cam_list = camera_list(cameras)
        if isinstance(depths, torch.Tensor) and depths.device.type != "cuda":  # parameters on the host: no forward there
            dev, d0 = depths.device, (depths[:, 0] if depths.dim() == 4 and depths.size(1) == 1 else depths)
            if d0.dim() != 3:
                raise ValueError(f"depths: a stacked tensor must be [n,H,W] (got {tuple(depths.shape)})")
        else:
            dev, d0 = stack(depths, "depths")
        n, H, W = d0.shape
        if n != len(cam_list):
            raise ValueError(f"{len(cam_list)} views but {n} depths")
        if n * H * W >= 2 ** 31:
            raise ValueError(f"chart deform: n H W = {n * H * W} must stay below 2^31")
        self.device, self.n, self.height, self.width = dev, n, H, W
        self.use_learnable_depth_encoding = bool(use_learnable_depth_encoding)
        self.use_multi_res_charts_encoding = bool(use_multi_res_charts_encoding)
        if use_multi_res_charts_encoding:
            self.charts_encoding_params = mrp
            C, sizes = int(mrp.encoding_dim_per_res), [(int(r * H), int(r * W)) for r in mrp.resolutions]
        else:
            self.charts_encoding_params = cep
            C, sizes = int(cep.encoding_dim), [(int(cep.resolution_factor * H), int(cep.resolution_factor * W))]
        self.depth_encoding_params, self.mlp_params = dep, mlp
        L, E = len(sizes), C * len(sizes)
        S, NL, B = int(mlp.deformation_layer_size), int(mlp.n_deformation_layers), int(dep.n_bins)
        if not 1 <= L <= MAX_LEVELS:
            raise ValueError(f"chart deform: 1 to {MAX_LEVELS} encoding levels (got {L})")
        if C < 4 or C % 4:
            raise ValueError(f"chart deform: the channels per level must be a positive multiple of 4 (got {C})")
        if E not in ENCODING_WIDTHS:
            raise ValueError(f"chart deform: the encoding width levels x channels must be one of {ENCODING_WIDTHS} (got {E})")
        if int(cep.encoding_dim) != E:  # the reference sizes the MLP's input by charts_encoding_params.encoding_dim
            raise ValueError(f"chart deform: charts_encoding_params.encoding_dim ({cep.encoding_dim}) must equal the encoding width {E}")
        if use_learnable_depth_encoding and int(dep.encoding_dim) != E:
            raise ValueError(f"chart deform: depth_encoding_params.encoding_dim ({dep.encoding_dim}) must equal the encoding width {E}")
        if S not in LAYER_SIZES:
            raise ValueError(f"chart deform: deformation_layer_size must be one of {LAYER_SIZES} (got {S})")
        if not MIN_LAYERS <= NL <= MAX_LAYERS:
            raise ValueError(f"chart deform: {MIN_LAYERS} to {MAX_LAYERS} deformation layers (got {NL})")
        if use_learnable_depth_encoding and not 1 <= B <= MAX_BINS:
            raise ValueError(f"chart deform: 1 to {MAX_BINS} depth bins (got {B})")
        for l, (h, w) in enumerate(sizes):
            if h < 1 or w < 1 or h * w > 2 ** 24:
                raise ValueError(f"chart deform: level {l} must have 1 x 1 to 2^24 texels (got {h} x {w} from a {H} x {W} chart)")
        # a single view has no extent (the reference divides by zero there): spatial_extent_override supplies one
        extent = spatial_extent(cam_list) if spatial_extent_override is None else float(spatial_extent_override)
        self.scene_radius = float(mlp.scene_radius_factor) * extent
        self.deformation_radius = float(mlp.deformation_radius_factor) * extent
        if not self.scene_radius > 0:
            raise ValueError(f"chart deform: the scene radius must be positive (got {self.scene_radius}; one camera centre only?)")
        self._sizes, self._C, self._E, self._B = sizes, C, E, (B if use_learnable_depth_encoding else 0)
        self._S, self._NL = S, NL

        levels = [_Encoding((n, C, h, w), self.charts_encoding_params.initialization_range, dev) for h, w in sizes]
        self.charts_encoding = _MultiRes(levels) if use_multi_res_charts_encoding else levels[0]
        self.deformation = _MLP(n, NL, S, E, dev)
        self.reset_mlp()
        self._d0 = d0.detach().float().contiguous()
        if use_learnable_depth_encoding:
            self.depth_coords = depth_coordinates(self._d0, B).contiguous()
            self.depth_encoding = _Encoding((n, E, B), dep.initialization_range, dev)
        else:
            self.depth_coords = self.depth_encoding = None
        self._cams = torch.as_tensor(ray_records(cam_list, W, H), device=dev)
        self._shape = _lib.G4sChartDeformShape(n, H, W, L, C, (ctypes.c_int * 8)(*([h for h, _ in sizes] + [0] * (8 - L))),
                                               (ctypes.c_int * 8)(*([w for _, w in sizes] + [0] * (8 - L))), self._B, NL, S,
                                               self.scene_radius, self.deformation_radius)
        self._workspace_bytes = None

    # ---- parameters ------------------------------------------------------------------------------------------------------
    def _levels(self):
        return list(self.charts_encoding.charts_encoding) if self.use_multi_res_charts_encoding else [self.charts_encoding]

    def _params(self):
        """levels, [depth encoding], weights, biases: the order of the library call"""
        lin = self.deformation.layers()
        return ([m.encodings for m in self._levels()] + ([self.depth_encoding.encodings] if self._B else []) + [m.weight for m in lin]
                + [m.bias for m in lin])

    def _split(self, tensors):
        L, NL, k = len(self._sizes), self._NL, 1 if self._B else 0
        return tensors[:L], (tensors[L] if k else None), tensors[L + k:L + k + NL], tensors[L + k + NL:]

    def _call_head(self, p):
        lv, de, ws, bs = self._split(p)
        return (ctypes.byref(self._shape), _lib.ptrs(lv), _lib.ptr(de), _lib.ptrs(ws), _lib.ptrs(bs), _lib.ptr(self.depth_coords),
                _lib.ptr(self._cams), _lib.ptr(self._d0))

    @property
    def workspace_bytes(self):
        """The backward's workspace: dL/dx [n, H W, E] and one partial of the weight, bias and depth-encoding gradients per
        WORKGROUP_PIXELS pixels of a chart.  The forward needs none."""
        if self._workspace_bytes is None:
            self._workspace_bytes = _lib.load().g4s_chart_deform_workspace(ctypes.byref(self._shape))
            if self._workspace_bytes == 0:
                raise ValueError(f"chart deform: {_lib.last_error()}")
        return self._workspace_bytes

    @torch.no_grad()
    def reset_encodings(self):
        """ParallelAligner.reset_encodings: the depth encoding first, then the levels, uniform in +- initialization_range."""
        if self._B:
            self.depth_encoding.reset()
        for m in self._levels():
            m.reset()

    @torch.no_grad()
    def reset_mlp(self, std=None):
        """ParallelAligner.reset_mlp: per head xavier_normal_ with the ReLU gain (normal_ with `std` if given), zero biases.
        The reference first constructs the layers on the host, which draws their default initialisation from the host
        generator; those draws are made here too and thrown away, so a run seeded like the reference draws the same values."""
        gain = torch.nn.init.calculate_gain("relu")
        for m in self.deformation.layers():
            w = torch.nn.init.kaiming_uniform_(torch.empty(tuple(m.weight.shape)), a=math.sqrt(5))
            fan_in, _ = torch.nn.init._calculate_fan_in_and_fan_out(w)
            torch.nn.init.uniform_(torch.empty(tuple(m.bias.shape)), -1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))
        for m in self.deformation.layers():
            for i in range(self.n):
                if std is not None:
                    torch.nn.init.normal_(m.weight[i], std=std)
                else:
                    torch.nn.init.xavier_normal_(m.weight[i], gain=gain)
            torch.nn.init.zeros_(m.bias)

    def load_reference_state_dict(self, state_dict):
        """Load the trainable parameters from a ParallelAligner.state_dict(); its other entries (_verts, _depths, _pts_uv,
        depth_coords, _confidence, ...) are not this module's.  A missing or misshapen parameter raises."""
        own = dict(self.named_parameters())
        missing = [k for k in own if k not in state_dict]
        if missing:
            raise KeyError(f"chart deform: the state dict lacks {missing}")
        with torch.no_grad():
            for k, p in own.items():
                v = torch.as_tensor(state_dict[k])
                if tuple(v.shape) != tuple(p.shape):
                    raise ValueError(f"chart deform: {k} must have the shape {tuple(p.shape)} (got {tuple(v.shape)})")
                p.copy_(v.to(p.device, p.dtype))

    # ---- the deformation ----------------------------------------------------------------------------------------------------
    def _check_device(self):
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("chart deform: deformed_depths needs the module on a HIP device (there is no CPU path)")

    def deformed_depths(self):
        """float32 [n,H,W]: the view-space depths of the deformed charts, differentiable in every parameter; value and
        gradients are bit-identical from run to run."""
        self._check_device()
        return _Deform.apply(self, False, *self._params())

    def reg_workspace_bytes(self, flags, forward=False):
        """The workspace of the weighted pair's backward: a double per workgroup, the plain pair's, then n H W floats (the norm's
        cotangent per pixel); forward=True: what the forward needs with the norm bit, the doubles alone.  A refusal (the total
        variation with fewer than 2 bins) raises ValueError with the library's message."""
        size = _lib.load().g4s_chart_deform_reg_forward_workspace if forward else _lib.load().g4s_chart_deform_reg_workspace
        nbytes = size(ctypes.byref(self._shape), int(flags))
        if nbytes == 0:
            raise ValueError(f"chart deform: {_lib.last_error()}")
        return nbytes

    def deformed_depths_and_regularizers(self, encoding_weights=None, norm=False, tv=False):
        """(depths float32 [n,H,W], reg float32 [2]) in one library call, its backward a second.  encoding_weights [n,H,W]
        (detached; the reference's 1 - exp(-(confidence - 1)^2 / 2)) multiply the chart encoding of each pixel before the
        depth encoding is added; reg[0] is the mean norm of the unweighted chart encoding over all pixels
        (regularize_chart_encodings_norms), reg[1] the mean |q[b+1] - q[b]| of the depth encoding
        (use_total_variation_on_depth_encodings); a term not asked for is exactly 0.  Both outputs are differentiable in every
        parameter; values and gradients are bit-identical from run to run, and with no weights and no terms the depths and
        their gradients are bit-identical to deformed_depths()."""
        flags = (REG_NORM if norm else 0) | (REG_TV if tv else 0)
        if tv and self._B < 2:
            raise ValueError(f"chart deform: the total variation needs at least 2 depth bins (got {self._B}; the reference's mean "
                             "over an empty tensor is NaN)")
        self._check_device()
        if encoding_weights is not None:
            encoding_weights = f32(maps_of_shape(encoding_weights, "encoding_weights", (self.n, self.height, self.width), self.device))
        return _DeformReg.apply(self, flags, encoding_weights, *self._params())

    @torch.no_grad()
    def deformations(self):
        """float32 [n,H,W]: delta, the displacement along each pixel's normalised ray (no autograd; for parity checks)."""
        self._check_device()
        return _Deform.apply(self, True, *self._params())[1]
