"""What the scene-stage wrappers (mesh, mesh_eval, visibility, planes, consistency, view_selection, depth_cues, chart_init, plane_masks, plane_fit)
share on the Python side of a library call: host arrays, device resolution, the per-view map checks, the view stack and the
one launch helper.  The C++ counterpart is csrc/tsdf/mesh_common.h and view_stack.h ("The Python side of a
wrapper")."""
import ctypes
import math

import numpy as np
import torch

from . import _lib


# ---- host arrays -----------------------------------------------------------------------------------------------------
def to_np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def host_f32(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    return (ctypes.c_float * len(a))(*a.tolist())


def host_array(ctype, values):
    """HOST array of `ctype` that is never zero-length: an empty list gives one zero element, so the library is always
    handed an address."""
    values = list(values)
    return (ctype * max(len(values), 1))(*values)


def focal_lengths(camera, width, height):
    """(fx, fy) in pixels, in double: W / (2 tan(FoVx / 2)) and H / (2 tan(FoVy / 2))."""
    return width / (2.0 * math.tan(float(camera.FoVx) / 2.0)), height / (2.0 * math.tan(float(camera.FoVy) / 2.0))


# ---- devices and tensors -----------------------------------------------------------------------------------------------
def hip_device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the mesh kernels need tensors on a HIP device (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)


def default_device():
    if not torch.cuda.is_available():
        raise RuntimeError("mesh operations need a HIP device (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def device_points(points, what="points"):
    if not isinstance(points, torch.Tensor):
        raise RuntimeError(f"{what} must be a tensor on a HIP device")
    return hip_device(points.device), points.detach().float().reshape(-1, 3).contiguous()


def mask_bytes(mask):
    """A bool or uint8 map as the uint8 the library reads (no copy)."""
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


# ---- per-view map checks: the steps the wrappers' dialects have in common ------------------------------------------------
def on_device(t, device, name):
    """The RuntimeError dialect (mesh, visibility, consistency): `t`, detached, if it is a tensor on `device`."""
    if not isinstance(t, torch.Tensor) or t.device != device:
        raise RuntimeError(f"{name} must be a tensor on {device}")
    return t.detach()


def drop_leading_one(t):
    """[1,H,W] as [H,W]; anything else as it is."""
    return t[0] if t.dim() == 3 and t.size(0) == 1 else t


def _plane_map(d):
    d = drop_leading_one(d.float())
    if d.dim() != 2:
        raise RuntimeError(f"depth must be [H,W] or [1,H,W] (got {tuple(d.shape)})")
    return d.contiguous()


def depth_map(depth, device=None):
    """A depth map as a contiguous float32 [H,W] device tensor (never written)."""
    if not isinstance(depth, torch.Tensor):
        raise RuntimeError("depth must be a tensor on a HIP device")
    dev = hip_device(depth.device if device is None else device)
    return dev, _plane_map(on_device(depth, dev, "depth"))


def view_list(maps, name, tail=""):
    """The ValueError dialect (depth_cues, chart_init): a list of per-view maps, or one stacked [V,H,W`tail`] tensor unbound."""
    if isinstance(maps, torch.Tensor):
        if maps.dim() != 3 + tail.count(","):
            raise ValueError(f"{name}: a stacked tensor must be [V,H,W{tail}] (got {tuple(maps.shape)})")
        return list(maps.unbind(0))
    return list(maps)


def check_view_count(maps, name, n):
    if n is not None and len(maps) != n:
        raise ValueError(f"{n} views but {len(maps)} {name}")


def check_dtype(t, dtypes, label):
    if t.dtype not in dtypes:
        raise ValueError(f"{label} must be {' or '.join(str(d) for d in dtypes)} (got {t.dtype})")


def same_device(t, dev, label):
    """The one HIP device of a call's maps: `dev`, or `t`'s when `dev` is still None; ValueError for a map elsewhere."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{label} must be a tensor on a HIP device")
    if dev is None:
        dev = hip_device(t.device)
    if t.device != dev:
        raise ValueError(f"{label} must be on {dev} (got {t.device})")
    return dev


# ---- the view stack (csrc/tsdf/view_stack.h) ---------------------------------------------------------------------------
class ViewStack:
    """The host arrays a view-stack entry point takes, and the device tensors they point into (kept alive here; nothing
    is allocated).  views: (camera, depth [H,W] / [1,H,W], rgb [3,H,W] or None) per view, maps on `device`.
    matrices(camera) gives the n_matrices 4x4 the kernels read per view; focal adds the cameras' focal lengths at the
    maps' sizes.  `head` is the run of arguments every entry point has: n_views, the matrices, focal, sizes, depth."""

    def __init__(self, views, device, need_rgb=False, n_matrices=0, matrices=lambda cam: [], focal=False):
        views = list(views)
        self.maps, sizes, dptr, cptr = [], [], [], []
        mats = [[] for _ in range(n_matrices)]
        for cam, depth, rgb in views:
            for m, M in zip(mats, matrices(cam)):
                m.extend(np.asarray(to_np(M), np.float32).reshape(16).tolist())
            depth = _plane_map(on_device(depth, device, "depth"))
            H, W = depth.shape
            self.maps.append(depth)
            dptr.append(depth.data_ptr())
            if need_rgb:
                if rgb is None:
                    raise RuntimeError("colours need the rgb map of every view")
                rgb = on_device(rgb, device, "rgb").float().contiguous()
                if tuple(rgb.shape) != (3, H, W):
                    raise RuntimeError(f"rgb must have shape {(3, H, W)} (got {tuple(rgb.shape)})")
                self.maps.append(rgb)
                cptr.append(rgb.data_ptr())
            sizes.extend([W, H])
        self.n = len(dptr)
        self.sizes = host_array(ctypes.c_int, sizes)
        self.depth = host_array(ctypes.c_void_p, dptr)
        self.rgb = host_array(ctypes.c_void_p, cptr) if need_rgb else None
        self.head = [self.n] + [host_array(ctypes.c_float, m) for m in mats]
        if focal:
            self.head.append(host_array(ctypes.c_float, [f for v, (cam, _d, _c) in enumerate(views)
                                                         for f in focal_lengths(cam, sizes[2 * v], sizes[2 * v + 1])]))
        self.head += [self.sizes, self.depth]

    def size(self, v):
        return self.sizes[2 * v + 1], self.sizes[2 * v]  # H, W


def camera_views(cameras, depths, device):
    """The stack of the visibility family: per view world_view_transform, the focal lengths, the depth map."""
    cameras, depths = list(cameras), list(depths)
    if len(cameras) != len(depths):
        raise ValueError(f"{len(cameras)} cameras but {len(depths)} depth maps")
    return ViewStack([(c, d, None) for c, d in zip(cameras, depths)], device, False, 1,
                     lambda cam: [cam.world_view_transform], focal=True)


# ---- the library call ------------------------------------------------------------------------------------------------
def launch(dev, name, *args, workspace=None, sync=False):
    """_lib.call(name, *args, workspace pointer, workspace bytes, stream) on the current stream of `dev`.

    workspace: None passes NULL, 0; a byte count allocates that many bytes; a tensor is passed as it is.  The workspace is
    returned, so that a count / emit pair shares one.  (The few entry points that take a stream and no workspace --
    g4s_mesh_observed_vertices, g4s_mesh_keep_*, g4s_mesh_sample_surface -- are called with _lib.call.)

    sync: wait for the stream before returning.  A wrapper asks for it when what the kernels read or write may be freed
    on its return: the workspace, a contiguous or float copy of an argument, a view stack's tensors.  The wrappers of
    the mesh operations, whose results feed the next launch on the same stream, leave it out."""
    with torch.cuda.device(dev):
        if workspace is not None and not isinstance(workspace, torch.Tensor):
            workspace = torch.empty(workspace, dtype=torch.uint8, device=dev)
        _lib.call(name, *args, _lib.ptr(workspace), 0 if workspace is None else workspace.numel(), _lib.stream(dev))
        if sync:
            torch.cuda.current_stream(dev).synchronize()
    return workspace


def voxel_downsample_count(pts, voxel_size, who):
    """g4s_voxel_downsample_count, the first phase of the two voxel down-samples: (workspace, number of voxels).  Status -1,
    an argument the library refuses, is `who`'s ValueError."""
    lib, dev, n = _lib.load(), pts.device, pts.size(0)
    count = ctypes.c_int(0)
    with torch.cuda.device(dev):
        ws = torch.empty(lib.g4s_voxel_downsample_workspace(n), dtype=torch.uint8, device=dev)
        rc = lib.g4s_voxel_downsample_count(n, _lib.ptr(pts), float(voxel_size), ctypes.byref(count), _lib.ptr(ws), ws.numel(),
                                            _lib.stream(dev))
    if rc == -1:
        raise ValueError(f"{who}: {_lib.last_error()}")
    if rc != 0:
        raise RuntimeError(f"g4s_voxel_downsample_count failed ({rc}): {_lib.last_error()}")
    return ws, count.value
