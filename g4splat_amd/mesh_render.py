"""A mesh seen from a camera: the triangle rasteriser and the dilated depth built on it.

The counterpart of matcha/dm_scene/meshes.py render_mesh_with_pytorch3d and of get_dilated_depth
(2d-gaussian-splatting/extract_mesh_adaptive_tsdf.py:50-137), over the C ABI of include/g4s_render_maps.h ("Mesh
rasteriser and dilated depth", which states the semantics; csrc/tsdf/mesh_render.hip).  The rule is this library's own --
a watertight top-left fill rule decided in integers, perspective-correct weights, the nearest face per pixel by a 64-bit
integer min -- and is not bit-equal to pytorch3d; two runs give the same bits.

    pix_to_face, zbuf, bary = rasterize_mesh(mesh, camera)       # [H,W] int32, [H,W], [H,W,3] on the device
    maps = render_mesh(mesh, camera)                              # rgb, depth, normal, pix_to_face, bary_coords
    keep = visible_face_mask(mesh, cameras)                       # bool [F]: faces that win a pixel somewhere
    mesh = cull_unseen_faces(mesh, cameras)                       # the kind it was given
    maps = dilated_depths(views, 1.5, max_dilation)               # [(depth, rgb or None)] of (camera, depth, rgb) views
    depth, rgb = get_dilated_depth(view, depth, 1.5, rgb=rgb)     # the reference's name and shapes

`mesh` is a TriangleMesh (numpy; uploaded) or a DeviceMesh; `camera` is a camera object or the pair
(world_view_transform, projection_matrix) of 4x4, which needs image_size = (H, W).  pixel_offset 0.5 puts the samples on
the surfel rasteriser's pixel centres, so that `depth` lines up with render()'s surf_depth; 0.0 is the convention of
adaptive_tsdf's sampler, which the dilated depth uses.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._device import ViewStack, hip_device, host_array, host_f32, launch, to_np
from .mesh import DeviceMesh, _returned, _view_and_projection, as_device_mesh, compact_mesh

FLIP_NORMALS, SURFELS_CONVENTION = 1, 2  # G4S_MESH_RASTER_*
MAX_CHANNELS = 16  # G4S_MESH_RASTER_MAX_CHANNELS


def _checked_mesh(mesh):
    """(DeviceMesh, was_host) with the arrays the kernels read: float32 [V,3] twice, int32 [F,3]."""
    if isinstance(mesh, DeviceMesh):
        v, c, t = mesh
        for name, a in (("vertices", v), ("vertex_colors", c), ("triangles", t)):
            if not isinstance(a, torch.Tensor) or a.dim() != 2 or a.size(1) != 3:
                raise RuntimeError(f"{name} must be a [n,3] tensor")
        if v.dtype != torch.float32 or c.dtype != torch.float32:
            raise RuntimeError("vertices and vertex_colors must be float32")
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise RuntimeError("triangles must be an integer tensor")
    return as_device_mesh(mesh)


def _camera_arrays(camera, image_size):
    """(Wv [4,4], Pm [4,4], centre [3], H, W) of a camera object or a (world_view_transform, projection_matrix) pair."""
    Wv, Pm = _view_and_projection(camera)
    Wv, Pm = np.asarray(to_np(Wv), np.float32).reshape(4, 4), np.asarray(to_np(Pm), np.float32).reshape(4, 4)
    if image_size is None:
        if not hasattr(camera, "image_height"):
            raise ValueError("image_size = (H, W) is needed with a camera that carries no image size")
        image_size = (int(camera.image_height), int(camera.image_width))
    H, W = (int(s) for s in image_size)
    centre = getattr(camera, "camera_center", None)
    if centre is None:
        centre = np.linalg.inv(Wv.astype(np.float64).T)[:3, 3]
    return Wv, Pm, np.asarray(to_np(centre), np.float32).reshape(3), H, W


def _raster(dm, camera, image_size, pixel_offset, znear, want, attributes=None, background=None, flags=0, seen=None):
    """One g4s_mesh_raster call.  want: the names among pix_to_face, zbuf, bary, attr, normal, stats to allocate and return
    (a dict); `seen` [F] uint8 is accumulated into."""
    v, _c, t = dm
    dev = v.device
    Wv, Pm, centre, H, W = _camera_arrays(camera, image_size)
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError("image_size must be positive with H * W below 2^31")
    V, F = v.size(0), t.size(0)
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError("a mesh must have fewer than 2^31 vertices and fewer than 2^31 faces")
    C = 0 if attributes is None else attributes.size(1)
    if C > MAX_CHANNELS:
        raise ValueError(f"at most {MAX_CHANNELS} attribute channels")
    shapes = {"pix_to_face": ((H, W), torch.int32), "zbuf": ((H, W), torch.float32), "bary": ((H, W, 3), torch.float32),
              "attr": ((H, W, max(C, 1)), torch.float32), "normal": ((H, W, 3), torch.float32), "stats": ((2,), torch.int32)}
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
    lib = _lib.load()
    launch(dev, "g4s_mesh_raster", V, _lib.ptr(v), F, _lib.ptr(t), host_f32(Wv), host_f32(Pm), host_f32(centre), W, H,
           float(pixel_offset), float(znear), C, _lib.ptr(attributes),
           host_array(ctypes.c_float, [] if background is None else [float(b) for b in background]), int(flags),
           _lib.ptr(out.get("pix_to_face")), _lib.ptr(out.get("zbuf")), _lib.ptr(out.get("bary")), _lib.ptr(out.get("attr")),
           _lib.ptr(out.get("normal")), _lib.ptr(seen), _lib.ptr(out.get("stats")),
           workspace=lib.g4s_mesh_raster_workspace(F, W, H))
    return out


def rasterize_mesh(mesh, camera, image_size=None, pixel_offset=0.5, znear=1e-6, return_stats=False):
    """(pix_to_face [H,W] int32 with -1 where nothing won, zbuf [H,W] with 0 there, bary_coords [H,W,3]) on the device; with
    return_stats also stats [2] int32: the faces skipped as behind or non-finite, and as beyond the guard band."""
    dm, _host = _checked_mesh(mesh)
    want = ("pix_to_face", "zbuf", "bary") + (("stats",) if return_stats else ())
    o = _raster(dm, camera, image_size, pixel_offset, znear, want)
    return tuple(o[k] for k in want)


def render_mesh(mesh, camera, image_size=None, pixel_offset=0.5, znear=1e-6, background_color=(0, 0, 0),
                use_gaussian_surfels_convention=True, flip_normals_toward_camera=True):
    """render_mesh_with_pytorch3d's dict: rgb [H,W,3] (the interpolated vertex colours over background_color), depth [H,W],
    normal [H,W,3] (the face normal in view space), pix_to_face [H,W], bary_coords [H,W,3], on the device."""
    dm, _host = _checked_mesh(mesh)
    if len(background_color) != 3:
        raise ValueError("background_color must have three components")
    flags = (FLIP_NORMALS if flip_normals_toward_camera else 0) | (SURFELS_CONVENTION if use_gaussian_surfels_convention else 0)
    o = _raster(dm, camera, image_size, pixel_offset, znear, ("pix_to_face", "zbuf", "bary", "attr", "normal"),
                attributes=dm.vertex_colors, background=background_color, flags=flags)
    return {"rgb": o["attr"], "depth": o["zbuf"], "normal": o["normal"], "pix_to_face": o["pix_to_face"], "bary_coords": o["bary"]}


def _visible(dm, cameras, image_sizes):
    cameras = list(cameras)
    sizes = [None] * len(cameras) if image_sizes is None else list(image_sizes)
    if len(sizes) != len(cameras):
        raise ValueError(f"{len(cameras)} cameras but {len(sizes)} image sizes")
    seen = torch.zeros(max(dm.triangles.size(0), 1), dtype=torch.uint8, device=dm.vertices.device)
    for cam, size in zip(cameras, sizes):
        _raster(dm, cam, size, 0.5, 1e-6, (), seen=seen)
    return seen[: dm.triangles.size(0)]


def visible_face_mask(mesh, cameras, image_sizes=None):
    """bool [F] on the device: the faces that win a pixel in at least one of the cameras' images."""
    dm, _host = _checked_mesh(mesh)
    return _visible(dm, cameras, image_sizes).bool()


def cull_unseen_faces(mesh, cameras, image_sizes=None):
    """The mesh without the faces no camera sees, and without the vertices nothing names any more (compact_mesh)."""
    dm, host = _checked_mesh(mesh)
    return _returned(compact_mesh(dm, _visible(dm, cameras, image_sizes)), host)


# ---- dilated depth -----------------------------------------------------------------------------------------------------
def dilated_depths(views, dilation_pixels=1.5, max_dilation=1e8, znear=1e-6):
    """g4s_depth_dilate over a stack of views (camera, depth [H,W] / [1,H,W], rgb [3,H,W] or None) of any sizes, the triples
    adaptive_tsdf takes: [(depth [H,W], rgb [3,H,W] or None)] per view -- every depth map back-projected into its own camera,
    moved by min(dilation_pixels / focal * depth, max_dilation) along its vertex normals, rendered back; the input where
    nothing was drawn.  rgb is given for every view or for none."""
    views = list(views)
    if not views:
        return []
    with_rgb = [rgb is not None for _cam, _d, rgb in views]
    if any(with_rgb) != all(with_rgb):
        raise RuntimeError("rgb must be given for every view or for none")
    first = views[0][1]
    if not isinstance(first, torch.Tensor):
        raise RuntimeError("depth must be a tensor on a HIP device")
    dev = hip_device(first.device)
    for _cam, d, _rgb in views:
        if not isinstance(d, torch.Tensor) or not d.dtype.is_floating_point:
            raise RuntimeError("depth must be a floating-point tensor on a HIP device")
    stack = ViewStack(views, dev, all(with_rgb), 1, lambda cam: [_view_and_projection(cam)[1]])
    out_d = [torch.empty(stack.size(v), dtype=torch.float32, device=dev) for v in range(stack.n)]
    out_c = [torch.empty((3,) + stack.size(v), dtype=torch.float32, device=dev) for v in range(stack.n)] if all(with_rgb) else None
    nbytes = _lib.load().g4s_depth_dilate_workspace(stack.n, stack.sizes)
    if nbytes == 0:
        raise ValueError("at most 65535 views with fewer than 2^31 pixels together")
    launch(dev, "g4s_depth_dilate", *stack.head, stack.rgb, float(dilation_pixels), float(max_dilation), float(znear),
           _lib.ptrs(out_d), None if out_c is None else _lib.ptrs(out_c), workspace=nbytes, sync=True)
    return [(d, None if out_c is None else out_c[v]) for v, d in enumerate(out_d)]


def get_dilated_depth(view, depth, dilation_pixels, rgb=None, max_dilation=1e8):
    """The reference's get_dilated_depth: depth (H,W), (1,H,W) or (H,W,1) and rgb (3,H,W) or (H,W,3) in, the same shapes
    out; (depth, None) without rgb."""
    if not isinstance(depth, torch.Tensor):
        raise RuntimeError("depth must be a tensor on a HIP device")
    if depth.dim() == 3 and depth.size(-1) == 1 and depth.size(0) != 1:
        plane = depth[..., 0]
    elif depth.dim() == 3 and depth.size(0) == 1:
        plane = depth[0]
    else:
        plane = depth
    if plane.dim() != 2:
        raise RuntimeError(f"depth must be (H,W), (1,H,W) or (H,W,1) (got {tuple(depth.shape)})")
    channels_first = True
    planes = rgb
    if rgb is not None:
        if not isinstance(rgb, torch.Tensor) or rgb.dim() != 3:
            raise RuntimeError("rgb must be a (3,H,W) or (H,W,3) tensor")
        channels_first = rgb.size(0) == 3  # the reference's test
        planes = rgb if channels_first else rgb.permute(2, 0, 1)
    (d, c), = dilated_depths([(view, plane, planes)], dilation_pixels, max_dilation)
    if c is not None and not channels_first:
        c = c.permute(1, 2, 0).contiguous()
    return d.reshape(depth.shape), c
