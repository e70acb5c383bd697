"""Mesh extraction from a trained scene: TSDF fusion of rendered depth and marching cubes on the GPU.

The counterpart of 2d-gaussian-splatting/utils/mesh_utils.py:73-182 (GaussianExtractor with open3d's
ScalableTSDFVolume; called from render.py:57-106), over the C ABI of include/g4s_render_maps.h (TSDF section, which
states the semantics).  Depth and colour maps stay on the device; the volume lives in device tensors that grow on the
host's decision (the library never overflows or reallocates anything).

    volume = TSDFVolume(voxel_size, sdf_trunc, depth_trunc, device)
    volume.integrate(depth, rgb, camera)           # per view
    mesh = volume.extract_triangle_mesh()          # TriangleMesh(vertices, vertex_colors, triangles), numpy

The rest of the reference's export (render_multires.py:139-206, utils/mesh_utils.py:22-43, utils/mesh_filter.py) runs on
the device too, over the "mesh operations" of the same header: cull_observed_faces, join_meshes,
cluster_connected_triangles, post_process_mesh, filter_mesh, and GaussianExtractor.extract_mesh_multires that chains
them.  Each takes a TriangleMesh (numpy; uploaded) or a DeviceMesh (tensors) and returns the kind it was given.

Unbounded scenes (mesh_utils.py:184-279 extract_mesh_unbounded, utils/mcube_utils.py) go through the "unbounded TSDF and
dense marching cubes" of the same header: GaussianExtractor.extract_mesh_unbounded fuses every view into a lattice of the
contracted space in one kernel (unbounded_tsdf_grid), extracts it (dense_marching_cubes) and colours the vertices
(unbounded_tsdf); nothing leaves the device before the mesh is complete.

The reference's default mesh (scripts/extract_tetra_mesh.py -> extract_mesh_adaptive_tsdf.py:259-377) goes through the
"adaptive TSDF at points and marching tetrahedra" of the same header (csrc/tsdf/tetra.hip):
GaussianExtractor.extract_mesh_tetra takes the tetra points of the Gaussians (tetra_points), triangulates them on the host
(triangulate) unless the cells are given, evaluates the field at the points (adaptive_tsdf), marches the tetrahedra
(marching_tetrahedra) and bisects every crossing edge against the field in one launch (bisect_surface).
"""
import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._device import ViewStack, default_device, device_points, focal_lengths, hip_device, host_f32, launch, on_device, to_np

VOXELS_PER_BLOCK = 512


class TriangleMesh(NamedTuple):
    vertices: np.ndarray       # [V,3] float32
    vertex_colors: np.ndarray  # [V,3] float32, 0..1
    triangles: np.ndarray      # [F,3] int32, indices into vertices


class DeviceMesh(NamedTuple):
    vertices: torch.Tensor       # [V,3] float32, on the HIP device
    vertex_colors: torch.Tensor  # [V,3] float32, 0..1
    triangles: torch.Tensor      # [F,3] int32, indices into vertices


def _projection_matrix(camera):
    """The camera's projection_matrix (row-vector convention, = Proj^T), or the one of its FoV and clip planes."""
    pm = getattr(camera, "projection_matrix", None)
    if pm is not None:
        return to_np(pm).astype(np.float32)
    from .synthetic import projection_matrix
    return projection_matrix(getattr(camera, "znear", 0.01), getattr(camera, "zfar", 100.0), camera.FoVx,
                             camera.FoVy).T.astype(np.float32)


def camera_intrinsics(camera):
    """(fx, fy, cx, cy) exactly as to_cam_open3d computes them (mesh_utils.py:45-60): projection_matrix @ ndc2pix in
    float32 -- a centred camera gets cx = (W-1)/2."""
    W, H = int(camera.image_width), int(camera.image_height)
    ndc2pix = np.array([[W / 2, 0, 0, (W - 1) / 2], [0, H / 2, 0, (H - 1) / 2], [0, 0, 0, 1]], np.float32).T
    intr = (_projection_matrix(camera) @ ndc2pix)[:3, :3].T
    return np.array([intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2]], np.float32)


def camera_extrinsic(camera):
    """world -> camera 4x4, = world_view_transform.T (mesh_utils.py:62)."""
    return np.ascontiguousarray(to_np(camera.world_view_transform).astype(np.float32).T)


class TSDFVolume:
    """Sparse TSDF volume of 8^3-voxel blocks on one HIP device (the legacy ScalableTSDFVolume with RGB8 colour, as the
    reference configures it; semantics: include/g4s_render_maps.h).  `initial_blocks` sizes the voxel pool; it grows
    (allocate larger, copy) whenever a view brings more new blocks than it holds."""

    def __init__(self, voxel_size, sdf_trunc, depth_trunc, device="cuda", initial_blocks=4096):
        if not (voxel_size > 0 and sdf_trunc > 0 and depth_trunc > 0):
            raise ValueError("voxel_size, sdf_trunc, depth_trunc must be positive")
        self.voxel_size, self.sdf_trunc, self.depth_trunc = float(voxel_size), float(sdf_trunc), float(depth_trunc)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume needs a HIP device (there is no CPU path)")
        self.num_blocks = 0
        self.grows = 0
        cap = max(1, int(initial_blocks))
        self.keys = torch.zeros(1, dtype=torch.int64, device=self.device)   # sorted packed block keys [num_blocks]
        self.slots = torch.zeros(1, dtype=torch.int32, device=self.device)  # pool slot of each key
        self.tsdf = torch.empty(cap * VOXELS_PER_BLOCK, dtype=torch.float32, device=self.device)
        self.weight = torch.empty_like(self.tsdf)
        self.color = torch.empty(cap * VOXELS_PER_BLOCK * 3, dtype=torch.float32, device=self.device)
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)

    @property
    def pool_blocks(self):
        return self.tsdf.numel() // VOXELS_PER_BLOCK

    def _workspace(self, nbytes):
        if self._ws.numel() < nbytes:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._ws

    def _grow(self, need):
        cap = max(need, 2 * self.pool_blocks)
        extra = (cap - self.pool_blocks) * VOXELS_PER_BLOCK
        self.tsdf = torch.cat([self.tsdf, self.tsdf.new_empty(extra)])
        self.weight = torch.cat([self.weight, self.weight.new_empty(extra)])
        self.color = torch.cat([self.color, self.color.new_empty(3 * extra)])
        self.grows += 1

    def integrate(self, depth, rgb, camera, mask=None):
        """Fuse one view: depth [1,H,W] or [H,W], rgb [3,H,W] (0..1), mask [1,H,W] / [H,W] (< 0.5: ignored), all on
        the volume's device; `camera` carries image_width / image_height / FoVx / FoVy / world_view_transform."""
        lib = _lib.load()
        W, H = int(camera.image_width), int(camera.image_height)
        depth = self._map(depth, (H, W), "depth")
        rgb = self._map(rgb, (3, H, W), "rgb")
        mask = None if mask is None else self._map(mask, (H, W), "mask")
        intr, ext = host_f32(camera_intrinsics(camera)), host_f32(camera_extrinsic(camera))
        v, T, D = self.voxel_size, self.sdf_trunc, self.depth_trunc
        cap = lib.g4s_tsdf_blocks_per_pixel(W, H, intr, v, T)
        if cap < 0:
            raise RuntimeError(f"g4s_tsdf_blocks_per_pixel failed ({cap}): {_lib.last_error()}")
        dev, ws = self.device, self._workspace(lib.g4s_tsdf_workspace(W, H, cap, 0))
        counts = (ctypes.c_int * 2)()
        launch(dev, "g4s_tsdf_alloc_count", W, H, _lib.ptr(depth), _lib.ptr(mask), intr, ext, v, T, D, cap, _lib.ptr(self.keys),
               self.num_blocks, counts, workspace=ws)
        m, n_new = counts[0], counts[1]
        n = self.num_blocks + n_new
        if n > self.pool_blocks:  # capacity is decided here, before anything is written
            self._grow(n)
        if m > 0:  # the merge writes the new table and gives every touched block its slot
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            slots = torch.empty(n, dtype=torch.int32, device=dev)
            launch(dev, "g4s_tsdf_merge", W, H, cap, _lib.ptr(self.keys), _lib.ptr(self.slots), self.num_blocks, m, n_new,
                   _lib.ptr(keys), _lib.ptr(slots), _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color),
                   self.pool_blocks, workspace=ws)
            self.keys, self.slots, self.num_blocks = keys, slots, n
            launch(dev, "g4s_tsdf_integrate", W, H, _lib.ptr(depth), _lib.ptr(mask), _lib.ptr(rgb), intr, ext, v, T, D, cap, m,
                   _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color), self.pool_blocks, workspace=ws)
        return m, n_new

    def _map(self, t, shape, name):
        t = on_device(t, self.device, name)
        if t.dim() == len(shape) + 1 and t.size(0) == 1:
            t = t[0]
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{name} must have shape {shape} (got {tuple(t.shape)})")
        return t.float().contiguous()

    def table(self):
        """(keys int64 [n], slots int32 [n]) of the allocated blocks, ascending key, on the host."""
        n = self.num_blocks
        return self.keys[:n].cpu().numpy(), self.slots[:n].cpu().numpy()

    def voxels(self):
        """(tsdf [n,512], weight [n,512], colour [n,512,3]) of the allocated blocks in table order, on the host."""
        _, slots = self.table()
        s = torch.as_tensor(slots, dtype=torch.int64, device=self.device)
        return (self.tsdf.view(-1, VOXELS_PER_BLOCK)[s].cpu().numpy(), self.weight.view(-1, VOXELS_PER_BLOCK)[s].cpu().numpy(),
                self.color.view(-1, VOXELS_PER_BLOCK, 3)[s].cpu().numpy())

    def extract_triangle_mesh(self, to_host=True):
        """Marching cubes over the volume (include/g4s_render_maps.h: indexed, oriented towards the cameras, in a
        defined order; bit-identical between runs).  to_host=False: the same arrays as a DeviceMesh."""
        lib = _lib.load()
        n = self.num_blocks
        if n == 0:
            if not to_host:
                return _empty_device_mesh(self.device)
            return TriangleMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
        dev, ws = self.device, self._workspace(lib.g4s_tsdf_workspace(0, 0, 0, n))
        totals = (ctypes.c_int * 2)()
        launch(dev, "g4s_tsdf_extract_count", _lib.ptr(self.keys), _lib.ptr(self.slots), n, _lib.ptr(self.tsdf),
               _lib.ptr(self.weight), self.pool_blocks, totals, workspace=ws)
        V, F = totals[0], totals[1]
        verts = torch.empty((max(V, 1), 3), dtype=torch.float32, device=dev)
        cols = torch.empty_like(verts)
        tris = torch.empty((max(F, 1), 3), dtype=torch.int32, device=dev)
        launch(dev, "g4s_tsdf_extract_emit", _lib.ptr(self.keys), _lib.ptr(self.slots), n, _lib.ptr(self.tsdf),
               _lib.ptr(self.weight), _lib.ptr(self.color), self.pool_blocks, self.voxel_size, _lib.ptr(verts), _lib.ptr(cols),
               _lib.ptr(tris), V, F, workspace=ws)
        return _returned(DeviceMesh(verts[:V], cols[:V], tris[:F]), to_host)


# ---- mesh operations (include/g4s_render_maps.h, "mesh operations"; csrc/tsdf/mesh_ops.hip) ---------------------------
def _empty_device_mesh(device):
    z = torch.zeros((0, 3), dtype=torch.float32, device=device)
    return DeviceMesh(z, z.clone(), torch.zeros((0, 3), dtype=torch.int32, device=device))


def as_device_mesh(mesh, device=None):
    """(DeviceMesh, was_host): a TriangleMesh is uploaded (to `device` or the current HIP device)."""
    if isinstance(mesh, DeviceMesh):
        dev = mesh.vertices.device
        if dev.type != "cuda" or mesh.vertex_colors.device != dev or mesh.triangles.device != dev:
            raise RuntimeError("a DeviceMesh lives on one HIP device")
        host = False
    else:
        dev = torch.device(device) if device is not None else default_device()
        host = True
    v = torch.as_tensor(np.ascontiguousarray(mesh.vertices, np.float32) if host else mesh.vertices, device=dev)
    c = torch.as_tensor(np.ascontiguousarray(mesh.vertex_colors, np.float32) if host else mesh.vertex_colors, device=dev)
    t = torch.as_tensor(np.ascontiguousarray(mesh.triangles, np.int32) if host else mesh.triangles, device=dev)
    v, c, t = v.float().reshape(-1, 3).contiguous(), c.float().reshape(-1, 3).contiguous(), t.reshape(-1, 3).contiguous()
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    if c.shape != v.shape:
        raise RuntimeError(f"vertex_colors {tuple(c.shape)} must match vertices {tuple(v.shape)}")
    return DeviceMesh(v, c, t), host


def _returned(mesh, host):
    if not host:
        return mesh
    return TriangleMesh(mesh.vertices.cpu().numpy(), mesh.vertex_colors.cpu().numpy(), mesh.triangles.cpu().numpy())


def _keep_mask(n, device):
    return torch.empty(max(n, 1), dtype=torch.uint8, device=device)


def compact_mesh(mesh, keep=None, compact_vertices=True):
    """Stable compaction of a DeviceMesh: the triangles with keep != 0 (all when None) and -- compact_vertices -- only the
    vertices they name, indices rewritten; otherwise the vertex arrays are passed through."""
    lib = _lib.load()
    v, c, t = mesh
    dev = v.device
    V, F = v.size(0), t.size(0)
    totals = (ctypes.c_int * 2)()
    ws = launch(dev, "g4s_mesh_compact_count", V, F, _lib.ptr(t), _lib.ptr(keep), int(compact_vertices), totals,
                workspace=lib.g4s_mesh_compact_workspace(V, F))
    Vo, Fo = totals[0], totals[1]
    to = torch.empty((max(Fo, 1), 3), dtype=torch.int32, device=dev)
    vo = co = None
    if compact_vertices:
        vo = torch.empty((max(Vo, 1), 3), dtype=torch.float32, device=dev)
        co = torch.empty_like(vo)
    launch(dev, "g4s_mesh_compact_emit", V, F, _lib.ptr(v), _lib.ptr(c), _lib.ptr(t), int(compact_vertices), _lib.ptr(vo),
           _lib.ptr(co), _lib.ptr(to), Vo, Fo, workspace=ws)
    if compact_vertices:
        return DeviceMesh(vo[:Vo], co[:Vo], to[:Fo])
    return DeviceMesh(v, c, to[:Fo])


def _camera_matrices(cameras, device):
    """([C,16] world_view_transform, [C,16] full_proj_transform) float32 on `device`, row-vector convention."""
    def stack(name):
        rows = [torch.as_tensor(getattr(cam, name)).detach().to(device=device, dtype=torch.float32).reshape(16)
                for cam in cameras]
        return torch.stack(rows).contiguous() if rows else torch.zeros((0, 16), dtype=torch.float32, device=device)
    return stack("world_view_transform"), stack("full_proj_transform")


def observed_face_mask(mesh, cameras, near_trunc):
    """Keep mask (uint8 [F], 1 = keep) of a DeviceMesh: 0 where all three vertices lie inside some camera's image and
    nearer to it than near_trunc (render_multires.py:164-177)."""
    v, _c, t = mesh
    dev = v.device
    V, F = v.size(0), t.size(0)
    wv, fp = _camera_matrices(cameras, dev)
    observed = _keep_mask(V, dev)
    keep = _keep_mask(F, dev)
    with torch.cuda.device(dev):  # these entry points take a stream and no workspace
        st = _lib.stream(dev)
        _lib.call("g4s_mesh_observed_vertices", V, _lib.ptr(v), wv.size(0), _lib.ptr(wv), _lib.ptr(fp), float(near_trunc),
                  _lib.ptr(observed), st)
        _lib.call("g4s_mesh_keep_unobserved", F, _lib.ptr(t), V, _lib.ptr(observed), _lib.ptr(keep), st)
    return keep[:F]


def cull_observed_faces(mesh, cameras, near_trunc):
    """Drop the faces a finer level already covers (observed_face_mask), then the vertices nothing names any more."""
    dm, host = as_device_mesh(mesh)
    return _returned(compact_mesh(dm, observed_face_mask(dm, cameras, near_trunc)), host)


def join_meshes(meshes):
    """One mesh of all (join_meshes_as_scene): arrays concatenated, indices offset by the vertices before them."""
    meshes = list(meshes)
    if not meshes:
        raise ValueError("join_meshes needs at least one mesh")
    host = not isinstance(meshes[0], DeviceMesh)
    if any(isinstance(m, DeviceMesh) == host for m in meshes):
        raise TypeError("join_meshes takes meshes of one kind")
    if host:
        offs = np.cumsum([0] + [len(m.vertices) for m in meshes[:-1]])
        return TriangleMesh(np.concatenate([np.asarray(m.vertices, np.float32).reshape(-1, 3) for m in meshes]),
                            np.concatenate([np.asarray(m.vertex_colors, np.float32).reshape(-1, 3) for m in meshes]),
                            np.concatenate([np.asarray(m.triangles, np.int32).reshape(-1, 3) + np.int32(o)
                                            for m, o in zip(meshes, offs)]))
    if sum(m.vertices.size(0) for m in meshes) > (2 ** 31 - 1) // 3:
        raise RuntimeError("joined mesh exceeds 2^31 / 3 vertices")
    tris, off = [], 0
    for m in meshes:
        tris.append(m.triangles + off)
        off += m.vertices.size(0)
    return DeviceMesh(torch.cat([m.vertices for m in meshes]), torch.cat([m.vertex_colors for m in meshes]), torch.cat(tris))


def _cluster(dm):
    lib = _lib.load()
    t = dm.triangles
    dev, F = t.device, t.size(0)
    labels = torch.empty(max(F, 1), dtype=torch.int32, device=dev)
    sizes = torch.empty_like(labels)
    launch(dev, "g4s_mesh_cluster_triangles", F, _lib.ptr(t), _lib.ptr(labels), _lib.ptr(sizes),
           workspace=lib.g4s_mesh_cluster_workspace(F))
    return labels[:F], sizes[:F]


def cluster_connected_triangles(mesh):
    """(labels [F], sizes [F]) int32: the smallest triangle index of each triangle's edge-connected cluster and that
    cluster's triangle count (open3d returns dense cluster numbers and per-cluster counts: the same partition)."""
    dm, host = as_device_mesh(mesh)
    labels, sizes = _cluster(dm)
    return (labels.cpu().numpy(), sizes.cpu().numpy()) if host else (labels, sizes)


def post_process_mesh(mesh, cluster_to_keep=1000):
    """mesh_utils.py:22-43: keep the clusters at least as large as the cluster_to_keep-th largest (never smaller than 50
    triangles; ties all kept), drop unreferenced vertices, then degenerate triangles.  With fewer clusters than
    cluster_to_keep the reference raises IndexError; here the smallest cluster size stands in for the k-th largest."""
    if cluster_to_keep < 1:
        raise ValueError("cluster_to_keep must be at least 1")
    dm, host = as_device_mesh(mesh)
    dev, F = dm.triangles.device, dm.triangles.size(0)
    if F == 0:
        return _returned(compact_mesh(dm), host)
    labels, sizes = _cluster(dm)
    # one entry per cluster (its root triangle); only this per-cluster array is sorted, only one number reaches the host
    cluster_sizes = sizes[labels == torch.arange(F, dtype=torch.int32, device=dev)]
    ordered = torch.sort(cluster_sizes, descending=True).values
    kth = int(ordered[min(int(cluster_to_keep), ordered.numel()) - 1])
    keep = _keep_mask(F, dev)
    with torch.cuda.device(dev):
        _lib.call("g4s_mesh_keep_min_size", F, _lib.ptr(sizes), max(kth, 50), _lib.ptr(keep), _lib.stream(dev))
    dm = compact_mesh(dm, keep)
    F = dm.triangles.size(0)
    with torch.cuda.device(dev):
        _lib.call("g4s_mesh_keep_nondegenerate", F, _lib.ptr(dm.triangles), _lib.ptr(keep), _lib.stream(dev))
    return _returned(compact_mesh(dm, keep, compact_vertices=False), host)


def filter_mesh(mesh, length_threshold=0.05):
    """utils/mesh_filter.py:6-32: drop the faces with an edge longer than length_threshold, then unreferenced vertices."""
    dm, host = as_device_mesh(mesh)
    dev, F = dm.triangles.device, dm.triangles.size(0)
    keep = _keep_mask(F, dev)
    with torch.cuda.device(dev):
        _lib.call("g4s_mesh_keep_short_edges", F, _lib.ptr(dm.triangles), dm.vertices.size(0), _lib.ptr(dm.vertices),
                  float(length_threshold), _lib.ptr(keep), _lib.stream(dev))
    return _returned(compact_mesh(dm, keep), host)


# ---- the views of the unbounded and the tetrahedral extraction (_device.ViewStack; csrc/tsdf/view_stack.h)
def _view_and_projection(cam):
    Wv, Pm = (cam.world_view_transform, _projection_matrix(cam)) if hasattr(cam, "world_view_transform") else cam
    return Wv, Pm


# The two fields' (n_matrices, matrices) of ViewStack and the query that sizes their view table.  In place of a camera the
# unbounded field takes the bare 4x4 full_proj_transform and the adaptive one the pair (world_view_transform,
# projection_matrix) of 4x4.
_UTSDF_VIEWS = (1, lambda cam: [getattr(cam, "full_proj_transform", cam)], "g4s_utsdf_workspace")
_ATSDF_VIEWS = (2, _view_and_projection, "g4s_atsdf_workspace")


def _field_views(views, dev, need_rgb, field):
    """(ViewStack, bytes of its view table) of one of the two fields."""
    n_matrices, matrices, query = field
    stack = ViewStack(views, dev, need_rgb, n_matrices, matrices)
    return stack, getattr(_lib.load(), query)(stack.n)


def _sample_views(entry, field, points, views, return_rgb, *field_args):
    """One g4s_*tsdf_sample call: tsdf [n] of `views` at points [n,3], and with return_rgb (tsdf, colour [n,3])."""
    dev, pts = device_points(points)
    n = pts.size(0)
    stack, nbytes = _field_views(views, dev, return_rgb, field)
    tsdf = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    col = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev) if return_rgb else None
    launch(dev, entry, n, _lib.ptr(pts), *field_args, *stack.head, stack.rgb, _lib.ptr(tsdf), _lib.ptr(col), workspace=nbytes,
           sync=True)
    return (tsdf[:n], col[:n]) if return_rgb else tsdf[:n]


# ---- unbounded extraction (include/g4s_render_maps.h, "Unbounded TSDF and dense marching cubes"; csrc/tsdf/unbounded.hip)
def unbounded_tsdf(points, views, center, radius, voxel_size, contracted=True, return_rgb=False):
    """g4s_utsdf_sample: the running-mean TSDF of `views` (see _UTSDF_VIEWS) at explicit points [n,3] (a device tensor) --
    points of the contracted, normalised space (contracted=True; center, radius map them to the world) or world points
    (contracted=False).  Returns tsdf [n], and with return_rgb (tsdf, colour [n,3])."""
    return _sample_views("g4s_utsdf_sample", _UTSDF_VIEWS, points, views, return_rgb, int(bool(contracted)),
                         host_f32(to_np(center)), float(radius), float(voxel_size))


def unbounded_tsdf_grid(resolution, R, views, center, radius, voxel_size, device=None):
    """g4s_utsdf_grid: the same evaluation at the resolution^3 lattice over [-R, R]^3 of the contracted space, generated in
    the kernel; returns tsdf [resolution^3] (x fastest) on the device."""
    dev = hip_device(device if device is not None else default_device())
    N = int(resolution)
    if N < 2 or N ** 3 >= 2 ** 31:
        raise ValueError("resolution must be at least 2 and resolution^3 below 2^31")
    stack, nbytes = _field_views(views, dev, False, _UTSDF_VIEWS)
    tsdf = torch.empty(N ** 3, dtype=torch.float32, device=dev)
    launch(dev, "g4s_utsdf_grid", N, float(R), host_f32(to_np(center)), float(radius), float(voxel_size), *stack.head,
           _lib.ptr(tsdf), workspace=nbytes, sync=True)
    return tsdf


def dense_marching_cubes(tsdf, R, center, radius, max_range=32.0, to_host=True):
    """Marching cubes over a dense lattice tsdf [N,N,N] (stored x fastest: tsdf[k,j,i]) or [N^3] of the contracted space
    over [-R, R]^3: (vertices [V,3] world, clamped to +-max_range; triangles [F,3] int32), numpy or -- to_host=False --
    device tensors.  A field without a sign change gives (0,3) arrays."""
    if not isinstance(tsdf, torch.Tensor):
        tsdf = torch.as_tensor(np.ascontiguousarray(tsdf, np.float32), device=default_device())
    dev = hip_device(tsdf.device)
    f = tsdf.detach().float().contiguous().reshape(-1)
    N = round(f.numel() ** (1.0 / 3.0))
    if N ** 3 != f.numel() or N < 2 or N ** 3 >= 2 ** 31:
        raise ValueError("tsdf must hold N^3 values, N at least 2 and N^3 below 2^31")
    lib = _lib.load()
    c = host_f32(to_np(center))
    totals = (ctypes.c_int * 2)()
    ws = launch(dev, "g4s_dense_mc_count", N, _lib.ptr(f), totals, workspace=lib.g4s_dense_mc_workspace(N))
    V, F = totals[0], totals[1]
    verts = torch.empty((max(V, 1), 3), dtype=torch.float32, device=dev)
    tris = torch.empty((max(F, 1), 3), dtype=torch.int32, device=dev)
    launch(dev, "g4s_dense_mc_emit", N, _lib.ptr(f), float(R), c, float(radius), float(max_range), _lib.ptr(verts),
           _lib.ptr(tris), V, F, workspace=ws, sync=True)
    if to_host:
        return verts[:V].cpu().numpy(), tris[:F].cpu().numpy()
    return verts[:V], tris[:F]


# ---- tetrahedral extraction (include/g4s_render_maps.h, "Adaptive TSDF at points and marching tetrahedra"; csrc/tsdf/tetra.hip)
def adaptive_tsdf(points, views, trunc_margin, return_rgb=False, znear=1e-6, zfar=1e6):
    """g4s_atsdf_sample: the running-mean TSDF of `views` (see _ATSDF_VIEWS) at points [n,3] (a device tensor), with the
    default flags of the reference's AdaptiveTSDF.integrate (matcha/dm_extractors/adaptive_tsdf.py:162-339): a point no
    view accepts keeps -1.  Returns tsdf [n], and with return_rgb (tsdf, colour [n,3])."""
    return _sample_views("g4s_atsdf_sample", _ATSDF_VIEWS, points, views, return_rgb, float(trunc_margin), float(znear),
                         float(zfar))


def _index_rows(rows, width, name, shape, sdf, dev):
    """With _point_sdf and _rows_in_range the checks of marching_tetrahedra and bisect_surface: rows as [m,width]."""
    if not isinstance(rows, torch.Tensor) or not isinstance(sdf, torch.Tensor) or rows.device != dev or sdf.device != dev:
        raise RuntimeError(f"{name} and sdf must be tensors on {dev}")
    if rows.dtype.is_floating_point or rows.numel() % width:
        raise RuntimeError(f"{name} must be an integer tensor {shape}")
    return rows.detach().reshape(-1, width)


def _point_sdf(sdf, n):
    f = sdf.detach().float().reshape(-1).contiguous()
    if f.numel() != n:
        raise RuntimeError(f"sdf must hold one value per point ({f.numel()} for {n} points)")
    return f


def _rows_in_range(rows, name, n):
    """rows as int32, every entry a point of [0, n)."""
    if rows.size(0) > 0 and (int(rows.min()) < 0 or int(rows.max()) >= n):
        raise RuntimeError(f"{name} name a point outside [0, {n})")
    return rows.to(torch.int32).contiguous()


def marching_tetrahedra(points, tets, sdf):
    """g4s_mtet_count / g4s_mtet_emit (utils/tetmesh.py:97-138): tets [T,4] over points [n,3] with the field sdf [n]
    (occupied: sdf > 0), all device tensors.  Returns (edges [E,2] int32: the crossing edges (lo, hi) in ascending order --
    vertex i of the mesh lies on edge i --, faces [F,3] int32 in tet order).  No crossing: (0,2) and (0,3) tensors."""
    dev, pts = device_points(points)
    n = pts.size(0)
    tets = _index_rows(tets, 4, "tets", "[T,4]", sdf, dev)
    f = _point_sdf(sdf, n)
    T = tets.size(0)
    if n >= 2 ** 31 or T > (2 ** 31 - 1) // 4:
        raise RuntimeError("marching tetrahedra takes fewer than 2^31 points and 2^29 tets")
    tets = _rows_in_range(tets, "tets", n)
    if tets.data_ptr() % 16:  # a view at an odd offset: the kernels read a tet as one 16-byte row
        tets = tets.clone()
    lib = _lib.load()
    totals = (ctypes.c_int * 2)()
    ws = launch(dev, "g4s_mtet_count", n, T, _lib.ptr(tets), _lib.ptr(f), totals, workspace=lib.g4s_mtet_workspace(T))
    E, F = totals[0], totals[1]
    edges = torch.empty((max(E, 1), 2), dtype=torch.int32, device=dev)
    faces = torch.empty((max(F, 1), 3), dtype=torch.int32, device=dev)
    launch(dev, "g4s_mtet_emit", n, T, _lib.ptr(tets), _lib.ptr(f), _lib.ptr(edges), _lib.ptr(faces), E, F, workspace=ws,
           sync=True)
    return edges[:E], faces[:F]


def bisect_surface(points, edges, sdf, views, trunc_margin, steps=8, znear=1e-6, zfar=1e6):
    """g4s_atsdf_bisect (extract_mesh_adaptive_tsdf.py:319-349): every crossing edge of marching_tetrahedra bisected `steps`
    times against the field of `views`, all steps in one launch.  Returns vertices [E,3] on the device."""
    dev, pts = device_points(points)
    n = pts.size(0)
    e = _rows_in_range(_index_rows(edges, 2, "edges", "[E,2]", sdf, dev), "edges", n)
    E = e.size(0)
    f = _point_sdf(sdf, n)
    if not 0 <= int(steps) <= 64:
        raise ValueError("steps must be in 0 .. 64")
    stack, nbytes = _field_views(views, dev, False, _ATSDF_VIEWS)
    verts = torch.empty((max(E, 1), 3), dtype=torch.float32, device=dev)
    launch(dev, "g4s_atsdf_bisect", E, _lib.ptr(e), n, _lib.ptr(pts), _lib.ptr(f), int(steps), float(trunc_margin),
           float(znear), float(zfar), *stack.head, _lib.ptr(verts), workspace=nbytes, sync=True)
    return verts[:E]


# corners of the box [-1, 1]^3 in the order of trimesh.creation.box, which the reference takes them from (x slowest)
_BOX_CORNERS = [(x, y, z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)]


@torch.no_grad()
def tetra_points(gaussians, downsample_ratio=None, gaussian_flatness=1e-3, points_idx=None, generator=None):
    """scene/gaussian_model.py:318-375 (get_tetra_points), plain torch: per Gaussian the 8 corners of its +-3 sigma box --
    the two scales padded with gaussian_flatness as the third --, then all the centres.  With downsample_ratio a random
    subset (torch.randperm, `generator`) of int(n * ratio) Gaussians is taken, with points_idx the named ones; their boxes
    grow by ratio^(-1/3).  Returns (points [9 m, 3], scale [9 m, 1]: the largest box half-extent of the point's Gaussian)."""
    from .densify import build_rotation
    xyz_all = gaussians.get_xyz.detach().float()
    rot = getattr(gaussians, "_rotation", None)
    rots = build_rotation((rot if rot is not None else gaussians.get_rotation).detach().float())
    scales = torch.nn.functional.pad(gaussians.get_scaling.detach().float()[:, :2], (0, 1), mode="constant",
                                     value=float(gaussian_flatness))
    if downsample_ratio is None and points_idx is None:
        xyz, scale = xyz_all, scales * 3.0
    else:
        if points_idx is None:
            n = xyz_all.size(0)
            idx = torch.randperm(n, generator=generator)[:int(n * downsample_ratio)].to(xyz_all.device)
        else:
            idx = torch.as_tensor(points_idx, device=xyz_all.device).long()
            downsample_ratio = idx.numel() / xyz_all.size(0)
        xyz, rots = xyz_all[idx], rots[idx]
        scale = scales[idx] * 3.0 / (downsample_ratio ** (1 / 3))
    box = torch.tensor(_BOX_CORNERS, dtype=torch.float32, device=xyz.device).T  # [3,8]
    corners = torch.bmm(rots, box[None] * scale[:, :, None]) + xyz[:, :, None]  # [m,3,8]
    points = torch.cat([corners.permute(0, 2, 1).reshape(-1, 3), xyz], 0).contiguous()
    smax = scale.max(dim=-1, keepdim=True)[0]
    return points, torch.cat([smax.repeat(1, 8).reshape(-1, 1), smax], 0)


def cameras_spatial_extent(cameras):
    """matcha/dm_scene/cameras.py:854-869 (get_spatial_extent): 1.1 x the largest distance of a camera centre from the
    mean of the centres."""
    centres = np.stack([np.linalg.inv(camera_extrinsic(cam).astype(np.float64))[:3, 3] for cam in cameras]).astype(np.float32)
    return 1.1 * float(np.linalg.norm(centres - centres.mean(0, keepdims=True), axis=-1).max())


def triangulate(points):
    """Delaunay tetrahedralisation of points [n,3] on the HOST (scipy.spatial.Delaunay; the reference's step is CGAL on
    the CPU too): int32 [T,4] on the points' device."""
    try:
        from scipy.spatial import Delaunay
    except ImportError as e:
        raise RuntimeError("triangulate needs scipy (scipy.spatial.Delaunay); install it or pass the cells") from e
    dev = points.device if isinstance(points, torch.Tensor) else None
    cells = Delaunay(to_np(points).astype(np.float64).reshape(-1, 3)).simplices
    return torch.as_tensor(np.ascontiguousarray(cells, np.int32), device=dev)


def quantile_linear(values, q):
    """numpy's default (linear-interpolation) quantile of a device tensor: sorted on the device, the two order statistics
    interpolated on the host in float64 (torch.quantile refuses large inputs)."""
    v = torch.sort(values.detach().reshape(-1)).values
    n = v.numel()
    if n == 0:
        raise ValueError("quantile of an empty tensor")
    pos = float(q) * (n - 1)
    lo = min(max(int(math.floor(pos)), 0), n - 1)
    hi = min(lo + 1, n - 1)
    a, b = float(v[lo]), float(v[hi])
    return a + (b - a) * (pos - lo)


def focus_point(c2ws):
    """The point nearest (least squares) to every camera's optical axis: argmin_p sum_i |(I - d_i d_i^T)(p - o_i)|^2,
    d_i the viewing direction (+z of the camera), o_i its centre."""
    c2ws = np.asarray(c2ws, np.float64)
    d, o = c2ws[:, :3, 2], c2ws[:, :3, 3]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    M = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    return np.linalg.solve(M.sum(0), (M @ o[:, :, None]).sum(0))[:, 0]


def sdf_tolerance(camera, depth, tolerance_in_pixels=1.5, max_tolerance=1e8):
    """min(tolerance_in_pixels / focal x depth, max_tolerance) with focal the mean of the camera's two focal lengths at the
    map's size: what evaluate_tsdf's use_sdf_tolerance subtracts from a depth map (an elementwise expression on the device)."""
    H, W = depth.shape[-2:]
    fx, fy = focal_lengths(camera, W, H)
    return (tolerance_in_pixels / ((fx + fy) / 2.0) * depth).clamp(max=max_tolerance)


class GaussianExtractor:
    """mesh_utils.py:73-182 (`GaussianExtractor`): render the views, fuse them into a TSDF volume on the GPU, extract
    the mesh.  `render(camera, gaussians, pipe=, bg_color=)` is gaussian_renderer.render."""

    def __init__(self, gaussians, render, pipe, bg_color=None):
        if bg_color is None:
            bg_color = [0, 0, 0]
        self.gaussians = gaussians
        self.device = gaussians.get_xyz.device
        self._render, self.pipe = render, pipe
        self.background = torch.tensor(bg_color, dtype=torch.float32, device=self.device)
        self.clean()

    def render(self, camera):
        return self._render(camera, self.gaussians, self.pipe, self.background)

    @torch.no_grad()
    def clean(self):
        self.depthmaps, self.rgbmaps, self.viewpoint_stack = [], [], []
        self.tetra = None  # (points, point scales, cells, sdf, edges) of the last extract_mesh_tetra over these maps

    @torch.no_grad()
    def reconstruction(self, viewpoint_stack):
        """Render every view and keep surf_depth / render ON THE DEVICE (the reference moves them to the CPU)."""
        self.clean()
        self.viewpoint_stack = list(viewpoint_stack)
        for cam in self.viewpoint_stack:
            pkg = self.render(cam)
            self.rgbmaps.append(pkg["render"].detach())
            self.depthmaps.append(pkg["surf_depth"].detach())
        self.estimate_bounding_sphere()

    def estimate_bounding_sphere(self):
        """center = the focus point of the cameras' optical axes, radius = the smallest camera distance to it
        (render.py derives depth_trunc = 2 radius from it)."""
        c2ws = np.array([np.linalg.inv(camera_extrinsic(cam).astype(np.float64)) for cam in self.viewpoint_stack])
        center = focus_point(c2ws)
        self.radius = float(np.linalg.norm(c2ws[:, :3, 3] - center, axis=-1).min())
        self.center = torch.from_numpy(center).float().to(self.device)

    @staticmethod
    def _mask(cam, mask_backgrond):
        m = getattr(cam, "gt_alpha_mask", None) if mask_backgrond else None
        return m

    @torch.no_grad()
    def extract_mesh_bounded(self, voxel_size=0.004, sdf_trunc=0.02, depth_trunc=3, mask_backgrond=True, to_host=True):
        """TSDF fusion of the maps of reconstruction() and marching cubes (the reference's spelling of the keyword)."""
        volume = TSDFVolume(voxel_size, sdf_trunc, depth_trunc, self.device)
        for cam, depth, rgb in zip(self.viewpoint_stack, self.depthmaps, self.rgbmaps):
            m = self._mask(cam, mask_backgrond)
            volume.integrate(depth, rgb, cam, None if m is None else m.to(self.device))
        self.volume = volume
        return volume.extract_triangle_mesh(to_host=to_host)

    @torch.no_grad()
    def extract_mesh_multires(self, multires_factors=(2, 8, 16), mesh_res=1024, mask_backgrond=True, to_host=True):
        """render_multires.py:129-190 over the maps of reconstruction(): one bounded extraction per factor with
        depth_trunc = radius * factor, voxel_size = depth_trunc / mesh_res, sdf_trunc = 5 voxel_size; every level after
        the first loses the faces the cameras see nearer than the previous level's depth_trunc; the levels are joined in
        order.  Meshes stay on the device between the steps and one volume is alive at a time.  Levels that end up
        without faces are skipped.  `self.level_meshes` keeps the (depth_trunc, voxel_size, faces before the cull,
        faces after) of every level."""
        levels, self.level_meshes, previous_trunc = [], [], None
        for factor in multires_factors:
            depth_trunc = self.radius * factor
            voxel_size = depth_trunc / mesh_res
            self.volume = None  # the previous level's pool is released before the next one is allocated
            mesh = self.extract_mesh_bounded(voxel_size=voxel_size, sdf_trunc=5.0 * voxel_size, depth_trunc=depth_trunc,
                                             mask_backgrond=mask_backgrond, to_host=False)
            before = mesh.triangles.size(0)
            if previous_trunc is not None and before > 0:
                mesh = compact_mesh(mesh, observed_face_mask(mesh, self.viewpoint_stack, previous_trunc))
            previous_trunc = depth_trunc
            self.level_meshes.append((depth_trunc, voxel_size, before, mesh.triangles.size(0)))
            if mesh.triangles.size(0) > 0:
                levels.append(mesh)
        self.volume = None
        joined = join_meshes(levels) if levels else _empty_device_mesh(self.device)
        return _returned(joined, to_host)

    def _unbounded_views(self):
        return list(zip(self.viewpoint_stack, self.depthmaps, self.rgbmaps))

    @torch.no_grad()
    def extract_mesh_unbounded(self, resolution=1024, to_host=True, max_range=32.0, keep_grid=False):
        """mesh_utils.py:184-279 over the maps of reconstruction(): a TSDF over a resolution^3 lattice of the contracted,
        normalised space (voxel_size = 2 radius / resolution, half extent R = min(q + 0.01, 1.9) with q the 0.95 quantile
        of the Gaussians' contracted norms), dense marching cubes, vertices back in the world and clamped to
        +-max_range, colours from a world-mode evaluation at the vertices.  Stated differences (include/g4s_render_maps.h):
        one lattice of any resolution instead of 512^3 crops, triangles face positive tsdf, no vertex merge (vertices are
        shared by construction).  keep_grid=True leaves the lattice in self.unbounded_tsdf."""
        N = int(resolution)
        voxel_size = self.radius * 2 / N
        x = (self.gaussians.get_xyz.detach().float() - self.center) / self.radius
        mag = torch.linalg.norm(x, ord=2, dim=-1)[..., None]
        contracted = torch.where(mag < 1, x, (2 - (1 / mag)) * (x / mag))
        R = min(quantile_linear(contracted.norm(dim=-1), 0.95) + 0.01, 1.9)
        self.unbounded_R, self.unbounded_voxel_size = R, voxel_size
        views = self._unbounded_views()
        self.unbounded_tsdf = unbounded_tsdf_grid(N, R, views, self.center, self.radius, voxel_size, self.device)
        verts, tris = dense_marching_cubes(self.unbounded_tsdf, R, self.center, self.radius, max_range, to_host=False)
        if not keep_grid:
            self.unbounded_tsdf = None
        if verts.size(0) > 0:
            _t, cols = unbounded_tsdf(verts, views, self.center, self.radius, voxel_size, contracted=False, return_rgb=True)
        else:
            cols = torch.zeros((0, 3), dtype=torch.float32, device=verts.device)
        return _returned(DeviceMesh(verts, cols, tris), to_host)

    @torch.no_grad()
    def extract_mesh_tetra(self, downsample_ratio=0.5, gaussian_flatness=2e-4, truncation_margin=5e-3, texture_mesh=True,
                           cells=None, n_binary_steps=8, to_host=True, generator=None, use_dilated_depth=False,
                           use_sdf_tolerance=False):
        """extract_mesh_adaptive_tsdf.py:259-377 over the maps of reconstruction() (rendered with pipe.depth_ratio = 1.0, as
        the reference's configuration does): tetra points of the Gaussians, their tetrahedralisation (`cells` [T,4] as the
        reference's cells.pt holds them, or triangulate()), the adaptive TSDF at the points with trunc = truncation_margin
        x the cameras' spatial extent, marching tetrahedra, n_binary_steps bisections of every crossing edge in one launch,
        and -- texture_mesh -- vertex colours from a second render pass at SH degree 0 evaluated at the final vertices.
        Stated differences (include/g4s_render_maps.h): triangles in tet order, only the default flags of
        AdaptiveTSDF.integrate, colours from the maps rendered here.  Without texture_mesh the colours are zero.
        Two additions to the reference's signature: `generator` seeds the random subset of tetra_points, and
        `self.tetra` keeps (points, point scales, cells, sdf, edges) of the run until the next reconstruction().
        use_dilated_depth replaces every view's depth -- and, for the colours, rgb -- by mesh_render.dilated_depths(..., 1.5,
        1e-3 x extent) before the sample, the bisection and the colouring; use_sdf_tolerance then subtracts
        min(1.5 / focal x depth, 1e-3 x extent) from the depth (evaluate_tsdf, extract_mesh_adaptive_tsdf.py:168-183).  With
        both off nothing changes."""
        extent = cameras_spatial_extent(self.viewpoint_stack)
        trunc = float(truncation_margin) * extent
        points, scale = tetra_points(self.gaussians, downsample_ratio, float(gaussian_flatness) * extent, generator=generator)
        if cells is None:
            cells = triangulate(points)
        cells = torch.as_tensor(cells).to(points.device)
        views = [(cam, d, None) for cam, d in zip(self.viewpoint_stack, self.depthmaps)]
        coloured = None
        if use_dilated_depth and texture_mesh:
            # the colour maps go through the dilation with the depth they belong to: rendered first, so that the stack is
            # dilated once for the sample, the bisection and the colouring
            coloured = self._adjusted_views([(cam, d, c) for (cam, d, _n), c in zip(views, self._flat_colour_maps())], extent,
                                            True, use_sdf_tolerance)
            views = [(cam, d, None) for cam, d, _c in coloured]
        elif use_dilated_depth or use_sdf_tolerance:
            views = self._adjusted_views(views, extent, use_dilated_depth, use_sdf_tolerance)
        sdf = adaptive_tsdf(points, views, trunc)
        edges, faces = marching_tetrahedra(points, cells, sdf)
        self.tetra = (points, scale, cells, sdf, edges)
        verts = bisect_surface(points, edges, sdf, views, trunc, steps=n_binary_steps)
        cols = torch.zeros_like(verts)
        if texture_mesh and verts.size(0) > 0:
            if coloured is None:
                coloured = [(cam, d, c) for (cam, d, _n), c in zip(views, self._flat_colour_maps())]
            _t, cols = adaptive_tsdf(verts, coloured, trunc, return_rgb=True)
        return _returned(DeviceMesh(verts, cols, faces), to_host)

    def _flat_colour_maps(self):
        """The colour map of every view rendered at SH degree 0."""
        degree = self.gaussians.active_sh_degree
        self.gaussians.active_sh_degree = 0
        try:
            return [self.render(cam)["render"].detach() for cam in self.viewpoint_stack]
        finally:
            self.gaussians.active_sh_degree = degree

    @staticmethod
    def _adjusted_views(views, extent, use_dilated_depth, use_sdf_tolerance):
        """The views as evaluate_tsdf's two depth switches leave them (extract_mesh_adaptive_tsdf.py:168-183)."""
        from .mesh_render import dilated_depths
        limit = 1e-3 * extent
        if use_dilated_depth:
            views = [(cam, d, c) for (cam, _d, _c), (d, c) in zip(views, dilated_depths(views, 1.5, limit))]
        if use_sdf_tolerance:
            views = [(cam, d - sdf_tolerance(cam, d, 1.5, limit), c) for cam, d, c in views]
        return views

    @torch.no_grad()
    def extract_mesh_bounded_streaming(self, viewpoint_stack, voxel_size=0.004, sdf_trunc=0.02, depth_trunc=3,
                                       mask_backgrond=True):
        """Same mesh as reconstruction() + extract_mesh_bounded(), but every view is fused right after it is rendered:
        no map is kept, so hundreds of full-resolution views need only one view's memory."""
        self.clean()
        self.viewpoint_stack = list(viewpoint_stack)
        volume = TSDFVolume(voxel_size, sdf_trunc, depth_trunc, self.device)
        for cam in self.viewpoint_stack:
            pkg = self.render(cam)
            m = self._mask(cam, mask_backgrond)
            volume.integrate(pkg["surf_depth"], pkg["render"], cam, None if m is None else m.to(self.device))
            del pkg
        self.volume = volume
        return volume.extract_triangle_mesh()
