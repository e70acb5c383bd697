"""Mesh extraction on the MI355X: TSDF fusion and marching cubes of g4splat_amd.mesh against the numpy restatement of
the contract (tests/tsdf_ref.py), capacity growth, determinism, and the end-to-end GaussianExtractor on a rendered room."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tsdf_ref
from g4splat_amd import mesh as mesh_mod
from g4splat_amd import synthetic
from support import DEV, dev, device_camera, devs, same_bits

pytestmark = pytest.mark.gpu

V, T = 0.04, 0.16


def _views(n=4, W=160, H=120, seed=0):
    """n views of a unit sphere from the axes (distance 6, 30 degree FoV), random colours partly outside [0,1], a few
    depths beyond depth_trunc, and a random mask on the second view."""
    rng = np.random.default_rng(seed)
    eyes = [(6, 0, 0), (0, 0, -6), (-6, 0.5, 0), (0, 6, 0.3), (0, 0, 6)][:n]
    out = []
    for i, e in enumerate(eyes):
        up = (0, 0, 1) if abs(e[1]) > 1 else (0, 1, 0)
        cam = synthetic.look_at_camera(e, (0, 0, 0), up, math.radians(30), W, H)
        intr, E = mesh_mod.camera_intrinsics(cam), mesh_mod.camera_extrinsic(cam)
        depth = tsdf_ref.sphere_depth(E, intr, W, H, (0, 0, 0), 1.0)
        depth[rng.random(depth.shape) < 0.01] = 50.0  # beyond depth_trunc: invalid
        rgb = rng.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
        mask = rng.random((H, W)).astype(np.float32) if i == 1 else None
        out.append((cam, intr, E, depth, rgb, mask))
    return out


def _gpu_volume(views, initial_blocks=100000):
    vol = mesh_mod.TSDFVolume(V, T, 10.0, DEV, initial_blocks=initial_blocks)
    counts = []
    for cam, _i, _e, depth, rgb, mask in views:
        counts.append(vol.integrate(dev(depth)[None], dev(rgb), cam, dev(mask)))
    torch.cuda.synchronize()
    return vol, counts


def _ref_volume(views):
    ref = tsdf_ref.RefVolume(V, T, 10.0)
    for _c, intr, E, depth, rgb, mask in views:
        ref.integrate(depth, rgb, intr, E, mask)
    return ref


@pytest.fixture(scope="module")
def sphere():
    views = _views()
    vol, counts = _gpu_volume(views)
    return views, vol, counts, _ref_volume(views)


def test_integration_matches_the_numpy_restatement(hip_lib, sphere):
    """Same block keys, same slot order, and bit-equal tsdf / weight / colour: the kernels evaluate the header's float32
    expressions in the header's order without FMA contraction, and / and sqrt are correctly rounded on both sides."""
    _views_, vol, counts, ref = sphere
    keys, slots = vol.table()
    assert vol.num_blocks > 100
    assert np.array_equal(keys, ref.keys)
    assert np.array_equal(slots, ref.slots)
    tsdf, weight, color = vol.voxels()
    rt, rw, rc = ref.voxels()
    assert np.array_equal(weight, rw)
    assert np.array_equal(tsdf, rt), np.abs(tsdf - rt).max()
    assert np.array_equal(color, rc), np.abs(color - rc).max()
    assert (weight > 0).sum() > 1000 and counts[0][1] == counts[0][0]  # the first view allocates all it touches


def test_extraction_matches_the_numpy_restatement_and_is_bit_reproducible(hip_lib, sphere):
    _views_, vol, _counts, ref = sphere
    mesh = vol.extract_triangle_mesh()
    rv, rc, rt = ref.extract()
    assert len(mesh.triangles) > 1000
    assert np.array_equal(mesh.triangles, rt)
    assert np.abs(mesh.vertices - rv).max() <= 1e-6
    assert np.abs(mesh.vertex_colors - rc).max() <= 1e-6
    again = vol.extract_triangle_mesh()
    same_bits(tuple(again), tuple(mesh), "second run")
    assert mesh.vertices.dtype == np.float32 and mesh.triangles.dtype == np.int32
    assert len(np.unique(mesh.triangles)) == len(mesh.vertices)  # no unreferenced vertex


def test_pool_growth_gives_the_same_volume_and_mesh(hip_lib, sphere):
    views, big, _counts, _ref = sphere
    small, _ = _gpu_volume(views, initial_blocks=1)
    assert small.grows >= 3
    for a, b in zip(small.table(), big.table()):
        assert np.array_equal(a, b)
    for a, b in zip(small.voxels(), big.voxels()):
        assert np.array_equal(a, b)
    for a, b in zip(small.extract_triangle_mesh(), big.extract_triangle_mesh()):
        assert np.array_equal(a, b)


def test_all_invalid_depth_gives_an_empty_mesh(hip_lib):
    cam = synthetic.look_at_camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 160, 120)
    vol = mesh_mod.TSDFVolume(V, T, 2.0, DEV)
    for d in (0.0, -1.0, 5.0, float("nan")):  # zero, negative, beyond depth_trunc, NaN: all invalid
        depth = torch.full((120, 160), d, device=DEV)
        assert vol.integrate(depth, torch.zeros((3, 120, 160), device=DEV), cam) == (0, 0)
    assert vol.num_blocks == 0
    mesh = vol.extract_triangle_mesh()
    assert mesh.vertices.shape == (0, 3) and mesh.triangles.shape == (0, 3)


# ---- end to end: the synthetic room rendered through render() ---------------------------------------------------
ROOM = (6.0, 4.0, 3.0)
SCALE_MEAN = 0.03
N_SURFELS = 400_000  # 108 m^2 of walls: ~14 surfels of 2-sigma radius 6 cm per point, opaque in every view
FACE_RGB = np.array([[0.9, 0.2, 0.2], [0.2, 0.8, 0.2], [0.2, 0.3, 0.9], [0.9, 0.8, 0.2], [0.2, 0.8, 0.8],
                     [0.8, 0.3, 0.8]], np.float32)


def _face_of(p):
    """Index of the box face nearest to each point: 2 * axis + (1 if on the + side)."""
    half = np.array(ROOM) / 2
    d = half[None] - np.abs(p)
    ax = np.argmin(d, 1)
    return 2 * ax + (p[np.arange(len(p)), ax] > 0)


def _box_distance(p):
    half = np.array(ROOM) / 2
    q = np.abs(p) - half[None]
    outside = np.linalg.norm(np.maximum(q, 0), axis=1)
    inside = np.minimum(q.max(1), 0)
    return np.abs(outside + inside)


def _room_model():
    from g4splat_amd.gaussian_model import GaussianModel
    sc = synthetic.scene_room(N_SURFELS, seed=4, size=ROOM, scale_mean=SCALE_MEAN, scale_sigma=0.2)
    cols = FACE_RGB[_face_of(sc.means3D.astype(np.float64))]
    m = GaussianModel(sh_degree=3)
    m.create_from_parameters(*devs((sc.means3D, sc.scales, sc.rotations, cols)))
    with torch.no_grad():
        m._opacity.fill_(math.log(0.97 / 0.03))
    m.active_sh_degree = 0
    return m


def test_gaussian_extractor_meshes_the_rendered_room(hip_lib):
    from g4splat_amd.gaussian_renderer import render
    model = _room_model()
    cams = [device_camera(c) for c in synthetic.room_cameras(8, 320, 240)]
    pipe = SimpleNamespace(depth_ratio=1.0, compute_cov3D_python=False, convert_SHs_python=False)
    ex = mesh_mod.GaussianExtractor(model, render, pipe)
    ex.reconstruction(cams)
    assert ex.radius > 0 and ex.center.shape == (3,)
    assert all(d.is_cuda for d in ex.depthmaps) and all(r.is_cuda for r in ex.rgbmaps)
    voxel = 0.02
    mesh = ex.extract_mesh_bounded(voxel_size=voxel, sdf_trunc=4 * voxel, depth_trunc=8.0)
    verts, cols, tris = mesh
    assert len(tris) > 50000
    # geometry: the vertices lie on the analytic walls
    dist = _box_distance(verts.astype(np.float64))
    assert (dist <= voxel + 2 * SCALE_MEAN).mean() >= 0.99, np.quantile(dist, [0.5, 0.99])
    # topology: closed and consistently oriented away from the open border (where observation stops)
    use = tsdf_ref.edge_use(tris)
    border = {v for (a, b), n in use.items() if use.get((b, a), 0) == 0 for v in (a, b)}
    cell = np.floor(verts / (2 * voxel)).astype(np.int64)
    marked = set()
    for c in cell[sorted(border)]:
        for d in np.ndindex(3, 3, 3):
            marked.add(tuple(c + np.array(d) - 1))
    near = np.array([tuple(c) in marked for c in cell])
    checked = 0
    for (a, b), n in use.items():
        if near[a] or near[b]:
            continue
        assert n == 1 and use.get((b, a), 0) == 1, (verts[a], verts[b])
        checked += 1
    assert checked > 0.5 * len(use)
    # colour: the colour of the wall the vertex lies on
    err = np.abs(cols - FACE_RGB[_face_of(verts.astype(np.float64))]).max(1)
    assert np.median(err) < 0.03 and np.quantile(err, 0.9) < 0.1, np.quantile(err, [0.5, 0.9])
    # the streaming path fuses each view right after rendering it: the same mesh
    streamed = ex.extract_mesh_bounded_streaming(cams, voxel_size=voxel, sdf_trunc=4 * voxel, depth_trunc=8.0)
    for a, b in zip(mesh, streamed):
        assert np.array_equal(a, b)
