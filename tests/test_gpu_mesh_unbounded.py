"""Unbounded mesh extraction on the MI355X: the explicit-point kernel against the numpy restatement of the contract
(tests/unbounded_ref.py) bit for bit, the lattice kernel against the explicit-point kernel bit for bit, the dense marching
cubes against the restatement, and GaussianExtractor.extract_mesh_unbounded end to end on analytic sphere views."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tsdf_ref
import unbounded_ref as ur
import view_tap_ref
from g4splat_amd import mesh as mesh_mod
from g4splat_amd import ply_io, synthetic
from support import DEV, dev, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene():
    """The golden's inputs: 5 views of 64x48, and the same maps at half resolution (32x24)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "unbounded_tsdf.npz"))
    full = [(g[f"v{i}_fpt"], g[f"v{i}_depth"], g[f"v{i}_rgb"]) for i in range(5)]
    half = [(M, np.ascontiguousarray(d[::2, ::2]), np.ascontiguousarray(c[:, ::2, ::2])) for M, d, c in full]
    frame = dict(center=g["center"], radius=float(g["radius"]), voxel_size=float(g["voxel_size"]))
    return SimpleNamespace(g=g, full=full, half=half, frame=frame)


def _gpu_views(views):
    return [(M, dev(d), dev(c)) for M, d, c in views]


def _gpu_sample(points, views, frame, contracted, rgb):
    out = mesh_mod.unbounded_tsdf(dev(points), _gpu_views(views), frame["center"], frame["radius"], frame["voxel_size"],
                                  contracted=contracted, return_rgb=rgb)
    return tuple(o.cpu().numpy() for o in out) if rgb else out.cpu().numpy()


@pytest.mark.parametrize("contracted", [True, False])
def test_sample_equals_the_restatement_bit_for_bit(hip_lib, scene, contracted):
    pts = scene.g["samples"] if contracted else scene.g["world"]
    f = scene.frame
    want_t, want_c, _m, used = ur.sample(pts, scene.full, f["center"], f["radius"], f["voxel_size"], contracted)
    assert used.any(1).sum() > 500
    got_t, got_c = _gpu_sample(pts, scene.full, f, contracted, True)
    same_bits(got_t, want_t)
    same_bits(got_c, want_c)
    only_t = _gpu_sample(pts, scene.full, f, contracted, False)  # the kernel without colours: the same tsdf
    same_bits(only_t, want_t)


@pytest.mark.parametrize("crop", ["one_column", "one_row", "one_pixel", "mixed"])
def test_sample_on_maps_one_pixel_wide(hip_lib, scene, crop):
    """The tap at the border: in a map of one column, one row or one pixel the upper corner always clamps onto the lower
    one.  World mode with colours, 257 points about the scene.  "mixed" puts a one-column view between two full ones:
    each view's own size is read."""
    rows, cols = {"one_column": (slice(None), slice(32, 33)), "one_row": (slice(24, 25), slice(None)),
                  "one_pixel": (slice(24, 25), slice(32, 33)), "mixed": (slice(None), slice(32, 33))}[crop]
    views = [(M, np.ascontiguousarray(d[rows, cols]), np.ascontiguousarray(c[:, rows, cols]))
             for M, d, c in scene.full]
    if crop == "mixed":
        views = [scene.full[0], views[1], scene.full[2]]
    pts, f = view_tap_ref.probe_points(257, 31), scene.frame
    want_t, want_c, _m, used = ur.sample(pts, views, f["center"], f["radius"], f["voxel_size"], False)
    print(crop, "accepted per view:", used.sum(0))
    assert (used.sum(0) >= 8).all()  # from the restatement alone
    got_t, got_c = _gpu_sample(pts, views, f, False, True)
    same_bits(got_t, want_t)
    same_bits(got_c, want_c)


def _stacks(scene):
    return {
        "five": scene.full,
        "none": [],
        "one": scene.full[2:3],
        "seventy_small": [scene.half[i % 5] for i in range(70)],
        "two_resolutions": [scene.full[0], scene.half[1], scene.full[2], scene.half[3], scene.half[4]],
    }


@pytest.mark.parametrize("N,stack", [(33, "five"), (64, "five"), (33, "none"), (33, "one"), (33, "seventy_small"),
                                     (33, "two_resolutions")])
def test_grid_equals_sample_on_the_explicit_lattice(hip_lib, scene, N, stack):
    """N = 33: partial micro-bricks on every axis (33 = 2 * 16 + 1 = 8 * 4 + 1); R = 1.9: corners beyond norm 2."""
    views, f, R = _stacks(scene)[stack], scene.frame, 1.9
    grid = mesh_mod.unbounded_tsdf_grid(N, R, _gpu_views(views), f["center"], f["radius"], f["voxel_size"], DEV).cpu().numpy()
    assert grid.shape == (N ** 3,)
    want = _gpu_sample(ur.lattice_points(N, R), views, f, True, False)
    same_bits(grid, want)
    if not views:
        assert (grid == 1.0).all()
    else:
        assert (grid < 1.0).sum() > 500 and (grid == 1.0).sum() > 100
        # one view cannot outweigh the prior of +1: (1 + t) / 2 >= 0
        assert (grid < 0).sum() > 20 if len(views) >= 5 else (grid >= 0).all()


@pytest.fixture(scope="module")
def lattice33(scene):
    f = scene.frame
    return mesh_mod.unbounded_tsdf_grid(33, 1.9, _gpu_views(scene.full), f["center"], f["radius"], f["voxel_size"], DEV)


def test_dense_cubes_of_the_lattice_match_the_restatement(hip_lib, scene, lattice33):
    f, R, N = scene.frame, 1.9, 33
    field = lattice33.cpu().numpy()
    same_bits(field, ur.lattice(N, R, scene.full, f["center"], f["radius"], f["voxel_size"]))
    verts, tris = mesh_mod.dense_marching_cubes(lattice33, R, f["center"], f["radius"])
    rv, rt = ur.dense_cubes(field, N, R, f["center"], f["radius"])
    assert len(rt) > 300 and verts.dtype == np.float32 and tris.dtype == np.int32
    assert np.array_equal(tris, rt)
    assert np.abs(verts - rv).max() <= 1e-6
    _t, cols = _gpu_sample(verts, scene.full, f, False, True)
    _rt, rc, _m, _u = ur.sample(rv, scene.full, f["center"], f["radius"], f["voxel_size"], False)
    assert np.abs(cols - rc).max() <= 1e-6
    again = mesh_mod.dense_marching_cubes(lattice33, R, f["center"], f["radius"])
    same_bits(tuple(again), (verts, tris), "second run")
    dv, dt = mesh_mod.dense_marching_cubes(lattice33, R, f["center"], f["radius"], to_host=False)
    assert dv.is_cuda and dt.is_cuda and np.array_equal(dv.cpu().numpy(), verts) and np.array_equal(dt.cpu().numpy(), tris)


def test_dense_cubes_of_analytic_fields(hip_lib):
    N, R = 33, 1.0
    y = ur.lattice_points(N, R).astype(np.float64)
    field = (np.linalg.norm(y, axis=1) - 0.5).astype(np.float32)
    verts, tris = mesh_mod.dense_marching_cubes(dev(field).reshape(N, N, N), R, (0.0, 0.0, 0.0), 1.0)
    rv, rt = ur.dense_cubes(field, N, R, (0.0, 0.0, 0.0), 1.0)
    assert np.array_equal(tris, rt) and np.abs(verts - rv).max() <= 1e-6
    assert len(tris) > 1000 and ur.closed_manifold(len(verts), tris) == 2
    assert np.abs(np.linalg.norm(verts.astype(np.float64), axis=1) - 0.5).max() < 2.0 / 32
    # un-contraction and the clamp of world units
    shell = (np.linalg.norm(y * 1.9, axis=1) - 1.5).astype(np.float32)  # the lattice over [-1.9, 1.9]^3
    verts, tris = mesh_mod.dense_marching_cubes(dev(shell), 1.9, (1.0, 2.0, 3.0), 20.0, max_range=32.0)
    rv, rt = ur.dense_cubes(shell, N, 1.9, (1.0, 2.0, 3.0), 20.0, max_range=32.0)
    assert np.array_equal(tris, rt) and np.abs(verts - rv).max() <= 1e-6 and np.abs(verts).max() == 32.0
    # N = 2: one cube, one negative corner
    for corner in (0, 5, 7):
        cube = np.ones(8, np.float32)
        cube[corner] = -0.25
        verts, tris = mesh_mod.dense_marching_cubes(dev(cube), 0.5, (0.0, 0.0, 0.0), 1.0)
        rv, rt = ur.dense_cubes(cube, 2, 0.5, (0.0, 0.0, 0.0), 1.0)
        assert verts.shape == (3, 3) and tris.shape == (1, 3)
        assert np.array_equal(tris, rt) and np.abs(verts - rv).max() <= 1e-6
    # no crossing: nothing is written, (0,3) arrays
    for value, n in ((1.0, 33), (-1.0, 2), (0.0, 5)):
        verts, tris = mesh_mod.dense_marching_cubes(torch.full((n ** 3,), value, device=DEV), 1.0, (0.0, 0.0, 0.0), 1.0)
        assert verts.shape == (0, 3) and tris.shape == (0, 3) and verts.dtype == np.float32 and tris.dtype == np.int32


def test_extract_mesh_unbounded_end_to_end(hip_lib, tmp_path):
    W, H, dist = 160, 120, 3.0
    rng = np.random.default_rng(5)
    cams, depths, rgbs = [], [], []
    for e in [(dist, 0, 0), (-dist, 0, 0), (0, dist, 0), (0, -dist, 0), (0, 0, dist), (0, 0, -dist)]:
        up = (0, 0, 1) if abs(e[1]) > 0 else (0, 1, 0)
        cam = synthetic.look_at_camera(e, (0, 0, 0), up, math.radians(50), W, H)
        intr, E = mesh_mod.camera_intrinsics(cam), mesh_mod.camera_extrinsic(cam)
        depths.append(dev(tsdf_ref.sphere_depth(E, intr, W, H, (0, 0, 0), 1.0))[None])
        rgbs.append(dev(rng.uniform(0, 1, (3, H, W)).astype(np.float32)))
        cams.append(cam)
    xyz = rng.normal(size=(5000, 3))
    xyz /= np.linalg.norm(xyz, axis=1, keepdims=True)
    gaussians = SimpleNamespace(get_xyz=dev(xyz.astype(np.float32)))
    ex = mesh_mod.GaussianExtractor(gaussians, None, None)
    ex.viewpoint_stack, ex.depthmaps, ex.rgbmaps = cams, depths, rgbs
    ex.estimate_bounding_sphere()
    assert abs(ex.radius - dist) < 1e-3
    mesh = ex.extract_mesh_unbounded(resolution=64)
    assert isinstance(mesh, mesh_mod.TriangleMesh) and ex.unbounded_tsdf is None
    voxel = ex.radius * 2 / 64
    assert ex.unbounded_voxel_size == pytest.approx(voxel) and ex.unbounded_R == pytest.approx(1.0 / 3.0 + 0.01, abs=2e-3)
    verts, cols, tris = mesh
    assert len(tris) > 1000 and cols.shape == verts.shape
    assert cols.min() >= 0.0 and cols.max() <= 1.0 and cols.max() > 0.2
    centre = ex.center.cpu().numpy().astype(np.float64)
    inside = np.linalg.norm((verts - centre) / ex.radius, axis=1) < 1
    assert inside.sum() > 1000
    off = np.abs(np.linalg.norm(verts[inside].astype(np.float64), axis=1) - 1.0)
    assert off.max() <= 6 * voxel, off.max()
    dm = ex.extract_mesh_unbounded(resolution=64, to_host=False, keep_grid=True)
    assert isinstance(dm, mesh_mod.DeviceMesh) and ex.unbounded_tsdf.shape == (64 ** 3,)
    for a, b in zip(mesh, dm):
        assert np.array_equal(a, b.cpu().numpy())
    # the rest of the export takes the result as it is
    kept = mesh_mod.post_process_mesh(mesh, cluster_to_keep=1)
    assert 0 < len(kept.triangles) <= len(tris)
    short = mesh_mod.filter_mesh(mesh, 1.0)
    assert np.array_equal(short.triangles, tris)  # no edge is that long
    path = str(tmp_path / "unbounded.ply")
    ply_io.write_triangle_mesh(path, mesh)
    v2, c2, t2 = ply_io.read_triangle_mesh(path)
    assert np.array_equal(v2, verts) and np.array_equal(t2, tris) and np.abs(c2 - cols).max() <= 0.5 / 255 + 1e-6
