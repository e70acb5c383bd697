"""Mesh extraction without a GPU: the marching-cubes table, watertightness and accuracy of the numpy restatement of
the TSDF contract (tests/tsdf_ref.py), host-side validation of the TSDF entry points, the mesh PLY round trip."""
import ctypes
import math
import os

import numpy as np
import pytest

import tsdf_ref
from g4splat_amd import mesh as mesh_mod
from g4splat_amd import ply_io, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_mc_table_is_the_generators_output():
    import gen_mc_table
    with open(os.path.join(ROOT, "g4splat_amd", "csrc", "tsdf", "tsdf_mc_table.h")) as f:
        assert f.read() == gen_mc_table.render_header()


def test_mc_table_cases_are_closed_polygons_facing_positive_tsdf():
    tab = tsdf_ref.mc_table()
    assert tab[0] == [] and tab[255] == []
    for cfg, tris in enumerate(tab):
        crossing = {e for e in range(12)
                    if (cfg >> tsdf_ref.gen_mc_table.EDGES[e][0] & 1) != (cfg >> tsdf_ref.gen_mc_table.EDGES[e][1] & 1)}
        assert {e for t in tris for e in t} == crossing, cfg
        # inside the cube every polygon edge is used once each way; the remaining edges lie on the cube's faces
        use = tsdf_ref.edge_use(tris)
        for (a, b), n in use.items():
            assert n == 1, (cfg, a, b)
    # one negative corner at the origin: the triangle's normal points away from it
    (a, b, c), = tab[1]
    mid = lambda e: np.add(*[np.array(tsdf_ref.gen_mc_table.corner_pos(k), float) for k in tsdf_ref.gen_mc_table.EDGES[e]]) / 2
    n = np.cross(mid(b) - mid(a), mid(c) - mid(a))
    assert (n > 0).all()


def _random_volume(seed, nb=2):
    """nb^3 blocks, every weight 1, a random smooth-ish tsdf in [-1, 1], random colours."""
    rng = np.random.default_rng(seed)
    coords = np.array([(x, y, z) for x in range(nb) for y in range(nb) for z in range(nb)])
    keys = tsdf_ref.pack_keys(coords)
    order = np.argsort(keys)
    keys, coords = keys[order], coords[order]
    n = 8 * nb
    g = np.linspace(0, 1, n)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    field = np.zeros_like(X)
    for _ in range(6):
        k = rng.normal(0, 6, 3)
        field += rng.normal() * np.sin(k[0] * X + k[1] * Y + k[2] * Z + rng.uniform(0, 6.3))
    field = np.clip(field / np.abs(field).max(), -1, 1).astype(np.float32)
    lane = np.arange(512)
    loc = np.stack([lane & 7, (lane >> 3) & 7, lane >> 6], 1)
    gv = coords[:, None, :] * 8 + loc[None]
    tsdf = field[gv[..., 0], gv[..., 1], gv[..., 2]]
    weight = np.ones_like(tsdf)
    color = rng.uniform(0, 255, tsdf.shape + (3,)).astype(np.float32)
    return keys, tsdf, weight, color, n


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_tsdf_mesh_is_watertight_away_from_the_grid_boundary(seed):
    keys, tsdf, weight, color, n = _random_volume(seed)
    v = 0.1
    verts, cols, tris = tsdf_ref.extract_mesh(keys, tsdf, weight, color, v)
    assert len(tris) > 100
    assert len(np.unique(tris)) == len(verts)  # no unreferenced vertex
    assert (tris[:, 0] != tris[:, 1]).all() and (tris[:, 1] != tris[:, 2]).all() and (tris[:, 0] != tris[:, 2]).all()
    g = verts / v - 0.5  # voxel units: the grid spans 0 .. n-1
    near = np.any((g < 1.0) | (g > n - 2.0), axis=1)
    use = tsdf_ref.edge_use(tris)
    checked = 0
    for (a, b), cnt in use.items():
        if near[a] or near[b]:
            continue
        assert cnt == 1 and use.get((b, a), 0) == 1, (a, b)
        checked += 1
    assert checked > 100
    assert (cols >= 0).all() and (cols <= 1).all()


def test_noise_tsdf_mesh_has_no_flat_or_repeated_triangles():
    """i.i.d. noise puts ambiguous faces everywhere: no triangle may lie in a cube face (the neighbour would emit it
    reversed), no directed edge may repeat anywhere, and the mesh is closed away from the grid boundary."""
    for cfg, tris in enumerate(tsdf_ref.mc_table()):
        for t in tris:
            faces = [tsdf_ref.gen_mc_table.edge_faces(e) for e in t]
            assert not (faces[0] & faces[1] & faces[2]), (cfg, t)
    rng = np.random.default_rng(7)
    keys, tsdf, weight, color, n = _random_volume(0)
    tsdf = rng.uniform(-1, 1, tsdf.shape).astype(np.float32)
    v = 0.1
    verts, _cols, tris = tsdf_ref.extract_mesh(keys, tsdf, weight, color, v)
    use = tsdf_ref.edge_use(tris)
    assert max(use.values()) == 1
    g = verts / v - 0.5
    near = np.any((g < 1.0) | (g > n - 2.0), axis=1)
    assert all(use.get((b, a), 0) == 1 for (a, b) in use if not (near[a] or near[b]))


def _sphere_views(W=160, H=120, n_views=6, dist=6.0, fov_deg=30.0):
    """Six views from the axes.  Far enough that every point near the sphere projects inside the sphere's silhouette
    in some view (from distance 3 the regions around the cube diagonals stay unobserved: holes)."""
    eyes = [(dist, 0, 0), (-dist, 0, 0), (0, dist, 0), (0, -dist, 0), (0, 0, dist), (0, 0, -dist)][:n_views]
    cams = []
    for e in eyes:
        up = (0, 0, 1) if abs(e[1]) > 0 else (0, 1, 0)
        cams.append(synthetic.look_at_camera(e, (0, 0, 0), up, math.radians(fov_deg), W, H))
    return cams


def test_numpy_pipeline_meshes_a_sphere_closed_and_accurate():
    r, v = 1.0, 0.04
    vol = tsdf_ref.RefVolume(v, 4 * v, 10.0)
    for cam in _sphere_views():
        intr, E = mesh_mod.camera_intrinsics(cam), mesh_mod.camera_extrinsic(cam)
        depth = tsdf_ref.sphere_depth(E, intr, cam.image_width, cam.image_height, (0, 0, 0), r)
        rgb = np.full((3, cam.image_height, cam.image_width), 0.5, np.float32)
        vol.integrate(depth, rgb, intr, E)
    verts, cols, tris = vol.extract()
    assert len(tris) > 1000
    dist = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert np.abs(dist - r).max() <= v
    use = tsdf_ref.edge_use(tris)
    assert all(cnt == 1 and use.get((b, a), 0) == 1 for (a, b), cnt in use.items())  # closed, consistently oriented
    # normals point outwards (towards the cameras, positive tsdf)
    p = verts[tris].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", nrm, p.mean(1)) > 0).mean() > 0.99
    assert np.abs(cols - 127 / 255).max() < 1e-6  # 0.5 * 255 = 127.5 -> 127


def test_camera_intrinsics_follow_to_cam_open3d():
    cam = synthetic.look_at_camera((0, 0, -3), (0, 0, 0), (0, 1, 0), math.radians(60), 160, 120)
    fx, fy, cx, cy = mesh_mod.camera_intrinsics(cam)
    assert cx == pytest.approx((160 - 1) / 2) and cy == pytest.approx((120 - 1) / 2)
    assert fx == pytest.approx(80 / math.tan(math.radians(30)), rel=1e-5)
    assert fy == pytest.approx(60 / math.tan(cam.FoVy / 2), rel=1e-5)
    assert np.array_equal(mesh_mod.camera_extrinsic(cam), cam.world_view_transform.T)


def test_focus_point_of_cameras_looking_at_a_point():
    cams = _sphere_views()
    c2ws = np.array([np.linalg.inv(mesh_mod.camera_extrinsic(c).astype(np.float64)) for c in cams])
    c2ws[:, :3, 3] += np.array([0.5, -0.25, 1.0])  # the rig shifted: every axis passes through the shift
    assert np.allclose(mesh_mod.focus_point(c2ws), [0.5, -0.25, 1.0], atol=1e-9)


def test_tsdf_argument_validation_is_host_side(hip_lib):
    """Every TSDF entry point rejects bad arguments before it touches the device: negative status + a message."""
    from g4splat_amd import _lib
    lib = hip_lib
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    intr = (ctypes.c_float * 4)(100.0, 100.0, 79.5, 59.5)
    bad_intr = (ctypes.c_float * 4)(0.0, 100.0, 79.5, 59.5)
    ext = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    counts = (ctypes.c_int * 2)()

    def expect(rc, text):
        assert rc < 0, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    cap = lib.g4s_tsdf_blocks_per_pixel(160, 120, intr, 0.01, 0.05)
    assert cap >= 4
    expect(lib.g4s_tsdf_blocks_per_pixel(0, 120, intr, 0.01, 0.05), "must be positive")
    expect(lib.g4s_tsdf_blocks_per_pixel(160, 120, bad_intr, 0.01, 0.05), "fx, fy must be positive")
    expect(lib.g4s_tsdf_blocks_per_pixel(160, 120, None, 0.01, 0.05), "NULL required pointer")
    expect(lib.g4s_tsdf_blocks_per_pixel(160, 120, intr, -1.0, 0.05), "must be positive")
    ws = lib.g4s_tsdf_workspace(160, 120, cap, 0)
    assert ws >= 160 * 120 * cap * 16
    assert lib.g4s_tsdf_workspace(0, 0, 0, 100) >= 100 * 512 * 4

    def alloc(W=160, depth=one, i=intr, e=ext, v=0.01, cap_=cap, keys=nul, nb=0, cnt=counts, w=one, wsb=ws):
        return lib.g4s_tsdf_alloc_count(W, 120, depth, nul, i, e, v, 0.05, 3.0, cap_, keys, nb, cnt, w, wsb, nul)
    expect(alloc(W=0), "must be positive")
    expect(alloc(depth=nul), "NULL required pointer")
    expect(alloc(e=None), "NULL required pointer")
    expect(alloc(i=bad_intr), "fx, fy must be positive")
    expect(alloc(v=0.0), "must be positive")
    expect(alloc(nb=5), "NULL required pointer")  # a table of 5 blocks without keys
    expect(alloc(nb=-1, keys=one), "must not be negative")
    expect(alloc(cnt=None), "NULL required pointer")
    expect(alloc(cap_=cap - 1), "blocks_per_pixel")
    expect(alloc(wsb=ws - 1), "workspace too small")
    expect(alloc(w=nul), "workspace too small")

    def merge(nb=10, m=5, nn=2, kin=one, kout=ctypes.c_void_p(512), tsdf=one, pool=100, wsb=ws):
        return lib.g4s_tsdf_merge(160, 120, cap, kin, one, nb, m, nn, kout, ctypes.c_void_p(768), tsdf, one, one, pool,
                                  one, wsb, nul)
    expect(merge(kin=nul), "NULL required pointer")
    expect(merge(tsdf=nul), "NULL required pointer")
    expect(merge(nn=6), "n_new <= n_touched")
    expect(merge(m=-1), "must not be negative")
    expect(merge(pool=11), "cannot hold")
    expect(merge(kout=one), "must not alias")
    expect(merge(wsb=16), "workspace too small")

    def integ(depth=one, rgb=one, m=5, pool=100, wsb=ws, v=0.01):
        return lib.g4s_tsdf_integrate(160, 120, depth, nul, rgb, intr, ext, v, 0.05, 3.0, cap, m, one, one, one, pool,
                                      one, wsb, nul)
    expect(integ(rgb=nul), "NULL required pointer")
    expect(integ(depth=nul), "NULL required pointer")
    expect(integ(m=-1), "not negative")
    expect(integ(m=200), "exceeds")
    expect(integ(v=float("nan")), "must be positive")
    expect(integ(wsb=0), "workspace too small")

    tot = (ctypes.c_int * 2)()
    expect(lib.g4s_tsdf_extract_count(nul, one, 4, one, one, 10, tot, one, 1 << 30, nul), "NULL required pointer")
    expect(lib.g4s_tsdf_extract_count(one, one, 4, one, one, 3, tot, one, 1 << 30, nul), "exceed pool_blocks")
    expect(lib.g4s_tsdf_extract_count(one, one, 4, one, one, 10, None, one, 1 << 30, nul), "NULL required pointer")
    expect(lib.g4s_tsdf_extract_count(one, one, 4, one, one, 10, tot, one, 64, nul), "workspace too small")
    assert lib.g4s_tsdf_extract_count(nul, nul, 0, nul, nul, 0, tot, nul, 0, nul) == 0 and tuple(tot) == (0, 0)
    expect(lib.g4s_tsdf_extract_emit(one, one, 4, one, one, nul, 10, 0.01, one, one, one, 5, 5, one, 1 << 30, nul),
           "NULL required pointer")
    expect(lib.g4s_tsdf_extract_emit(one, one, 4, one, one, one, 10, 0.01, nul, one, one, 5, 5, one, 1 << 30, nul),
           "NULL required pointer")
    expect(lib.g4s_tsdf_extract_emit(one, one, 4, one, one, one, 10, 0.0, one, one, one, 5, 5, one, 1 << 30, nul),
           "must be positive")
    expect(lib.g4s_tsdf_extract_emit(one, one, 4, one, one, one, 10, 0.01, one, one, one, -5, 5, one, 1 << 30, nul),
           "must not be negative")
    expect(lib.g4s_tsdf_extract_emit(one, one, 4, one, one, one, 10, 0.01, one, one, one, 5, 5, one, 64, nul),
           "workspace too small")
    assert _lib.last_error() != ""
    assert lib.g4s_tsdf_blocks_per_pixel(160, 120, intr, 0.01, 0.05) == cap and _lib.last_error() == ""  # a good call clears it


def test_triangle_mesh_ply_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    verts = rng.normal(size=(50, 3)).astype(np.float32)
    cols = (rng.integers(0, 256, (50, 3)) / 255.0).astype(np.float32)
    tris = rng.integers(0, 50, (80, 3)).astype(np.int32)
    path = str(tmp_path / "mesh.ply")
    ply_io.write_triangle_mesh(path, mesh_mod.TriangleMesh(verts, cols, tris))
    v2, c2, t2 = ply_io.read_triangle_mesh(path)
    assert np.array_equal(v2, verts) and np.array_equal(t2, tris)
    assert np.abs(c2 - cols).max() < 1e-6
    with open(path, "rb") as f:
        head = f.read(400).split(b"end_header")[0].decode()
    assert "binary_little_endian" in head and "property uchar red" in head and "property list uchar int vertex_indices" in head
    empty = str(tmp_path / "empty.ply")
    ply_io.write_triangle_mesh(empty, mesh_mod.TriangleMesh(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))))
    v3, c3, t3 = ply_io.read_triangle_mesh(empty)
    assert v3.shape == (0, 3) and t3.shape == (0, 3)
