"""Mesh operations on the MI355X (g4splat_amd.mesh over csrc/tsdf/mesh_ops.hip) against the numpy restatement of the
header's semantics (tests/mesh_ops_ref.py): clustering, post_process_mesh, the observed-face cull, filter_mesh, device
residency, and the multi-resolution export end to end on a rendered room.  Inputs come from tsdf_ref / synthetic only."""
import math
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_ops_ref as ref
import tsdf_ref
from g4splat_amd import mesh as mesh_mod
from g4splat_amd import ply_io, synthetic
from support import DEV, device_camera, devs, hosts, same_bits

pytestmark = pytest.mark.gpu


def _assert_mesh_equal(got, want):
    for name, g, w in zip(("vertices", "vertex_colors", "triangles"), got, want):
        same_bits(g, w, name)


# ---- inputs -------------------------------------------------------------------------------------------------------
def _noise_mesh(seed=7, nb=6, shift=0.4, voxel=0.05):
    """Marching cubes (numpy restatement) of an i.i.d.-noise volume of nb^3 blocks, 30 % of the voxels negative: below
    the percolation threshold of the lattice, so the surface falls into thousands of closed pieces of mixed size."""
    rng = np.random.default_rng(seed)
    coords = np.array([(x, y, z) for x in range(nb) for y in range(nb) for z in range(nb)])
    keys = np.sort(tsdf_ref.pack_keys(coords))
    tsdf = (rng.uniform(-1, 1, (len(keys), 512)) + shift).astype(np.float32)
    color = rng.uniform(0, 255, tsdf.shape + (3,)).astype(np.float32)
    return tsdf_ref.extract_mesh(keys, tsdf, np.ones_like(tsdf), color, voxel)


def _sphere_volume(voxel=0.02):
    """The unit sphere fused from six axis views (depth from tsdf_ref.sphere_depth) into a GPU volume."""
    vol = mesh_mod.TSDFVolume(voxel, 4 * voxel, 10.0, DEV, initial_blocks=20000)
    for e in [(6, 0, 0), (-6, 0, 0), (0, 6, 0), (0, -6, 0), (0, 0, 6), (0, 0, -6)]:
        up = (0, 0, 1) if abs(e[1]) > 0 else (0, 1, 0)
        cam = synthetic.look_at_camera(e, (0, 0, 0), up, math.radians(30), 160, 120)
        depth = tsdf_ref.sphere_depth(mesh_mod.camera_extrinsic(cam), mesh_mod.camera_intrinsics(cam), 160, 120, (0, 0, 0), 1.0)
        rgb = np.broadcast_to(np.array([0.8, 0.6, 0.2], np.float32)[:, None, None], (3, 120, 160)).copy()
        vol.integrate(torch.as_tensor(depth, device=DEV), torch.as_tensor(rgb, device=DEV), cam)
    return vol


def _odd_triangles(first_vertex):
    """Hand-made non-manifold fans (five triangles on one edge, twice), repeated-index triangles hanging on them, and
    isolated degenerate triangles; on 40 vertices from first_vertex."""
    f = first_vertex
    fans = [[f, f + 1, f + 2 + k] for k in range(5)] + [[f + 11, f + 10, f + 12 + k] for k in range(5)]
    odd = [[f, f + 2, f + 2], [f + 20, f + 20, f + 20], [f + 21, f + 22, f + 21], [f + 22, f + 21, f + 23],
           [f + 30, f + 31, f + 31], [f + 31, f + 31, f + 30], [f + 12, f + 10, f + 10]]
    return np.array(fans + odd, np.int32)


@pytest.fixture(scope="module")
def sphere_volume(hip_lib):
    return _sphere_volume()


@pytest.fixture(scope="module")
def big_mesh(sphere_volume):
    """Noise pieces + sphere + fans, triangle order shuffled: (vertices, colours, triangles) numpy, and the restatement's
    (labels, sizes)."""
    noise = _noise_mesh()
    sphere = sphere_volume.extract_triangle_mesh()
    nv = len(noise[0]) + len(sphere[0])
    rng = np.random.default_rng(3)
    extra = (rng.normal(size=(40, 3)).astype(np.float32), rng.uniform(0, 1, (40, 3)).astype(np.float32), _odd_triangles(0))
    v, c, t = ref.join_meshes([noise, tuple(sphere), extra])
    assert t.max() < nv + 40 == len(v)
    t = np.ascontiguousarray(t[rng.permutation(len(t))])
    t0 = time.time()
    labels, sizes = ref.cluster_connected_triangles(t)
    print(f"\n[mesh_ops] big mesh: {len(t)} triangles, {len(v)} vertices, {len(np.unique(labels))} clusters, "
          f"sphere {len(sphere[2])} triangles; restatement clustering {time.time() - t0:.1f} s")
    return (v, c, t), labels, sizes


def test_clustering_matches_the_restatement_and_is_bit_reproducible(hip_lib, big_mesh):
    mesh, labels, sizes = big_mesh
    cluster_sizes = sizes[labels == np.arange(len(labels))]
    assert len(mesh[2]) >= 200_000 and len(cluster_sizes) >= 200
    assert cluster_sizes.max() > 10_000 and (cluster_sizes == 1).sum() >= 1 and len(np.unique(cluster_sizes)) > 30
    dm = mesh_mod.DeviceMesh(*devs(mesh))
    torch.cuda.synchronize()
    t0 = time.time()
    got_l, got_s = mesh_mod.cluster_connected_triangles(dm)
    torch.cuda.synchronize()
    print(f"\n[mesh_ops] cluster_connected_triangles: {1e3 * (time.time() - t0):.1f} ms for {len(labels)} triangles")
    assert got_l.device == DEV and got_l.dtype == torch.int32 and got_s.dtype == torch.int32
    assert np.array_equal(got_l.cpu().numpy(), labels)
    assert np.array_equal(got_s.cpu().numpy(), sizes)
    again_l, again_s = mesh_mod.cluster_connected_triangles(dm)
    assert torch.equal(again_l, got_l) and torch.equal(again_s, got_s)
    host_l, host_s = mesh_mod.cluster_connected_triangles(mesh_mod.TriangleMesh(*mesh))  # numpy in, numpy out
    assert isinstance(host_l, np.ndarray) and np.array_equal(host_l, labels) and np.array_equal(host_s, sizes)


@pytest.mark.parametrize("k", [1, 5, 10_000])
def test_post_process_mesh_matches_the_restatement(hip_lib, big_mesh, k):
    mesh, labels, sizes = big_mesh
    n_clusters = int((labels == np.arange(len(labels))).sum())
    kept = sizes >= ref.cluster_threshold(labels, sizes, k)
    print(f"\n[mesh_ops] post_process k={k}: keeps {kept.mean():.3f} of {len(kept)} triangles, {n_clusters} clusters")
    if k == 5:  # an all-or-nothing answer cannot pass
        assert 0.1 <= kept.mean() <= 0.9
    if k == 10_000:
        assert n_clusters < k
    want = ref.post_process_mesh(mesh, k)
    got = mesh_mod.post_process_mesh(mesh_mod.DeviceMesh(*devs(mesh)), cluster_to_keep=k)
    assert isinstance(got, mesh_mod.DeviceMesh) and all(a.device == DEV for a in got)
    assert len(want[2]) > 0
    _assert_mesh_equal(hosts(got), want)
    if k == 5:
        _assert_mesh_equal(mesh_mod.post_process_mesh(mesh_mod.TriangleMesh(*mesh), cluster_to_keep=k), want)


def test_filter_mesh_matches_the_restatement(hip_lib, big_mesh):
    mesh, _l, _s = big_mesh
    lengths = ref.edge_lengths(mesh)
    valid = lengths[np.isfinite(lengths).all(1)]
    thr = float(np.sort(valid.max(1))[len(valid) // 2])  # a length that occurs: the median longest edge (<= keeps it)
    want = ref.filter_mesh(mesh, thr)
    assert 0.3 < len(want[2]) / len(mesh[2]) < 0.7
    got = mesh_mod.filter_mesh(mesh_mod.DeviceMesh(*devs(mesh)), length_threshold=thr)
    _assert_mesh_equal(hosts(got), want)
    _assert_mesh_equal(hosts(mesh_mod.filter_mesh(mesh_mod.DeviceMesh(*devs(mesh)))), ref.filter_mesh(mesh))  # the default 0.05


def test_compaction_handles_empty_results_and_out_of_range_indices(hip_lib):
    rng = np.random.default_rng(1)
    verts, cols = rng.normal(size=(8, 3)).astype(np.float32), rng.uniform(0, 1, (8, 3)).astype(np.float32)
    tris = np.array([[7, 5, 6], [0, 1, 2], [5, 9, 7], [2, 2, 2], [-1, 3, 4]], np.int32)
    dm = mesh_mod.DeviceMesh(*devs((verts, cols, tris)))
    for keep in ([1, 0, 1, 1, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]):
        k = torch.tensor(keep, dtype=torch.uint8, device=DEV)
        _assert_mesh_equal(hosts(mesh_mod.compact_mesh(dm, k)), ref.compact((verts, cols, tris), np.array(keep, bool)))
        _assert_mesh_equal(hosts(mesh_mod.compact_mesh(dm, k, compact_vertices=False)),
                           ref.compact((verts, cols, tris), np.array(keep, bool), compact_vertices=False))
    empty = mesh_mod.post_process_mesh(mesh_mod.TriangleMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32),
                                                             np.zeros((0, 3), np.int32)))
    assert empty.vertices.shape == (0, 3) and empty.triangles.shape == (0, 3)
    labels, sizes = mesh_mod.cluster_connected_triangles(dm)
    want_l, want_s = ref.cluster_connected_triangles(tris)
    assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(sizes.cpu().numpy(), want_s)


def test_device_residency(hip_lib, sphere_volume):
    host = sphere_volume.extract_triangle_mesh()
    dev = sphere_volume.extract_triangle_mesh(to_host=False)
    assert isinstance(host, mesh_mod.TriangleMesh) and isinstance(dev, mesh_mod.DeviceMesh)
    assert all(isinstance(a, torch.Tensor) and a.device == DEV for a in dev)
    assert len(host.triangles) > 10_000
    _assert_mesh_equal(hosts(dev), host)
    cam = synthetic.look_at_camera((6, 0, 0), (0, 0, 0), (0, 1, 0), math.radians(30), 160, 120)
    outs = [mesh_mod.cull_observed_faces(dev, [cam], 6.0), mesh_mod.join_meshes([dev, dev]),
            mesh_mod.post_process_mesh(dev, cluster_to_keep=1), mesh_mod.filter_mesh(dev, 0.03)]
    for out in outs:
        assert isinstance(out, mesh_mod.DeviceMesh) and all(a.device == DEV for a in out)
        assert out.vertices.dtype == torch.float32 and out.triangles.dtype == torch.int32
    assert 0 < outs[0].triangles.size(0) < dev.triangles.size(0)  # the half facing the camera is nearer than 6
    _assert_mesh_equal(hosts(outs[1]), ref.join_meshes([tuple(host), tuple(host)]))
    assert all(isinstance(a, torch.Tensor) and a.device == DEV for a in mesh_mod.cluster_connected_triangles(dev))
    back = mesh_mod.cull_observed_faces(host, [cam], 6.0)
    assert isinstance(back, mesh_mod.TriangleMesh)
    _assert_mesh_equal(back, hosts(outs[0]))


# ---- the rendered room (builders as in tests/test_gpu_mesh.py) -------------------------------------------------------
ROOM = (6.0, 4.0, 3.0)
SCALE_MEAN = 0.03
N_SURFELS = 400_000
FACE_RGB = np.array([[0.9, 0.2, 0.2], [0.2, 0.8, 0.2], [0.2, 0.3, 0.9], [0.9, 0.8, 0.2], [0.2, 0.8, 0.8],
                     [0.8, 0.3, 0.8]], np.float32)
MESH_RES = 256
TRUNC0 = 3.5  # depth_trunc of the first level: the x = +-3 walls are 4.2 from the cameras that face them


def _face_of(p):
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


def _icosahedron(center, radius):
    g = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                  [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    v = (v / np.linalg.norm(v[0]) * radius + np.asarray(center)).astype(np.float32)
    return v, np.full_like(v, 0.5), f


@pytest.fixture(scope="module")
def room(hip_lib):
    from g4splat_amd.gaussian_renderer import render
    host_cams = synthetic.room_cameras(8, 320, 240)
    cams = [device_camera(c) for c in host_cams]
    pipe = SimpleNamespace(depth_ratio=1.0, compute_cov3D_python=False, convert_SHs_python=False)
    ex = mesh_mod.GaussianExtractor(_room_model(), render, pipe)
    ex.reconstruction(cams)
    return ex, host_cams


def test_cull_matches_the_restatement_on_sphere_plus_room(hip_lib, room, sphere_volume):
    ex, host_cams = room
    voxel = 0.03
    room_mesh = ex.extract_mesh_bounded(voxel_size=voxel, sdf_trunc=4 * voxel, depth_trunc=8.0)
    mesh = ref.join_meshes([tuple(sphere_volume.extract_triangle_mesh()), tuple(room_mesh)])
    # a ninth camera near the +x wall looking at it: almost every vertex lies behind it (the w <= 0 path)
    cams = host_cams + [synthetic.look_at_camera((2.0, 0.3, 0.2), (3.0, 0.3, 0.2), (0, 1, 0), math.radians(90), 320, 240)]
    hw = np.c_[mesh[0], np.ones(len(mesh[0]), np.float32)] @ np.asarray(cams[-1].full_proj_transform, np.float32)[:, 3]
    assert (hw <= 0).mean() > 0.5
    near = 2.5
    obs = ref.observed_vertices(mesh[0], cams, near)
    keep = ref.keep_unobserved(mesh[2], obs)
    print(f"\n[mesh_ops] cull: {len(mesh[2])} faces, restatement removes {1 - keep.mean():.3f}")
    assert 0.1 <= 1 - keep.mean() <= 0.9
    dm = mesh_mod.DeviceMesh(*devs(mesh))
    got_keep = mesh_mod.observed_face_mask(dm, cams, near)
    assert got_keep.device == DEV and got_keep.dtype == torch.uint8
    assert np.array_equal(got_keep.cpu().numpy().astype(bool), keep)
    want = ref.compact(mesh, keep)
    _assert_mesh_equal(hosts(mesh_mod.cull_observed_faces(dm, cams, near)), want)
    # cameras given as device tensors, and more of them than one LDS chunk holds (the same nine, repeated)
    dev_cams = [device_camera(c) for c in cams]
    many = [dev_cams[i % 9] for i in range(150)]
    assert np.array_equal(mesh_mod.observed_face_mask(dm, many, near).cpu().numpy().astype(bool), keep)
    only_last = mesh_mod.observed_face_mask(dm, [dev_cams[0]] * 70 + [dev_cams[8]], near).cpu().numpy().astype(bool)
    assert np.array_equal(only_last, ref.keep_unobserved(mesh[2], ref.observed_vertices(mesh[0], [cams[0], cams[8]], near)))


def test_multires_export_of_the_rendered_room(hip_lib, room, tmp_path):
    ex, host_cams = room
    f0 = TRUNC0 / ex.radius
    depths = torch.stack([d.reshape(240, 320) for d in ex.depthmaps])
    beyond = float((depths > TRUNC0).float().mean())
    print(f"\n[mesh_ops] room: radius {ex.radius:.3f}, f0 {f0:.3f}, {beyond:.3f} of the depth pixels beyond {TRUNC0}")
    assert 0.05 < beyond < 0.95  # the first level truncates inside the room
    torch.cuda.synchronize()
    t0 = time.time()
    joined = ex.extract_mesh_multires(multires_factors=(f0, 4 * f0), mesh_res=MESH_RES, to_host=False)
    torch.cuda.synchronize()
    print(f"[mesh_ops] extract_mesh_multires: {time.time() - t0:.2f} s, levels {ex.level_meshes}")
    assert isinstance(joined, mesh_mod.DeviceMesh) and all(a.device == DEV for a in joined)
    (trunc0, voxel0, before0, after0), (trunc1, voxel1, before1, after1) = ex.level_meshes
    assert trunc0 == pytest.approx(TRUNC0) and trunc1 == pytest.approx(4 * TRUNC0)
    assert voxel0 == pytest.approx(TRUNC0 / MESH_RES) and before0 == after0 > 50_000
    assert 0 < after1 < before1  # the far walls come from the second level, the near ones were culled from it
    v, c, t = hosts(joined)
    assert len(t) == after0 + after1
    # the first level is the head of the result, unchanged
    level0 = ex.extract_mesh_bounded(voxel_size=voxel0, sdf_trunc=5.0 * voxel0, depth_trunc=trunc0)
    V0 = len(level0.vertices)
    same_bits([t[:after0], v[:V0], c[:V0]], [level0.triangles, level0.vertices, level0.vertex_colors])
    # the tail is the second level after the restatement's cull, bit for bit
    level1 = ex.extract_mesh_bounded(voxel_size=voxel1, sdf_trunc=5.0 * voxel1, depth_trunc=trunc1)
    assert len(level1.triangles) == before1
    want1 = ref.cull_observed_faces(tuple(level1), host_cams, trunc0)
    _assert_mesh_equal((v[V0:], c[V0:], t[after0:] - V0), want1)
    obs = ref.observed_vertices(v[V0:], host_cams, trunc0)
    assert (~obs[t[after0:] - V0]).any(1).all()  # every kept face has an unobserved vertex
    # geometry: the vertices lie on the analytic walls, each level within its own voxel
    for name, p, voxel in (("level 0", v[:V0], voxel0), ("level 1", v[V0:], voxel1)):
        dist = _box_distance(p.astype(np.float64))
        frac = (dist <= voxel + 2 * SCALE_MEAN).mean()
        print(f"[mesh_ops] {name}: {len(p)} vertices, {frac:.4f} within {voxel + 2 * SCALE_MEAN:.4f} of the walls")
        assert frac >= 0.99, np.quantile(dist, [0.5, 0.99])
    far = np.abs(v[V0:][:, 0]) > 2.8  # on the x = +-3 walls, which no camera sees nearer than the first truncation
    print(f"[mesh_ops] level 1 after the cull: {far.mean():.3f} of its vertices on the far walls")
    assert far.sum() > 0
    # floaters: five icosahedra (20 faces each) mid-room disappear, the walls stay
    centres = np.array([(0.4 * i - 0.8, 0.3, 0.1 * i) for i in range(5)])
    floaters = [mesh_mod.DeviceMesh(*devs(_icosahedron(ctr, 0.05))) for ctr in centres]
    with_floaters = mesh_mod.join_meshes([joined] + floaters)
    assert with_floaters.triangles.size(0) == len(t) + 100
    t0 = time.time()
    post = mesh_mod.post_process_mesh(with_floaters, cluster_to_keep=1)
    torch.cuda.synchronize()
    pv, pc, pt = hosts(post)
    print(f"[mesh_ops] post_process_mesh: {time.time() - t0:.2f} s, {len(pt)} of {len(t)} wall triangles remain")
    assert len(pt) >= 0.95 * len(t)
    fv = hosts(with_floaters)[0]
    near_floater = lambda p: (np.linalg.norm(p[:, None, :].astype(np.float64) - centres[None], axis=2) < 0.06).any(1)
    assert near_floater(fv).sum() == 60 and near_floater(pv).sum() == 0  # the floaters' vertices are gone
    assert len(np.unique(pt)) == len(pv) and pt.min() == 0 and pt.max() == len(pv) - 1
    path = str(tmp_path / "multires_tsdf_post.ply")
    ply_io.write_triangle_mesh(path, post)
    rv, rc, rt = ply_io.read_triangle_mesh(path)
    same_bits([rv, rt], [pv, pt])
    assert np.abs(rc - pc).max() <= 0.5 / 255 + 1e-6
    filtered = mesh_mod.filter_mesh(joined, length_threshold=3 * voxel0)  # drops the coarse level's long edges only
    assert after0 <= filtered.triangles.size(0) < len(t)
