"""Tetrahedral mesh extraction without a GPU: the numpy restatement of the contract (tests/tetra_ref.py) against the
reference's recorded results (tests/golden/tetra_tsdf.npz) and against closed-form facts, the generated table, the host
side of the new entry points, and the plain-torch helpers of g4splat_amd/mesh.py."""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tetra_ref as tr
from g4splat_amd import mesh as mesh_mod
from g4splat_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _canon(tri):
    k = int(np.argmin(tri))
    return tuple(int(x) for x in np.roll(tri, -k))


def test_committed_table_is_the_generators_output():
    with open(os.path.join(ROOT, "g4splat_amd", "csrc", "tsdf", "tsdf_mtet_table.h")) as f:
        assert f.read() == tr.gen_mtet_table.render_header()


def test_kuhn_lattice_sphere():
    """6^3 lattice, sdf = |p - 2.4| - 1.9: the counts the reference's marching_tetrahedra gives on this input."""
    p, tets = tr.kuhn_lattice(6)
    assert tets.shape == (750, 4)
    c = np.array([2.4, 2.4, 2.4])
    sdf = (np.linalg.norm(p.astype(np.float64) - c, axis=1) - 1.9).astype(np.float32)
    edges, faces = tr.marching_tetrahedra(len(p), tets, sdf)
    assert edges.shape == (206, 2) and faces.shape == (408, 3)
    assert (edges[:, 0] < edges[:, 1]).all() and ((sdf[edges[:, 0]] > 0) != (sdf[edges[:, 1]] > 0)).all()
    key = edges[:, 0].astype(np.int64) << 32 | edges[:, 1]
    assert (np.diff(key) > 0).all()
    use = tr.edge_use(faces)
    assert all(n + use.get((b, a), 0) == 2 for (a, b), n in use.items())  # every mesh edge: exactly two triangles
    assert all(n == 1 for n in use.values())                              # ... once each way: consistently oriented
    assert len(np.unique(faces)) == 206
    v = (p[edges[:, 0]] + p[edges[:, 1]]).astype(np.float64) / 2
    normal = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    side = (normal * (v[faces].mean(1) - c)).sum(1)
    assert (side > 0).all()  # towards the occupied (sdf > 0) side everywhere: the tets are all positively oriented


@pytest.mark.parametrize("case", range(16))
def test_single_tet_sign_cases(case):
    occ = [(case >> c) & 1 for c in range(4)]
    sdf = np.array([0.5 if o else -0.5 for o in occ], np.float32)
    tets = np.array([[2, 0, 3, 1]], np.int32)  # corner c is point tets[0][c]
    edges, faces = tr.marching_tetrahedra(4, tets, sdf[np.argsort(tets[0])])
    n_occ = sum(occ)
    assert len(faces) == (0, 1, 2, 1, 0)[n_occ]
    want = {tuple(sorted((int(tets[0][a]), int(tets[0][b])))) for a, b in tr.gen_mtet_table.EDGES if occ[a] != occ[b]}
    assert {tuple(e) for e in edges.tolist()} == want and len(edges) == (0, 3, 4, 3, 0)[n_occ]
    if len(faces):
        assert sorted(np.unique(faces).tolist()) == list(range(len(edges)))
        # normals towards the occupied corners, mirrored with the tet's orientation
        pts = np.array([[0.1, 0.2, 0.0], [1.0, 0.1, 0.2], [0.0, 1.1, 0.1], [0.2, 0.0, 0.9]])
        q = pts[tets[0]]
        det = np.linalg.det(np.stack([q[1] - q[0], q[2] - q[0], q[3] - q[0]]))
        v = (pts[edges[:, 0]] + pts[edges[:, 1]]) / 2
        o = np.array([bool(x) for x in occ])
        towards = q[o].mean(0) - q[~o].mean(0)
        for f in faces:
            nrm = np.cross(v[f[1]] - v[f[0]], v[f[2]] - v[f[0]])
            assert (nrm @ towards) * det > 0


def test_zero_and_nan_are_unoccupied_and_bad_tets_are_skipped():
    sdf = np.array([0.0, 1.0, np.nan, -1.0, 2.0], np.float32)
    edges, faces = tr.marching_tetrahedra(5, np.array([[0, 1, 2, 3]], np.int32), sdf)
    assert edges.tolist() == [[0, 1], [1, 2], [1, 3]] and len(faces) == 1
    edges, faces = tr.marching_tetrahedra(5, np.array([[0, 1, 2, 5], [-1, 1, 2, 3]], np.int32), sdf)
    assert edges.shape == (0, 2) and faces.shape == (0, 3)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "tetra_tsdf.npz"))
    views = [(g[f"v{i}_wv"], g[f"v{i}_pm"], g[f"v{i}_depth"], g[f"v{i}_rgb"]) for i in range(5)]
    return SimpleNamespace(g=g, views=views)


def test_restatement_matches_the_reference_field(golden):
    """tsdf and colours of AdaptiveTSDF.integrate, run for real when the golden was made.  tol = 4 x the largest difference
    measured then (5.0e-5 in tsdf, 4.7e-6 in colour: grid_sample's float32 coordinate round trip times the depth slope
    over trunc); no sample is excluded here."""
    g = golden.g
    tsdf, col, used = tr.adaptive_tsdf(g["points"], golden.views, float(g["trunc"]))
    assert used.any(1).sum() > 1500 and (tsdf == -1).sum() > 1500 and (tsdf > 0).sum() > 1000
    tol = float(g["tol"])
    assert 0 < tol <= 1e-3
    assert np.array_equal(tsdf == -1, g["tsdf"] == -1)
    assert np.abs(tsdf - g["tsdf"]).max() <= tol
    assert np.abs(col - g["colors"]).max() <= tol


def test_restatement_matches_the_reference_marching_tetrahedra(golden):
    g = golden.g
    edges, faces = tr.marching_tetrahedra(len(g["lattice"]), g["tets"], g["lattice_sdf"])
    assert len(g["edges"]) > 500 and len(g["faces"]) > 1000
    assert np.array_equal(edges, g["edges"])  # the set, and torch.unique's order too
    mine = sorted(_canon(f) for f in faces)
    ref = sorted(_canon(f) for f in g["faces"])
    assert mine == ref  # the multiset, up to a rotation of each triple, winding kept


def test_host_side_argument_validation(hip_lib):
    lib = hip_lib
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # never dereferenced: validation fails first

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    expect(lib.g4s_atsdf_sample(-1, one, 0.1, 1e-6, 1e6, 0, nul, nul, nul, nul, nul, one, nul, nul, 0, nul), "must not be negative")
    expect(lib.g4s_atsdf_sample(4, one, 0.0, 1e-6, 1e6, 0, nul, nul, nul, nul, nul, one, nul, nul, 0, nul), "trunc_margin")
    expect(lib.g4s_atsdf_sample(4, one, 0.1, 1.0, 0.5, 0, nul, nul, nul, nul, nul, one, nul, nul, 0, nul), "zfar")
    expect(lib.g4s_atsdf_sample(4, nul, 0.1, 1e-6, 1e6, 0, nul, nul, nul, nul, nul, one, nul, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_atsdf_sample(4, one, 0.1, 1e-6, 1e6, 0, nul, nul, nul, nul, nul, nul, nul, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_atsdf_sample(4, one, 0.1, 1e-6, 1e6, 2, nul, one, one, one, nul, one, nul, one, 1 << 20, nul),
           "NULL required pointer")
    mats, sizes, maps = (ctypes.c_float * 32)(), (ctypes.c_int * 4)(64, 48, 0, 48), (ctypes.c_void_p * 2)(256, 256)
    expect(lib.g4s_atsdf_sample(4, one, 0.1, 1e-6, 1e6, 2, mats, mats, sizes, maps, nul, one, nul, one, 8, nul),
           "workspace too small")
    expect(lib.g4s_atsdf_sample(4, one, 0.1, 1e-6, 1e6, 2, mats, mats, sizes, maps, nul, one, nul, one, 1 << 20, nul),
           "view 1: width, height")
    expect(lib.g4s_atsdf_bisect(4, one, 9, one, one, 65, 0.1, 1e-6, 1e6, 0, nul, nul, nul, nul, one, nul, 0, nul), "steps")
    expect(lib.g4s_atsdf_bisect(4, one, 9, one, one, 8, 0.1, 1e-6, 1e6, 0, nul, nul, nul, nul, nul, nul, 0, nul),
           "NULL required pointer")
    expect(lib.g4s_atsdf_bisect(-4, one, 9, one, one, 8, 0.1, 1e-6, 1e6, 0, nul, nul, nul, nul, one, nul, 0, nul),
           "must not be negative")
    assert lib.g4s_atsdf_bisect(0, nul, 9, nul, nul, 8, 0.1, 1e-6, 1e6, 0, nul, nul, nul, nul, nul, nul, 0, nul) == 0
    assert lib.g4s_atsdf_sample(0, nul, 0.1, 1e-6, 1e6, 0, nul, nul, nul, nul, nul, nul, nul, nul, 0, nul) == 0
    totals = (ctypes.c_int * 2)(7, 7)
    expect(lib.g4s_mtet_count(-1, 4, one, one, totals, one, 1 << 20, nul), "n_points")
    expect(lib.g4s_mtet_count(9, 1 << 29, one, one, totals, one, 1 << 20, nul), "n_tets")
    expect(lib.g4s_mtet_count(9, 4, nul, one, totals, one, 1 << 20, nul), "NULL required pointer")
    expect(lib.g4s_mtet_count(9, 4, one, one, nul, one, 1 << 20, nul), "NULL required pointer")
    expect(lib.g4s_mtet_count(9, 4, one, one, totals, one, 8, nul), "workspace too small")
    odd = ctypes.c_void_p(260)  # a tet is read as one 16-byte row
    expect(lib.g4s_mtet_count(9, 4, odd, one, totals, one, 1 << 20, nul), "16-byte aligned")
    expect(lib.g4s_mtet_emit(9, 4, odd, one, one, one, 3, 1, one, 1 << 20, nul), "16-byte aligned")
    assert lib.g4s_mtet_count(9, 0, nul, nul, totals, nul, 0, nul) == 0 and list(totals) == [0, 0]  # T = 0: empty, no launch
    expect(lib.g4s_mtet_emit(9, 4, one, one, one, one, -1, 0, one, 1 << 20, nul), "must not be negative")
    expect(lib.g4s_mtet_emit(9, 4, one, one, nul, one, 3, 1, one, 1 << 20, nul), "NULL required pointer")
    expect(lib.g4s_mtet_emit(9, 4, one, one, one, one, 17, 1, one, 1 << 20, nul), "four per tet")
    expect(lib.g4s_mtet_emit(9, 4, one, one, one, one, 3, 1, one, 8, nul), "workspace too small")
    assert lib.g4s_mtet_emit(9, 4, one, one, nul, nul, 0, 0, nul, 0, nul) == 0  # nothing crosses: nothing to write


def test_workspace_sizes_are_monotone_and_nonzero(hip_lib):
    lib = hip_lib
    sizes = [lib.g4s_atsdf_workspace(v) for v in (0, 1, 2, 70, 1000)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[3] >= 70 * 152
    sizes = [lib.g4s_mtet_workspace(t) for t in (0, 1, 257, 24576, 1 << 20, (1 << 29) - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[3] < sizes[4] < sizes[5]
    assert sizes[4] >= (1 << 20) * (16 + 2 * 32)  # per tet: four counters and two buffers of four 8-byte keys
    assert lib.g4s_mtet_workspace(-1) == 0 and lib.g4s_mtet_workspace(1 << 29) == 0


def test_triangulate_on_the_host():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1, 1, (60, 3)).astype(np.float32)
    cells = mesh_mod.triangulate(torch.from_numpy(pts))
    assert cells.dtype == torch.int32 and cells.dim() == 2 and cells.size(1) == 4 and cells.size(0) > 60
    c = cells.numpy()
    assert c.min() == 0 and c.max() == 59
    q = pts.astype(np.float64)[c]
    vol = np.abs(np.linalg.det(q[:, 1:] - q[:, :1])).sum() / 6
    from scipy.spatial import ConvexHull
    assert vol == pytest.approx(ConvexHull(pts.astype(np.float64)).volume, rel=1e-9)  # the cells tile the hull


def test_tetra_points_layout():
    """scene/gaussian_model.py:318-375: 8 box corners per Gaussian (Gaussian-major), then the centres."""
    rng = np.random.default_rng(11)
    n = 7
    g = SimpleNamespace(get_xyz=torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)),
                        get_scaling=torch.from_numpy(rng.uniform(0.1, 0.3, (n, 2)).astype(np.float32)),
                        _rotation=torch.from_numpy(rng.normal(size=(n, 4)).astype(np.float32)))
    pts, scale = mesh_mod.tetra_points(g, gaussian_flatness=0.01)
    assert pts.shape == (9 * n, 3) and scale.shape == (9 * n, 1)
    assert torch.equal(pts[8 * n:], g.get_xyz)
    corners = pts[:8 * n].reshape(n, 8, 3)
    assert torch.allclose(corners.mean(1), g.get_xyz, atol=1e-6)
    s3 = torch.cat([g.get_scaling, torch.full((n, 1), 0.01)], 1) * 3
    assert torch.allclose((corners - g.get_xyz[:, None]).norm(dim=-1), s3.norm(dim=-1)[:, None].expand(n, 8), atol=1e-5)
    # corner 0 and corner 7 are opposite, corner 1 differs from corner 0 along the (flat) third axis only
    assert torch.allclose(corners[:, 0] + corners[:, 7], 2 * g.get_xyz, atol=1e-5)
    assert torch.allclose((corners[:, 1] - corners[:, 0]).norm(dim=-1), torch.full((n,), 0.06), atol=1e-5)
    assert torch.allclose(scale[:8 * n].reshape(n, 8), s3.max(1).values[:, None].expand(n, 8))
    assert torch.allclose(scale[8 * n:, 0], s3.max(1).values)
    # downsampling: int(n * ratio) Gaussians, boxes grown by ratio^(-1/3); points_idx names them
    gen = torch.Generator().manual_seed(5)
    sub, sub_scale = mesh_mod.tetra_points(g, downsample_ratio=0.5, gaussian_flatness=0.01, generator=gen)
    assert sub.shape == (9 * 3, 3)
    idx = torch.tensor([4, 1])
    two, two_scale = mesh_mod.tetra_points(g, gaussian_flatness=0.01, points_idx=idx)
    assert torch.equal(two[16:], g.get_xyz[idx])
    assert torch.allclose(two_scale[16:, 0], s3.max(1).values[idx] / (2 / 7) ** (1 / 3))


def test_cameras_spatial_extent():
    eyes = [(3.0, 0, 0), (-3.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0)]
    cams = [synthetic.look_at_camera(e, (0, 0, 0.5), (0, 0, 1), math.radians(50), 32, 24) for e in eyes]
    assert mesh_mod.cameras_spatial_extent(cams) == pytest.approx(3.3, rel=1e-5)
