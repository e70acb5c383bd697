"""Tetrahedral mesh extraction on the MI355X: the point TSDF, the marching tetrahedra and the fused bisection against the
numpy restatement of the contract (tests/tetra_ref.py) bit for bit, and GaussianExtractor.extract_mesh_tetra end to end."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tetra_ref as tr
import view_tap_ref
from g4splat_amd import mesh as mesh_mod
from g4splat_amd import ply_io, synthetic
from support import DEV, dev, device_camera, same_bits

pytestmark = pytest.mark.gpu

TRUNC = 0.1


@pytest.fixture(scope="module")
def scene():
    """5 analytic views of the unit sphere, 64x48, and the same maps at half resolution; sample points around it."""
    full = [v[1:] for v in tr.sphere_views(64, 48, background=0.0, seed=7)]
    half = [(Wv, Pm, np.ascontiguousarray(d[::2, ::2]), np.ascontiguousarray(c[:, ::2, ::2])) for Wv, Pm, d, c in full]
    return SimpleNamespace(full=full, half=half, points=view_tap_ref.probe_points(257, 31))


def _gpu_views(views, rgb=True):
    return [((Wv, Pm), dev(d), dev(c) if rgb else None) for Wv, Pm, d, c in views]


def _stacks(scene):
    return {"five": scene.full, "none": [], "one": scene.full[2:3],
            "two_sizes": [scene.full[0], scene.half[1], scene.full[2], scene.half[3], scene.half[4]]}


@pytest.mark.parametrize("stack,n", [("five", 257), ("five", 255), ("five", 1), ("none", 257), ("one", 257), ("two_sizes", 257)])
def test_adaptive_tsdf_equals_the_restatement_bit_for_bit(hip_lib, scene, stack, n):
    # n = 1 is the first point, in the band around the sphere, so that the one-thread launch does arithmetic too
    views, pts = _stacks(scene)[stack], scene.points[-n:] if n > 1 else scene.points[:1]
    want_t, want_c, used = tr.adaptive_tsdf(pts, views, TRUNC)
    assert n > 1 or (used.any() and want_t[0] != -1)
    got_t, got_c = (o.cpu().numpy() for o in mesh_mod.adaptive_tsdf(dev(pts), _gpu_views(views), TRUNC, return_rgb=True))
    assert got_t.shape == (n,) and got_c.shape == (n, 3)
    same_bits(got_t, want_t)
    same_bits(got_c, want_c)
    only_t = mesh_mod.adaptive_tsdf(dev(pts), _gpu_views(views, rgb=False), TRUNC).cpu().numpy()  # without colours
    same_bits(only_t, want_t)
    assert n < 4 or ((got_t[-4:] == -1).all() and not used[-4:].any())  # unseen keeps -1
    if stack == "none":
        assert (got_t == -1).all() and (got_c == 0).all()
    elif n > 200:
        # The case is not vacuous (a statement about the scene, taken from the restatement alone): a view accepts a point
        # only where its ray meets the sphere and the point is at most trunc behind it, a small share of the points, so
        # the floors count per view -- every view accepts some points, and accepted-outside and unseen points both occur.
        assert (used.sum(0) >= 8).all() and (want_t > 0).sum() >= 8 and (want_t == -1).sum() >= 8


def _cropped(view, rows, cols):
    Wv, Pm, d, c = view
    return Wv, Pm, np.ascontiguousarray(d[rows, cols]), np.ascontiguousarray(c[:, rows, cols])


@pytest.mark.parametrize("crop,floor", [("two_columns", 7), ("two_rows", 7), ("two_by_two", 2), ("mixed", 7)])
def test_adaptive_tsdf_on_maps_two_pixels_wide(hip_lib, scene, crop, floor):
    """The tap at the border: in a map two pixels wide or high every accepted point has its lower corner on the first
    pixel or exactly on the last, where the upper corner clamps.  (A map one pixel wide accepts nothing under
    0 <= ix <= W-1.)  "mixed" puts a two-column view between two full ones: each view's own size is read."""
    rows, cols = {"two_columns": (slice(None), slice(31, 33)), "two_rows": (slice(23, 25), slice(None)),
                  "two_by_two": (slice(23, 25), slice(31, 33)), "mixed": (slice(None), slice(31, 33))}[crop]
    views = [_cropped(v, rows, cols) for v in scene.full]
    if crop == "mixed":
        views = [scene.full[0], views[1], scene.full[2]]
    want_t, want_c, used = tr.adaptive_tsdf(scene.points, views, TRUNC)
    print(crop, "accepted per view:", used.sum(0))
    assert (used.sum(0) >= floor).all()  # from the restatement alone
    got = mesh_mod.adaptive_tsdf(dev(scene.points), _gpu_views(views), TRUNC, return_rgb=True)
    got_t, got_c = (o.cpu().numpy() for o in got)
    same_bits(got_t, want_t)
    same_bits(got_c, want_c)


def _sphere_field(p, centre, radius):
    return (np.linalg.norm(p.astype(np.float64) - np.asarray(centre), axis=1) - radius).astype(np.float32)


def _gpu_mtet(points, tets, sdf):
    e, f = mesh_mod.marching_tetrahedra(dev(points), dev(tets), dev(sdf))
    assert e.dtype == torch.int32 and f.dtype == torch.int32 and e.is_cuda and f.is_cuda
    return e.cpu().numpy(), f.cpu().numpy()


@pytest.fixture(scope="module")
def lattice17():
    p, tets = tr.kuhn_lattice(17)
    sdf = _sphere_field(p, (8.3, 7.9, 8.1), 6.2)
    return p, tets, sdf, tr.marching_tetrahedra(len(p), tets, sdf)


def test_marching_tetrahedra_of_the_17_lattice(hip_lib, lattice17):
    """24 576 tets, lattice edges shared by up to 6 tets; a closed sphere."""
    p, tets, sdf, (want_e, want_f) = lattice17
    assert len(tets) == 24576 and len(want_f) > 3000
    e, f = _gpu_mtet(p, tets, sdf)
    assert np.array_equal(e, want_e) and np.array_equal(f, want_f)
    key = e[:, 0].astype(np.int64) << 32 | e[:, 1]
    assert (np.diff(key) > 0).all()  # no duplicate vertices
    use = tr.edge_use(f)
    assert all(n == 1 and use.get((b, a), 0) == 1 for (a, b), n in use.items())  # each mesh edge used twice
    e2, f2 = _gpu_mtet(p, tets, sdf)
    assert np.array_equal(e, e2) and np.array_equal(f, f2)


@pytest.mark.parametrize("T", [0, 1, 257])
def test_marching_tetrahedra_small_counts(hip_lib, lattice17, T):
    p, tets, sdf, _ = lattice17
    crossing = np.nonzero((tr.tet_cases(len(p), tets, sdf) % 15) != 0)[0]
    sel = tets[crossing[0]: crossing[0] + T]  # starts at a crossing tet
    e, f = _gpu_mtet(p, sel, sdf)
    want_e, want_f = tr.marching_tetrahedra(len(p), sel, sdf)
    assert e.shape == want_e.shape and f.shape == want_f.shape and (T == 0 or len(f) > 0)
    assert np.array_equal(e, want_e) and np.array_equal(f, want_f)


def test_marching_tetrahedra_field_edges(hip_lib, lattice17):
    p, tets, _sdf, _ = lattice17
    for value in (1.0, -1.0, 0.0):  # all outside, all inside, all exactly zero: nothing crosses
        e, f = _gpu_mtet(p, tets, np.full(len(p), value, np.float32))
        assert e.shape == (0, 2) and f.shape == (0, 3)
    # exact zeros at lattice points: a plane through them; zero counts as unoccupied
    plane = (p[:, 0] - 8.0).astype(np.float32)
    assert (plane == 0).sum() == 17 * 17
    e, f = _gpu_mtet(p, tets, plane)
    want_e, want_f = tr.marching_tetrahedra(len(p), tets, plane)
    assert len(want_f) > 500 and np.array_equal(e, want_e) and np.array_equal(f, want_f)
    assert ((plane[e[:, 0]] > 0) != (plane[e[:, 1]] > 0)).all() and (plane[e] >= 0).all()
    # NaN is unoccupied too
    holes = plane.copy()
    holes[::7] = np.nan
    e, f = _gpu_mtet(p, tets, holes)
    want_e, want_f = tr.marching_tetrahedra(len(p), tets, holes)
    assert np.array_equal(e, want_e) and np.array_equal(f, want_f)


def test_marching_tetrahedra_of_more_than_65536_points(hip_lib):
    """41^3 = 68 921 points: point indices of 17 bits, so each key field takes three sort passes where the smaller
    lattices take two.  Every fifth tet of the lattice, an open surface."""
    p, tets = tr.kuhn_lattice(41)
    tets = np.ascontiguousarray(tets[::5])
    sdf = _sphere_field(p, (20.3, 19.9, 20.1), 19.8)
    want_e, want_f = tr.marching_tetrahedra(len(p), tets, sdf)
    assert len(p) > 1 << 16 and len(tets) == 76800 and len(want_f) > 3000
    assert want_e.max() >= 1 << 16 and want_e[:, 0].max() >= 1 << 16  # the 17th bit is set in both key fields
    e, f = _gpu_mtet(p, tets, sdf)
    assert np.array_equal(e, want_e) and np.array_equal(f, want_f)


def test_marching_tetrahedra_takes_a_view_at_an_odd_offset(hip_lib, lattice17):
    """tets as a view that starts 4 bytes into its storage: the front-end hands the kernels an aligned copy."""
    p, tets, sdf, (want_e, want_f) = lattice17
    flat = torch.cat([torch.zeros(1, dtype=torch.int32, device=DEV), dev(tets).reshape(-1)])
    view = flat[1:].reshape(-1, 4)
    assert view.data_ptr() % 16 == 4
    e, f = mesh_mod.marching_tetrahedra(dev(p), view, dev(sdf))
    assert np.array_equal(e.cpu().numpy(), want_e) and np.array_equal(f.cpu().numpy(), want_f)


def test_marching_tetrahedra_indices_near_the_top_of_a_lattice(hip_lib):
    """The crossing lies in the last cubes of a 9^3 lattice: the largest point indices, in both key fields."""
    p, tets = tr.kuhn_lattice(9)
    sdf = _sphere_field(p, (8.0, 8.0, 8.0), 1.7)
    e, f = _gpu_mtet(p, tets, sdf)
    want_e, want_f = tr.marching_tetrahedra(len(p), tets, sdf)
    assert len(want_f) > 20 and want_e.max() == 9 ** 3 - 1 and want_e.min() > 400
    assert np.array_equal(e, want_e) and np.array_equal(f, want_f)


def test_out_of_range_tets_are_refused(hip_lib, lattice17):
    p, tets, sdf, _ = lattice17
    for bad in (len(p), -1):
        t = tets[:300].copy()
        t[123, 2] = bad
        with pytest.raises(RuntimeError, match="outside"):
            mesh_mod.marching_tetrahedra(dev(p), dev(t), dev(sdf))
    with pytest.raises(RuntimeError, match="outside"):
        mesh_mod.bisect_surface(dev(p), dev(np.array([[0, len(p)]], np.int32)), dev(sdf), [], TRUNC)
    with pytest.raises(RuntimeError, match="integer"):
        mesh_mod.bisect_surface(dev(p), dev(np.array([[0.0, 1.0]], np.float32)), dev(sdf), [], TRUNC)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh_mod.adaptive_tsdf(torch.zeros(4, 3), [], TRUNC)


@pytest.fixture(scope="module")
def sphere_mesh(hip_lib, scene):
    """A 13^3 lattice over [-1.5, 1.5]^3 with the fused field of the five views on it."""
    p, tets = tr.kuhn_lattice(13)
    p = ((p / np.float32(12)) * np.float32(3.0) - np.float32(1.5)).astype(np.float32)
    views = _gpu_views(scene.full, rgb=False)
    pts = dev(p)
    sdf = mesh_mod.adaptive_tsdf(pts, views, TRUNC)
    edges, faces = mesh_mod.marching_tetrahedra(pts, dev(tets), sdf)
    return SimpleNamespace(p=p, pts=pts, views=views, sdf=sdf, edges=edges, faces=faces)


def test_bisection_equals_eight_explicit_rounds(hip_lib, scene, sphere_mesh):
    m = sphere_mesh
    E = m.edges.size(0)
    assert E > 300
    got = mesh_mod.bisect_surface(m.pts, m.edges, m.sdf, m.views, TRUNC, steps=8)
    e = m.edges.long()
    l, r, ls = m.pts[e[:, 0]].clone(), m.pts[e[:, 1]].clone(), m.sdf[e[:, 0]].clone()
    for _ in range(8):
        mid = (l + r) / 2
        ms = mesh_mod.adaptive_tsdf(mid, m.views, TRUNC)
        low = ((ms < 0) & (ls < 0)) | ((ms > 0) & (ls > 0))
        l = torch.where(low[:, None], mid, l)
        r = torch.where(low[:, None], r, mid)
        ls = torch.where(low, ms, ls)
    want = ((l + r) / 2).cpu().numpy()
    assert got.shape == (E, 3)
    same_bits(got, want)
    ref = tr.bisect(m.p, m.edges.cpu().numpy(), m.sdf.cpu().numpy(), scene.full, TRUNC, steps=8)
    same_bits(got, ref)
    # steps = 0: the edge midpoints
    mid0 = mesh_mod.bisect_surface(m.pts, m.edges, m.sdf, m.views, TRUNC, steps=0).cpu().numpy()
    same_bits(mid0, (m.pts[e[:, 0]] + m.pts[e[:, 1]]) / 2)
    # every vertex, the rim crossings included, stays on its edge: a midpoint of two floats lies between them
    ends = np.stack([m.p[m.edges.cpu().numpy()[:, 0]], m.p[m.edges.cpu().numpy()[:, 1]]])
    g = got.cpu().numpy()
    assert (g >= ends.min(0)).all() and (g <= ends.max(0)).all()
    # towards the surface, on the edges that straddle the unit sphere.  This is narrower than "the bisected vertices lie
    # closer to the sphere": the other crossings are the rims of what the views see (an unseen point counts as inside),
    # where the field's zero is not the sphere, so nothing is claimed of them beyond staying on their edge.
    r = np.linalg.norm(m.p.astype(np.float64), axis=1)[m.edges.cpu().numpy()]
    straddle = (r.min(1) < 1.0) & (r.max(1) > 1.0)
    off_mid = np.abs(np.linalg.norm(mid0.astype(np.float64), axis=1) - 1.0)[straddle]
    off_bis = np.abs(np.linalg.norm(got.cpu().numpy().astype(np.float64), axis=1) - 1.0)[straddle]
    print(f"straddling edges {straddle.sum()} of {E}: |r - 1| midpoints mean {off_mid.mean():.4f} median "
          f"{np.median(off_mid):.4f}, bisected mean {off_bis.mean():.4f} median {np.median(off_bis):.4f}")
    assert straddle.sum() > 100 and off_bis.mean() < off_mid.mean() and np.median(off_bis) < np.median(off_mid)


def _room_model(n=20000):
    from g4splat_amd.gaussian_model import GaussianModel
    sc = synthetic.scene_room(n, seed=4, size=(6.0, 4.0, 3.0), scale_mean=0.12, scale_sigma=0.2)
    rng = np.random.default_rng(1)
    m = GaussianModel(sh_degree=3)
    m.create_from_parameters(dev(sc.means3D), dev(sc.scales), dev(sc.rotations),
                             dev(rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)))
    with torch.no_grad():
        m._opacity.fill_(math.log(0.97 / 0.03))
    m.active_sh_degree = 2
    return m


def test_extract_mesh_tetra_end_to_end(hip_lib, tmp_path):
    from g4splat_amd.gaussian_renderer import render
    model = _room_model()
    cams = [device_camera(c) for c in synthetic.room_cameras(6, 160, 120)]
    pipe = SimpleNamespace(depth_ratio=1.0, compute_cov3D_python=False, convert_SHs_python=False)
    ex = mesh_mod.GaussianExtractor(model, render, pipe)
    ex.reconstruction(cams)
    n_points = 9 * int(20000 * 0.1)
    k = int(round(n_points ** (1 / 3))) - 1
    lattice_cells = dev(tr.kuhn_lattice(k)[1])  # any cells over the points will do for the plumbing
    runs = [dict(cells=lattice_cells)]
    try:
        import scipy  # noqa: F401
        runs.append(dict(cells=None))
    except ImportError:
        pass
    for kw in runs:
        gen = lambda: torch.Generator().manual_seed(9)
        mesh = ex.extract_mesh_tetra(downsample_ratio=0.1, generator=gen(), **kw)
        assert isinstance(mesh, mesh_mod.TriangleMesh) and model.active_sh_degree == 2
        verts, cols, tris = mesh
        assert len(tris) > 100 and verts.dtype == np.float32 and tris.dtype == np.int32 and cols.shape == verts.shape
        assert tris.min() == 0 and tris.max() == len(verts) - 1 and np.isfinite(verts).all()
        assert cols.min() >= 0.0 and cols.max() <= 1.0 and cols.max() > 0.2
        assert ex.tetra[0].shape == (n_points, 3) and ex.tetra[3].shape == (n_points,)
        again = ex.extract_mesh_tetra(downsample_ratio=0.1, generator=gen(), to_host=False, **kw)
        assert isinstance(again, mesh_mod.DeviceMesh)
        for a, b in zip(mesh, again):
            assert np.array_equal(a, b.cpu().numpy())
        bare = ex.extract_mesh_tetra(downsample_ratio=0.1, generator=gen(), texture_mesh=False, **kw)
        assert np.array_equal(bare.vertices, verts) and (bare.vertex_colors == 0).all()
        # the rest of the export takes the result as it is
        short = mesh_mod.filter_mesh(mesh, 1e6)
        assert np.array_equal(short.triangles, tris) and np.array_equal(short.vertices, verts)
        cut = mesh_mod.filter_mesh(mesh, 0.5)
        assert len(cut.triangles) <= len(tris) and (kw["cells"] is not None or 0 < len(cut.triangles) < len(tris))
        path = str(tmp_path / "tetra.ply")
        ply_io.write_triangle_mesh(path, mesh)
        v2, c2, t2 = ply_io.read_triangle_mesh(path)
        assert np.array_equal(v2, verts) and np.array_equal(t2, tris) and np.abs(c2 - cols).max() <= 0.5 / 255 + 1e-6
