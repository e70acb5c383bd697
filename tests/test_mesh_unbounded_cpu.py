"""Unbounded mesh extraction without a GPU: the numpy restatement of the contract (tests/unbounded_ref.py) against what the
reference's own extract_mesh_unbounded recorded (tests/golden/unbounded_tsdf.npz), its dense marching cubes on analytic
fields, and the host-side validation of the library's entry points."""
import ctypes
import os

import numpy as np
import pytest

import unbounded_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # G4S_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "unbounded_tsdf.npz"))
    views = [(g[f"v{i}_fpt"], g[f"v{i}_depth"], g[f"v{i}_rgb"]) for i in range(5)]
    return g, views


def _check(got, want, margin, tol, what):
    """|got - want| <= tol; at most 5 samples may exceed it, each of them within 1e-5 of deciding otherwise."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if err.ndim == 2:
        err = err.max(1)
    bad = np.nonzero(~(err <= tol))[0]
    print(f"{what}: max error {np.nanmax(err):.3e}, tol {tol:.3e}, {len(bad)} beyond it, their margins {margin[bad]}")
    assert len(bad) <= 5, (what, len(bad))
    assert (margin[bad] < 1e-5).all(), (what, bad, err[bad], margin[bad])


def test_restatement_matches_the_reference_recording(golden):
    g, views = golden
    tol = float(g["tol"])
    assert 0 < tol < 1e-3 and int(g["n_disagree"]) <= 22
    samples = g["samples"]
    norms = np.linalg.norm(samples.astype(np.float64), axis=1)
    assert (norms == 0).any() and (norms == 1).any() and (norms >= 2).sum() > 1000 and norms.max() > 3.2
    tsdf, _col, margins, used = ur.sample(samples, views, g["center"], float(g["radius"]), float(g["voxel_size"]), True)
    assert used.any(1).mean() > 0.3  # the samples inside the contraction ball are observed, many beyond are not
    assert (tsdf < 0).sum() > 500 and ((tsdf > 0) & (tsdf < 1)).sum() > 500
    _check(tsdf, g["tsdf"], margins.min(1), tol, "tsdf of the contracted samples")
    wt, wc, wm, wu = ur.sample(g["world"], views, g["center"], float(g["radius"]), float(g["voxel_size"]), False)
    assert wu.any(1).mean() > 0.5 and wc.max() > 0.3
    _check(wc, g["world_rgb"], wm.min(1), tol, "colours of the world points")
    # the +1 prior darkens: a point seen by n views carries n / (n + 1) of the mean colour, so never more than 5 / 6
    assert wc.max() <= 5.0 / 6.0 + 1e-6


def _sphere_field(N, R):
    y = ur.lattice_points(N, R).astype(np.float64)
    return (np.linalg.norm(y, axis=1) - 0.5).astype(np.float32)


def test_dense_cubes_of_a_sphere_field_are_a_closed_surface():
    N, R = 17, 1.0
    verts, tris = ur.dense_cubes(_sphere_field(N, R), N, R, (0.0, 0.0, 0.0), 1.0)
    assert len(tris) > 200 and verts.dtype == np.float32 and tris.dtype == np.int32
    assert ur.closed_manifold(len(verts), tris) == 2  # V - E + F of a sphere
    # radius 1, centre 0, |y| < 1: contracted = world; the vertices lie on the sphere to within a cell
    assert np.abs(np.linalg.norm(verts.astype(np.float64), axis=1) - 0.5).max() < 2.0 / 16
    # normals face positive tsdf: outwards
    p = verts[tris].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", nrm, p.mean(1)) >= -1e-12).all()


def test_dense_cubes_uncontract_and_clamp():
    """A sphere of contracted radius 1.5 lies at world distance radius / (2 - 1.5) = 2 radius: with radius 20 the
    vertices would sit 40 from the centre and are clamped to the +-32 cube coordinate by coordinate."""
    N, R = 13, 1.9
    y = ur.lattice_points(N, R).astype(np.float64)
    field = (np.linalg.norm(y, axis=1) - 1.5).astype(np.float32)
    verts, tris = ur.dense_cubes(field, N, R, (1.0, 2.0, 3.0), 20.0, max_range=32.0)
    assert len(tris) > 100 and np.isfinite(verts).all()
    assert np.abs(verts).max() == 32.0 and (np.abs(verts) == 32.0).any(1).mean() > 0.3
    free, _ = ur.dense_cubes(field, N, R, (1.0, 2.0, 3.0), 20.0, max_range=1e6)
    d = np.linalg.norm(free.astype(np.float64) - np.array([1.0, 2.0, 3.0]), axis=1)
    assert 20.0 < d.min() and d.max() < 80.0 and abs(np.median(d) - 40.0) < 8.0


def test_field_without_a_crossing_gives_an_empty_mesh():
    verts, tris = ur.dense_cubes(np.ones(5 ** 3, np.float32), 5, 1.0, (0, 0, 0), 1.0)
    assert verts.shape == (0, 3) and tris.shape == (0, 3)
    verts, tris = ur.dense_cubes(np.full(8, -1.0, np.float32), 2, 1.0, (0, 0, 0), 1.0)
    assert verts.shape == (0, 3) and tris.shape == (0, 3)


def test_unbounded_argument_validation_is_host_side(hip_lib):
    """Every entry point refuses bad arguments before it touches the device: G4S_ERR_INVALID_ARGUMENT and a message."""
    lib = hip_lib
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    center = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    proj = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    sizes = (ctypes.c_int * 2)(64, 48)
    maps = (ctypes.c_void_p * 1)(256)
    no_map = (ctypes.c_void_p * 1)(0)
    totals = (ctypes.c_int * 2)(7, 7)
    big = 1 << 40

    def expect(rc, text):
        assert rc == INVALID, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    def grid(n=16, R=1.0, c=center, radius=1.0, voxel=0.1, nv=1, p=proj, s=sizes, d=maps, out=one, ws=one, wsb=big):
        return lib.g4s_utsdf_grid(n, R, c, radius, voxel, nv, p, s, d, out, ws, wsb, nul)
    expect(grid(n=1), "n^3 below 2^31")
    expect(grid(n=0), "n^3 below 2^31")
    expect(grid(n=-4), "n^3 below 2^31")
    expect(grid(n=1291), "n^3 below 2^31")  # 1291^3 >= 2^31 > 1290^3
    expect(grid(n=70000), "n^3 below 2^31")
    expect(grid(R=0.0), "half_extent must be positive")
    expect(grid(R=float("nan")), "half_extent must be positive")
    expect(grid(c=None), "NULL required pointer")
    expect(grid(radius=-1.0), "radius must be positive")
    expect(grid(voxel=0.0), "voxel_size must be positive")
    expect(grid(nv=-1), "n_views must not be negative")
    expect(grid(out=nul), "NULL required pointer")
    expect(grid(p=None), "NULL required pointer")
    expect(grid(d=None), "NULL required pointer")
    expect(grid(d=no_map), "NULL map pointer")
    expect(grid(s=(ctypes.c_int * 2)(0, 48)), "width, height must be positive")
    expect(grid(ws=nul), "workspace too small")
    expect(grid(wsb=8), "workspace too small")
    assert lib.g4s_utsdf_workspace(10) >= 10 * 88 and lib.g4s_utsdf_workspace(0) > 0

    def sample(n=5, pts=one, contracted=1, c=center, nv=1, d=maps, rgb=maps, t=one, col=one, wsb=big, voxel=0.1):
        return lib.g4s_utsdf_sample(n, pts, contracted, c, 1.0, voxel, nv, proj, sizes, d, rgb, t, col, one, wsb, nul)
    expect(sample(n=-1), "n_points must be in")
    expect(sample(pts=nul), "NULL required pointer")
    expect(sample(t=nul, col=nul), "NULL required pointer")      # null outputs with a non-zero size
    expect(sample(rgb=None), "NULL required pointer")             # colours without rgb maps
    expect(sample(rgb=no_map), "NULL map pointer")
    expect(sample(c=None), "NULL required pointer")               # contracted mode needs the frame
    expect(sample(nv=-2), "n_views must not be negative")
    expect(sample(voxel=-0.1), "voxel_size must be positive")
    expect(sample(wsb=0), "workspace too small")

    assert lib.g4s_dense_mc_workspace(1) == 0 and lib.g4s_dense_mc_workspace(1291) == 0
    assert lib.g4s_dense_mc_workspace(33) >= 33 ** 3 * 2
    expect(lib.g4s_dense_mc_count(1, one, totals, one, big, nul), "n^3 below 2^31")
    expect(lib.g4s_dense_mc_count(1291, one, totals, one, big, nul), "n^3 below 2^31")
    expect(lib.g4s_dense_mc_count(16, nul, totals, one, big, nul), "NULL required pointer")
    expect(lib.g4s_dense_mc_count(16, one, None, one, big, nul), "NULL required pointer")
    expect(lib.g4s_dense_mc_count(16, one, totals, one, 64, nul), "workspace too small")
    expect(lib.g4s_dense_mc_count(16, one, totals, nul, big, nul), "workspace too small")
    assert tuple(totals) == (7, 7)  # untouched

    def emit(n=16, f=one, R=1.0, c=center, radius=1.0, mr=32.0, v=one, t=one, nvert=5, ntri=5, wsb=big):
        return lib.g4s_dense_mc_emit(n, f, R, c, radius, mr, v, t, nvert, ntri, one, wsb, nul)
    expect(emit(n=1), "n^3 below 2^31")
    expect(emit(n=2000), "n^3 below 2^31")
    expect(emit(nvert=-1), "counts must not be negative")
    expect(emit(ntri=-1), "counts must not be negative")
    expect(emit(v=nul), "NULL required pointer")
    expect(emit(t=nul), "NULL required pointer")
    expect(emit(f=nul), "NULL required pointer")
    expect(emit(R=-1.0), "must be positive")
    expect(emit(mr=0.0), "must be positive")
    expect(emit(c=None), "NULL required pointer")
    expect(emit(radius=0.0), "radius must be positive")
    expect(emit(wsb=16), "workspace too small")
    assert emit(v=nul, t=nul, nvert=0, ntri=0) == 0 and lib.g4s_last_error() == b""  # an empty mesh: nothing to write
