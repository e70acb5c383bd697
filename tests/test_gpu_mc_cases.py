"""The marching-cubes kernels on the MI355X against the numpy restatements, on the adversarial cases of tests/mc_cases.py:
the sparse-block extraction (tsdf_mc_count_kernel / tsdf_mc_emit_kernel) against tsdf_ref.extract_mesh and the dense one
(dmc_count_kernel / dmc_emit_kernel) against unbounded_ref.dense_cubes.  tests/test_mc_cases_cpu.py shows what each case
contains: all 256 configurations, invalid cubes and unused crossings, every adjacency class of the 27-neighbourhood,
blocks at the ends of the key fields, non-zero counts on both sides of the scan's chunk boundary."""
import numpy as np
import pytest
import torch

import mc_cases
import tsdf_ref
import unbounded_ref as ur
from g4splat_amd import mesh as mesh_mod
from support import DEV, same_bits, words

pytestmark = pytest.mark.gpu

_REF = {}


def _sparse(name):
    """(case, reference mesh), computed once per module run and never modified."""
    if name not in _REF:
        case = mc_cases.SPARSE[name]()
        _REF[name] = (case, tsdf_ref.extract_mesh(*case))
    return _REF[name]


def _dense(name):
    if name not in _REF:
        field, N = mc_cases.DENSE[name]()
        _REF[name] = (field, N, ur.dense_cubes(field, N, mc_cases.DENSE_R, (0.0, 0.0, 0.0), 1.0))
    return _REF[name]


def _load(case, seed, grow=False):
    """A TSDFVolume holding the case: the table as given, the voxels scattered over the pool by a random permutation.
    The pool is about 1.5 times the table; its unused slots hold tsdf NaN, weight 1 and colour 1e9, so a wrong slot or a
    read beyond the table shows in the mesh.  grow = True starts from a pool of one block and enlarges it the way
    integrate() does (TSDFVolume._grow, doubling) until the table fits: the pool was smaller than the table, its size is
    whatever the doubling gives (exactly the table at 1024 blocks: no spare slot).  Allocating this exact block set by
    integrating depth views is not practical -- integration would also overwrite the voxel values the case is about."""
    keys, tsdf, weight, color, v = case
    n = len(keys)
    if grow:
        vol = mesh_mod.TSDFVolume(v, 4 * v, 10.0, DEV, initial_blocks=1)
        while vol.pool_blocks < n:
            vol._grow(vol.pool_blocks + 1)
        assert vol.grows >= 10
    else:
        vol = mesh_mod.TSDFVolume(v, 4 * v, 10.0, DEV, initial_blocks=n + n // 2 + 1)
    pool = vol.pool_blocks
    rng = np.random.default_rng(seed)
    slots = rng.permutation(pool)[:n].astype(np.int32)
    pt = np.full((pool, 512), np.nan, np.float32)
    pw = np.ones((pool, 512), np.float32)
    pc = np.full((pool, 512, 3), 1e9, np.float32)
    pt[slots], pw[slots], pc[slots] = tsdf, weight, color
    vol.keys = torch.as_tensor(np.ascontiguousarray(keys, np.int64), device=DEV)
    vol.slots = torch.as_tensor(slots, device=DEV)
    vol.num_blocks = n
    vol.tsdf = torch.as_tensor(pt.reshape(-1), device=DEV)
    vol.weight = torch.as_tensor(pw.reshape(-1), device=DEV)
    vol.color = torch.as_tensor(pc.reshape(-1), device=DEV)
    return vol


def _check_sparse(name, vol, far=False):
    _case, (rv, rc, rt) = _sparse(name)
    mesh = vol.extract_triangle_mesh()
    verts, cols, tris = mesh
    assert tris.dtype == np.int32 and verts.dtype == np.float32 and cols.dtype == np.float32
    assert verts.shape == rv.shape and cols.shape == rc.shape and tris.shape == rt.shape
    assert np.isfinite(verts).all() and np.isfinite(cols).all()
    assert np.array_equal(tris, rt)
    assert tris.min() >= 0 and tris.max() < len(verts)
    dv, dc = np.abs(verts - rv), np.abs(cols - rc)
    print(f"\n{name}: V={len(verts)} F={len(tris)} max|dv|={dv.max():.3g} max|dc|={dc.max():.3g} "
          f"unequal bits: verts {(words(verts) != words(rv)).sum()}, colours {(words(cols) != words(rc)).sum()}")
    if far:
        assert (dv <= 2 * np.spacing(np.abs(rv))).all(), (dv / np.spacing(np.abs(rv))).max()
    else:
        assert np.abs(rv).max() < 4.0 and dv.max() <= 1e-6
    assert dc.max() <= 1e-6
    again = vol.extract_triangle_mesh()
    same_bits(tuple(again), tuple(mesh), "second run")
    return mesh


@pytest.mark.parametrize("name", ["noise", "noise_holes", "gaps", "exact_zeros", "subnormals", "single", "single_holes",
                                  "holes_zero_block", "many_1023", "many_1024", "many_1025"])
def test_sparse_extraction_matches_the_restatement(hip_lib, name):
    """Triangles equal, vertices and colours within 1e-6 (|coordinate| < 4), nothing non-finite, every index below V, a
    second extraction byte-identical.  subnormals: a subnormal tsdf counts as its sign and divides exactly, as the
    header states.  holes_zero_block: the block stays in the table and contributes nothing."""
    case, _ref = _sparse(name)
    _check_sparse(name, _load(case, seed=len(name)))


def test_sparse_extraction_at_far_keys(hip_lib):
    """Blocks at both ends of the 21-bit key fields and at the farthest allocatable coordinate; a block whose +y (+z)
    neighbour's key would wrap onto another block's key must not take it as a neighbour.  Vertices to two ulp of the
    reference coordinate (the bar of the other cases scaled to the magnitude: slack for the division only)."""
    case, _ref = _sparse("far_keys")
    _check_sparse("far_keys", _load(case, seed=5), far=True)


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_many_blocks_in_a_pool_grown_from_one_block(hip_lib, n):
    case, _ref = _sparse(f"many_{n}")
    vol = _load(case, seed=n, grow=True)
    assert vol.pool_blocks == (1024 if n <= 1024 else 2048)
    _check_sparse(f"many_{n}", vol)


@pytest.mark.parametrize("name", list(mc_cases.DENSE))
def test_dense_cubes_match_the_restatement(hip_lib, name):
    """N^3 no multiple of the 256-point workgroup (27, 125, 4913, 35937) and one that is (4096); signed zeros and
    subnormals; scan_65: the dense path scans its per-workgroup counts with the chunked scan_u32 (scan.h), 65^3 points
    are 1073 workgroups and the noise puts non-zero counts on both sides of workgroup 1024.  Centre 0, radius 1 and
    R = 0.5 keep the un-contraction linear."""
    field, N, (rv, rt) = _dense(name)
    R = mc_cases.DENSE_R
    t = torch.as_tensor(field, device=DEV)
    verts, tris = mesh_mod.dense_marching_cubes(t, R, (0.0, 0.0, 0.0), 1.0)
    assert verts.dtype == np.float32 and tris.dtype == np.int32
    assert verts.shape == rv.shape and tris.shape == rt.shape and len(tris) > 0
    assert np.array_equal(tris, rt)
    assert tris.min() >= 0 and tris.max() < len(verts)
    dv = np.abs(verts - rv)
    print(f"\n{name}: V={len(verts)} F={len(tris)} max|dv|={dv.max():.3g} unequal bits: {(words(verts) != words(rv)).sum()}")
    assert np.isfinite(verts).all() and dv.max() <= 1e-6
    again = mesh_mod.dense_marching_cubes(t, R, (0.0, 0.0, 0.0), 1.0)
    dev = mesh_mod.dense_marching_cubes(t, R, (0.0, 0.0, 0.0), 1.0, to_host=False)
    assert dev[0].is_cuda and dev[1].is_cuda
    same_bits(tuple(again), (verts, tris), "second run")
    same_bits(tuple(dev), (verts, tris), "device result")
