"""Mesh evaluation on the MI355X (g4splat_amd.mesh_eval over csrc/tsdf/mesh_eval.hip) against the numpy restatement of the
header's semantics (tests/mesh_eval_ref.py), bit for bit unless stated: the search at its tree-size edges and on degenerate
clouds, the down-sample, the sampler, evaluate end to end and the command line."""
import functools

import numpy as np
import pytest
import torch

import mc_cases
import mesh_eval_ref as ref
import tsdf_ref
from g4splat_amd import mesh as mesh_mod
from g4splat_amd import mesh_eval as me
from g4splat_amd import ply_io
from support import DEV, devs, hosts, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32


def _search(cloud, query):
    """The library's (dist2, index) as numpy, through the public wrapper's workspace handling."""
    lib = me._lib.load()
    r, q = me._cloud(cloud, DEV), me._cloud(query, DEV)
    d2 = torch.empty(len(q), dtype=torch.float32, device=DEV)
    idx = torch.empty(len(q), dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.g4s_nn_workspace(len(r), len(q)), dtype=torch.uint8, device=DEV)
    me._lib.call("g4s_nn_search", len(r), me._lib.ptr(r), len(q), me._lib.ptr(q), me._lib.ptr(d2), me._lib.ptr(idx),
                 me._lib.ptr(ws), ws.numel(), me._lib.stream(DEV))
    return d2.cpu().numpy(), idx.cpu().numpy()


def _check_search(cloud, query):
    d2, idx = _search(cloud, query)
    want_d2, want_idx = ref.nn_search(cloud, query)
    assert np.array_equal(idx, want_idx), np.nonzero(idx != want_idx)[0][:8]
    same_bits(d2, want_d2)
    dist, index = me.nearest_neighbors(cloud, query)  # the public form: sqrt in float32
    same_bits(dist, np.sqrt(want_d2))
    assert np.array_equal(index.cpu().numpy(), want_idx)
    return d2, idx


@functools.lru_cache(maxsize=None)
def _cube(n, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(f32)


# ---- search ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_query", [1, 63, 65, 1000])
@pytest.mark.parametrize("n_ref", [1, 63, 64, 65, 4096, 4097, 262145])
def test_search_sizes(hip_lib, n_ref, n_query):
    """A partial leaf, exactly one leaf, two leaves, one and two mid nodes, two top nodes; the queries reach a little
    beyond the reference cube."""
    _check_search(_cube(n_ref, 100 + n_ref), _cube(n_query, 200 + n_query, -1.1, 1.1))


def test_search_coincident_references(hip_lib):
    cloud = np.tile(f32([[0.25, -0.5, 2.0]]), (3000, 1))
    _d2, idx = _check_search(cloud, _cube(300, 1, -3.0, 3.0))
    assert not idx.any()


def test_search_lattice_ties(hip_lib):
    """References on an integer lattice, shuffled; queries at cell centres: eight exact ties, the smallest index wins."""
    g = np.arange(12, dtype=f32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lattice = lattice[np.random.default_rng(2).permutation(len(lattice))]
    h = np.arange(11, dtype=f32) + f32(0.5)
    centres = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    d2, idx = _check_search(lattice, centres)
    assert (d2 == f32(0.75)).all() and len(np.unique(idx)) > 100


def test_search_every_query_among_the_references(hip_lib):
    cloud = _cube(5000, 3)
    query = cloud[np.random.default_rng(4).permutation(5000)[:700]]
    d2, _idx = _check_search(cloud, query)
    assert not d2.any()


def test_search_far_queries_and_two_clusters(hip_lib):
    rng = np.random.default_rng(5)
    cloud = np.concatenate([rng.normal(0, 0.01, (2500, 3)), rng.normal(0, 0.01, (2500, 3)) + [50.0, -20.0, 7.0]]).astype(f32)
    cloud = cloud[rng.permutation(len(cloud))]
    query = np.concatenate([rng.uniform(-1e4, 1e4, (300, 3)), rng.normal(0, 0.02, (200, 3)) + [50.0, -20.0, 7.0],
                            rng.uniform(-60, 60, (300, 3)), [[1e30, -1e30, 0.0], [3e38, 3e38, 3e38]]]).astype(f32)
    _check_search(cloud, query)


@pytest.mark.parametrize("free_axes", [2, 1, 0])
def test_search_zero_extent(hip_lib, free_axes):
    """References on a plane, on a line, at a point."""
    cloud = np.zeros((2000, 3), f32) + f32([0.5, -1.5, 2.5])
    cloud[:, :free_axes] = _cube(2000, 6)[:, :free_axes]
    _check_search(cloud, _cube(500, 7, -2.0, 3.0))


def test_search_non_finite_points(hip_lib):
    cloud = _cube(1000, 8).copy()
    cloud[17, 1] = np.nan
    cloud[500] = (np.inf, 0.0, 0.0)
    cloud[999, 2] = -np.inf
    query = _cube(300, 9, -1.2, 1.2).copy()
    query[5] = cloud[17]
    query[100, 0] = np.nan
    query[101, 2] = np.inf
    d2, idx = _check_search(cloud, query)
    assert not np.isin(idx, [17, 500, 999]).any()
    for k in (5, 100, 101):
        assert d2[k] == ref.FLT_MAX and idx[k] == -1
    assert (idx[np.setdiff1d(np.arange(300), [5, 100, 101])] >= 0).all()
    d2, idx = _check_search(np.full((70, 3), np.nan, f32), query)  # no finite reference at all
    assert (d2 == ref.FLT_MAX).all() and (idx == -1).all()


def test_search_swapped_and_repeated(hip_lib):
    a, b = _cube(4097, 10), _cube(1500, 11, -0.5, 1.5)
    first = _check_search(a, b)
    _check_search(b, a)
    again = _search(a, b)
    same_bits(first[:2], again[:2])


def test_search_refuses_an_empty_reference(hip_lib):
    with pytest.raises(ValueError, match="empty"):
        me.nearest_neighbors(np.zeros((0, 3), f32), _cube(5, 1))
    dist, idx = me.nearest_neighbors(_cube(5, 1), np.zeros((0, 3), f32))
    assert dist.shape == (0,) and idx.shape == (0,)


# ---- down-sample ----------------------------------------------------------------------------------------------------
def _check_down_sample(points, voxel):
    got = me.voxel_down_sample(points, voxel).cpu().numpy()
    same_bits(got, ref.voxel_down_sample(points, voxel))
    return got


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_down_sample_sizes(hip_lib, n):
    _check_down_sample(_cube(n, 20 + n), 0.1)


def test_down_sample_edge_clouds(hip_lib):
    assert len(_check_down_sample(ref.boundary_cloud(), 0.25)) == 9 ** 3
    assert len(_check_down_sample(ref.one_voxel_cloud(), 0.1)) == 1
    own = ref.own_voxel_cloud()
    assert len(_check_down_sample(own, 0.1)) == len(own)


def test_down_sample_key_width_limit(hip_lib):
    """n = 2 takes one index bit: 2e6^3 cells fit the other 63, 2.5e6^3 need 64, 3e6^3 overflow 64 bits, 1e33 a double."""
    assert len(_check_down_sample(f32([[0, 0, 0], [2e6, 2e6, 2e6]]), 1.0)) == 2
    for far in (2.5e6, 3e6, 1e30):
        with pytest.raises(ValueError, match="cell bits and index bits exceed 64"):
            me.voxel_down_sample(f32([[0, 0, 0], [far, far, far]]), 1.0 if far < 1e7 else 1e-3)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_down_sample_refuses_non_finite_points(hip_lib, bad):
    p = _cube(300, 30).copy()
    p[123, 1] = bad
    with pytest.raises(ValueError, match="points must be finite"):
        me.voxel_down_sample(p, 0.1)
    with pytest.raises(ValueError, match="voxel_size must be finite and positive"):
        me.voxel_down_sample(_cube(300, 30), 0.0)


# ---- sampler --------------------------------------------------------------------------------------------------------
def _check_sampler(mesh, u, cum=None):
    """cum = None: the device's own cumulative areas, downloaded for the restatement."""
    dm = mesh_mod.DeviceMesh(*devs(mesh))
    cum = me.cumulative_areas(dm) if cum is None else torch.as_tensor(cum, device=DEV)
    got = hosts(me.sample_surface(dm, len(u), u=torch.as_tensor(u, device=DEV), cum_area=cum))
    want = ref.sample_surface(u, cum.cpu().numpy(), mesh[2], mesh[0])
    for name, g, w in zip(("points", "normals", "face"), got, want):
        same_bits(g, w, name)
    return got


def test_sampler_edges(hip_lib):
    mesh = ref.sampler_mesh()
    _p, _n, face = _check_sampler(mesh, ref.sampler_edge_u(4000))
    assert face[0] == 1 and face[1] == 5 and not np.isin(face, [0, 2, 3, 6]).any()
    # a face that names a vertex outside the mesh: no area of its own accord, NaN point and zero normal if the caller gives it one
    bad = (mesh[0], mesh[1], np.concatenate([mesh[2][:5], [[3, 4, 99]]]).astype(np.int32))
    dm = mesh_mod.DeviceMesh(*(torch.as_tensor(a, device=DEV) for a in bad))
    assert me.cumulative_areas(dm).cpu().numpy().tolist() == [0.0, 0.5, 0.5, 0.5, 2.5, 2.5]
    points, normals, face = _check_sampler(bad, ref.sampler_edge_u(500), np.array([0.0, 0.5, 0.5, 0.5, 2.5, 3.5]))
    assert np.isnan(points[face == 5]).all() and not normals[face == 5].any() and (face == 5).any()


def test_sampler_on_a_noise_mesh_and_its_generator(hip_lib, noise_mesh):
    _check_sampler(noise_mesh, np.random.default_rng(40).random((5000, 3), dtype=f32))
    g = torch.Generator(device=DEV)
    g.manual_seed(41)
    a = me.sample_surface(mesh_mod.TriangleMesh(*noise_mesh), 1000, g)
    g.manual_seed(41)
    b = me.sample_surface(mesh_mod.TriangleMesh(*noise_mesh), 1000, g)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].device.type == "cuda"
    with pytest.raises(ValueError, match="no triangles"):
        me.sample_surface(mesh_mod.TriangleMesh(noise_mesh[0], noise_mesh[1], np.zeros((0, 3), np.int32)), 10)


# ---- evaluate -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise_mesh():
    """Marching cubes (numpy restatement) of 15^3 cubes of i.i.d. noise, voxel 0.1."""
    return tsdf_ref.extract_mesh(*mc_cases.noise())


N_SAMPLES = 3000


def _evaluate_both_ways(pred, trgt, device_meshes, threshold=0.05, down_sample=0.02):
    """(library's metrics, restatement's on the same samples and the device's own cumulative areas)."""
    wrap = (lambda m: mesh_mod.DeviceMesh(*devs(m))) if device_meshes \
        else (lambda m: mesh_mod.TriangleMesh(*m))
    g = torch.Generator(device=DEV)
    g.manual_seed(50)
    got = me.evaluate(wrap(pred), wrap(trgt), threshold, down_sample, N_SAMPLES, g)
    g.manual_seed(50)
    u_pred = torch.rand((N_SAMPLES, 3), dtype=torch.float32, device=DEV, generator=g).cpu().numpy()
    u_trgt = torch.rand((N_SAMPLES, 3), dtype=torch.float32, device=DEV, generator=g).cpu().numpy()
    cums = [me.cumulative_areas(me.as_device_mesh(mesh_mod.TriangleMesh(*m), DEV)[0]).cpu().numpy() for m in (pred, trgt)]
    want = ref.evaluate(pred, trgt, u_pred, u_trgt, threshold, down_sample, cums[0], cums[1])
    return got, want


def _assert_metrics_agree(got, want, n_terms):
    assert tuple(got) == ref.METRIC_KEYS
    for k in ("Prec", "Recal", "F-score"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ref.METRIC_KEYS:
        assert abs(got[k] - want[k]) <= n_terms * 2.0 ** -53 * abs(want[k]), (k, got[k], want[k])


@pytest.mark.parametrize("device_meshes", [False, True])
def test_evaluate_two_planes(hip_lib, device_meshes):
    pred, trgt = ref.plane_mesh(40, 1.0, 0.0), ref.plane_mesh(40, 1.0, 0.03)
    got, want = _evaluate_both_ways(pred, trgt, device_meshes)
    _assert_metrics_agree(got, want, max(N_SAMPLES, len(pred[0])))
    assert 2.9 <= got["Acc"] <= 3.1 and 2.9 <= got["Comp"] <= 3.1
    assert got["Normal-Acc"] > 99.9 and got["Normal-Comp"] > 99.9


@pytest.mark.parametrize("device_meshes", [False, True])
def test_evaluate_plane_against_noise(hip_lib, noise_mesh, device_meshes):
    plane = ref.plane_mesh(40, 1.0, 0.0)
    got, want = _evaluate_both_ways(noise_mesh, plane, device_meshes, threshold=0.1, down_sample=0.05)
    _assert_metrics_agree(got, want, max(N_SAMPLES, len(noise_mesh[0])))
    assert 0 < got["Prec"] < 100 and got["Recal"] > 0 and 20 < got["Normal-Consistency"] < 99


def test_evaluate_a_mesh_against_itself(hip_lib):
    """Acc = Comp = 0, F-score = 100; every sample's nearest sample has the same normal, up to the rounding of |n . n|."""
    v, c, t = ref.plane_mesh(40, 1.0, 0.0)
    rot = np.array([[0.8, 0.0, 0.6], [0.36, 0.8, -0.48], [-0.48, 0.6, 0.64]])
    mesh = mesh_mod.TriangleMesh((v.astype(np.float64) @ rot.T).astype(f32), c, t)
    got = me.evaluate(mesh, mesh, n_samples=N_SAMPLES)
    assert got["Acc"] == 0.0 and got["Comp"] == 0.0 and got["Chamfer-L1"] == 0.0
    assert got["Prec"] == got["Recal"] == got["F-score"] == 100.0
    # a normal's components carry about 4 eps each (three squares, two sums, a root, a division): |n . n'| = 1 +- 8 eps
    assert abs(got["Normal-Consistency"] - 100.0) <= 100.0 * 10 * 2.0 ** -24
    with pytest.raises(ValueError, match="no vertices"):
        me.evaluate(mesh, mesh_mod.TriangleMesh(v[:0], c[:0], t[:0]))


def test_command_line(hip_lib, tmp_path, capsys):
    a, b, out = tmp_path / "pred.ply", tmp_path / "gt.ply", tmp_path / "metrics.txt"
    ply_io.write_triangle_mesh(str(a), mesh_mod.TriangleMesh(*ref.plane_mesh(40, 1.0, 0.0)))
    ply_io.write_triangle_mesh(str(b), mesh_mod.TriangleMesh(*ref.plane_mesh(40, 1.0, 0.03)))
    out.write_text("earlier: line\n")
    me.main(["--input_mesh", str(a), "--gt_mesh", str(b), "--output_txt", str(out)])
    printed = capsys.readouterr().out.strip().splitlines()
    written = out.read_text().splitlines()
    assert written[0] == "earlier: line" and written[1:] == printed  # appended
    assert [line.split(": ")[0] for line in printed] == list(ref.METRIC_KEYS)
    values = {k: float(v) for k, v in (line.split(": ") for line in printed)}
    assert 2.9 <= values["Acc"] <= 3.1 and values["F-score"] == 100.0 and values["Normal-Consistency"] > 99.9
