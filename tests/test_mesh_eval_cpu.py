"""The numpy restatement of the mesh-evaluation semantics (tests/mesh_eval_ref.py) pinned without a GPU: its search and
its evaluate against scikit-learn's KDTree (the reference's own search), its down-sample and sampler on their edge cases,
and the host-side argument validation of the new entry points."""
import ctypes

import numpy as np
import pytest
from sklearn.neighbors import KDTree

import mesh_eval_ref as ref

f32, f64 = np.float32, np.float64
EPS = 2.0 ** -24


def _kd_nearest(cloud, query, k=1):
    d, i = KDTree(np.asarray(cloud, f64)).query(np.asarray(query, f64), k=k)
    return (d[:, 0], i[:, 0]) if k == 1 else (d, i)


def test_restated_search_against_kdtree():
    """Indices equal wherever the KDTree's two nearest distances differ; d^2 within a relative 6 * 2^-24 (three rounded
    subtractions, squared, and two rounded sums: at most 5 eps)."""
    rng = np.random.default_rng(0)
    cloud = rng.uniform(-1, 1, (2000, 3)).astype(f32)
    cloud[1500:1600] = cloud[100:200]  # duplicates: ties the condition leaves out
    query = np.concatenate([rng.uniform(-1.5, 1.5, (1400, 3)).astype(f32), cloud[100:200]])
    d2, idx = ref.nn_search(cloud, query)
    kd, ki = _kd_nearest(cloud, query, k=2)
    distinct = kd[:, 0] != kd[:, 1]
    assert distinct.sum() >= 1300 and (~distinct).sum() >= 100
    assert np.array_equal(idx[distinct], ki[distinct, 0])
    assert (idx[~distinct] == np.minimum(ki[~distinct, 0], ki[~distinct, 1])).all()  # the smallest index of the tie
    want = kd[:, 0] ** 2
    assert (np.abs(d2.astype(f64) - want) <= 6 * EPS * want).all()
    # the stated exceptions
    d2, idx = ref.nn_search(np.array([[np.nan, 0, 0], [np.inf, 0, 0], [1, 1, 1]], f32), np.array([[0, 0, 0], [np.nan, 0, 0]], f32))
    assert d2.tolist() == [3.0, ref.FLT_MAX] and idx.tolist() == [2, -1]


def _bumpy_plane(seed, z):
    v, c, t = ref.plane_mesh(12, 1.0, z)
    v = v.copy()
    v[:, 2] += np.random.default_rng(seed).uniform(-0.02, 0.02, len(v)).astype(f32)
    return v, c, t


def _formulas_over_kdtree(verts_pred, verts_trgt, pts_pred, nrm_pred, pts_trgt, nrm_trgt, threshold):
    """The reference's figures in float64 over KDTree, on clouds and samples that are given."""
    to_trgt, _ = _kd_nearest(verts_trgt, verts_pred)   # accuracy: predicted -> target
    to_pred, _ = _kd_nearest(verts_pred, verts_trgt)   # completeness: target -> predicted
    prec, recal = np.mean(to_trgt < threshold), np.mean(to_pred < threshold)
    _, at_trgt = _kd_nearest(pts_trgt, pts_pred)
    _, at_pred = _kd_nearest(pts_pred, pts_trgt)
    n_acc = np.mean(np.abs(np.sum(nrm_pred.astype(f64) * nrm_trgt[at_trgt].astype(f64), axis=1)))
    n_comp = np.mean(np.abs(np.sum(nrm_trgt.astype(f64) * nrm_pred[at_pred].astype(f64), axis=1)))
    fscore = 2 * prec * recal / (prec + recal)
    return {"Acc": to_trgt.mean() * 100, "Comp": to_pred.mean() * 100, "Chamfer-L1": (to_trgt.mean() + to_pred.mean()) / 2 * 100,
            "Prec": prec * 100, "Recal": recal * 100, "F-score": fscore * 100,
            "Normal-Acc": n_acc * 100, "Normal-Comp": n_comp * 100, "Normal-Consistency": (n_acc + n_comp) * 0.5 * 100}


def test_restated_evaluate_against_the_formulas_over_kdtree():
    """Same down-sampled clouds, same samples: the nine keys within a relative 1e-5 (the float32 rounding of the distances
    is 2^-24 per term), the count ratios equal."""
    pred, trgt = _bumpy_plane(1, 0.0), _bumpy_plane(2, 0.03)
    rng = np.random.default_rng(8)
    u_pred, u_trgt = rng.random((1500, 3), dtype=f32), rng.random((1500, 3), dtype=f32)
    threshold, voxel = 0.04, 0.05
    got = ref.evaluate(pred, trgt, u_pred, u_trgt, threshold, voxel)
    vp, vt = ref.voxel_down_sample(pred[0], voxel), ref.voxel_down_sample(trgt[0], voxel)
    pp, npd, _ = ref.sample_surface(u_pred, ref.cumulative_areas(pred[0], pred[2]), pred[2], pred[0])
    pt, ntg, _ = ref.sample_surface(u_trgt, ref.cumulative_areas(trgt[0], trgt[2]), trgt[2], trgt[0])
    want = _formulas_over_kdtree(vp, vt, pp, npd, pt, ntg, threshold)
    assert tuple(got) == ref.METRIC_KEYS == tuple(want)
    for k in ref.METRIC_KEYS:
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
    for k in ("Prec", "Recal", "F-score"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert 0 < got["Prec"] < 100 and 0 < got["Recal"] < 100 and 90 < got["Normal-Consistency"] < 100  # nothing degenerate


def _check_means(points, voxel, out):
    """Every output point is np.mean in float64, in index order, of the points of its voxel; voxels ascend in (cz, cy, cx)."""
    c = ref.voxel_cells(points, voxel)
    keys = [tuple(r) for r in c[:, ::-1]]
    uniq = sorted(set(keys))
    assert len(out) == len(uniq)
    keys = np.array(keys)
    for o, k in zip(out, uniq):
        members = np.nonzero((keys == k).all(axis=1))[0]
        assert np.array_equal(o, np.mean(points[members].astype(f64), axis=0).astype(f32)), k


def test_restated_down_sample_edges():
    p = ref.boundary_cloud()
    assert (p < 0).any()
    k = np.rint(p.astype(f64) / 0.125).astype(np.int64)  # p = k / 8, lo = -9 / 8: cell = floor((k + 9) / 2), exactly
    assert np.array_equal(ref.voxel_cells(p, 0.25), (k + 9) // 2)
    out = ref.voxel_down_sample(p, 0.25)
    assert out.shape == (9 ** 3, 3)
    _check_means(p, 0.25, out)
    one = ref.one_voxel_cloud()
    out = ref.voxel_down_sample(one, 0.1)
    assert out.shape == (1, 3)
    _check_means(one, 0.1, out)
    own = ref.own_voxel_cloud()
    out = ref.voxel_down_sample(own, 0.1)
    assert out.shape == own.shape
    c = ref.voxel_cells(own, 0.1)
    assert np.array_equal(out, own[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))])  # a mean of one point is the point
    _check_means(own, 0.1, out)


def test_sampler_restatement_edges():
    v, _c, t = ref.sampler_mesh()
    cum = ref.cumulative_areas(v, t)
    assert cum.tolist() == [0.0, 0.5, 0.5, 0.5, 2.5, 3.5, 3.5]
    u = ref.sampler_edge_u()
    points, normals, face = ref.sample_surface(u, cum, t, v)
    assert face[0] == 1        # u0 = 0: the first face of positive area, not the leading zero-area one
    assert face[1] == 5        # u0 = 1 - 2^-24: the last face of positive area, not the trailing zero-area one
    assert not np.isin(face, [0, 2, 3, 6]).any()
    for s in (2, 3, 4):        # a + b == 1 is not flipped: the point lies on the edge v1 v2
        a, b = u[s, 1], u[s, 2]
        v0, v1, v2 = v[t[face[s]]]
        assert np.array_equal(points[s], v0 + (a * (v1 - v0) + b * (v2 - v0)))
        assert np.allclose(points[s], b * v2.astype(f64) + a * v1.astype(f64), atol=1e-6)
    assert np.array_equal(normals[face == 1], np.broadcast_to(f32([0, 0, 1]), ((face == 1).sum(), 3)))
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)
    # a degenerate face drawn on purpose (the only face): zero normal
    p1, n1, f1 = ref.sample_surface(u[:4], np.array([0.0]), t[:1], v)
    assert f1.tolist() == [0] * 4 and not n1.any()


def test_sampler_face_counts_follow_the_areas():
    """200 000 seeded draws: every face's count within 5 sigma of the binomial of its area share; zero-area faces: none."""
    v, _c, t = ref.sampler_mesh()
    cum = ref.cumulative_areas(v, t)
    n = 200000
    u = np.random.default_rng(2024).random((n, 3), dtype=f32)
    _p, _n, face = ref.sample_surface(u, cum, t, v)
    counts = np.bincount(face, minlength=len(t))
    share = np.diff(np.concatenate([[0.0], cum])) / cum[-1]
    for f, (k, s) in enumerate(zip(counts, share)):
        assert abs(k - n * s) <= 5 * np.sqrt(n * s * (1 - s)), (f, k, n * s)
    assert counts[[0, 2, 3, 6]].tolist() == [0, 0, 0, 0]


def test_new_entry_points_validate_on_the_host(hip_lib):
    """Every mesh-evaluation entry point rejects bad arguments before it touches the device: -1 and a message, no launch."""
    lib = hip_lib
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    big = 1 << 30

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    assert lib.g4s_nn_workspace(1000, 1000) > 1000 * 16 * 2
    expect(lib.g4s_nn_search(0, one, 5, one, one, one, one, big, nul), "n_ref must be positive")
    expect(lib.g4s_nn_search(-3, one, 0, one, one, one, one, big, nul), "n_ref must be positive")
    expect(lib.g4s_nn_search(5, one, -1, one, one, one, one, big, nul), "must not be negative")
    for k in range(4):
        args = [one, one, one, one]
        args[k] = nul
        expect(lib.g4s_nn_search(5, args[0], 5, args[1], args[2], args[3], one, big, nul), "NULL required pointer")
    expect(lib.g4s_nn_search(5, one, 5, one, one, one, nul, big, nul), "workspace too small")
    expect(lib.g4s_nn_search(5, one, 5, one, one, one, one, 64, nul), "workspace too small")
    assert lib.g4s_nn_search(5, one, 0, nul, nul, nul, nul, 0, nul) == 0  # no query: nothing to do
    assert lib.g4s_last_error() == b""

    count = ctypes.c_int(7)
    assert lib.g4s_voxel_downsample_workspace(1000) > 1000 * 16
    expect(lib.g4s_voxel_downsample_count(-1, one, 0.1, ctypes.byref(count), one, big, nul), "must not be negative")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        expect(lib.g4s_voxel_downsample_count(5, one, bad, ctypes.byref(count), one, big, nul), "voxel_size must be finite and positive")
    expect(lib.g4s_voxel_downsample_count(5, nul, 0.1, ctypes.byref(count), one, big, nul), "NULL required pointer")
    expect(lib.g4s_voxel_downsample_count(5, one, 0.1, nul, one, big, nul), "NULL required pointer")
    expect(lib.g4s_voxel_downsample_count(5, one, 0.1, ctypes.byref(count), one, 64, nul), "workspace too small")
    assert lib.g4s_voxel_downsample_count(0, nul, 0.1, ctypes.byref(count), nul, 0, nul) == 0 and count.value == 0
    expect(lib.g4s_voxel_downsample_emit(5, one, 6, one, one, big, nul), "n_voxels must lie in 0..n")
    expect(lib.g4s_voxel_downsample_emit(5, one, -1, one, one, big, nul), "n_voxels must lie in 0..n")
    expect(lib.g4s_voxel_downsample_emit(5, nul, 2, one, one, big, nul), "NULL required pointer")
    expect(lib.g4s_voxel_downsample_emit(5, one, 2, nul, one, big, nul), "NULL required pointer")
    expect(lib.g4s_voxel_downsample_emit(5, one, 2, one, one, 64, nul), "workspace too small")
    assert lib.g4s_voxel_downsample_emit(5, one, 0, nul, nul, 0, nul) == 0

    expect(lib.g4s_mesh_sample_surface(-1, one, one, 4, one, 4, one, one, one, one, nul), "must not be negative")
    expect(lib.g4s_mesh_sample_surface(5, one, one, 0, one, 4, one, one, one, one, nul), "n_triangles must be positive")
    for k in range(7):
        args = [one] * 7
        args[k] = nul
        expect(lib.g4s_mesh_sample_surface(5, args[0], args[1], 4, args[2], 4, args[3], args[4], args[5], args[6], nul),
               "NULL required pointer")
    assert lib.g4s_mesh_sample_surface(0, nul, nul, 4, nul, 4, nul, nul, nul, nul, nul) == 0
