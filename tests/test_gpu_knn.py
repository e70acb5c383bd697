"""distCUDA2 (g4splat_amd/csrc/knn.hip) at the edges of its tree -- 64 points per leaf, 64 children per node, three
levels, a search that starts from the own leaf and its two neighbours -- and on degenerate clouds, against the oracle's
brute force (pinned by tests/test_knn_cpu.py), exact equality everywhere."""
import ctypes

import numpy as np
import pytest

import knn_clouds

pytestmark = pytest.mark.gpu


def gpu_dist(pts):
    import torch
    from g4splat_amd.simple_knn._C import distCUDA2
    return distCUDA2(torch.as_tensor(pts, device="cuda")).cpu().numpy()


def cloud_with_duplicates(P, seed):
    """A normal cloud with a few exact duplicates (distance 0 takes part); returns (points, duplicated rows)."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(P, 3)).astype(np.float32)
    n = min(16, P // 4)
    rows = rng.choice(P, 2 * n, replace=False) if n else np.zeros((0,), np.int64)
    pts[rows[:n]] = pts[rows[n:]]
    return pts, rows


@pytest.mark.parametrize("P", [2, 63, 64, 65, 128, 129, 192, 193, 4095, 4096, 4097, 8193])
def test_leaf_and_node_boundaries(hip_lib, oracle_mod, P):
    """P on either side of a leaf (64) and of a level-1 node (4096 = 64 leaves), every row compared."""
    pts, _ = cloud_with_duplicates(P, seed=P)
    np.testing.assert_array_equal(gpu_dist(pts), oracle_mod.distCUDA2(pts))


@pytest.mark.parametrize("P", [262_143, 262_144, 262_145, 262_209])
def test_top_node_boundary(hip_lib, oracle_mod, P):
    """P on either side of a top node (262 144 = 64 x 64 leaves; 262 209 = one more leaf and one point).  About 4000 query
    rows: the 64 smallest and 64 largest coordinates of each axis (the ends of the curve), every planted duplicate, and
    random rows."""
    pts, dup = cloud_with_duplicates(P, seed=P)
    rng = np.random.default_rng(P + 1)
    ends = [np.argsort(pts[:, a], kind="stable")[s] for a in range(3) for s in (slice(0, 64), slice(-64, None))]
    q = np.unique(np.concatenate(ends + [dup, rng.choice(P, 3600, replace=False)])).astype(np.int32)
    assert 3600 <= q.size <= 4100
    got = gpu_dist(pts)
    np.testing.assert_array_equal(got[q], oracle_mod.distCUDA2_queries(pts, q))
    assert np.isfinite(got).all() and (got >= 0).all()


@pytest.mark.parametrize("name", knn_clouds.DEGENERATE)
def test_degenerate_clouds(hip_lib, oracle_mod, name):
    P = 8000 if name == "lattice" else 5000  # (the lattice: 20 x 20 x 20)
    pts = knn_clouds.degenerate_cloud(name, P, seed=11)
    assert pts.shape[0] == P
    want = oracle_mod.distCUDA2(pts)
    if name == "coincident":
        assert (want == 0).all()
    if name == "nonfinite":
        bad = knn_clouds.nonfinite_rows(P)
        assert np.isposinf(want[bad]).all() and np.isfinite(np.delete(want, bad)).all()
    np.testing.assert_array_equal(gpu_dist(pts), want)


@pytest.mark.parametrize("P", [1, 64, 65, 4097, 300_000])
def test_workspace_is_enough(hip_lib, oracle_mod, P):
    """g4s_knn_mean_dist writes nothing behind the g4s_knn_workspace(P) bytes it asks for."""
    import torch
    pts, _ = cloud_with_duplicates(P, seed=P + 5)
    nbytes = int(hip_lib.g4s_knn_workspace(P))
    tail = 4096
    ws = torch.full((nbytes + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    d_pts = torch.as_tensor(pts, device="cuda")
    out = torch.zeros((P,), dtype=torch.float32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = hip_lib.g4s_knn_mean_dist(P, ctypes.c_void_p(d_pts.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                   ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(nbytes), stream)
    assert rc == 0, hip_lib.g4s_last_error()
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xA5).all().item(), "bytes behind the advertised workspace were written"
    q = np.unique(np.concatenate([np.arange(min(P, 200)), np.random.default_rng(P).choice(P, min(P, 2000), replace=False)])).astype(np.int32)
    np.testing.assert_array_equal(out.cpu().numpy()[q], oracle_mod.distCUDA2_queries(pts, q))
