"""Pins the oracle's brute-force distCUDA2 (oracle/surfel_oracle.c: oracle_knn, oracle_knn_queries) -- what the GPU tests
of the k-NN search trust -- to a float32 numpy restatement of the definition, bit for bit, on the degenerate clouds of
tests/test_gpu_knn.py and on the clouds too small to have three neighbours."""
import numpy as np
import pytest

import knn_clouds
from support import same_bits


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_oracle_knn_fewer_than_three_neighbours(oracle_mod, P):
    pts = np.random.default_rng(P).normal(size=(P, 3)).astype(np.float32)
    want = knn_clouds.knn_mean3_numpy(pts)
    same_bits(oracle_mod.distCUDA2(pts), want)
    if P < 3:  # two or three FLT_MAX terms are left over: their sum overflows
        assert np.isposinf(want).all()
    elif P == 3:  # one FLT_MAX term: (d0 + d1) + FLT_MAX rounds to FLT_MAX
        assert (want == knn_clouds.FLT_MAX / np.float32(3.0)).all()
    else:
        assert np.isfinite(want).all()


@pytest.mark.parametrize("P", [64, 65, 1000])
def test_oracle_knn_normal_cloud(oracle_mod, P):
    pts = np.random.default_rng(P).normal(size=(P, 3)).astype(np.float32)
    pts[P // 2] = pts[3]  # a duplicate: distance 0 takes part
    same_bits(oracle_mod.distCUDA2(pts), knn_clouds.knn_mean3_numpy(pts))


@pytest.mark.parametrize("name", knn_clouds.DEGENERATE)
def test_oracle_knn_degenerate_clouds(oracle_mod, name):
    pts = knn_clouds.degenerate_cloud(name, 2000, seed=7)
    assert 1700 <= pts.shape[0] <= 2000
    want = knn_clouds.knn_mean3_numpy(pts)
    same_bits(oracle_mod.distCUDA2(pts), want)
    q = np.arange(0, pts.shape[0], 7, dtype=np.int32)
    same_bits(oracle_mod.distCUDA2_queries(pts, q), want[q])
    if name == "coincident":
        assert (want == 0).all()
    if name == "nonfinite":
        bad = knn_clouds.nonfinite_rows(pts.shape[0])
        assert np.isposinf(want[bad]).all()
        assert np.isfinite(np.delete(want, bad)).all()
    if name == "lattice":  # an inner point has six neighbours at distance 1
        assert want.min() == 1.0
