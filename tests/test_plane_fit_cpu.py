"""The host side of the global plane fit (g4splat_amd/plane_fit.py) and its numpy restatement (tests/plane_fit_ref.py) without a
GPU: the constrained solver against scipy's SLSQP and numpy's SVD, the replay of sklearn's RANSAC loop against sklearn, the
argument checks, the size queries, and the restatement against the reference's recorded results (tests/golden/plane_fit.npz,
written by tests/golden/make_golden_plane_fit.py)."""

import numpy as np
import pytest
import torch

import plane_fit_ref as R
from g4splat_amd import plane_fit as pf
from plane_fit_ref import within_yardstick
from support import PLANE_FIT_KEYS as KEYS, load_plane_fit_golden, plane_fit_scene


@pytest.fixture(scope="module")
def golden():
    return load_plane_fit_golden()


# ---- the solver ---------------------------------------------------------------------------------------------------------------
def moments(points):
    X = np.asarray(points, np.float64)
    cen = X.mean(axis=0)
    E = X - cen
    C = E.T @ E / len(X)
    return cen, np.array([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])


def slsqp_fit(points, prior, alpha):
    """The reference's way to the constrained fit: SLSQP over (a, b, c, d) from the prior, |n| = 1 as an equality."""
    from scipy.optimize import minimize
    X = np.asarray(points, np.float64)
    x0 = np.concatenate([prior, [-np.dot(prior, X.mean(axis=0))]])
    res = minimize(lambda q: R.objective(q, X, prior, alpha) if np.linalg.norm(q[:3]) >= 1e-8 else 1e10, x0, method="SLSQP",
                   constraints={"type": "eq", "fun": lambda q: q[0] * q[0] + q[1] * q[1] + q[2] * q[2] - 1.0})
    return res.x if res.success else x0


def solver_cases():
    """400 seeded cases: (points, prior); half are three points, half 500 points of a noisy plane; the prior is 0.01 .. 1 rad off."""
    rng = np.random.default_rng(400)
    cases = []
    for i in range(400):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        u = np.cross(n, rng.normal(size=3))
        u /= np.linalg.norm(u)
        w = np.cross(n, u)
        m = 3 if i < 200 else 500
        uv = rng.uniform(-1, 1, size=(m, 2))
        X = rng.normal(size=3) + uv[:, :1] * u + uv[:, 1:] * w + (0.0 if m == 3 else 0.01) * rng.normal(size=(m, 1)) * n
        angle = np.exp(rng.uniform(np.log(0.01), np.log(1.0)))
        prior = np.cos(angle) * n + np.sin(angle) * (np.cos(i) * u + np.sin(i) * w)
        cases.append((X.astype(np.float32).astype(np.float64), prior / np.linalg.norm(prior)))
    return cases


def test_solver_is_never_above_slsqp():
    pytest.importorskip("scipy")
    cases = solver_cases()
    mom = [moments(X) for X, _p in cases]
    coef = R.solve(np.stack([m[0] for m in mom]), np.stack([m[1] for m in mom]), np.stack([p for _X, p in cases]), 1.0)
    worst, gain = -np.inf, 0.0
    for (X, prior), c in zip(cases, coef):
        g_exact, g_slsqp = R.objective(c, X, prior, 1.0), R.objective(slsqp_fit(X, prior, 1.0), X, prior, 1.0)
        worst, gain = max(worst, g_exact - g_slsqp), max(gain, g_slsqp - g_exact)
        assert g_exact <= g_slsqp + 1e-12, (g_exact, g_slsqp)
    print(f"largest g_exact - g_slsqp {worst:.3e}; SLSQP above the optimum by up to {gain:.3e}")
    assert np.abs(np.linalg.norm(coef[:, :3], axis=1) - 1.0).max() < 1e-15 * 4


def test_solver_hard_case_collinear_and_duplicate_points():
    hard = R.hypotheses(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), [[0, 1, 2]], [1.0, 0.0, 0.0])[0]
    # the prior is perpendicular to the smallest eigenvector (0, 0, 1): A_xy y = p gives (18, 9) / 21, completed along +z
    assert np.allclose(hard[:3], [18 / 21, 9 / 21, 6 / 21], atol=1e-15) and hard[2] > 0
    X = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    for flip in (1.0, -1.0):  # both completions have the same objective, and nothing on the sphere is lower
        assert abs(R.objective([hard[0], hard[1], flip * hard[2], hard[3]], X, [1.0, 0.0, 0.0]) - 1.0 / 7.0) < 1e-15
    d = np.random.default_rng(0).normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    low = min(R.objective(np.concatenate([n, [-np.dot(n, X.mean(axis=0))]]), X, [1.0, 0.0, 0.0]) for n in d[:2000])
    assert low >= 1.0 / 7.0 - 1e-12
    prior = np.array([0.6, 0.8, 0.0])
    line = R.hypotheses(np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32), [[0, 1, 2]], prior)[0]
    L = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float64)
    assert np.isfinite(line).all() and abs(np.linalg.norm(line[:3]) - 1.0) < 4e-16
    low = min(R.objective(np.concatenate([n, [-np.dot(n, L.mean(axis=0))]]), L, prior) for n in d[:2000])
    assert R.objective(line, L, prior) <= low  # rank one: the normal trades the line against the prior
    same = R.hypotheses(np.array([[1, 2, 3]] * 3, np.float32), [[0, 1, 2], [0, 0, 0]], prior)
    assert np.allclose(same[:, :3], prior, atol=1e-15) and np.allclose(same[:, 3], -2.2)  # one point: the prior through it
    free = R.hypotheses(np.array([[1, 2, 3]] * 3, np.float32), [[0, 1, 2]])[0]
    assert np.isfinite(free).all() and abs(np.linalg.norm(free[:3]) - 1.0) < 1e-15
    outside = R.hypotheses(np.zeros((3, 3), np.float32), [[0, 1, 3], [-1, 1, 2]], prior)
    assert np.isnan(outside).all()


def test_solver_without_prior_is_the_svd_normal():
    rng = np.random.default_rng(5)
    for m in (3, 50):
        X = rng.normal(size=(40, m, 3)).astype(np.float32).astype(np.float64) * [1.0, 0.7, 0.1]
        mom = [moments(x) for x in X]
        coef = R.solve(np.stack([a for a, _b in mom]), np.stack([b for _a, b in mom]))
        for x, c in zip(X, coef):
            n = np.linalg.svd(x - x.mean(axis=0), full_matrices=False)[2][-1]
            assert abs(abs(np.dot(n, c[:3])) - 1.0) < 1e-12
            assert c[:3][np.argmax(np.abs(c[:3]))] > 0  # the stated sign
            assert abs(c[3] + np.dot(c[:3], x.mean(axis=0))) < 1e-15 * 8


# ---- the choice ---------------------------------------------------------------------------------------------------------------
RECORDED = []


def _estimator_class():
    from sklearn.base import BaseEstimator, RegressorMixin

    class PlaneEstimator(RegressorMixin, BaseEstimator):
        """ax + by + cz + d = 0 by the restated solver; records its three-row fits."""

        def __init__(self, alpha=1.0, prior=None):
            self.alpha, self.prior = alpha, prior

        def fit(self, X, y=None):
            cen, C = R.triple_moments(X[:1], X[1:2], X[2:3]) if len(X) == 3 else [m[None] for m in moments(X)]
            self.coef_ = R.solve(cen, C, None if self.prior is None else np.asarray(self.prior)[None], self.alpha)[0]
            if len(X) == 3:
                RECORDED.append(self.coef_)
            return self

        def predict(self, X):
            return R.distances(X, self.coef_)

    return PlaneEstimator


@pytest.mark.parametrize("outliers,noise", [(0.1, 0.002), (0.3, 0.002), (0.6, 0.002), (0.1, 0.006), (0.3, 0.006), (0.6, 0.006)])
def test_choose_trial_replays_sklearn(outliers, noise):
    pytest.importorskip("sklearn")
    from sklearn.linear_model import RANSACRegressor
    from sklearn.utils import check_random_state
    from sklearn.utils.random import sample_without_replacement
    rng = np.random.default_rng(int(1000 * outliers + 1e5 * noise))
    N, T = 2000, 1000
    n = np.array([0.3, -0.5, 0.81])
    n /= np.linalg.norm(n)
    X = rng.uniform(-1, 1, size=(N, 3))
    X -= ((X @ n) - 0.2)[:, None] * n
    X += noise * rng.normal(size=(N, 1)) * n
    bad = rng.random(N) < outliers
    X[bad] += rng.uniform(-0.5, 0.5, size=(int(bad.sum()), 1)) * n
    X = X.astype(np.float32)
    prior = pf.unit(n + [0.05, 0.02, -0.03])
    # the replay, from sklearn's sample stream alone
    stream = check_random_state(42)
    samples = np.stack([sample_without_replacement(N, 3, random_state=stream) for _ in range(T)])
    hyp = R.hypotheses(X, samples, prior, 1.0)
    counts = R.score(X, hyp, 0.01)
    best, trials = pf.choose_trial(counts, N)
    # sklearn
    del RECORDED[:]
    ransac = RANSACRegressor(estimator=_estimator_class()(1.0, prior), residual_threshold=0.01, min_samples=3, max_trials=T,
                             random_state=42)
    ransac.fit(X.astype(np.float64), np.zeros(N))
    print(f"outliers {outliers}, noise {noise}: {ransac.n_trials_} trials, best {best}, {int(counts[best])} inliers")
    assert trials == ransac.n_trials_
    assert len(RECORDED) >= trials and all(np.array_equal(RECORDED[t], hyp[t]) for t in range(trials))
    mask = np.abs(R.distances(X, hyp[best])) <= 0.01
    assert np.array_equal(mask, ransac.inlier_mask_) and int(mask.sum()) == int(counts[best])
    cen, C = moments(X[mask])
    assert np.array_equal(ransac.estimator_.coef_, R.solve(cen[None], C[None], prior[None], 1.0)[0])


def test_choose_trial_ties_stops_and_no_fit():
    assert pf.choose_trial([5, 7, 7, 3, 7, 2], 1000) == (4, 6)  # a tie goes to the later trial
    assert pf.choose_trial([0, 0, 0], 10) == (None, 3)            # no trial with an inlier: no fit
    assert pf.choose_trial([0, 1, 0], 10) == (1, 3)               # one inlier is enough
    assert pf.choose_trial([10, 0, 0], 10) == (0, 1)              # all points are inliers: sklearn stops at once
    counts = [900] + [0] * 999
    best, trials = pf.choose_trial(counts, 1000)
    assert best == 0 and trials == int(np.ceil(np.log(0.01) / np.log(1 - 0.9 ** 3)))
    assert pf.choose_trial([1] * 50, 10 ** 6) == (49, 50)


def test_draw_sample_triples_are_distinct_in_range_and_repeat():
    a = pf.draw_sample_triples([3, 4, 1000], 500).numpy()
    assert a.shape == (3, 500, 3) and a.dtype == np.int32
    for p, n in enumerate((3, 4, 1000)):
        s = a[p]
        assert s.min() >= 0 and s.max() < n
        assert (s[:, 0] != s[:, 1]).all() and (s[:, 0] != s[:, 2]).all() and (s[:, 1] != s[:, 2]).all()
    assert set(np.unique(a[1])) == {0, 1, 2, 3} and len({tuple(r) for r in a[0]}) == 6
    assert np.array_equal(a, pf.draw_sample_triples([3, 4, 1000], 500, torch.Generator().manual_seed(42)).numpy())
    assert not np.array_equal(a, pf.draw_sample_triples([3, 4, 1000], 500, torch.Generator().manual_seed(1)).numpy())
    with pytest.raises(ValueError, match="needs three"):
        pf.draw_sample_triples([2], 5)


def test_get_plane_params_picks_the_axis_of_the_reference():
    n, c = pf.get_plane_params([0.0, 0.6, 0.8, -1.6])
    assert np.allclose(n, [0, 0.6, 0.8]) and np.allclose(c, [0, 0, 2.0])
    n, c = pf.get_plane_params([0.6, 0.8, 1e-6, -1.6])
    assert np.allclose(c, [0, 2.0, 0])
    n, c = pf.get_plane_params([2.0, 0.0, 0.0, -3.0])
    assert np.allclose(n, [1, 0, 0]) and np.allclose(c, [1.5, 0, 0])


# ---- argument checks and size queries -------------------------------------------------------------------------------------------
def test_wrappers_refuse_before_any_library_call(monkeypatch):
    from g4splat_amd import _lib
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("the library was called"))
    cpu = torch.zeros((4, 5))
    with pytest.raises(ValueError, match="HIP device"):
        pf.fit_global_planes([None], [cpu], [torch.zeros((4, 5, 3))], [cpu.int()], [cpu.bool()], {0: [(0, 1)]})
    with pytest.raises(ValueError, match="HIP device"):
        pf.plane_hypotheses(torch.zeros((5, 3)), [0, 5], torch.zeros((1, 4, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="names view 3"):
        pf.pair_table({0: [(3, 1)]}, 2)
    with pytest.raises(ValueError, match="must be positive"):
        pf.pair_table({0: [(0, 0)]}, 2)
    assert pf.pair_table({7: [(0, 2), (1, 5)], 9: [], 4: [(1, 5)]}, 2) == ([7, 9, 4], [0, 2, 2, 3], [0, 1, 1], [2, 5, 5])
    for bad in (dict(min_samples=4), dict(max_trials=0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(alpha=0.0)):
        args = dict(threshold=0.01, min_samples=3, max_trials=10, alpha=1.0)
        args.update(bad)
        with pytest.raises(ValueError):
            pf._check_fit_args(**args)
    with pytest.raises(ValueError, match="non-zero"):
        pf._check_priors([[0.0, 0.0, 0.0]], 1)
    with pytest.raises(ValueError, match="at least three"):
        pf.fit_plane_ransac(np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="non-empty"):
        pf.normals_cluster_1d(torch.zeros((0, 3)))


def test_size_queries_and_refusals_are_host_code(hip_lib):
    import ctypes
    lib = hip_lib
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
    sizes = ints(64, 48, 5, 7)
    wide = ints(800, 600, 5, 7)
    small = lib.g4s_plane_fit_gather_workspace(2, wide, 1, ints(1))
    big = lib.g4s_plane_fit_gather_workspace(2, wide, 3, ints(0, 0, 1))
    assert 0 < small and big - small >= 2 * 2 * 4 * 1875 - 4 * 256  # two scan words per block of 256 pixels, less the alignment
    assert lib.g4s_plane_fit_gather_workspace(2, sizes, 1, ints(2)) == 0       # a view that is not there
    assert lib.g4s_plane_fit_gather_workspace(2, ints(64, 0, 5, 7), 1, ints(0)) == 0
    assert lib.g4s_plane_fit_gather_workspace(2, sizes, 65536, nul) == 0
    assert 0 < lib.g4s_plane_fit_members_workspace(0, 0, 0) < lib.g4s_plane_fit_members_workspace(100000, 10, 3)
    assert lib.g4s_plane_fit_members_workspace(-1, 0, 0) == 0 and lib.g4s_plane_fit_members_workspace(5, 65536, 1) == 0
    a = pf.fit_workspace_bytes([0, 10, 10, 5000])
    assert 0 < a < pf.fit_workspace_bytes([0, 10, 10, 5000 + 65 * pf.SUM_SPAN])
    assert pf.fit_workspace_bytes([1, 10]) == 0 and pf.fit_workspace_bytes([0, 10, 5]) == 0

    def expect(rc, text):
        assert rc == -1 and text.encode() in lib.g4s_last_error(), (rc, lib.g4s_last_error())

    ptrs = (ctypes.c_void_p * 2)(256, 256)
    expect(lib.g4s_plane_fit_gather_count(2, sizes, ptrs, ptrs, ptrs, ptrs, 1, ints(2), ints(1), ints(0), one, 1 << 20, nul), "pairs:")
    expect(lib.g4s_plane_fit_gather_count(2, sizes, ptrs, (ctypes.c_void_p * 2)(256, 0), ptrs, ptrs, 1, ints(0), ints(1), ints(0), one,
                                          1 << 20, nul), "normals[1]: NULL pointer")
    expect(lib.g4s_plane_fit_gather_count(2, sizes, ptrs, ptrs, ptrs, ptrs, 1, ints(0), ints(1), ints(0), one, 8, nul),
           "workspace too small")
    expect(lib.g4s_plane_fit_members_count(5, 1, ints(0, 4), one, ints(0), 1, ints(0, 1), ints(0, 0), one, 1 << 20, nul), "pair_offset")
    po = ints(0, 10)
    expect(lib.g4s_plane_fit_hypotheses(1, po, one, 0, one, nul, 1.0, one, one, 1 << 20, nul), "n_trials")
    expect(lib.g4s_plane_fit_hypotheses(1, ints(0, -1), one, 4, one, nul, 1.0, one, one, 1 << 20, nul), "plane_offset")
    expect(lib.g4s_plane_fit_hypotheses(1, po, one, 4, one, (ctypes.c_double * 3)(0, 0, 1), 0.0, one, one, 1 << 20, nul), "alpha")
    expect(lib.g4s_plane_fit_hypotheses(1, po, one, 4, nul, nul, 1.0, one, one, 1 << 20, nul), "NULL required pointer")
    expect(lib.g4s_plane_fit_score(1, po, one, 4, one, -0.5, one, one, 1 << 20, nul), "threshold")
    expect(lib.g4s_plane_fit_score(1, po, one, 4, one, 0.01, one, one, 8, nul), "workspace too small")
    expect(lib.g4s_plane_fit_refit(1, po, one, 4, one, ints(4), 0.01, nul, 1.0, one, one, one, one, 1 << 20, nul), "best[0]")
    assert lib.g4s_plane_fit_score(0, ints(0), nul, 4, nul, 0.01, nul, nul, 0, nul) == 0  # no plane: nothing to do


# ---- against the reference's recorded results -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated_scene(golden):
    """The restated fit loop over the golden scene, computed once: {key: fields of plane_fit_ref.fit_global_planes}."""
    return R.fit_global_planes(*plane_fit_scene(golden))


@pytest.mark.parametrize("key", KEYS)
def test_restated_fit_of_the_reference_points_lies_within_the_yardstick(golden, key):
    """The fit alone: the reference's own points and prior of its raster-order run."""
    pts, prior = golden[f"ref_points_{key}"], golden[f"ref_prior_{key}"]
    r = R.fit_points(pts, prior, pf.draw_sample_triples([len(pts)], 1000)[0].numpy())
    assert r["best"] is not None and r["trials"] < 1000  # most points are inliers: sklearn's rule stops early
    normal, centre = pf.get_plane_params(r["coef"])
    within_yardstick(golden, key, normal, centre)


def test_restated_loop_over_the_scene_lies_within_the_yardstick(golden, restated_scene):
    """The whole loop with the library's own seeds and samples: gather, k-means, members, prior, fit."""
    assert sorted(restated_scene) == list(KEYS)  # plane 13 has the 19-pixel pair alone: no entry
    for key in KEYS:
        r = restated_scene[key]
        assert len(r["pairs"]) == 4  # the 19-pixel pair of plane 12 is left out
        normal, centre = pf.get_plane_params(r["coef"])
        within_yardstick(golden, key, normal, centre)
        lo, hi = golden[f"ref_count_{key}"].min(), golden[f"ref_count_{key}"].max()
        assert 0.7 * lo <= len(r["points"]) <= 1.3 * hi  # the top clusters are of the reference's size
