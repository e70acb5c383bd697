"""The plane-fit kernels on the GPU (g4splat_amd/plane_fit.py over csrc/tsdf/plane_fit.hip) against the numpy restatement
tests/plane_fit_ref.py, bit for bit, at the sizes where a kernel takes another trip or another branch; every call is made twice
and must give the same bits.  The restatement itself is held against scipy, sklearn and the reference's recorded results in
tests/test_plane_fit_cpu.py."""
import numpy as np
import pytest
import torch

import plane_fit_ref as R
import plane_masks_ref as PM
from g4splat_amd import depth_cues, plane_fit as pf, plane_masks as pm, visibility
from g4splat_amd.synthetic import look_at_camera
from plane_fit_ref import within_yardstick
from plane_masks_ref import unit_normals
from support import DEV, PLANE_FIT_KEYS as KEYS, dev, host, load_plane_fit_golden, plane_fit_scene, same_bits, twice

pytestmark = pytest.mark.gpu

SPAN = pf.SCORE_SPAN


def plane_cloud(rng, n, normal=(0.2, -0.3, 0.93), offset=0.4, noise=0.004, outliers=0.2):
    normal = np.asarray(normal) / np.linalg.norm(normal)
    X = rng.uniform(-1, 1, size=(n, 3))
    X -= ((X @ normal) - offset)[:, None] * normal
    X += noise * rng.normal(size=(n, 1)) * normal
    far = rng.random(n) < outliers
    X[far] += rng.uniform(-0.3, 0.3, size=(int(far.sum()), 1)) * normal
    return X.astype(np.float32)


# ---- gather -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gather_case():
    rng = np.random.default_rng(3)
    shapes = [(5, 7), (37, 29), (64, 48), (130, 70)]  # (W, H); the last has more than two 4096-pixel spans
    cams = [look_at_camera((1.5 + 0.2 * v, 1.0, 0.8), (0.0, 0.1 * v, 0.0), (0.0, 0.0, 1.0), 0.9, W, H) for v, (W, H) in enumerate(shapes)]
    depths = [rng.uniform(1.0, 3.0, (H, W)).astype(np.float32) for W, H in shapes]
    normals = [unit_normals(rng, H, W) for W, H in shapes]
    masks = [np.zeros((H, W), np.int32) for W, H in shapes]
    confs = [np.ones((H, W), bool) for W, H in shapes]
    masks[0].reshape(-1)[3:22] = 1       # 19 valid pixels: left out
    masks[1].reshape(-1)[100:125] = 2
    confs[1].reshape(-1)[100:105] = False  # exactly 20 valid pixels: kept
    masks[2][10:30, 5:40] = 4
    masks[3][:, :] = 3
    masks[3][60:, 100:] = 9
    normals[3][2, 3, 1] = np.nan          # dropped pixels of pair (3, 3)
    normals[3][69, 50, 0] = np.inf
    depths[3][40, 40] = np.nan
    depths[3][41, 41] = np.inf
    confs[3][5:9, :] = False
    pairs = [(0, 1), (1, 2), (2, 77), (3, 3), (2, 4), (3, 3), (3, 9)]  # 77 is in no mask; (3, 3) is listed twice
    return cams, depths, normals, masks, confs, pairs


def test_gather_equals_the_restatement_and_depths_to_points(gather_case):
    cams, depths, normals, masks, confs, pairs = gather_case
    pv, pi = [p[0] for p in pairs], [p[1] for p in pairs]
    d_depths, d_normals = [dev(d) for d in depths], [dev(n) for n in normals]
    d_masks, d_confs = [dev(m) for m in masks], [dev(c) for c in confs]
    pts, nrm, offset, counts = twice(lambda: pf.gather_pairs(cams, d_depths, d_normals, d_masks, d_confs, pv, pi))
    want, want_counts = R.gather_pairs(cams, depths, normals, masks, confs, pv, pi)
    assert counts == want_counts and counts[0] == 19 and counts[1] == 20 and counts[2] == 0 and counts[3] == counts[5] > 2 * 4096
    assert want[0] is None and want[2] is None and want[1] is not None
    assert offset == list(np.cumsum([0] + [c if c >= 20 else 0 for c in counts]))
    for e, w in enumerate(want):
        if w is None:
            assert offset[e + 1] == offset[e]
            continue
        same_bits(pts[offset[e]:offset[e + 1]], w[0])
        same_bits(nrm[offset[e]:offset[e + 1]], w[1])
        v = pv[e]
        valid = torch.from_numpy(R.valid_pixels(depths[v], normals[v], masks[v], confs[v], pi[e]).reshape(-1)).to(DEV)
        assert torch.equal(pts[offset[e]:offset[e + 1]], visibility.depths_to_points(d_depths[v], cams[v])[valid])
    assert np.isfinite(host(pts)).all() and np.isfinite(host(nrm)).all()


# ---- k-means over pairs, seeds, normals_cluster_1d ------------------------------------------------------------------------------
def test_kmeans_over_pairs_of_span_edge_sizes_equals_the_restatement():
    rng = np.random.default_rng(8)
    sizes = [20, PM.SPAN - 1, PM.SPAN, PM.SPAN + 1]
    rows = [unit_normals(rng, 1, n, 4, 0.15)[0] for n in sizes]
    offset = [0] + list(np.cumsum(sizes))
    seeds = np.stack([r[:5] for r in rows])
    normals = dev(np.concatenate(rows))
    labels, centres, counts = twice(lambda: pf._cluster_pairs(DEV, normals, offset, [0, 1, 2, 3], 5, seeds, None))
    for e, r in enumerate(rows):
        want = PM.kmeans_normals(r.reshape(-1, 1, 3), seeds[e])
        assert (host(labels)[offset[e]:offset[e + 1]] == want[0].reshape(-1)).all(), e
        same_bits(centres[e], want[1])
        assert counts[e].tolist() == want[2].tolist()


def test_pair_seeds_equal_kmeanspp_seeds_of_the_whole_pair():
    rng = np.random.default_rng(9)
    sizes = [20, 4096, 3 * 4096 + 5]
    rows = [unit_normals(rng, 1, n)[0] for n in sizes]
    offset = [0] + list(np.cumsum(sizes))
    got = pf._pair_seeds(dev(np.concatenate(rows)), offset, [0, 1, 2], 8, torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(5)
    same_bits(got, np.stack([pm.kmeanspp_seeds(r, 8, g) for r in rows]))


def test_normals_cluster_1d_keeps_the_large_clusters_largest_first():
    rng = np.random.default_rng(10)
    rows = np.eye(3)[rng.integers(0, 3, 3000)] + 0.05 * rng.normal(size=(3000, 3))
    rows[:5] = [-1.0, -1.0, -1.0]  # a cluster of its own below 0.4 % of the rows
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    init = np.concatenate([rows[5:12], rows[:1]])
    masks, centres = twice(lambda: pf.normals_cluster_1d(dev(rows), n_clusters=8, init=init))
    labels, c, counts, _it = PM.kmeans_normals(rows.reshape(-1, 1, 3), init)
    assert counts[7] == 5
    order = [j for j in sorted(range(8), key=lambda j: (-counts[j], j)) if counts[j] >= 3000 * 0.004]
    assert len(masks) == len(order) and 7 not in order and len(order) >= 3
    for m, ctr, j in zip(masks, centres, order):
        assert (host(m) == (labels.reshape(-1) == j)).all()
        assert np.array_equal(ctr, c[j].astype(np.float64) / np.linalg.norm(c[j].astype(np.float64)))
    fewer, _c = pf.normals_cluster_1d(dev(rows), n_clusters=2, init=init)
    assert len(fewer) == 2 and torch.equal(fewer[0], masks[0]) and torch.equal(fewer[1], masks[1])


# ---- members ---------------------------------------------------------------------------------------------------------------------
def test_members_and_offsets_equal_the_restatement():
    rng = np.random.default_rng(11)
    sizes = [20, 1500, 25, 4097, 300]
    offset = [0] + list(np.cumsum(sizes))
    N = offset[-1]
    pts = rng.normal(size=(N, 3)).astype(np.float32)
    labels = rng.integers(0, 4, N).astype(np.int8)
    top = [0, 3, 2, 1, 5]  # the last pair has no member
    plane_pair = [0, 2, 2, 4, 5]  # the second plane has no pair
    got, plane_offset = twice(lambda: pf._members(DEV, dev(pts), offset, dev(labels), top, plane_pair))
    member = np.concatenate([labels[offset[e]:offset[e + 1]] == top[e] for e in range(5)])
    same_bits(got, pts[member])
    first = [int(member[:offset[plane_pair[p]]].sum()) for p in range(5)]
    assert plane_offset == first and plane_offset[1] == plane_offset[2] and plane_offset[3] == plane_offset[4]


# ---- hypotheses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [True, False], ids=["prior", "no_prior"])
def test_hypotheses_equal_the_restatement_bit_for_bit(with_prior):
    rng = np.random.default_rng(12)
    a = plane_cloud(rng, 500)
    b = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1], [2, 2, 2], [1, 2, 3], [1, 2, 3], [1, 2, 3], [0.5, 0.25, 0]], np.float32)
    T = 300
    samples = np.stack([pf.draw_sample_triples([500], T)[0].numpy(), rng.integers(0, 9, (T, 3)).astype(np.int32)])
    samples[1, :6] = [[0, 1, 2], [0, 3, 4], [5, 6, 7], [5, 5, 5], [0, 1, 8], [2, 1, 0]]  # hard, collinear, duplicates, on a line
    samples[1, 6:8] = [[0, 1, 9], [-1, 1, 2]]                                              # outside the plane's points
    priors = pf.unit(np.array([[0.1, -0.2, 1.0], [1.0, 0.0, 0.0]])) if with_prior else None
    pts = dev(np.concatenate([a, b]))
    hyp = twice(lambda: pf.plane_hypotheses(pts, [0, 500, 509], torch.from_numpy(samples), priors, 1.0))
    seen = None if priors is None else pf.unit(priors)  # the module normalises the priors it is given
    for p, x in enumerate((a, b)):
        same_bits(hyp[p], R.hypotheses(x, samples[p], None if seen is None else seen[p], 1.0))
    h = host(hyp)
    assert np.isnan(h[1, 6:8]).all() and np.isfinite(h[0]).all() and np.isfinite(h[1, :6]).all()
    if with_prior:
        assert np.allclose(h[1, 0, :3], [18 / 21, 9 / 21, 6 / 21], atol=1e-15)  # the hard case


# ---- scoring ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def score_clouds():
    rng = np.random.default_rng(13)
    return [plane_cloud(rng, n) for n in (3, SPAN - 1, SPAN, SPAN + 1, 65 * SPAN + 7)]


def check_scores(clouds, T, seed):
    n = [len(c) for c in clouds]
    offset = [0] + list(np.cumsum(n))
    pts = dev(np.concatenate(clouds))
    samples = pf.draw_sample_triples(n, T, torch.Generator().manual_seed(seed))
    priors = pf.unit(np.tile([[0.25, -0.3, 0.9]], (len(n), 1)))
    hyp = pf.plane_hypotheses(pts, offset, samples, priors, 1.0)
    counts = host(twice(lambda: pf.score_hypotheses(pts, offset, hyp, 0.01)))
    h = host(hyp)
    for p, c in enumerate(clouds):
        assert counts[p].tolist() == R.score(c, h[p], 0.01).tolist(), (p, T)
    return counts


@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257])
def test_scores_of_planes_of_very_different_sizes_in_one_launch(score_clouds, T):
    counts = check_scores(score_clouds, T, T)
    assert counts.shape == (5, T) and counts.max() > 3


def test_scores_of_a_thousand_trials(score_clouds):
    check_scores([score_clouds[0], score_clouds[3], score_clouds[4][:20000]], 1000, 7)


def test_a_point_exactly_at_the_threshold_is_an_inlier():
    pts = dev(np.array([[0.3, -0.2, 0.75], [0.1, 0.9, 0.75 + 2.0 ** -20], [0.0, 0.0, 0.25], [0.0, 0.0, 0.25 - 2.0 ** -22],
                        [np.nan, 0.0, 0.5]], np.float32))
    hyp = dev(np.array([[[0.0, 0.0, 1.0, -0.5]]], np.float64))
    assert host(pf.score_hypotheses(pts, [0, 5], hyp, 0.25)).tolist() == [[2]]
    mask, moments, _coef = pf.refit_planes(pts, [0, 5], hyp, [0], 0.25)
    assert host(mask).tolist() == [1, 0, 1, 0, 0] and host(moments)[0, 0] == 2.0


# ---- refit -----------------------------------------------------------------------------------------------------------------------
def test_refit_masks_moments_and_coefficients_equal_the_restatement():
    rng = np.random.default_rng(14)
    flat = rng.uniform(-1, 1, size=(700, 3)).astype(np.float32)
    flat[:, 2] = 0.5                               # every point is an inlier of its chosen trial
    three = plane_cloud(rng, 50, noise=0.0, outliers=0.0)
    three[3:] += np.float32(0.5)                   # exactly three inliers
    clouds = [flat, three, plane_cloud(rng, 65 * pf.SUM_SPAN + 7), plane_cloud(rng, pf.SUM_SPAN + 1), plane_cloud(rng, 40)]
    n = [len(c) for c in clouds]
    offset = [0] + list(np.cumsum(n))
    pts = dev(np.concatenate(clouds))
    samples = pf.draw_sample_triples(n, 8)
    samples[1, 0] = torch.tensor([0, 1, 2])
    priors = pf.unit(np.array([[0.0, 0.0, 1.0]] + [[0.2, -0.3, 0.93]] * 4))  # the planes' own normals
    for pr in (priors, None):
        hyp = pf.plane_hypotheses(pts, offset, samples, pr, 1.0)
        best = [3, 0, 5, 7, -1]  # the last plane has no trial
        mask, moments, coef = twice(lambda: pf.refit_planes(pts, offset, hyp, best, 0.01, pr, 1.0))
        h = host(hyp)
        for p, c in enumerate(clouds):
            want = R.refit(c, None if best[p] < 0 else h[p, best[p]], 0.01, None if pr is None else pf.unit(pr)[p], 1.0)
            same_bits(mask[offset[p]:offset[p + 1]], want[0])
            same_bits(moments[p], want[1])
            same_bits(coef[p], want[2])
        m = host(moments)
        assert m[0, 0] == 700 and m[1, 0] == 3 and m[4, 0] == 0 and np.isnan(host(coef)[4]).all() and np.isfinite(host(coef)[:4]).all()


def test_fit_plane_ransac_takes_arrays_tensors_and_samples():
    rng = np.random.default_rng(15)
    cloud = plane_cloud(rng, 3000)
    prior = [0.2, -0.3, 0.9]
    samples = pf.draw_sample_triples([3000], 1000)[0]
    want = R.fit_points(cloud, prior, samples.numpy())
    n_want, c_want = pf.get_plane_params(want["coef"])
    normal, centre, mask = twice(lambda: pf.fit_plane_ransac(cloud, prior_normal=prior))
    assert normal.dtype == np.float32 and mask.dtype == bool and isinstance(mask, np.ndarray)
    same_bits(normal, n_want.astype(np.float32))
    same_bits(centre, c_want.astype(np.float32))
    assert (mask == want["mask"].astype(bool)).all()
    n2, c2, m2 = pf.fit_plane_ransac(dev(cloud), prior_normal=prior, samples=samples)
    assert isinstance(m2, torch.Tensor) and m2.is_cuda and (host(m2) == mask).all() and (n2 == normal).all() and (c2 == centre).all()
    free = pf.fit_plane_ransac(cloud)
    assert abs(abs(float(np.dot(free[0], normal))) - 1.0) < 1e-3
    with pytest.raises(ValueError, match="no trial has an inlier"):
        pf.fit_plane_ransac(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32), samples=[[0, 1, 3]])


# ---- the golden scene end to end -----------------------------------------------------------------------------------------------
def test_golden_scene_end_to_end():
    g = load_plane_fit_golden()
    cams, depths, normals, masks, confs, gdict = plane_fit_scene(g)
    args = (cams, [dev(d) for d in depths], [dev(n) for n in normals], [dev(m) for m in masks], [dev(c) for c in confs], gdict)

    def run():
        planes, info = pf.fit_global_planes(*args)
        return [planes[k] for k in sorted(planes)], [[info[k][f] for f in ("points", "inliers", "best_trial", "trials")] for k in sorted(info)]
    twice(run)
    planes, info = pf.fit_global_planes(*args)
    assert sorted(planes) == list(KEYS) == sorted(info)  # plane 13 has the 19-pixel pair alone: no entry
    want = R.fit_global_planes(cams, depths, normals, masks, confs, gdict)
    for key in KEYS:
        normal, centre = planes[key]
        within_yardstick(g, key, normal, centre)
        assert (3, 99) not in info[key]["pairs"] and len(info[key]["pairs"]) == 4
        w = want[key]
        n_want, c_want = pf.get_plane_params(w["coef"])
        same_bits(normal, n_want.astype(np.float32))
        same_bits(centre, c_want.astype(np.float32))
        assert info[key]["points"] == len(w["points"]) and info[key]["inliers"] == int(w["mask"].sum())
        assert (info[key]["best_trial"], info[key]["trials"]) == (w["best"], w["trials"]) and info[key]["d"] == w["coef"][3]
        assert np.array_equal(info[key]["prior"], w["prior"])
    # the dict goes straight into the depth stage; all four views are input views, so nothing is refilled
    refined = depth_cues.refine_depths_with_planes(cams, args[1], args[3], args[4], args[1], gdict, planes, 4)
    again, planes2, _info = pf.refine_depth_with_planes(cams, args[1], args[2], args[3], args[4], args[1], gdict, 4)
    for v in range(4):
        assert torch.equal(refined[v], again[v])
        r, d = host(refined[v]), depths[v]
        listed = np.isin(masks[v], [p for pairs in gdict.values() for vv, p in pairs if vv == v])
        assert np.array_equal(r[~listed], d[~listed]) and np.isfinite(r).all()
        on_plane = listed & (masks[v] != 99)
        assert np.abs(r[on_plane] - d[on_plane]).max() < 0.2 and np.abs(r[on_plane] - d[on_plane]).mean() < 0.02
    assert all(np.array_equal(planes[k][0], planes2[k][0]) for k in KEYS)
