"""numpy restatement of include/g4s_render_maps.h, "Plane fit", operation for operation: the valid pixels of a pair, the
members, the constrained solver (cyclic Jacobi, the secular equation by bisection, the hard case), the hypotheses of sample
triples, the float64 inlier counts and the refit on fixed-order moments; and the whole fit loop over them with the host rules
of g4splat_amd/plane_fit.py (seeds, top cluster, prior, samples, choice).  The solver is vectorised over cases; a select
evaluates both sides, as the kernels do."""
import numpy as np

import plane_masks_ref as PM
import visibility_ref as VR

SWEEPS = 8       # G4S_PLANE_FIT_SWEEPS
BISECTIONS = 80  # G4S_PLANE_FIT_BISECTIONS
MIN_PIXELS = 20
f64 = np.float64


# ---- A. gather ----------------------------------------------------------------------------------------------------------------
def valid_pixels(depth, normals, mask, conf, plane_id):
    return (np.asarray(mask) == plane_id) & (np.asarray(conf) != 0) & np.isfinite(normals).all(axis=2) & np.isfinite(depth)


def gather_pairs(cams, depths, normals, masks, confs, pair_view, pair_id):
    """Per pair (points float32 [n,3], normals float32 [n,3]) in raster order, or None below MIN_PIXELS; and the counts."""
    out, counts = [], []
    for v, pid in zip(pair_view, pair_id):
        valid = valid_pixels(depths[v], normals[v], masks[v], confs[v], pid).reshape(-1)
        counts.append(int(valid.sum()))
        if counts[-1] < MIN_PIXELS:
            out.append(None)
            continue
        pts = VR.depths_to_points(depths[v], cams[v])
        out.append((pts[valid], np.asarray(normals[v], np.float32).reshape(-1, 3)[valid]))
    return out, counts


# ---- C. the solver ------------------------------------------------------------------------------------------------------------
def _key(i, j):
    return (i, j) if i <= j else (j, i)


def _rotate(a, V, p, q, r):
    app, aqq, apq = a[(p, p)], a[(q, q)], a[_key(p, q)]
    theta = (aqq - app) / (2.0 * apq)
    tf = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    ts = np.where(theta < 0.0, -tf, tf)
    t = np.where(apq != 0.0, ts, 0.0)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    a[(p, p)] = app - h
    a[(q, q)] = aqq + h
    a[_key(p, q)] = np.zeros_like(apq)
    rp, rq = a[_key(r, p)], a[_key(r, q)]
    a[_key(r, p)] = c * rp - s * rq
    a[_key(r, q)] = s * rp + c * rq
    for k in range(3):
        vp, vq = V[k][p], V[k][q]
        V[k][p] = c * vp - s * vq
        V[k][q] = s * vp + c * vq


def _order(l, V, i, j):
    swap = l[j] < l[i]
    l[i], l[j] = np.where(swap, l[j], l[i]), np.where(swap, l[i], l[j])
    for k in range(3):
        V[k][i], V[k][j] = np.where(swap, V[k][j], V[k][i]), np.where(swap, V[k][i], V[k][j])


def _sign(V, i):
    big = V[0][i]
    big = np.where(np.abs(V[1][i]) > np.abs(big), V[1][i], big)
    big = np.where(np.abs(V[2][i]) > np.abs(big), V[2][i], big)
    neg = big < 0.0
    for k in range(3):
        V[k][i] = np.where(neg, -V[k][i], V[k][i])


def _ratio(b, den):
    return np.where(b == 0.0, 0.0, b / den)


def solve(cen, C, prior=None, alpha=1.0):
    """cen [M,3], C [M,6] = (xx, xy, xz, yy, yz, zz), prior None or [M,3] (unit) -> (n, d) float64 [M,4]."""
    cen, C = np.asarray(cen, f64).reshape(-1, 3), np.asarray(C, f64).reshape(-1, 6)
    M = len(cen)
    alpha = f64(alpha)
    with np.errstate(all="ignore"):
        a = {(0, 0): C[:, 0].copy(), (0, 1): C[:, 1].copy(), (0, 2): C[:, 2].copy(), (1, 1): C[:, 3].copy(), (1, 2): C[:, 4].copy(),
             (2, 2): C[:, 5].copy()}
        if prior is not None:
            p = np.asarray(prior, f64).reshape(-1, 3)
            q = [alpha * p[:, i] for i in range(3)]
            for (i, j) in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
                a[(i, j)] = a[(i, j)] + q[i] * p[:, j]
        V = [[np.full(M, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
        for _ in range(SWEEPS):
            _rotate(a, V, 0, 1, 2)
            _rotate(a, V, 0, 2, 1)
            _rotate(a, V, 1, 2, 0)
        l = [a[(0, 0)], a[(1, 1)], a[(2, 2)]]
        _order(l, V, 0, 1)
        _order(l, V, 1, 2)
        _order(l, V, 0, 1)
        for i in range(3):
            _sign(V, i)
        y = [np.ones(M), np.zeros(M), np.zeros(M)]
        if prior is not None:
            b = [alpha * ((V[0][i] * p[:, 0] + V[1][i] * p[:, 1]) + V[2][i] * p[:, 2]) for i in range(3)]
            g1, g2 = l[1] - l[0], l[2] - l[0]
            h1, h2 = _ratio(b[1], g1), _ratio(b[2], g2)
            hh = h1 * h1 + h2 * h2
            lo, hi = np.zeros(M), np.full(M, alpha)
            for _ in range(BISECTIONS):
                mid = (lo + hi) * 0.5
                t0, t1, t2 = _ratio(b[0], mid), _ratio(b[1], g1 + mid), _ratio(b[2], g2 + mid)
                s = (t0 * t0 + t1 * t1) + t2 * t2
                up = s > 1.0
                lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
            hard = (b[0] == 0.0) & (hh < 1.0)
            y = [np.where(hard, np.sqrt(1.0 - hh), _ratio(b[0], hi)), np.where(hard, h1, _ratio(b[1], g1 + hi)),
                 np.where(hard, h2, _ratio(b[2], g2 + hi))]
        n = [(V[k][0] * y[0] + V[k][1] * y[1]) + V[k][2] * y[2] for k in range(3)]
        nn = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        n = [x / nn for x in n]
        d = -((n[0] * cen[:, 0] + n[1] * cen[:, 1]) + n[2] * cen[:, 2])
    return np.stack([n[0], n[1], n[2], d], axis=1)


def objective(coef, points, prior=None, alpha=1.0):
    """GeneralPlaneRegressor's objective of (a, b, c, d), normalised as it normalises."""
    coef, X = np.asarray(coef, f64), np.asarray(points, f64)
    norm = np.sqrt((coef[:3] ** 2).sum())
    n, d = coef[:3] / norm, coef[3] / norm
    loss = np.mean((X @ n + d) ** 2)
    if prior is not None:
        loss += alpha * (1.0 - abs(np.dot(np.asarray(prior, f64), n))) ** 2
    return loss


# ---- D. hypotheses ------------------------------------------------------------------------------------------------------------
def triple_moments(x0, x1, x2):
    """The centroid [M,3] and covariance [M,6] of three points each, float64 [M,3]."""
    cen = ((x0 + x1) + x2) / 3.0
    e = [x0 - cen, x1 - cen, x2 - cen]
    C = [((e[0][:, i] * e[0][:, j] + e[1][:, i] * e[1][:, j]) + e[2][:, i] * e[2][:, j]) / 3.0 for i in range(3) for j in range(i, 3)]
    return cen, np.stack(C, axis=1)


def hypotheses(points, samples, prior=None, alpha=1.0):
    """points float32 [n,3], samples [T,3] -> float64 [T,4]; four NaN for a triple with an index outside 0 .. n - 1."""
    X = np.asarray(points, np.float32).astype(f64)
    S = np.asarray(samples, np.int64).reshape(-1, 3)
    ok = ((S >= 0) & (S < len(X))).all(axis=1)
    Sc = np.where(ok[:, None], S, 0)
    cen, C = triple_moments(X[Sc[:, 0]], X[Sc[:, 1]], X[Sc[:, 2]])
    out = solve(cen, C, None if prior is None else np.broadcast_to(np.asarray(prior, f64), (len(S), 3)), alpha)
    out[~ok] = np.nan
    return out


# ---- E. scoring, F. refit -----------------------------------------------------------------------------------------------------
def distances(points, h):
    X = np.asarray(points, np.float32).astype(f64)
    with np.errstate(invalid="ignore"):
        return ((X[:, 0] * h[0] + X[:, 1] * h[1]) + X[:, 2] * h[2]) + h[3]


def score(points, hyp, threshold):
    """int32 [T]: per hypothesis the points with |distance| <= threshold."""
    X = np.asarray(points, np.float32).astype(f64)
    hyp = np.asarray(hyp, f64).reshape(-1, 4)
    out = np.zeros(len(hyp), np.int32)
    step = max(1, (1 << 22) // max(len(X), 1))
    with np.errstate(invalid="ignore"):
        for t in range(0, len(hyp), step):
            h = hyp[t:t + step]
            r = ((X[:, None, 0] * h[None, :, 0] + X[:, None, 1] * h[None, :, 1]) + X[:, None, 2] * h[None, :, 2]) + h[None, :, 3]
            out[t:t + step] = (np.abs(r) <= threshold).sum(axis=0)
    return out


def refit(points, h, threshold, prior=None, alpha=1.0):
    """(mask uint8 [n], moments float64 [10], coefficients float64 [4]); h None = no trial: nothing is an inlier."""
    X = np.asarray(points, np.float32).astype(f64)
    with np.errstate(invalid="ignore"):
        mask = np.zeros(len(X), bool) if h is None else np.abs(distances(points, h)) <= threshold
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    vals = np.stack([np.ones(len(X)), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=1)
    s = PM.fixed_sum(np.where(mask[:, None], vals, 0.0)) if len(X) else np.zeros(10)
    if not s[0] > 0.0:
        return mask.astype(np.uint8), s, np.full(4, np.nan)
    n = s[0]
    cen = np.array([s[1] / n, s[2] / n, s[3] / n])
    C = np.array([s[4] / n - cen[0] * cen[0], s[5] / n - cen[0] * cen[1], s[6] / n - cen[0] * cen[2], s[7] / n - cen[1] * cen[1],
                  s[8] / n - cen[1] * cen[2], s[9] / n - cen[2] * cen[2]])
    coef = solve(cen[None], C[None], None if prior is None else np.asarray(prior, f64)[None], alpha)[0]
    return mask.astype(np.uint8), s, coef


# ---- the whole loop -----------------------------------------------------------------------------------------------------------
def fit_points(points, prior, samples, threshold=0.01, alpha=1.0):
    """Steps 5-8 for one plane: dict(hyp, counts, best, trials, mask, moments, coef)."""
    from g4splat_amd import plane_fit as pf
    prior = None if prior is None else pf.unit(prior)  # the module normalises what it is given
    hyp = hypotheses(points, samples, prior, alpha)
    counts = score(points, hyp, threshold)
    best, trials = pf.choose_trial(counts, len(points))
    mask, moments, coef = refit(points, None if best is None else hyp[best], threshold, prior, alpha)
    return {"hyp": hyp, "counts": counts, "best": best, "trials": trials, "mask": mask, "moments": moments, "coef": coef}


def fit_global_planes(cams, depths, normals, masks, confs, gdict, threshold=0.01, max_trials=1000, alpha=1.0, generator=None):
    """{key: dict(points, prior, members per pair, and fit_points' fields)} for the planes that keep a pair: the host rules of
    g4splat_amd.plane_fit.fit_global_planes over this file's restatement of the kernels."""
    from g4splat_amd import plane_fit as pf
    from g4splat_amd import plane_masks as pm
    keys, plane_pair, pair_view, pair_id = pf.pair_table(gdict, len(depths))
    pairs, _counts = gather_pairs(cams, depths, normals, masks, confs, pair_view, pair_id)
    clustered = {}
    for e, pr in enumerate(pairs):  # seeds first for all pairs in order, as the module draws them
        if pr is None:
            continue
        rows = pr[1][::max(1, -(-len(pr[1]) // pm.SEED_SAMPLE))]
        seeds = pm.kmeanspp_seeds(rows, 8, generator)
        labels, centres, counts, _it = PM.kmeans_normals(pr[1].reshape(-1, 1, 3), seeds)
        top = pf.top_cluster(counts)
        clustered[e] = (pr[0][labels.reshape(-1) == top], pf.unit(centres[top]))
    planes = []
    for p, key in enumerate(keys):
        mine = [e for e in range(plane_pair[p], plane_pair[p + 1]) if e in clustered]
        if not mine:
            continue
        prior = np.stack([clustered[e][1] for e in mine]).mean(axis=0)
        planes.append((key, np.concatenate([clustered[e][0] for e in mine]), pf.unit(prior), mine))
    samples = pf.draw_sample_triples([len(pl[1]) for pl in planes], max_trials, generator).numpy() if planes else []
    out = {}
    for i, (key, pts, prior, mine) in enumerate(planes):
        out[key] = dict(fit_points(pts, prior, samples[i], threshold, alpha), points=pts, prior=prior, pairs=mine)
    return out


def within_yardstick(g, key, normal, centre, factor=2.0):
    """The plane lies within `factor` times the recorded yardstick of EVERY one of the reference's eight results: the angle
    between the normals, and the offset along the normal at the common point.  Returns the two largest figures."""
    angle_bar, offset_bar = factor * g[f"yardstick_{key}"]
    common = g[f"common_{key}"]
    normal, centre = np.asarray(normal, np.float64), np.asarray(centre, np.float64)
    worst_angle = worst_offset = 0.0
    for rn, rc in zip(g[f"ref_normal_{key}"], g[f"ref_centre_{key}"]):
        n = normal * (1.0 if np.dot(normal, rn) >= 0 else -1.0)
        worst_angle = max(worst_angle, float(np.arccos(min(1.0, np.dot(n, rn)))))
        worst_offset = max(worst_offset, abs(float(np.dot(n, common - centre)) - float(np.dot(rn, common - rc))))
    print(f"plane {key}: angle {worst_angle:.3e} (bar {angle_bar:.3e}), offset {worst_offset:.3e} (bar {offset_bar:.3e})")
    assert worst_angle <= angle_bar and worst_offset <= offset_bar, (key, worst_angle, angle_bar, worst_offset, offset_bar)
    return worst_angle, worst_offset
