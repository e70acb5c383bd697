"""Global plane fit (include/g4s_render_maps.h, "Plane fit"; csrc/tsdf/plane_fit.hip).

Lines 547-603 of the reference's planes/refine_depth_with_planes.py, the link between the global-plane merge (planes.py) and
the plane depths (depth_cues.py): one plane per global id, fitted to the points of its (view, local plane) pairs.

  gather_pairs               the valid pixels of all pairs as world points and rendered normals, in one pass.
  normals_cluster_1d         the reference-named k-means over a list of normals (plane_masks.kmeans_normals underneath).
  draw_sample_triples,       the host side of RANSAC: which three points a trial fits, and sklearn's walk over the trials'
  choose_trial               inlier counts that picks the trial and stops early.
  fit_plane_ransac           the reference-named fit of one point set.
  fit_global_planes          the whole loop: {global id: (normal, centre)} for depth_cues.apply_global_planes.
  refine_depth_with_planes   the fit followed by depth_cues.refine_depths_with_planes: the reference's script without its
                             file I/O.

Everything per point runs in the library: gather, k-means, the members of the top clusters, the hypotheses of all trials of
all planes, their inlier counts and the refit, each in a number of launches that does not depend on the number of views, pairs
or planes; there is no torch path.  The host sees a few numbers per pair and per trial.  Two runs give the same bits.
INTEGRATION.md section S lists the differences from the reference.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, depth_cues
from . import plane_masks as pm
from ._device import (check_dtype, check_view_count, default_device, drop_leading_one, host_array, host_f32, launch, mask_bytes,
                      same_device, to_np, view_list)
from .visibility import ray_record

MIN_PIXELS = 20      # a pair with fewer valid pixels is skipped (the reference's `continue`)
SCORE_SPAN = 2048    # G4S_PLANE_FIT_SCORE_SPAN
SUM_SPAN = 4096      # G4S_PLANE_FIT_SUM_SPAN
MAX_PAIRS = 65535
_EPSILON = float(np.spacing(1))
c_d = ctypes.c_double
c_ll = ctypes.c_longlong


# ---- host side: argument checks (no device code: tests/test_plane_fit_cpu.py runs them) -------------------------------------
def _check_maps(maps, name, dev, dtypes, trailing=(), shapes=None, n=None):
    """The maps as contiguous tensors [H,W,*trailing] on one HIP device; ValueError for anything else."""
    maps = view_list(maps, name, "".join(",%d" % s for s in trailing))
    check_view_count(maps, name, n)
    out = []
    for v, t in enumerate(maps):
        label = f"{name}[{v}]"
        dev = same_device(t, dev, label)
        check_dtype(t, dtypes, label)
        if not trailing:
            t = drop_leading_one(t)
        if t.dim() != 2 + len(trailing) or tuple(t.shape[2:]) != tuple(trailing) or t.numel() == 0:
            raise ValueError(f"{label} must be a non-empty [H,W{''.join(',%d' % s for s in trailing)}] map (got {tuple(t.shape)})")
        if shapes is not None and tuple(t.shape[:2]) != shapes[v]:
            raise ValueError(f"{label} must have shape {shapes[v]} (got {tuple(t.shape[:2])})")
        out.append(t.detach().contiguous())
    return dev, out


def pair_table(global_3Dplane_ID_dict, n_views):
    """(keys, plane_pair [P+1], pair_view [E], pair_id [E]): the (view, id) pairs of all planes in dict order.  ValueError: a
    view outside 0 .. n_views - 1, an id that is not positive, more than 65535 pairs or planes."""
    keys, plane_pair, pair_view, pair_id = [], [0], [], []
    for key, pairs in global_3Dplane_ID_dict.items():
        for v, p in pairs:
            v, p = int(v), int(p)
            if not 0 <= v < n_views:
                raise ValueError(f"global_3Dplane_ID_dict names view {v} but there are {n_views} views")
            if p <= 0:
                raise ValueError(f"global_3Dplane_ID_dict: plane id {p} of view {v} must be positive")
            pair_view.append(v)
            pair_id.append(p)
        keys.append(key)
        plane_pair.append(len(pair_view))
    if len(pair_view) > MAX_PAIRS or len(keys) > MAX_PAIRS:
        raise ValueError(f"at most {MAX_PAIRS} planes and pairs (got {len(keys)} and {len(pair_view)})")
    return keys, plane_pair, pair_view, pair_id


def _check_fit_args(threshold, min_samples, max_trials, alpha):
    if int(min_samples) != 3:
        raise ValueError(f"min_samples must be 3: a trial fits three points (got {min_samples})")
    if not 1 <= int(max_trials) <= 1 << 20:
        raise ValueError(f"max_trials must be in 1 .. 2^20 (got {max_trials})")
    if not (0.0 <= float(threshold) < math.inf):
        raise ValueError(f"threshold must be finite and not negative (got {threshold})")
    if not (0.0 < float(alpha) < math.inf):
        raise ValueError(f"alpha must be positive and finite (got {alpha})")


def unit(p):
    """p [...,3] float64 over sqrt((x x + y y) + z z)."""
    p = np.asarray(p, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return p / np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])[..., None]


def _check_priors(priors, n_planes):
    """None, or float64 [P,3] of unit vectors (normalised here, as fit_plane_ransac does)."""
    if priors is None:
        return None
    p = unit(np.asarray(priors, np.float64).reshape(-1, 3))
    if len(p) != n_planes or not np.isfinite(p).all():
        raise ValueError(f"prior normals must be {n_planes} finite non-zero vectors")
    return p


def fit_workspace_bytes(plane_offset):
    """g4s_plane_fit_workspace for the offsets [P+1]: pure host code, 0 for offsets out of range."""
    po = [int(o) for o in plane_offset]
    return _lib.load().g4s_plane_fit_workspace(len(po) - 1, host_array(_lib.c_i, po))


# ---- 4. sample triples, 7. the choice (host) -------------------------------------------------------------------------------
def draw_sample_triples(n_points, max_trials, generator=None):
    """int32 [P,T,3] (CPU): per plane T triples of distinct indices below n_points[p], drawn from `generator` (a CPU
    torch.Generator; None: one seeded with 42).  Plane after plane, three draws of T numbers each: i below n, j below n - 1, k
    below n - 2, shifted past the earlier picks.  These are not sklearn's random_state=42 samples."""
    if generator is None:
        generator = torch.Generator().manual_seed(42)
    T = int(max_trials)
    if T < 1:
        raise ValueError(f"max_trials must be at least 1 (got {max_trials})")
    out = torch.empty((len(n_points), T, 3), dtype=torch.int32)
    for p, n in enumerate(n_points):
        n = int(n)
        if n < 3:
            raise ValueError(f"plane {p} has {n} points: a trial needs three")
        i = torch.randint(n, (T,), generator=generator)
        j = torch.randint(n - 1, (T,), generator=generator)
        k = torch.randint(n - 2, (T,), generator=generator)
        j = j + (j >= i)
        lo, hi = torch.minimum(i, j), torch.maximum(i, j)
        k = k + (k >= lo)
        k = k + (k >= hi)
        out[p] = torch.stack([i, j, k], dim=1).to(torch.int32)
    return out


def _dynamic_max_trials(n_inliers, n_samples, min_samples, probability):
    """sklearn.linear_model._ransac._dynamic_max_trials."""
    inlier_ratio = n_inliers / float(n_samples)
    nom = max(_EPSILON, 1 - probability)
    denom = max(_EPSILON, 1 - inlier_ratio ** min_samples)
    if nom == 1:
        return 0
    if denom == 1:
        return float("inf")
    return abs(float(np.ceil(np.log(nom) / np.log(denom))))


def choose_trial(counts, n_points, min_samples=3, stop_probability=0.99):
    """sklearn's RANSACRegressor loop over the inlier counts [T] of one plane's trials: (best trial or None, trials run).
    The best count starts at 1; a trial with at least the best count replaces the best (the score of a constant target is 0
    for every trial, so a tie goes to the later trial); after every replacement the number of trials is cut to
    ceil(log(1 - stop_probability) / log(1 - (best / n_points)^min_samples)) with sklearn's epsilon clamps."""
    counts = np.asarray(to_np(counts)).reshape(-1)
    max_trials = len(counts)
    best, best_count, t = None, 1, 0
    while t < max_trials:
        t += 1
        c = int(counts[t - 1])
        if c < best_count:
            continue
        best, best_count = t - 1, c
        max_trials = min(max_trials, _dynamic_max_trials(best_count, int(n_points), min_samples, stop_probability))
    return best, t


def get_plane_params(coef):
    """GeneralPlaneRegressor.get_plane_params: (normal, centre) float64 from (a, b, c, d); the centre is the plane's point on
    the z axis, or on the y or x axis where |c| (|b|) is at most 1e-5."""
    a, b, c, d = (float(x) for x in coef)
    norm = math.sqrt(a * a + b * b + c * c)
    normal = np.array([a, b, c]) / norm
    if abs(c) > 1e-5:
        centre = np.array([0.0, 0.0, -1.0 * d / c])
    elif abs(b) > 1e-5:
        centre = np.array([0.0, -1.0 * d / b, 0.0])
    else:
        centre = np.array([-1.0 * d / a, 0.0, 0.0])
    return normal, centre


# ---- 1. pair gather ------------------------------------------------------------------------------------------------------------
def _gather(dev, cameras, depths, normals, masks, confs, pair_view, pair_id):
    """(points [N,3], normals [N,3], pair_offset [E+1] with skipped pairs empty, counts [E]) over checked maps."""
    V, E = len(depths), len(pair_view)
    sizes = host_array(_lib.c_i, [s for t in depths for s in (t.shape[1], t.shape[0])])
    views, ids = host_array(_lib.c_i, pair_view), host_array(_lib.c_i, pair_id)
    counts = host_array(_lib.c_i, [0] * E)
    maps = (_lib.ptrs(depths), _lib.ptrs(normals), _lib.ptrs(masks), _lib.ptrs([mask_bytes(c) for c in confs]))
    ws = launch(dev, "g4s_plane_fit_gather_count", V, sizes, *maps, E, views, ids, counts,
                workspace=_lib.load().g4s_plane_fit_gather_workspace(V, sizes, E, views))
    n = [counts[e] for e in range(E)]
    rows, offset = [], [0]
    for c in n:
        rows.append(offset[-1] if c >= MIN_PIXELS else -1)
        offset.append(offset[-1] + (c if c >= MIN_PIXELS else 0))
    N = offset[-1]
    points = torch.empty((N, 3), dtype=torch.float32, device=dev)
    out_normals = torch.empty((N, 3), dtype=torch.float32, device=dev)
    if N:
        rays = np.concatenate([ray_record(c, d.shape[1], d.shape[0]) for c, d in zip(cameras, depths)])
        launch(dev, "g4s_plane_fit_gather_emit", V, sizes, host_f32(rays), *maps, E, views, ids, counts, host_array(c_ll, rows), N,
               _lib.ptr(points), _lib.ptr(out_normals), workspace=ws, sync=True)
    return points, out_normals, offset, n


def _gather_args(cameras, depths, rend_normals, plane_masks, conf_maps):
    cameras = list(cameras)
    V = len(cameras)
    dev, depths = _check_maps(depths, "depths", None, (torch.float32,), (), None, V)
    shapes = [tuple(d.shape) for d in depths]
    _d, normals = _check_maps(rend_normals, "rend_normals", dev, (torch.float32,), (3,), shapes, V)
    _d, masks = _check_maps(plane_masks, "plane_masks", dev, (torch.int32,), (), shapes, V)
    _d, confs = _check_maps(conf_maps, "conf_maps", dev, (torch.bool, torch.uint8), (), shapes, V)
    return dev, cameras, depths, normals, masks, confs


def gather_pairs(cameras, depths, rend_normals, plane_masks, conf_maps, pair_view, pair_id):
    """(points float32 [N,3], normals float32 [N,3], pair_offset [E+1], counts [E]): for every pair (pair_view[e], pair_id[e])
    the pixels with plane_mask == id, conf set and a finite normal and depth, in raster order, as world points
    (visibility.depths_to_points(depth, camera)[valid], bit for bit) and rendered normals; pair after pair.  A pair with fewer
    than 20 such pixels is left out: its range of pair_offset is empty; counts holds every pair's number."""
    dev, cameras, depths, normals, masks, confs = _gather_args(cameras, depths, rend_normals, plane_masks, conf_maps)
    _k, _pp, pair_view, pair_id = pair_table({0: list(zip(pair_view, pair_id))}, len(depths))
    if not depths or not pair_view:
        return torch.zeros((0, 3)), torch.zeros((0, 3)), [0] * (len(pair_view) + 1), [0] * len(pair_view)
    return _gather(dev, cameras, depths, normals, masks, confs, pair_view, pair_id)


# ---- 2. normal clusters ----------------------------------------------------------------------------------------------------------
def _pair_seeds(normals, offset, kept, k, generator):
    """kmeanspp_seeds of every kept pair, [len(kept),k,3]: at most 4096 rows per pair cross to the host, taken on the device at
    kmeanspp_seeds' own stride, in one copy."""
    parts = [normals[offset[e]:offset[e + 1]:max(1, -(-(offset[e + 1] - offset[e]) // pm.SEED_SAMPLE))] for e in kept]
    sizes = [len(p) for p in parts]
    rows = to_np(torch.cat(parts))
    seeds, at = [], 0
    for s in sizes:
        seeds.append(pm.kmeanspp_seeds(rows[at:at + s], k, generator))
        at += s
    return np.stack(seeds)


def _cluster_pairs(dev, normals, offset, kept, k, init, generator):
    """g4s_kmeans_normals over the kept pairs' normals as [n,1,3] views: (labels int8 [N], centres [E',k,3], counts [E',k]).
    Every row of `normals` belongs to a kept pair."""
    views = [normals[offset[e]:offset[e + 1]] for e in kept]
    seeds = _pair_seeds(normals, offset, kept, k, generator) if init is None else np.asarray(init, np.float32)
    if seeds.shape != (len(kept), seeds.shape[1], 3) or not 1 <= seeds.shape[1] <= pm.MAX_K or not np.isfinite(seeds).all():
        raise ValueError(f"init must be finite [{len(kept)},K,3] with K in 1 .. {pm.MAX_K} (got {seeds.shape})")
    K = seeds.shape[1]
    E = len(kept)
    labels = torch.empty(normals.shape[0], dtype=torch.int8, device=dev)
    centres = torch.empty((E, K, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((E, K), dtype=torch.int32, device=dev)
    n_iter = host_array(_lib.c_i, [0] * E)
    sizes = host_array(_lib.c_i, [s for v in views for s in (1, v.shape[0])])
    launch(dev, "g4s_kmeans_normals", E, sizes, _lib.ptrs(views), K, host_array(_lib.c_f, seeds.reshape(-1).tolist()), 300, 1e-4,
           _lib.ptrs([labels[offset[e]:offset[e + 1]] for e in kept]), _lib.ptr(centres), _lib.ptr(counts), n_iter,
           workspace=_lib.load().g4s_kmeans_normals_workspace(E, sizes), sync=True)
    return labels, to_np(centres), to_np(counts)


def top_cluster(counts):
    """The label with the most members; the smallest among equals."""
    return pm._top(counts, 1)[0]


def normals_cluster_1d(normals, n_init_clusters=8, n_clusters=6, min_size_ratio=0.004, init="k-means++", generator=None):
    """planes/refine_depth_with_planes.py normals_cluster_1d: (masks, centres) of the at most n_clusters largest k-means
    clusters of the normals [N,3] (a device tensor) that hold at least N * min_size_ratio of them, largest first (the
    smaller label among equal sizes): a list of bool [N] device tensors and their normalised centres, float64 [m,3].
    init: "k-means++" for plane_masks.kmeanspp_seeds(normals, n_init_clusters, generator), or [K,3] seeds."""
    if not isinstance(normals, torch.Tensor) or normals.dim() != 2 or normals.shape[1] != 3 or normals.shape[0] == 0:
        raise ValueError("normals must be a non-empty [N,3] tensor on a HIP device")
    labels, centres, counts, _n_iter = pm.kmeans_normals(normals.reshape(-1, 1, 3), init, k=n_init_clusters, generator=generator)
    counts, centres = to_np(counts), to_np(centres).astype(np.float64)
    bar = normals.shape[0] * min_size_ratio
    kept = [j for j in pm._top(counts, min(int(n_clusters), len(counts))) if counts[j] >= bar]
    flat = labels.reshape(-1)
    return [flat == j for j in kept], np.array([centres[j] / np.linalg.norm(centres[j]) for j in kept])


# ---- 3. members ------------------------------------------------------------------------------------------------------------------
def _members(dev, points, offset, labels, top, plane_pair):
    """(plane_points [N_total,3], plane_offset [P+1]): per plane the points of its pairs' top clusters, in row order.
    offset [E+1], top [E] and plane_pair [P+1] are over the same pairs."""
    N, E, P = points.shape[0], len(top), len(plane_pair) - 1
    offset, top, plane_pair = [int(o) for o in offset], [int(t) for t in top], [int(p) for p in plane_pair]
    plane_offset = host_array(_lib.c_i, [0] * (P + 1))
    ws = launch(dev, "g4s_plane_fit_members_count", N, E, host_array(_lib.c_i, offset), _lib.ptr(labels), host_array(_lib.c_i, top), P,
                host_array(_lib.c_i, plane_pair), plane_offset, workspace=_lib.load().g4s_plane_fit_members_workspace(N, E, P))
    plane_offset = [plane_offset[p] for p in range(P + 1)]
    out = torch.empty((plane_offset[-1], 3), dtype=torch.float32, device=dev)
    launch(dev, "g4s_plane_fit_members_emit", N, E, P, _lib.ptr(points), plane_offset[-1], _lib.ptr(out), workspace=ws, sync=True)
    return out, plane_offset


# ---- 5.-8. hypotheses, scoring, choice, refit ----------------------------------------------------------------------------------
def plane_hypotheses(points, plane_offset, samples, priors=None, alpha=1.0):
    """float64 [P,T,4] (device): (normal, d) of the constrained fit of every sample triple int32 [P,T,3] of the planes' points
    (rows plane_offset[p] .. plane_offset[p + 1] - 1 of the float32 [N,3] device tensor `points`)."""
    dev, points, po, samples, priors = _fit_inputs(points, plane_offset, samples, priors)
    _check_fit_args(0.0, 3, samples.shape[1], alpha)
    P, T = samples.shape[:2]
    hyp = torch.empty((P, T, 4), dtype=torch.float64, device=dev)
    if P:
        offs = host_array(_lib.c_i, po)
        launch(dev, "g4s_plane_fit_hypotheses", P, offs, _lib.ptr(points), T, _lib.ptr(samples),
               None if priors is None else host_array(c_d, priors.reshape(-1).tolist()), float(alpha), _lib.ptr(hyp),
               workspace=_lib.load().g4s_plane_fit_workspace(P, offs), sync=True)
    return hyp


def score_hypotheses(points, plane_offset, hypotheses, threshold=0.01):
    """int32 [P,T] (device): per hypothesis the plane's points within `threshold` of it, in float64."""
    dev, points, po, _s, _p = _fit_inputs(points, plane_offset, None, None)
    P, T = _check_hypotheses(hypotheses, dev, len(po) - 1)
    _check_fit_args(threshold, 3, T, 1.0)
    counts = torch.empty((P, T), dtype=torch.int32, device=dev)
    if P:
        offs = host_array(_lib.c_i, po)
        launch(dev, "g4s_plane_fit_score", P, offs, _lib.ptr(points), T, _lib.ptr(hypotheses), float(threshold), _lib.ptr(counts),
               workspace=_lib.load().g4s_plane_fit_workspace(P, offs), sync=True)
    return counts


def refit_planes(points, plane_offset, hypotheses, best, threshold=0.01, priors=None, alpha=1.0):
    """(inlier_mask uint8 [N], moments float64 [P,10], coefficients float64 [P,4]) on the device: the inliers of every plane's
    hypothesis best[p] (-1: none), the sums of 1, x, y, z, xx, xy, xz, yy, yz, zz over them in a fixed order, and the
    constrained fit on those moments."""
    dev, points, po, _s, priors = _fit_inputs(points, plane_offset, None, priors)
    P, T = _check_hypotheses(hypotheses, dev, len(po) - 1)
    _check_fit_args(threshold, 3, T, alpha)
    best = [int(b) for b in best]
    if len(best) != P or any(not -1 <= b < T for b in best):
        raise ValueError(f"best must hold {P} trials in -1 .. {T - 1}")
    mask = torch.empty(po[-1], dtype=torch.uint8, device=dev)
    moments = torch.empty((P, 10), dtype=torch.float64, device=dev)
    coef = torch.empty((P, 4), dtype=torch.float64, device=dev)
    if P:
        offs = host_array(_lib.c_i, po)
        launch(dev, "g4s_plane_fit_refit", P, offs, _lib.ptr(points), T, _lib.ptr(hypotheses), host_array(_lib.c_i, best),
               float(threshold), None if priors is None else host_array(c_d, priors.reshape(-1).tolist()), float(alpha),
               _lib.ptr(mask), _lib.ptr(moments), _lib.ptr(coef), workspace=_lib.load().g4s_plane_fit_workspace(P, offs), sync=True)
    return mask, moments, coef


def _fit_inputs(points, plane_offset, samples, priors):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a [N,3] tensor on a HIP device")
    check_dtype(points, (torch.float32,), "points")
    dev = same_device(points, None, "points")
    po = [int(o) for o in plane_offset]
    if not po or po[0] != 0 or po[-1] != points.shape[0] or any(b < a for a, b in zip(po, po[1:])) or len(po) - 1 > MAX_PAIRS:
        raise ValueError(f"plane_offset must ascend from 0 to {points.shape[0]} over at most {MAX_PAIRS} planes")
    P = len(po) - 1
    if samples is not None:
        if not isinstance(samples, torch.Tensor) or samples.dim() != 3 or samples.shape[0] != P or samples.shape[2] != 3:
            raise ValueError(f"samples must be an int32 [{P},T,3] tensor (got {tuple(getattr(samples, 'shape', ()))})")
        check_dtype(samples, (torch.int32,), "samples")
        samples = samples.to(dev).contiguous()
    return dev, points.detach().contiguous(), po, samples, _check_priors(priors, P)


def _check_hypotheses(hypotheses, dev, P):
    if not isinstance(hypotheses, torch.Tensor) or hypotheses.dim() != 3 or hypotheses.shape[0] != P or hypotheses.shape[2] != 4:
        raise ValueError(f"hypotheses must be a float64 [{P},T,4] tensor")
    check_dtype(hypotheses, (torch.float64,), "hypotheses")
    same_device(hypotheses, dev, "hypotheses")
    if not hypotheses.is_contiguous():
        raise ValueError("hypotheses must be contiguous")
    return P, hypotheses.shape[1]


def _fit(points, plane_offset, priors, threshold, min_samples, max_trials, alpha, generator, samples):
    """Steps 4-8 for planes with at least three points each: a dict of per-plane results."""
    _check_fit_args(threshold, min_samples, max_trials, alpha)
    n = [b - a for a, b in zip(plane_offset, plane_offset[1:])]
    if samples is None:
        samples = draw_sample_triples(n, max_trials, generator)
    hyp = plane_hypotheses(points, plane_offset, samples, priors, alpha)
    counts = to_np(score_hypotheses(points, plane_offset, hyp, threshold))  # the one read-back of the trials
    picks = [choose_trial(counts[p], n[p], min_samples) for p in range(len(n))]
    best = [-1 if b is None else b for b, _t in picks]
    mask, moments, coef = refit_planes(points, plane_offset, hyp, best, threshold, priors, alpha)
    return {"best": best, "trials": [t for _b, t in picks], "counts": counts, "mask": mask, "moments": to_np(moments),
            "coef": to_np(coef), "hypotheses": hyp, "samples": samples}


# ---- 9. public interface ---------------------------------------------------------------------------------------------------------
def fit_plane_ransac(pnts, threshold=0.01, min_samples=3, max_trials=1000, alpha=1.0, prior_normal=None, generator=None,
                     samples=None):
    """planes/refine_depth_with_planes.py fit_plane_ransac: (normal float32 [3], centre float32 [3], inlier_mask bool [N]) of
    the RANSAC fit of ax + by + cz + d = 0 to pnts [N,3] (a device tensor, or an array that is copied to the current
    device), with the constrained estimator when prior_normal is given.  samples: int32 [T,3] triples of the caller's
    instead of draw_sample_triples([N], max_trials, generator).  The mask is a device tensor for a tensor, else an array.
    ValueError if no trial has an inlier (sklearn's)."""
    as_tensor = isinstance(pnts, torch.Tensor)
    N = int(np.prod(pnts.shape)) // 3
    if N < 3:
        raise ValueError(f"fit_plane_ransac needs at least three points (got {N})")
    _check_fit_args(threshold, min_samples, max_trials, alpha)
    if as_tensor and pnts.is_cuda:
        points = pnts.detach().float()
    else:
        points = torch.from_numpy(np.ascontiguousarray(to_np(pnts), np.float32)).to(default_device())
    points = points.reshape(-1, 3).contiguous()
    if samples is not None:
        samples = torch.as_tensor(to_np(samples)).to(torch.int32).reshape(1, -1, 3)
        if samples.numel() == 0 or int(samples.min()) < 0 or int(samples.max()) >= N:
            raise ValueError(f"samples must index the {N} points")
        max_trials = samples.shape[1]
    r = _fit(points, [0, N], None if prior_normal is None else [to_np(prior_normal)], threshold, min_samples, max_trials, alpha,
             generator, samples)
    if r["best"][0] < 0:
        raise ValueError("RANSAC could not find a valid consensus set: no trial has an inlier")
    normal, centre = get_plane_params(r["coef"][0])
    mask = r["mask"].bool()
    return normal.astype(np.float32), centre.astype(np.float32), mask if as_tensor else to_np(mask)


def fit_global_planes(cameras, depths, rend_normals, plane_masks, conf_maps, global_3Dplane_ID_dict, threshold=0.01,
                      max_trials=1000, alpha=1.0, generator=None, return_points=False):
    """The fit loop of planes/refine_depth_with_planes.py for all global planes at once: (planes, info).
    planes = {global id: (normal float32 [3], centre float32 [3])} as depth_cues.apply_global_planes takes it; a plane none of
    whose pairs has 20 valid pixels, or that no trial fits, has no entry.  info = {global id: dict(points, inliers,
    best_trial, trials, prior, d, centroid, pairs)}; d is the offset of the unit normal and centroid the inliers' mean, both
    float64 (the axis point `centre` can lie far away for a steep plane).  generator: a CPU torch.Generator that first seeds
    the k-means (None: plane_masks.kmeanspp_seeds' own default) and then draws the samples (None: seeded with 42).
    return_points adds info[id]["plane_points"] and ["inlier_mask"] (device tensors)."""
    dev, cameras, depths, normals, masks, confs = _gather_args(cameras, depths, rend_normals, plane_masks, conf_maps)
    keys, plane_pair, pair_view, pair_id = pair_table(global_3Dplane_ID_dict, len(depths))
    _check_fit_args(threshold, 3, max_trials, alpha)
    if not depths or not pair_view:
        return {}, {}
    pts, nrm, offset, _n = _gather(dev, cameras, depths, normals, masks, confs, pair_view, pair_id)
    kept = [e for e in range(len(pair_view)) if offset[e + 1] > offset[e]]
    if not kept:
        return {}, {}
    labels, centres, counts = _cluster_pairs(dev, nrm, offset, kept, 8, None, generator)
    top = [top_cluster(counts[i]) for i in range(len(kept))]
    pair_prior = [unit(centres[i][top[i]]) for i in range(len(kept))]
    # the planes that keep a pair, and their runs of kept pairs
    fitted, kept_pair, priors = [], [0], []
    at = 0
    for p in range(len(keys)):
        mine = [i for i in range(at, len(kept)) if kept[i] < plane_pair[p + 1]]
        at += len(mine)
        if not mine:
            continue
        prior = np.stack([pair_prior[i] for i in mine]).mean(axis=0)
        fitted.append(p)
        kept_pair.append(at)
        priors.append(unit(prior))
    kept_offset = [offset[e] for e in kept] + [offset[-1]]
    plane_points, plane_offset = _members(dev, pts, kept_offset, labels, top, kept_pair)
    # the largest of eight clusters of 20 or more rows has at least three: every plane can be sampled
    r = _fit(plane_points, plane_offset, priors, threshold, 3, max_trials, alpha, generator, None)
    planes, info = {}, {}
    for i, p in enumerate(fitted):
        if r["best"][i] < 0:
            continue
        normal, centre = get_plane_params(r["coef"][i])
        m = r["moments"][i]
        planes[keys[p]] = (normal.astype(np.float32), centre.astype(np.float32))
        info[keys[p]] = {"points": int(plane_offset[i + 1] - plane_offset[i]), "inliers": int(m[0]), "best_trial": r["best"][i],
                         "trials": r["trials"][i], "prior": priors[i], "d": float(r["coef"][i][3]), "centroid": m[1:4] / m[0],
                         "pairs": [(pair_view[e], pair_id[e]) for e in kept if plane_pair[p] <= e < plane_pair[p + 1]]}
        if return_points:
            info[keys[p]]["plane_points"] = plane_points[plane_offset[i]:plane_offset[i + 1]]
            info[keys[p]]["inlier_mask"] = r["mask"][plane_offset[i]:plane_offset[i + 1]].bool()
    return planes, info


def refine_depth_with_planes(cameras, depths, rend_normals, plane_masks, conf_maps, mono_depths, global_3Dplane_ID_dict,
                             n_input_views, threshold=0.01, max_trials=1000, alpha=1.0, generator=None, return_points=False):
    """planes/refine_depth_with_planes.py without its file I/O: fit_global_planes, then
    depth_cues.refine_depths_with_planes with the fitted planes.  Returns (refined depth maps or (maps, points), planes,
    info)."""
    planes, info = fit_global_planes(cameras, depths, rend_normals, plane_masks, conf_maps, global_3Dplane_ID_dict, threshold,
                                     max_trials, alpha, generator)
    refined = depth_cues.refine_depths_with_planes(cameras, depths, plane_masks, conf_maps, mono_depths, global_3Dplane_ID_dict,
                                                   planes, n_input_views, return_points)
    return refined, planes, info
