"""The "Depth cues" contract of include/g4s_render_maps.h in numpy, one operation per rounding, parameterised by dtype:
float32 is the library's arithmetic bit for bit (the per-pixel stages) or to the last place (the coefficients, whose sums
are exact here -- math.fsum -- and float64 in a fixed order there); float64 is what tests/test_depth_cues_cpu.py holds
against the reference's float64 run.  Nothing here imports the product."""
import math
from types import SimpleNamespace

import numpy as np

DISPARITY, DEPTH, INVERSE_SOURCE = 0, 1, 2
f64 = np.float64


# ---- cameras -----------------------------------------------------------------------------------------------------------------
def ray_record(cam, W, H, dtype):
    """o[3], D[3][3]: computed in double as the contract says, then rounded to dtype."""
    wvt = np.asarray(cam.world_view_transform, f64).reshape(4, 4)
    full = np.asarray(cam.full_proj_transform, f64).reshape(4, 4)
    c2w = np.linalg.inv(wvt.T)
    ndc2pix = np.array([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], f64).T
    intr = ((c2w.T @ full) @ ndc2pix)[:3, :3].T
    D = c2w[:3, :3] @ np.linalg.inv(intr)
    return c2w[:3, 3].astype(dtype), D.astype(dtype)


def plane_camera(cam, W, H, dtype):
    """o[3], R[3][3] (camera -> world), fx, fy: in double, then rounded to dtype."""
    c2w = np.linalg.inv(np.asarray(cam.world_view_transform, f64).reshape(4, 4)).T
    fx = W / (2.0 * math.tan(float(cam.FoVx) / 2.0))
    fy = H / (2.0 * math.tan(float(cam.FoVy) / 2.0))
    return c2w[:3, 3].astype(dtype), c2w[:3, :3].astype(dtype), dtype(fx), dtype(fy)


# ---- A. alignment ------------------------------------------------------------------------------------------------------------
def _exact_sum(x):
    """The correctly rounded float64 sum; with a non-finite term, what IEEE addition gives (NaN or inf)."""
    x = np.asarray(x, f64)
    if np.isfinite(x).all():
        return f64(math.fsum(x.tolist()))
    with np.errstate(all="ignore"):
        return f64(np.sum(x))


def align_terms(src, tgt, mask, domain, dtype):
    """t and d of the masked pixels, in dtype."""
    s = np.asarray(src, dtype).reshape(-1)[np.asarray(mask).reshape(-1).astype(bool)]
    g = np.asarray(tgt, dtype).reshape(-1)[np.asarray(mask).reshape(-1).astype(bool)]
    with np.errstate(all="ignore"):
        t = g if domain == DEPTH else dtype(1) / g
        d = dtype(1) / s if domain == INVERSE_SOURCE else s
    return t, d


def align_coeffs(src, tgt, mask, domain, dtype):
    """(alpha, beta, n): exact sums, the two quotients in float64, rounded to dtype."""
    t, d = align_terms(src, tgt, mask, domain, dtype)
    t, d = t.astype(f64), d.astype(f64)
    with np.errstate(all="ignore"):
        n = f64(len(t))
        St, Sd, Std, Sdd = _exact_sum(t), _exact_sum(d), _exact_sum(t * d), _exact_sum(d * d)
        beta = (Std - St * Sd / n) / (Sdd - Sd * Sd / n)
        alpha = (St - beta * Sd) / n
        return dtype(alpha), dtype(beta), int(n)


def variance_share(src, tgt, mask, domain, dtype):
    """(Sdd - Sd^2 / n) / Sdd: the share of the denominator that survives its cancellation."""
    _t, d = align_terms(src, tgt, mask, domain, dtype)
    d = d.astype(f64)
    Sd, Sdd = _exact_sum(d), _exact_sum(d * d)
    return float((Sdd - Sd * Sd / len(d)) / Sdd)


def aligned(alpha, beta, src, domain, dtype):
    src = np.asarray(src, dtype)
    with np.errstate(all="ignore"):
        d = dtype(1) / src if domain == INVERSE_SOURCE else src
        lin = dtype(alpha) + dtype(beta) * d
        return lin if domain == DEPTH else dtype(1) / lin


# ---- B. cue maps -------------------------------------------------------------------------------------------------------------
def back_project(cam, depth, dtype):
    """[H,W,3]: o + depth * ((D[r][0] x + D[r][1] y) + D[r][2])."""
    H, W = depth.shape
    o, D = ray_record(cam, W, H, dtype)
    x = np.arange(W, dtype=dtype)[None, :]
    y = np.arange(H, dtype=dtype)[:, None]
    with np.errstate(all="ignore"):
        return np.stack([o[r] + np.asarray(depth, dtype) * ((D[r, 0] * x + D[r, 1] * y) + D[r, 2]) for r in range(3)], -1)


def cue_maps(cam, disp, warp, alpha_map, threshold, alpha, beta, dtype):
    """dict: visibility, mono_depth, aligned_depth, depth, normal_world, normal_cam of one view."""
    disp = np.asarray(disp, dtype)
    H, W = disp.shape
    vis = np.asarray(alpha_map, np.float32) > np.float32(threshold)
    with np.errstate(all="ignore"):
        mono = dtype(1) / disp
        a = aligned(alpha, beta, disp, DISPARITY, dtype)
        merged = np.where(vis, np.asarray(warp, dtype), a)
        nw, nc = np.zeros((H, W, 3), dtype), np.zeros((H, W, 3), dtype)  # the border is +0 in both
        if H >= 3 and W >= 3:
            P = back_project(cam, a, dtype)
            dx = P[2:, 1:-1] - P[:-2, 1:-1]
            dy = P[1:-1, 2:] - P[1:-1, :-2]
            n = np.stack([dx[..., 1] * dy[..., 2] - dx[..., 2] * dy[..., 1], dx[..., 2] * dy[..., 0] - dx[..., 0] * dy[..., 2],
                          dx[..., 0] * dy[..., 1] - dx[..., 1] * dy[..., 0]], -1)
            length = np.fmax(np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]), dtype(1e-12))
            m = n / length[..., None]
            Wv = np.asarray(cam.world_view_transform, dtype).reshape(4, 4)
            nw[1:-1, 1:-1] = m
            nc[1:-1, 1:-1] = np.stack([(m[..., 0] * Wv[0, j] + m[..., 1] * Wv[1, j]) + m[..., 2] * Wv[2, j] for j in range(3)], -1)
    return {"visibility": vis, "mono_depth": mono, "aligned_depth": a, "depth": merged, "normal_world": nw, "normal_cam": nc}


def view_geometry_cues(cams, disps, warps, alpha_maps, threshold, dtype):
    out = []
    for cam, d, w, am in zip(cams, disps, warps, alpha_maps):
        vis = np.asarray(am, np.float32) > np.float32(threshold)
        alpha, beta, n = align_coeffs(d, w, vis, DISPARITY, dtype)
        out.append(dict(cue_maps(cam, d, w, am, threshold, alpha, beta, dtype), coeffs=(alpha, beta), count=n))
    return out


# ---- C. plane depths ---------------------------------------------------------------------------------------------------------
def fitted_pairs(gdict, planes, n_views):
    """Per view {mask id: global key}: the pairs of the keys `planes` holds, later keys overwriting earlier ones."""
    per_view = [dict() for _ in range(n_views)]
    for key, pairs in gdict.items():
        if key not in planes:
            continue
        for v, p in pairs:
            per_view[int(v)][int(p)] = key
    return per_view


def plane_depth_image(normal, centre, cam, H, W, dtype):
    """(z [H,W], valid [H,W]): the whole image against one plane, before the paste."""
    o, R, fx, fy = plane_camera(cam, W, H, dtype)
    n, c = np.asarray(normal, dtype).reshape(3), np.asarray(centre, dtype).reshape(3)
    x = np.arange(W, dtype=dtype)[None, :]
    y = np.arange(H, dtype=dtype)[:, None]
    with np.errstate(all="ignore"):
        dcx = (x - dtype(W) * dtype(0.5)) / fx + np.zeros((H, 1), dtype)
        dcy = (y - dtype(H) * dtype(0.5)) / fy + np.zeros((1, W), dtype)
        w = [(R[r, 0] * dcx + R[r, 1] * dcy) + R[r, 2] for r in range(3)]
        length = np.fmax(np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]), dtype(1e-12))
        nd = (n[0] * (w[0] / length) + n[1] * (w[1] / length)) + n[2] * (w[2] / length)
        ndc = np.copysign(np.fmax(np.abs(nd), dtype(1e-8)), nd)
        num = (n[0] * (c[0] - o[0]) + n[1] * (c[1] - o[1])) + n[2] * (c[2] - o[2])
        t = num / ndc
        z = t / length
    return z, (t > 0) & (z > 0)


def plane_terms(normal, centre, cam, H, W, dtype):
    """(nd [H,W], num, length [H,W]) of plane_depth_image: the normal against the unit ray, before the 1e-8 clamp; the
    normal against centre - camera; the length of the ray at unit camera depth.  A test reads from them which pixels the
    clamp decides and in which sign; z = num / copysign(max(|nd|, 1e-8), nd) / length."""
    o, R, fx, fy = plane_camera(cam, W, H, dtype)
    n, c = np.asarray(normal, dtype).reshape(3), np.asarray(centre, dtype).reshape(3)
    x = np.arange(W, dtype=dtype)[None, :]
    y = np.arange(H, dtype=dtype)[:, None]
    with np.errstate(all="ignore"):
        dcx = (x - dtype(W) * dtype(0.5)) / fx + np.zeros((H, 1), dtype)
        dcy = (y - dtype(H) * dtype(0.5)) / fy + np.zeros((1, W), dtype)
        w = [(R[r, 0] * dcx + R[r, 1] * dcy) + R[r, 2] for r in range(3)]
        length = np.fmax(np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]), dtype(1e-12))
        nd = (n[0] * (w[0] / length) + n[1] * (w[1] / length)) + n[2] * (w[2] / length)
        num = (n[0] * (c[0] - o[0]) + n[1] * (c[1] - o[1])) + n[2] * (c[2] - o[2])
    return nd, num, length


def fitted_ids(gdict, planes, n_views):
    """Per view the ascending mask ids that have a fitted plane: the runs the library's id table holds."""
    return [sorted(pairs) for pairs in fitted_pairs(gdict, planes, n_views)]


def apply_global_planes(cams, depths, masks, gdict, planes, dtype):
    """(new depths, replaced [V], zeroed [V], touched [V] bool maps, valid [V] bool maps)."""
    V = len(cams)
    pairs = fitted_pairs(gdict, planes, V)
    outs, replaced, zeroed, touched, valids = [], [], [], [], []
    for v in range(V):
        d = np.array(depths[v], dtype)
        H, W = d.shape
        touch, ok = np.zeros((H, W), bool), np.zeros((H, W), bool)
        for pid, key in pairs[v].items():
            region = np.asarray(masks[v]) == pid
            if not region.any():
                continue
            z, valid = plane_depth_image(planes[key][0], planes[key][1], cams[v], H, W, dtype)
            d[region] = np.where(valid, z, dtype(0))[region]
            touch |= region
            ok |= region & valid
        outs.append(d)
        touched.append(touch)
        valids.append(ok)
        replaced.append(int(ok.sum()))
        zeroed.append(int((touch & ~ok).sum()))
    return outs, np.array(replaced, np.int32), np.array(zeroed, np.int32), touched, valids


# ---- D. refill ---------------------------------------------------------------------------------------------------------------
def refill(depths, monos, masks, confs, n_input, dtype):
    """(new depths, coeffs per view -- (0, 0) for an input view --, counts)."""
    outs, coeffs, counts = [], [], []
    for v, d in enumerate(depths):
        d = np.array(d, dtype)
        if v < n_input:
            outs.append(d)
            coeffs.append((dtype(0), dtype(0)))
            counts.append(0)
            continue
        conf = np.asarray(confs[v]).astype(bool)
        alpha, beta, n = align_coeffs(monos[v], d, conf, INVERSE_SOURCE, dtype)
        region = (np.asarray(masks[v]) == 0) & ~conf
        d[region] = aligned(alpha, beta, monos[v], INVERSE_SOURCE, dtype)[region]
        outs.append(d)
        coeffs.append((alpha, beta))
        counts.append(n)
    return outs, coeffs, counts


def refine_depths_with_planes(cams, depths, masks, confs, monos, gdict, planes, n_input, dtype):
    """(refined depths, coeffs, touched, valid)."""
    planed, _r, _z, touched, valid = apply_global_planes(cams, depths, masks, gdict, planes, dtype)
    outs, coeffs, _counts = refill(planed, monos, masks, confs, n_input, dtype)
    return outs, coeffs, touched, valid


# ---- scenes that two test files share: built here once, pinned without a GPU by tests/test_depth_cues_cpu.py -----------------
ID_RUNS = (2, 0, 1, 3, 7, 64, 65)  # fitted ids per view: the view without any sits between two that have some
ID_SIZES = ((45, 67), (48, 64), (45, 67), (48, 64), (45, 67), (48, 64), (45, 67))
ID_TOP = 2 ** 31 - 1
_ID_FORCED = {0: [], 1: [1000], 2: [5, 6], 3: [6, 1000, ID_TOP - 1], 7: [5, 6], 64: [5, 6, 1001], 65: [1, 5, 6, ID_TOP]}


def id_search_scene(seed=31):
    """A scene for the id search of the plane depths: per view of ID_SIZES a run of ID_RUNS sparse fitted ids between 1 and
    2^31 - 1, spread over five planes whose indices do not ascend with the id, and a mask in which every fitted id occurs, and
    beside them 0, negative values and unfitted ids below the first, between neighbours and above the last fitted one (two of
    them listed under key 99, which has no plane; among them the table's entries just before and just behind the view's run,
    which belong to other views).  A namespace: sizes, depths, masks, gdict, planes, fitted, unfitted."""
    rng = np.random.default_rng(seed)
    planes = {40: ((0.1, 0.2, 0.97), (0.0, 0.0, 0.3)), 7: ((0.9, -0.1, 0.2), (0.4, 0.0, 0.0)), 19: ((0.0, 1.0, 0.05), (0.0, 0.6, 0.0)),
              3: ((-0.3, 0.1, 0.95), (0.0, 0.0, -0.2)), 88: ((0.2, -0.9, 0.3), (0.0, -0.5, 0.1))}
    keys = list(planes)
    gdict = {key: [] for key in keys + [99]}
    interior = np.unique(rng.integers(2000, ID_TOP - 1000, 400)).tolist()
    depths, masks, fitted, unfitted = [], [], [], []
    for v, n in enumerate(ID_RUNS):
        forced = _ID_FORCED[n]
        ids = sorted(forced + rng.choice(interior, n - len(forced), replace=False).tolist())
        assert len(set(ids)) == n
        for p in ids:
            gdict[keys[int(rng.integers(len(keys)))]].append((v, p))
        fitted.append(ids)
    table = [p for ids in fitted for p in ids]  # the library's id table: the runs one behind the other
    for v, (ids, (H, W)) in enumerate(zip(fitted, ID_SIZES)):
        first = sum(len(run) for run in fitted[:v])
        beside = table[max(first - 1, 0):first] + table[first + len(ids):first + len(ids) + 1]  # the entries next to the run
        near = [q for p in ids for q in (p - 1, p + 1)] + [(a + b) // 2 for a, b in zip(ids, ids[1:])] + [1, 2, ID_TOP, ID_TOP - 7]
        others = sorted({q for q in near + beside if 1 <= q <= ID_TOP} - set(ids))
        gdict[99] += [(v, others[0]), (v, others[-1])]
        values = ids + others + [0, -1, -(2 ** 31)] + [-p for p in ids[:3]]
        mask = rng.choice(np.array(values, np.int64), H * W)
        mask[rng.permutation(H * W)[:len(values)]] = values  # every value occurs
        depths.append(rng.uniform(1.0, 4.0, (H, W)).astype(np.float32))
        masks.append(mask.astype(np.int32).reshape(H, W))
        unfitted.append(others)
    return SimpleNamespace(sizes=list(ID_SIZES), depths=depths, masks=masks, gdict=gdict, planes=planes, fitted=fitted,
                           unfitted=unfitted)


def clamp_scene(seed=41):
    """A 48 x 64 view of an identity camera (w = (dcx, dcy, 1)) whose mask spreads three planes over the image: ids 1 and 2,
    n = (+-1e-9, 0, 0) through (5, 0, 0), have |n.d| < 1e-8 in every pixel, in both signs and exactly zero in column W / 2;
    id 3 passes through the camera centre (num = 0).  A namespace: cam, H, W, depth, mask, gdict, planes."""
    rng = np.random.default_rng(seed)
    H, W = 48, 64
    cam = SimpleNamespace(world_view_transform=np.eye(4, dtype=np.float32), full_proj_transform=np.eye(4, dtype=np.float32),
                          FoVx=1.0, FoVy=0.8, image_width=W, image_height=H)
    planes = {1: ((1e-9, 0.0, 0.0), (5.0, 0.0, 0.0)), 2: ((-1e-9, 0.0, 0.0), (5.0, 0.0, 0.0)), 3: ((0.0, 0.0, 1.0), (2.0, -3.0, 0.0))}
    return SimpleNamespace(cam=cam, H=H, W=W, depth=rng.uniform(1.0, 4.0, (H, W)).astype(np.float32),
                           mask=rng.integers(0, 4, (H, W)).astype(np.int32), gdict={k: [(0, k)] for k in planes}, planes=planes)
