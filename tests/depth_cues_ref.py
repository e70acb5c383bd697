"""The "Depth cues" contract of include/g4s_render_maps.h in numpy, one operation per rounding, parameterised by dtype:
float32 is the library's arithmetic bit for bit (the per-pixel stages) or to the last place (the coefficients, whose sums
are exact here -- math.fsum -- and float64 in a fixed order there); float64 is what tests/test_depth_cues_cpu.py holds
against the reference's float64 run.  Nothing here imports the product."""
import math

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
