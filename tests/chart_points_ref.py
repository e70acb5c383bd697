"""The chart points' contract (include/g4s_losses.h, "Chart points") restated in numpy, operation for operation, in a float
type of the caller's choice: float32 mirrors the kernels' order of operations, so stored floats can be compared bit for bit;
float64 pins the restatement against the reference's float64 run.  Nothing here touches a GPU.

Points are packed: points [N,3] with offsets [n+1]; chart [N] is the chart of each point."""
from types import SimpleNamespace

import numpy as np

SPAN = 4096  # G4S_CHART_POINTS_SPAN
CHUNK = 64   # G4S_CHART_POINTS_CHUNK


def camera_records(cameras):
    """float64 [n,32]: world_view_transform and full_proj_transform, row-major.  The kernels read its float32 rounding."""
    return np.stack([np.concatenate([np.asarray(c.world_view_transform, np.float64).reshape(16),
                                     np.asarray(c.full_proj_transform, np.float64).reshape(16)]) for c in cameras])


def pack(point_lists):
    """(points [N,3] float32, offsets int32 [n+1], chart int32 [N]) of a ragged list."""
    counts = [len(p) for p in point_lists]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    points = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in point_lists]) if sum(counts) else np.zeros((0, 3), np.float32)
    chart = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    return points, offsets, chart


def _rows(p, M, c):
    return ((p[:, 0] * M[:, 0, c] + p[:, 1] * M[:, 1, c]) + p[:, 2] * M[:, 2, c]) + M[:, 3, c]


def project(cameras, points, chart, H, W, ftype=np.float32):
    """z [N], ix [N], iy [N] (a clipped point at (-2, -2)), clipped bool [N]."""
    T = ftype
    rec = camera_records(cameras).astype(T)
    p = np.asarray(points, T).reshape(-1, 3)
    V, F = rec[chart, :16].reshape(-1, 4, 4), rec[chart, 16:].reshape(-1, 4, 4)
    with np.errstate(all="ignore"):
        z = _rows(p, V, 2)
        q0, q1, q3 = _rows(p, F, 0), _rows(p, F, 1), _rows(p, F, 3)
        gx, gy = q0 / q3, q1 / q3
        clipped = ~(q3 > 0) | ~np.isfinite(gx) | ~np.isfinite(gy)
        ix = ((gx + T(1)) * T(W) - T(1)) / T(2)
        iy = ((gy + T(1)) * T(H) - T(1)) / T(2)
    return z, np.where(clipped, T(-2), ix), np.where(clipped, T(-2), iy), clipped


def taps(ix, iy, H, W):
    """(index [N,4] into the chart's map, -1 outside; weight [N,4]) in the order nw, ne, sw, se."""
    T = ix.dtype.type
    with np.errstate(all="ignore"):
        fx0, fy0 = np.floor(ix), np.floor(iy)
        wx1, wy1 = ix - fx0, iy - fy0
        wx0, wy0 = (fx0 + T(1)) - ix, (fy0 + T(1)) - iy
        inx = [(fx0 >= 0) & (fx0 <= W - 1), (fx0 >= -1) & (fx0 <= W - 2)]
        iny = [(fy0 >= 0) & (fy0 <= H - 1), (fy0 >= -1) & (fy0 <= H - 2)]
        x0 = np.where(inx[0] | inx[1], fx0, 0).astype(np.int64)
        y0 = np.where(iny[0] | iny[1], fy0, 0).astype(np.int64)
        idx, wts = [], []
        for dy, dx, w in ((0, 0, wx0 * wy0), (0, 1, wx1 * wy0), (1, 0, wx0 * wy1), (1, 1, wx1 * wy1)):
            inside = inx[dx] & iny[dy]
            idx.append(np.where(inside, (y0 + dy) * W + (x0 + dx), -1))
            wts.append(w)
    return np.stack(idx, -1), np.stack(wts, -1)


def sample(maps, chart, ix, iy):
    """(value [N], fov bool [N]) of maps [n,H,W] in the coordinates' float type."""
    T = ix.dtype.type
    n, H, W = maps.shape
    m = np.asarray(maps, T).reshape(n, H * W)
    idx, w = taps(ix, iy, H, W)
    with np.errstate(all="ignore"):
        v = [np.where(idx[:, c] >= 0, w[:, c] * m[chart, np.maximum(idx[:, c], 0)], T(0)) for c in range(4)]
        value = ((v[0] + v[1]) + v[2]) + v[3]
    return value, value > 0


def fit(z, d, offsets, use_fov_mask=False, ftype=np.float32):
    """(coeffs [n,2] of `ftype`, counts int32 [n]): float64 sums, alpha and beta in float64, rounded once."""
    n = len(offsets) - 1
    coeffs, counts = np.zeros((n, 2), ftype), np.zeros(n, np.int32)
    for c in range(n):
        zc, dc = z[offsets[c]:offsets[c + 1]], d[offsets[c]:offsets[c + 1]]
        if use_fov_mask:
            keep = dc > 0
            zc, dc = zc[keep], dc[keep]
        with np.errstate(all="ignore"):
            t = (z.dtype.type(1) / zc).astype(np.float64)
            dd = dc.astype(np.float64)
            cnt = np.float64(len(dd))
            St, Sd, Std, Sdd = t.sum(), dd.sum(), (t * dd).sum(), (dd * dd).sum()
            beta = (Std - St * Sd / cnt) / (Sdd - Sd * Sd / cnt)
            alpha = (St - beta * Sd) / cnt
        coeffs[c] = (alpha, beta)
        counts[c] = len(dd)
    return coeffs, counts


def apply(disparities, coeffs, scale=1.0):
    T = coeffs.dtype.type
    d = np.asarray(disparities, T)
    with np.errstate(all="ignore"):
        return T(scale) * (T(1) / (coeffs[:, 0, None, None] + coeffs[:, 1, None, None] * d))


def view_depths(cameras, points, chart, scale=1.0, ftype=np.float32):
    """z of scale P for packed points [N,3] with their charts."""
    T = ftype
    rec = camera_records(cameras).astype(T)
    p = T(scale) * np.asarray(points, T).reshape(-1, 3)
    return _rows(p, rec[chart, :16].reshape(-1, 4, 4), 2)


def view_depths_of_point_maps(cameras, point_maps, scale=1.0, ftype=np.float32):
    n, H, W = point_maps.shape[:3]
    chart = np.repeat(np.arange(n), H * W)
    return view_depths(cameras, point_maps.reshape(-1, 3), chart, scale, ftype).reshape(n, H, W)


def _signed(v):
    return (v > 0).astype(v.dtype) - (v < 0).astype(v.dtype)  # sign(0) = 0


def spread(grad_points, chart, ix, iy, n, H, W):
    """dL/dmap [n,H,W] of dL/dvalue [N]: per pixel the sum of its taps in ascending (point, corner) order, in chunks of CHUNK,
    in the gradient's float type (float32: the kernels' order; float64: the same order, which then hardly matters)."""
    T = grad_points.dtype.type
    idx, w = taps(ix, iy, H, W)
    N = len(ix)
    pix = np.where(idx >= 0, chart[:, None].astype(np.int64) * (H * W) + idx, -1).reshape(-1)
    term = (grad_points[:, None] * w).reshape(-1)
    ids = np.flatnonzero(pix >= 0)
    order = ids[np.argsort(pix[ids], kind="stable")]  # ids ascend, so (pixel, point, corner)
    spix = pix[order]
    total, acc = np.zeros(n * H * W, T), np.zeros(n * H * W, T)
    if len(order):
        first = np.flatnonzero(np.r_[True, spix[1:] != spix[:-1]])
        rank = np.arange(len(order)) - np.repeat(first, np.diff(np.r_[first, len(order)]))
        for r in range(int(rank.max()) + 1):
            if r and r % CHUNK == 0:
                total = total + acc
                acc = np.zeros_like(acc)
            sel = rank == r
            acc[spix[sel]] = acc[spix[sel]] + term[order[sel]]
    return (total + acc).reshape(n, H, W)


def point_reference_loss(depths, chart, ix, iy, z, confidence=None, cw=0.2, cotangent=1.0, need_grad=True):
    """The point-reference term and its gradients: a namespace with loss (the float type's rounding of the float64 mean), s, k,
    e per point and, with need_grad, d_depths and d_confidence [n,H,W] (None without a confidence)."""
    T = ix.dtype.type
    n, H, W = depths.shape
    N = len(ix)
    s, _ = sample(depths, chart, ix, iy)
    k = sample(confidence, chart, ix, iy)[0] if confidence is not None else None
    with np.errstate(all="ignore"):
        e = np.abs(s - z)
        term = e if k is None else k * e - T(cw) * np.log(k)
        out = SimpleNamespace(loss=T(term.astype(np.float64).sum() / np.float64(N)), s=s, k=k, e=e)
        if need_grad:
            c = T(cotangent) / T(N)
            sg = _signed(s - z)
            ds = c * sg if k is None else (c * k) * sg
            out.d_depths = spread(ds, chart, ix, iy, n, H, W)
            out.d_confidence = None if k is None else spread(c * (e - T(cw) / k), chart, ix, iy, n, H, W)
    return out


def scale_factor(cameras, target_scale=5.0):
    """target_scale / (1.1 x the largest distance of a camera centre from the mean centre), in double."""
    c = np.stack([np.linalg.inv(np.asarray(cam.world_view_transform, np.float64).reshape(4, 4).T)[:3, 3] for cam in cameras])
    return target_scale / (1.1 * float(np.linalg.norm(c - c.mean(axis=0, keepdims=True), axis=1).max()))


def optimize_with_points(c, params, raw, point_lists, n_iterations, weights, weighted, lam=0.2, encodings_lr=1e-2, mlp_lr=1e-3,
                         confidence_lr=1e-3, T=np.float64):
    """chart_aligner_ref.optimize with 3D points as the reference: the same loop, the depth term replaced by the point-reference
    term (the fused terms run with an all-zero mask, which makes their depth term exactly 0).  Returns the losses of every
    iteration."""
    import chart_align_ref
    import chart_aligner_ref as ar
    import chart_deform_ref as cd
    c = SimpleNamespace(**vars(c))
    params = {k: np.asarray(v, T).copy() for k, v in params.items()}
    raw = np.asarray(raw, T).copy()
    names = ar.group_names(c)
    lrs = dict(zip(names, ar.group_learning_rates(names, encodings_lr, mlp_lr, confidence_lr)))
    state = {k: (np.zeros_like(raw if k == "_confidence" else params[k]), np.zeros_like(raw if k == "_confidence" else params[k]))
             for k in names}
    d0 = c.d0.astype(T)
    zeros = np.zeros_like(d0)
    nu0 = chart_align_ref.normals(c.cams, d0, T)
    curv0 = chart_align_ref.curvatures(nu0)
    flags = ((chart_align_ref.GRADIENT if weights.get("gradient") is not None else 0)
             | (chart_align_ref.NORMAL if weights.get("normal") is not None else 0)
             | (chart_align_ref.CURVATURE if weights.get("curvature") is not None else 0))
    use_norm, use_tv = (weights.get(k) is not None for k in ("norm", "tv"))
    points, _offsets, chart = pack(point_lists)
    z, ix, iy, _clipped = project(c.cams, points, chart, c.H, c.W, T)
    losses = []
    for i in range(n_iterations):
        ar.set_parameters(c, params)
        conf, w = ar.confidence(raw, T)
        w = w if weighted else None
        f = ar.forward(c, w, T)
        reg = ar.regularizers(c, f, use_norm, use_tv, T)
        args = (c.cams, f.depths, zeros, d0, nu0, curv0)
        terms = list(chart_align_ref.evaluate(*args, confidence=conf, masks=zeros, lam=lam, flags=flags, ftype=T).means)
        assert terms[0] == 0
        cot = (0.0, weights.get("gradient") or 0.0, weights.get("normal") or 0.0, weights.get("curvature") or 0.0)
        gd, dconf = chart_align_ref.gradients(*args, confidence=conf, masks=zeros, lam=lam, flags=flags, cotangents=cot, ftype=T)
        pt = point_reference_loss(f.depths.astype(T), chart, ix, iy, z, conf.astype(T), lam)
        terms[0] = pt.loss
        gd, dconf = gd + pt.d_depths, dconf + pt.d_confidence
        losses.append(float(ar.total_loss(terms, reg, None, weights)))
        grads = cd.flat_gradients(c, ar.gradients(c, gd, (weights.get("norm") or 0.0, weights.get("tv") or 0.0), w, use_norm, use_tv, T))
        grads["_confidence"] = ar.confidence_backward(raw, dconf, T)
        for k in names:
            m, v = state[k]
            if k == "_confidence":
                raw, m, v = ar.adam_step(raw, grads[k], m, v, i + 1, lrs[k])
            else:
                params[k], m, v = ar.adam_step(params[k], grads[k], m, v, i + 1, lrs[k])
            state[k] = (m, v)
    return losses
