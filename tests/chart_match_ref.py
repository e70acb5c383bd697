"""The chart matcher's contract (include/g4s_losses.h, "Chart matcher") restated in numpy, operation for operation, in a
float type of the caller's choice: float32 for the bit comparisons with the kernels, float64 for pinning against the
reference's float64 run.  Nothing here touches a GPU.  The bilinear tap follows tests/view_tap_ref.py's style, with
grid_sample's zero padding: a tap off the map adds nothing to the value and nothing to a gradient.

Axes: i the TARGET view (whose camera projects and whose depth map is tapped), j the SOURCE view (whose pixel p = y W + x
is back-projected)."""
from types import SimpleNamespace

import numpy as np

ZNEAR = 1e-6
NO_MATCH = 1e8


def camera_records(cameras, W, H):
    """float64 [n,44] per view: ray origin o[3], ray matrix D[3][3] (dir = D @ (x, y, 1), the record of
    g4splat_amd.visibility.ray_record), world_view_transform[4][4], projection_matrix[4][4], row-major.  The kernels read
    its float32 rounding."""
    out = []
    for cam in cameras:
        wvt = np.asarray(cam.world_view_transform, np.float64).reshape(4, 4)
        full = np.asarray(cam.full_proj_transform, np.float64).reshape(4, 4)
        proj = np.asarray(cam.projection_matrix, np.float64).reshape(4, 4)
        c2w = np.linalg.inv(wvt.T)
        ndc2pix = np.array([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], np.float64).T
        intr = ((c2w.T @ full) @ ndc2pix)[:3, :3].T
        D = c2w[:3, :3] @ np.linalg.inv(intr)
        out.append(np.concatenate([c2w[:3, 3], D.reshape(9), wvt.reshape(16), proj.reshape(16)]))
    return np.stack(out)


def _signed(v):
    return (v > 0).astype(v.dtype) - (v < 0).astype(v.dtype)  # sign(0) = 0


def evaluate(cameras, depths, ftype=np.float32, need_grad=False):
    """Every pair (i, j, p) at the depths [n,H,W]: a namespace of [n,n,H*W] arrays
        z, s (the sampled depth before the fov product), fov, e = |z - s fov|, ix, iy, w (the clamped divisor's input)
    and, with need_grad, dsrc = d(z - s)/dD_j[p] through the source point plus taps = (index [n,n,HW,4] into the target
    map, weight [n,n,HW,4], inside [n,n,HW,4])."""
    T = ftype
    D = np.ascontiguousarray(depths, T)
    n, H, W = D.shape
    N = H * W
    rec = camera_records(cameras, W, H).astype(T)
    m = min(H, W)
    fax, fay, fbx, fby = T(W / m), T(H / m), T(-m / W), T(-m / H)
    x = np.tile(np.arange(W, dtype=T), H)[None, :]
    y = np.repeat(np.arange(H, dtype=T), W)[None, :]
    o, R = rec[:, 0:3], rec[:, 3:12].reshape(n, 3, 3)
    dirs = [(R[:, k, 0:1] * x + R[:, k, 1:2] * y) + R[:, k, 2:3] for k in range(3)]   # [n_j, N]
    d = D.reshape(n, N)
    q = [d * dirs[k] + o[:, k:k + 1] for k in range(3)]
    WV, P = rec[:, 12:28].reshape(n, 1, 1, 4, 4), rec[:, 28:44].reshape(n, 1, 1, 4, 4)

    def rows3(a, M, c, last):  # ((a0 M0c + a1 M1c) + a2 M2c) [+ M3c]
        r = (a[0] * M[..., 0, c] + a[1] * M[..., 1, c]) + a[2] * M[..., 2, c]
        return r + M[..., 3, c] if last else r

    qb = [t[None] for t in q]  # [1, n_j, N]
    with np.errstate(all="ignore"):
        v = [rows3(qb, WV, c, True) for c in range(3)]
        z = v[2]
        a = [-v[0], -v[1], z]
        pr = {c: rows3(a, P, c, True) for c in (0, 1, 3)}
        zn = T(ZNEAR)
        wc = np.where(pr[3] < zn, zn, pr[3])
        g0x, g0y = pr[0] / wc, pr[1] / wc
        fin = np.isfinite(g0x) & np.isfinite(g0y)
        g0x, g0y = np.where(np.isfinite(g0x), g0x, T(0)), np.where(np.isfinite(g0y), g0y, T(0))
        gx, gy = (g0x * fax) * fbx, (g0y * fay) * fby
        ix, iy = ((gx + T(1)) * T(W) - T(1)) / T(2), ((gy + T(1)) * T(H) - T(1)) / T(2)
        fx0, fy0 = np.floor(ix), np.floor(iy)
        wx1, wy1 = ix - fx0, iy - fy0
        wx0, wy0 = (fx0 + T(1)) - ix, (fy0 + T(1)) - iy
        inx = [(fx0 >= 0) & (fx0 <= W - 1), (fx0 >= -1) & (fx0 <= W - 2)]
        iny = [(fy0 >= 0) & (fy0 <= H - 1), (fy0 >= -1) & (fy0 <= H - 2)]
        x0 = np.where(inx[0] | inx[1], fx0, 0).astype(np.int64)
        y0 = np.where(iny[0] | iny[1], fy0, 0).astype(np.int64)
        view = np.arange(n)[:, None, None]
        s = np.zeros_like(z)
        six, siy = np.zeros_like(z), np.zeros_like(z)
        taps = []
        for dy, dx, wt, gxs, gys in ((0, 0, wx0 * wy0, -wy0, -wx0), (0, 1, wx1 * wy0, wy0, -wx1),
                                    (1, 0, wx0 * wy1, -wy1, wx0), (1, 1, wx1 * wy1, wy1, wx1)):
            inside = inx[dx] & iny[dy]
            idx = np.where(inside, (y0 + dy) * W + (x0 + dx), 0)
            val = D.reshape(n, N)[view, idx]
            s = np.where(inside, s + wt * val, s)
            six = np.where(inside, six + val * gxs, six)
            siy = np.where(inside, siy + val * gys, siy)
            taps.append((idx, np.where(inside, wt, T(0)), inside))
        fov = (z > 0) & fin & (s > 0)
        e = np.abs(z - s * fov.astype(T))
    out = SimpleNamespace(n=n, H=H, W=W, z=z, s=s, fov=fov, e=e, ix=ix, iy=iy, w=pr[3], fin=fin)
    if need_grad:
        with np.errstate(all="ignore"):
            db = [t[None] for t in dirs]
            dv = [rows3(db, WV, c, False) for c in range(3)]
            da = [-dv[0], -dv[1], dv[2]]
            dpr = {c: rows3(da, P, c, False) for c in (0, 1, 3)}
            dwc = np.where(pr[3] >= zn, dpr[3], T(0))
            dgx = ((dpr[0] / wc - (g0x / wc) * dwc) * fax) * fbx
            dgy = ((dpr[1] / wc - (g0y / wc) * dwc) * fay) * fby
            dix, diy = dgx * T(W / 2), dgy * T(H / 2)
            out.dsrc = dv[2] - (six * dix + siy * diy)
        out.taps = (np.stack([t[0] for t in taps], -1), np.stack([t[1] for t in taps], -1), np.stack([t[2] for t in taps], -1))
    return out


def match(cameras, depths, thr, ftype=np.float32):
    """(matches bool [n,n,H,W], errors [n,n,H,W] with 1e8 outside the fov, fov bool [n,n,H,W]) at the reference depths."""
    r = evaluate(cameras, depths, ftype)
    shape = (r.n, r.n, r.H, r.W)
    err = np.where(r.fov, r.e, ftype(NO_MATCH))
    return (err < ftype(thr)).reshape(shape), err.reshape(shape), r.fov.reshape(shape)


def reprojection_errors(cameras, depths, ftype=np.float32):
    """(errors, fov) [n,n,H,W] of compute_reprojection_errors: nan_to_num(|z - s fov|) and the fov mask."""
    r = evaluate(cameras, depths, ftype)
    shape = (r.n, r.n, r.H, r.W)
    return np.nan_to_num(r.e).reshape(shape), r.fov.reshape(shape)


def pack_words(matches):
    """uint32 [n,n,ceil(HW/32)]: bit p mod 32 of word p // 32; the tail word's unused bits are 0."""
    n = matches.shape[0]
    flat = matches.reshape(n, n, -1)
    N = flat.shape[2]
    nw = (N + 31) // 32
    padded = np.zeros((n, n, nw * 32), bool)
    padded[:, :, :N] = flat
    bits = padded.reshape(n, n, nw, 32).astype(np.uint32)
    return (bits << np.arange(32, dtype=np.uint32)).sum(axis=-1, dtype=np.uint32)


def unpack_words(words, H, W):
    n = words.shape[0]
    bits = (words[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(n, n, -1)[:, :, :H * W].astype(bool).reshape(n, n, H, W)


def _clamped(weights, weight_max, ftype):
    w = np.asarray(weights, ftype)
    return w if weight_max is None else np.clip(w, ftype(-weight_max), ftype(weight_max))


def loss(cameras, depths, matches, weights=None, ftype=np.float32, weight_max=None):
    """The mean over (i, j, p) of w_j[p] match fov nan_to_num(|z - s|), summed in `ftype` by numpy; the weights clamped to
    +-weight_max where one is given."""
    r = evaluate(cameras, depths, ftype)
    t = np.where(r.fov & matches.reshape(r.n, r.n, -1), np.nan_to_num(r.e), ftype(0))
    if weights is not None:
        t = t * _clamped(weights, weight_max, ftype).reshape(1, r.n, -1)
    return ftype(t.sum(dtype=ftype) / ftype(t.size))


def loss_grad(cameras, depths, matches, weights=None, cotangent=1.0, ftype=np.float32, weight_max=None, with_bound=False):
    """dL/dD [n,H,W], analytic: the part through the source point and the part through the four taps.  with_bound: also
    [n,H,W], per element, how far two evaluations of these same float32 terms may lie apart when only the ORDER and the
    format of their sums differ (summation_bound)."""
    r = evaluate(cameras, depths, ftype, need_grad=True)
    n, N = r.n, r.H * r.W
    active = r.fov & matches.reshape(n, n, N) & np.isfinite(r.e)
    k = ftype(cotangent) / ftype(n * n * N)
    G = np.where(active, _signed(r.z - r.s), ftype(0))
    if weights is not None:
        G = G * _clamped(weights, weight_max, ftype).reshape(1, n, N)
    with np.errstate(all="ignore"):
        terms = np.where(active, G * r.dsrc, ftype(0))
        src = terms.sum(axis=0, dtype=ftype)
    grad = (k * src).astype(ftype)
    idx, wt, inside = r.taps
    tap, tap_abs, tap_count = np.zeros((n, N), ftype), np.zeros((n, N), np.float64), np.zeros((n, N), np.int64)
    for i in range(n):
        use = inside[i] & active[i][..., None]
        np.add.at(tap[i], idx[i][use], -(G[i][..., None] * wt[i])[use])
        if with_bound:
            np.add.at(tap_abs[i], idx[i][use], np.abs((G[i][..., None] * wt[i])[use]).astype(np.float64))
            np.add.at(tap_count[i], idx[i][use], 1)
    out = (grad + k * tap).reshape(n, r.H, r.W).astype(ftype)
    if not with_bound:
        return out
    return out, summation_bound(float(k), np.abs(terms).sum(axis=0, dtype=np.float64), n, tap_abs, tap_count, out).reshape(out.shape)


def summation_bound(k, src_abs, n_src, tap_abs, tap_count, grad):
    """First-order bound on |a - b| per element of dL/dD for two evaluations a, b that form the SAME float32 terms and
    differ only in how they add them: a float32 sum of T terms in any order is within (T - 1) u S of the exact sum, S the
    sum of the terms' magnitudes and u = 2^-24, so two of them are within 2 (T - 1) u S of each other; the fixed-point tap
    sum is within T 2^-37 of exact and rounds once to float32.  Each side then multiplies the two sums by k and adds them
    (three roundings of results no larger than k (S_src + S_tap)), hence
        2 u k ((n - 1) S_src + (T - 1) S_tap) + 8 u k (S_src + S_tap) + k T 2^-37 + 2 u |grad|.
    It is computed from the terms, never from the result it bounds."""
    u = 2.0 ** -24
    T = np.maximum(tap_count, 1).astype(np.float64)
    return (2 * u * abs(k) * ((n_src - 1) * src_abs + (T - 1) * tap_abs) + 8 * u * abs(k) * (src_abs + tap_abs)
            + abs(k) * T * 2.0 ** -37 + 2 * u * np.abs(np.asarray(grad, np.float64)).reshape(src_abs.shape))


def loss_sum_bound(n, N, value):
    """The same for the loss, whose terms are non-negative: the device adds a thread's n terms in turn, 8 levels of a tree
    over the block and the partials in double; numpy adds float32 in blocks of 128 with 8 running sums (16 steps) and a
    pairwise tree over at most n n N / 128 blocks; each result is within (depth) u of the exact sum relatively, one more
    rounding for the division and one for the result."""
    depth = (n + 8 + 2) + (16 + max(1, int(np.ceil(np.log2(max(2.0, n * n * N / 128.0))))) + 3 + 2)
    return depth * 2.0 ** -24 * abs(float(value))


def spatial_extent(cameras):
    """1.1 x the largest distance of a camera centre from the mean centre (float64)."""
    c = np.stack([np.linalg.inv(np.asarray(cam.world_view_transform, np.float64).reshape(4, 4).T)[:3, 3] for cam in cameras])
    return 1.1 * float(np.linalg.norm(c - c.mean(axis=0, keepdims=True), axis=1).max())


# ---- the golden cases (tests/golden/chart_match.npz, make_golden_chart_match.py) ----------------------------------------
GOLDEN_CASES = ("n1", "n2", "n3", "n4")


def load_case(g, name):
    """One case of the golden file as a namespace: cameras, depths, thr, weights (or None), the reference's results."""
    ref = np.asarray(g[f"{name}_ref_depths"])
    n, H, W = ref.shape
    shape = (n, n, H, W)

    def bits(key):
        return np.unpackbits(g[key])[: n * n * H * W].astype(bool).reshape(shape)

    cams = [SimpleNamespace(world_view_transform=w, projection_matrix=p, full_proj_transform=f, image_width=W, image_height=H)
            for w, p, f in zip(g[f"{name}_wvt"], g[f"{name}_proj"], g[f"{name}_full"])]
    c = SimpleNamespace(name=name, n=n, H=H, W=W, cams=cams, ref_depths=ref, cur_depths=np.asarray(g[f"{name}_cur_depths"]),
                        thr=float(g[f"{name}_thr"]), weights=g[f"{name}_weights"] if f"{name}_weights" in g else None,
                        matches=bits(f"{name}_matches"), cotangent=float(g["cotangent"]))
    for t in (32, 64):
        setattr(c, f"r{t}", SimpleNamespace(match_errors=g[f"{name}_match_errors{t}"], match_fov=bits(f"{name}_match_fov{t}"),
                                            errors=g[f"{name}_errors{t}"], fov=bits(f"{name}_fov{t}"), loss=g[f"{name}_loss{t}"],
                                            grad=g[f"{name}_grad{t}"].reshape(n, H, W),
                                            grad_c037=g[f"{name}_grad{t}_c037"].reshape(n, H, W)))
    return c


# ---- generated scenes for the GPU tests ------------------------------------------------------------------------------------
def generated_scene(n, H, W, seed=0):
    """(cameras, reference depths [n,H,W] float32): n views on an arc looking at the slanted plane 0.3 x + 0.2 y + z = 4 with
    2 % of noise on the depths, zero-depth holes in view 0 and, from four views on, a last view that looks the other way.
    The comparisons that use it are between two float32 evaluations of one contract, so no edge has to be avoided."""
    rng = np.random.default_rng(seed)
    cams = []
    for v in range(n):
        t = 0.0 if n == 1 else v / (n - 1) - 0.5
        yaw, pitch, centre = -0.5 * t, 0.1 * np.sin(3.0 * v), np.array([2.4 * t, 0.3 * np.cos(2.0 * v), 0.2 * np.sin(v)])
        if n >= 4 and v == n - 1:
            yaw, centre = np.pi - 0.2, np.array([0.1, 0.0, -1.0])
        cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        wvt = np.eye(4)
        wvt[:3, :3], wvt[3, :3] = R, -centre @ R
        P = np.zeros((4, 4))
        P[0, 0] = 1.5 + 0.05 * v
        P[1, 1] = P[0, 0] * W / max(H, 4)
        P[2, 0], P[2, 1] = (0.02 * (v % 3 - 1), 0.015 * (v % 2))
        P[2, 2], P[2, 3], P[3, 2] = 100.0 / 99.99, 1.0, -100.0 * 0.01 / 99.99
        wvt32, P32 = wvt.astype(np.float32), P.astype(np.float32)
        cams.append(SimpleNamespace(world_view_transform=wvt32, projection_matrix=P32, image_width=W, image_height=H,
                                    full_proj_transform=(wvt32.astype(np.float64) @ P32.astype(np.float64)).astype(np.float32)))
    rec = camera_records(cams, W, H)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depths = []
    for v in range(n):
        o, D = rec[v, 0:3], rec[v, 3:12].reshape(3, 3)
        dirs = np.stack([D[k, 0] * xx + D[k, 1] * yy + D[k, 2] for k in range(3)], -1)
        normal, c = (np.array([0.12, -0.2, -1.0]), 5.0) if (n >= 4 and v == n - 1) else (np.array([0.3, 0.2, 1.0]), 4.0)
        depths.append(np.abs((c - normal @ o) / (dirs @ normal)) * (1.0 + 0.02 * rng.standard_normal((H, W))))
    depths = np.stack(depths).astype(np.float32)
    depths[0, H // 3: H // 3 + max(1, H // 6), W // 4: W // 4 + max(1, W // 6)] = 0.0
    return cams, depths
