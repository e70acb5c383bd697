"""numpy restatement of the visibility-grid contract (include/g4s_render_maps.h, "Visibility grid").

Every float operation is float32 in the header's order, so grids, maps, counts and points can be compared with the HIP
library exactly.  `dtype=np.float64` evaluates the same expressions in double (only the golden generator's cross-check
uses it).  Slow and simple: for tests only.

A camera is anything with world_view_transform, full_proj_transform, FoVx and FoVy; a view is (camera, depth [H,W]).
"""
import math

import numpy as np

f32 = np.float32
FREE, SURFACE = 0, 1


def _as(a, ft):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, ft)


def focal(cam, W, H, dtype=f32):
    """(fx, fy): W / (2 tan(FoVx / 2)), H / (2 tan(FoVy / 2)) in double, rounded to dtype."""
    return dtype(W / (2.0 * math.tan(float(cam.FoVx) / 2.0))), dtype(H / (2.0 * math.tan(float(cam.FoVy) / 2.0)))


def project(points, cam, W, H, dtype=f32):
    """(z [n], u [n], v [n], in_image [n]) of points [n,3] in a view whose map is W x H."""
    ft = dtype
    p = _as(points, ft).reshape(-1, 3)
    M = _as(cam.world_view_transform, ft).reshape(4, 4)
    fx, fy = focal(cam, W, H, ft)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = [((p[:, 0] * M[0, j] + p[:, 1] * M[1, j]) + p[:, 2] * M[2, j]) + M[3, j] for j in range(3)]
        z = c[2]
        u = (c[0] / z) * fx + ft(W) * ft(0.5)
        v = (c[1] / z) * fy + ft(H) * ft(0.5)
        inside = (u >= 0) & (u < ft(W)) & (v >= 0) & (v < ft(H))
    return z, u, v, inside


def view_pass(points, view, mode=FREE, depth_threshold=0.1, dtype=f32):
    """bool [n]: the predicate of `mode` for every point in one view."""
    ft = dtype
    cam, depth = view
    depth = _as(depth, ft)
    depth = depth.reshape(depth.shape[-2:])
    H, W = depth.shape
    z, u, v, inside = project(points, cam, W, H, ft)
    out = np.zeros(len(z), bool)
    idx = np.nonzero(inside)[0]
    col = np.minimum(u[idx].astype(np.int64), W - 1)
    row = np.minimum(v[idx].astype(np.int64), H - 1)
    d = depth[row, col]
    zi = z[idx]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if mode == FREE:
            ok = (zi > 0) & (zi < d)
        else:
            ok = (zi > 0) & (np.abs(zi - d) / (zi + ft(1e-6)) < ft(depth_threshold))
    out[idx] = ok
    return out


def view_counts(points, views, mode=FREE, depth_threshold=0.1, skip_view=None, dtype=f32):
    """int32 [n]: the number of views, skip_view left out, that pass."""
    n = _as(points, dtype).reshape(-1, 3).shape[0]
    counts = np.zeros(n, np.int32)
    for vi, view in enumerate(views):
        if skip_view is not None and vi == skip_view:
            continue
        counts += view_pass(points, view, mode, depth_threshold, dtype)
    return counts


# ---- the grid ---------------------------------------------------------------------------------------------------------
def grid_frame(bbox_min, bbox_max, R, dtype=f32):
    """(bbox_min, extent, grid_size), each [3]."""
    lo, hi = _as(bbox_min, dtype).reshape(3), _as(bbox_max, dtype).reshape(3)
    extent = hi - lo
    return lo, extent, extent / dtype(R)


def grid_centers(bbox_min, bbox_max, R, dtype=f32):
    """[R^3,3] voxel centres in flat-index order (z fastest)."""
    lo, _e, cell = grid_frame(bbox_min, bbox_max, R, dtype)
    ix, iy, iz = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    axes = [lo[a] + (i.reshape(-1).astype(dtype) + dtype(0.5)) * cell[a] for a, i in enumerate((ix, iy, iz))]
    return np.stack(axes, 1).astype(dtype)


def build(bbox_min, bbox_max, R, views, dtype=f32):
    """bool [R^3]: voxel visible iff some view passes FREE at its centre."""
    c = grid_centers(bbox_min, bbox_max, R, dtype)
    vis = np.zeros(len(c), bool)
    for view in views:
        todo = np.nonzero(~vis)[0]
        vis[todo] = view_pass(c[todo], view, FREE, 0.0, dtype)
    return vis


def pack(bits):
    """uint64 [ceil(n / 64)]: bit (i & 63) of word (i >> 6) = bits[i]; tail bits zero."""
    bits = np.asarray(bits, bool).reshape(-1)
    n_words = (len(bits) + 63) // 64
    padded = np.zeros(n_words * 64, np.uint8)
    padded[: len(bits)] = bits
    return np.packbits(padded.reshape(n_words, 64), axis=1, bitorder="little").view("<u8").reshape(n_words)


def unpack(words, n):
    words = np.ascontiguousarray(np.asarray(words).astype("<u8"))
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def voxel_index(points, bbox_min, bbox_max, R, dtype=f32):
    """int64 [n] flat index of the voxel of each point; ([n,3] per-axis indices come with it)."""
    ft = dtype
    lo, extent, _c = grid_frame(bbox_min, bbox_max, R, ft)
    p = _as(points, ft).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = ((p - lo[None]) / extent[None]) * ft(R)
        g = np.fmin(np.fmax(g, ft(0)), ft(R - 1))
    i = g.astype(np.int64)
    return (i[:, 0] * R + i[:, 1]) * R + i[:, 2], i


def sample(bits, points, bbox_min, bbox_max, R, dtype=f32):
    """bool [n]: visibility of the voxel of each point."""
    return np.asarray(bits, bool).reshape(-1)[voxel_index(points, bbox_min, bbox_max, R, dtype)[0]]


# ---- rays -------------------------------------------------------------------------------------------------------------
def ray_record(cam, W, H, dtype=f32):
    """(o [3], D [3,3]) computed in double, rounded to dtype: dir = D @ (x, y, 1), point = o + t dir."""
    wvt = _as(cam.world_view_transform, np.float64).reshape(4, 4)
    full = _as(cam.full_proj_transform, np.float64).reshape(4, 4)
    c2w = np.linalg.inv(wvt.T)
    ndc2pix = np.array([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], np.float64).T
    intr = ((c2w.T @ full) @ ndc2pix)[:3, :3].T
    D = c2w[:3, :3] @ np.linalg.inv(intr)
    return c2w[:3, 3].astype(dtype), D.astype(dtype)


def ray_dirs(cam, W, H, dtype=f32):
    """[H*W,3] in pixel order i = y W + x."""
    _o, D = ray_record(cam, W, H, dtype)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = x.reshape(-1).astype(dtype), y.reshape(-1).astype(dtype)
    return np.stack([(D[r, 0] * x + D[r, 1] * y) + D[r, 2] for r in range(3)], 1).astype(dtype)


def depths_to_points(depth, cam, dtype=f32):
    """[H*W,3]: o + depth * dir per pixel."""
    depth = _as(depth, dtype)
    H, W = depth.shape[-2:]
    o, _D = ray_record(cam, W, H, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return (o[None] + depth.reshape(-1, 1) * ray_dirs(cam, W, H, dtype)).astype(dtype)


def linspace_t(S, dtype=f32):
    """torch.linspace(0, 1, S): the lower half counts up from 0, the upper half down from 1 with ONE rounding
    (torch's kernel fuses the multiply-subtract).  For float32, step * m is exact in double, so is 1 - that."""
    if S == 1:
        return np.zeros(1, dtype)
    k = np.arange(S)
    step = dtype(1) / dtype(S - 1)
    lo = step * k.astype(dtype)
    if dtype == f32:
        hi = (np.float64(1) - np.float64(step) * (S - 1 - k).astype(np.float64)).astype(f32)
    else:
        hi = dtype(1) - step * (S - 1 - k).astype(dtype)
    return np.where(k < S // 2, lo, hi).astype(dtype)


def n_samples(depth, min_grid_size):
    """The reference's S: int(m / min(grid_size)) + 1, m the largest depth with every invalid pixel counted as 1e-3;
    the division is the host's, in double, of the two float32 values."""
    d = np.asarray(depth, f32)
    m = float(np.where(d <= f32(1e-6), f32(1e-3), d).max())
    return int(m / float(f32(min_grid_size))) + 1


def march(bits, bbox_min, bbox_max, R, depth, cam, S=None, dtype=f32):
    """float32 [H,W], 0 / 1: the ray march of a depth map through the grid."""
    ft = dtype
    depth = _as(depth, ft)
    depth = depth.reshape(depth.shape[-2:])
    H, W = depth.shape
    if S is None:
        S = n_samples(depth, grid_frame(bbox_min, bbox_max, R, f32)[2].min())
    bits = np.asarray(bits, bool).reshape(-1)
    o, _D = ray_record(cam, W, H, ft)
    dirs = ray_dirs(cam, W, H, ft)
    q = depth.reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = ~(q <= ft(1e-6))
    alive = valid.copy()
    t = linspace_t(S, ft)
    for k in range(max(S - 10, 0)):
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            break
        with np.errstate(invalid="ignore", over="ignore"):
            tk = t[k] * q[idx]
            p = o[None] + tk[:, None] * dirs[idx]
        alive[idx] = sample(bits, p, bbox_min, bbox_max, R, ft)
    return alive.astype(f32).reshape(H, W)


def sphere_depth(cam, W, H, radius=1.0, background=0.0):
    """float32 [H,W] test scene: the camera-space depth at which each pixel's ray (of the ray record, in double) first
    meets the sphere of `radius` about the origin; `background` where it misses."""
    o, D = ray_record(cam, W, H, np.float64)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([x.reshape(-1), y.reshape(-1), np.ones(H * W)], 1) @ D.T
    a = (dirs * dirs).sum(1)
    b = 2.0 * (dirs @ o)
    c = float(o @ o) - radius * radius
    disc = b * b - 4.0 * a * c
    t = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a)
    return np.where((disc > 0) & (t > 0), t, background).astype(f32).reshape(H, W)


# ---- the reference's entry points ----------------------------------------------------------------------------------------
def check_valid_camera_center_by_depth(cameras, depths, points, dtype=f32):
    return view_counts(points, list(zip(cameras, depths)), FREE, 0.0, None, dtype) > 0


def get_visible_mask_for_input_views(cameras, depths, points, depth_threshold=0.1, dtype=f32):
    return view_counts(points, list(zip(cameras, depths)), SURFACE, depth_threshold, None, dtype) > 0


def build_visibility_masks(cameras, depths, points=None, depth_threshold=0.1, least_num_views=1, return_origin_masks=False,
                           dtype=f32):
    """List of float32 [1,H,W]: per view the number of OTHER views that pass SURFACE at its points (points[i] [H*W,3], or
    with points=None the back-projection of its own depth map), or whether that number reaches least_num_views."""
    views = list(zip(cameras, depths))
    out = []
    for i, (cam, depth) in enumerate(views):
        depth = _as(depth, dtype)
        H, W = depth.shape[-2:]
        pts = depths_to_points(depth, cam, dtype) if points is None else _as(points[i], dtype).reshape(-1, 3)
        n = view_counts(pts, views, SURFACE, depth_threshold, i, dtype).reshape(1, H, W)
        out.append(n.astype(f32) if return_origin_masks else (n >= least_num_views).astype(f32))
    return out
