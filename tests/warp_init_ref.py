"""numpy restatement of the warp-surfel contract (include/g4s_render_maps.h, "Warp surfels"), operation for operation.

Every float operation is float32 in the header's order and numpy fuses nothing, so keep masks and rows can be compared with
the HIP library bit for bit (a NaN's payload aside).  dtype=np.float64 evaluates the same expressions in double: the golden
generator's cross-check.  Slow and simple: for tests only.  The projection and the back-projection are visibility_ref's:
there is no second one here either.

Also the scene family the golden and the GPU tests share: a height field with a nearer patch, ray-cast in float64 from
nearby poses, with depth noise and a block of zero depths.
"""
import math
from types import SimpleNamespace

import numpy as np

import visibility_ref as vr

f32, f64 = np.float32, np.float64
EPS = 1e-12


# ---- the contract's small functions: every min, max and clamp of this section propagates a NaN ---------------------------
def _at_least(t, lo):
    return np.where(t < lo, lo, t).astype(t.dtype)


def _dist(a, b):
    d = a - b
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _normalize(a):
    n = a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]
    for k in range(2, a.shape[-1]):
        n = n + a[..., k] * a[..., k]
    return a / _at_least(np.sqrt(n), a.dtype.type(EPS))[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _depth(depth, ft):
    depth = vr._as(depth, ft)
    return depth.reshape(depth.shape[-2:])


def point_map(depth, cam, dtype=f32):
    """[H,W,3]: the back-projection of every pixel, whatever its depth."""
    depth = _depth(depth, dtype)
    return vr.depths_to_points(depth, cam, dtype).reshape(depth.shape + (3,))


def scale_map(P, g=-1):
    """[H,W]: s of the contract for every pixel."""
    ft = P.dtype.type
    H, W = P.shape[:2]
    if W == 1 or H == 1:
        s = np.full((H, W), ft(1e-3), P.dtype)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            dh, dv = _dist(P[:, 1:], P[:, :-1]), _dist(P[1:], P[:-1])
        r, l = np.concatenate([dh, dh[:, -1:]], 1), np.concatenate([dh[:, :1], dh], 1)
        d, u = np.concatenate([dv, dv[-1:]], 0), np.concatenate([dv[:1], dv], 0)
        s = np.minimum(np.minimum(np.minimum(r, l), d), u)  # np.minimum propagates a NaN
    with np.errstate(invalid="ignore", over="ignore"):
        s = s * ft(0.5)
        return s * ft(g) if g > 0 else s


def normal_map(P):
    """[H,W,3]: the normal of the contract for every pixel (the interior normal at the clamped pixel)."""
    H, W = P.shape[:2]
    n = np.zeros_like(P)
    if H < 3 or W < 3:
        n[..., 2] = 1
        return n
    sy, sx = np.clip(np.arange(H), 1, H - 2)[:, None], np.clip(np.arange(W), 1, W - 2)[None, :]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _normalize(_cross(P[sy + 1, sx] - P[sy - 1, sx], P[sy, sx + 1] - P[sy, sx - 1]))


def quaternions(n):
    """[n,4] (w, x, y, z): the contract's quaternion of every normal [n,3]."""
    ft = n.dtype.type
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = _normalize(n)
        ref = np.zeros_like(z)
        par = np.abs(z[:, 0]) > ft(0.9)
        ref[par, 1] = 1
        ref[~par, 0] = 1
        x = _normalize(_cross(ref, z))
        y = _cross(z, x)
        m = np.stack([x, y, z], axis=-1)  # columns
        one, two, zero, eps = ft(1), ft(2), ft(0), ft(EPS)
        m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
        q = [np.sqrt(_at_least(((one + m00) + m11) + m22, zero)) / two, np.sqrt(_at_least(((one + m00) - m11) - m22, zero)) / two,
             np.sqrt(_at_least(((one - m00) + m11) - m22, zero)) / two, np.sqrt(_at_least(((one - m00) - m11) + m22, zero)) / two]
        q[1] = q[1] * np.sign((m[:, 2, 1] - m[:, 1, 2]) + eps)
        q[2] = q[2] * np.sign((m[:, 0, 2] - m[:, 2, 0]) + eps)
        q[3] = q[3] * np.sign((m[:, 1, 0] - m[:, 0, 1]) + eps)
        return _normalize(np.stack(q, axis=-1))


def quaternion_to_matrix(q):
    """[n,3,3] in float64: the rotation of each (w, x, y, z), normalised here."""
    q = np.asarray(q, f64)
    w, x, y, z = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def coverage(points, cam, depth, depth_error_thresh, dtype=f32):
    """Points [n,3] against one earlier view: (covered [n], u, v, z, relative depth error where in the image, else NaN)."""
    ft = dtype
    depth = _depth(depth, ft)
    H, W = depth.shape
    z, u, v, _inside = vr.project(points, cam, W, H, ft)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inside = (u >= 0) & (u <= ft(W - 1)) & (v >= 0) & (v <= ft(H - 1)) & (z > 0)
        idx = np.nonzero(inside)[0]
        d = depth[np.rint(v[idx]).astype(np.int64), np.rint(u[idx]).astype(np.int64)]  # rint: round half to even
        rel = np.full(len(z), np.nan, ft)
        rel[idx] = np.abs(z[idx] - d) / (z[idx] + ft(1e-6))
        covered = np.zeros(len(z), bool)
        covered[idx] = (d > 0) & (rel[idx] < ft(depth_error_thresh))
    return covered, u, v, z, rel


def warp_surfels(depths, cams, images, depth_error_thresh=0.01, min_scale=0.0005, max_scale=0.05, g=-1, dtype=f32):
    """The whole contract.  keep, covered, scales, normals: per view [H,W] / [H,W,3] maps; means, scale_rows, quaternions,
    colors: the rows; pairs[(i, j)] = coverage(...) of view i's points in view j."""
    ft = dtype
    step = g if g > 0 else 1
    out = SimpleNamespace(keep=[], covered=[], scales=[], normals=[], points=[], pairs={})
    rows = {k: [] for k in ("means", "scale_rows", "quaternions", "colors")}
    for i, (depth, cam) in enumerate(zip(depths, cams)):
        depth = _depth(depth, ft)
        H, W = depth.shape
        P = point_map(depth, cam, ft)
        lattice = np.zeros((H, W), bool)
        lattice[::step, ::step] = True
        candidate = lattice & (depth > 0)
        covered = np.zeros(H * W, bool)
        for j in range(i):
            out.pairs[(i, j)] = coverage(P.reshape(-1, 3), cams[j], depths[j], depth_error_thresh, ft)
            covered |= out.pairs[(i, j)][0]
        covered = covered.reshape(H, W) & candidate
        s = scale_map(P, g)
        with np.errstate(invalid="ignore"):
            keep = candidate & ~covered & (s < ft(max_scale))
        n = normal_map(P)
        out.keep.append(keep), out.covered.append(covered), out.scales.append(s), out.normals.append(n), out.points.append(P)
        rows["means"].append(P[keep])
        rows["scale_rows"].append(np.repeat(_at_least(s[keep], ft(min_scale))[:, None], 2, axis=1))
        rows["quaternions"].append(quaternions(n[keep]))
        rows["colors"].append(vr._as(images[i], ft)[:, keep].T)
    for k, v in rows.items():
        setattr(out, k, np.concatenate(v, axis=0).astype(ft) if v else np.zeros((0, 3), ft))
    return out


# ---- the scene family ------------------------------------------------------------------------------------------------------
def camera(W, H, pose, fovx_deg=60.0):
    """A pinhole camera of W x H at (tx, ty, tz) turned by `yaw` about the y axis, with the reference's matrices."""
    from g4splat_amd.synthetic import make_camera
    tx, ty, tz, yaw = pose
    c, s = math.cos(yaw), math.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], f64)  # camera to world
    fovx = math.radians(fovx_deg)
    fovy = 2.0 * math.atan(math.tan(fovx / 2) * H / W)
    cam = make_camera(R, -R.T @ np.array([tx, ty, tz], f64), fovx, fovy, W, H)
    return SimpleNamespace(**cam._asdict())


def surface(x, y):
    """The scene's depth along +z at (x, y): a height field and a nearer patch."""
    z = 2.1 + 0.3 * np.sin(2.6 * x) * np.cos(2.2 * y)
    return np.where((np.abs(x - 0.25) < 0.22) & (np.abs(y) < 0.25), 1.3, z)


def ray_cast(cam, W, H):
    """float64 [H,W]: the camera-z depth at which each pixel's ray first meets the surface (a march and a bisection)."""
    o, D = vr.ray_record(cam, W, H, f64)
    y, x = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    dirs = np.stack([(D[r, 0] * x + D[r, 1] * y) + D[r, 2] for r in range(3)], -1)
    below = lambda t: (o[2] + t * dirs[..., 2]) - surface(o[0] + t * dirs[..., 0], o[1] + t * dirs[..., 1]) >= 0
    ts = np.linspace(0.5, 4.0, 701)
    lo, hi = np.full((H, W), ts[0]), np.full((H, W), ts[-1])
    found = np.zeros((H, W), bool)
    for a, b in zip(ts[:-1], ts[1:]):
        hit = below(b) & ~found
        lo[hit], hi[hit] = a, b
        found |= hit
    assert found.all()
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        inside = below(mid)
        hi, lo = np.where(inside, mid, hi), np.where(inside, lo, mid)
    return hi


POSES = ((0.0, 0.0, 0.0, 0.0), (0.18, 0.03, 0.05, -0.06), (-0.15, 0.05, -0.03, 0.05), (0.05, -0.12, 0.1, 0.02))


def scene(sizes, poses=POSES, seed=7, noise=0.012, hole=(3, 4)):
    """(cameras, float32 depths [H,W], float32 images [3,H,W]) of views of (W, H) = sizes[v] at poses[v]: the ray-cast depth
    with +-noise uniform relative noise and a zero-depth block [:hole[0], :hole[1]]; images are uniform in [-0.2, 1.2]."""
    rng = np.random.default_rng(seed)
    cams, depths, images = [], [], []
    for (W, H), pose in zip(sizes, poses):
        cam = camera(W, H, pose)
        d = ray_cast(cam, W, H) * (1.0 + rng.uniform(-noise, noise, (H, W)))
        d[: hole[0], : hole[1]] = 0.0
        cams.append(cam), depths.append(d.astype(f32)), images.append(rng.uniform(-0.2, 1.2, (3, H, W)).astype(f32))
    return cams, depths, images


def jittered_poses(n, seed=11, spread=0.15, yaw=0.05):
    rng = np.random.default_rng(seed)
    return [tuple(rng.uniform(-spread, spread, 3)) + (float(rng.uniform(-yaw, yaw)),) for _ in range(n)]


# ---- the golden ---------------------------------------------------------------------------------------------------------------
GOLDEN_SIZES = ((24, 18), (20, 20), (24, 18), (17, 23))
RECORDINGS = {"A": dict(g=-1, min_scale=0.035, max_scale=0.05), "B": dict(g=3, min_scale=0.035, max_scale=0.16)}
DEPTH_ERROR_THRESH = 0.01


def load_golden():
    """tests/golden/warp_init.npz as a namespace: cams, depths, images, and per recording the reference's float64 results."""
    import json
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp_init.npz"))
    V = len(g["wvt"])
    sizes = [tuple(int(n) for n in s) for s in g["sizes"]]
    cams = [SimpleNamespace(world_view_transform=g["wvt"][v], full_proj_transform=g["full"][v], FoVx=float(g["fov"][v][0]),
                            FoVy=float(g["fov"][v][1]), image_width=sizes[v][0], image_height=sizes[v][1]) for v in range(V)]
    split = lambda flat, comps=1: [flat[o * comps:(o + H * W) * comps].reshape((H, W) if comps == 1 else (comps, H, W))
                                   for (W, H), o in zip(sizes, np.cumsum([0] + [w * h for w, h in sizes[:-1]]))]
    rec = {}
    for name in RECORDINGS:
        rec[name] = SimpleNamespace(keep=split(g[name + "_keep"]), near=split(g[name + "_near"]),
                                    **{k: g[f"{name}_{k}"] for k in ("means", "scales", "quaternions", "colors")},
                                    yard=json.loads(str(g[name + "_yardstick"])), **RECORDINGS[name])
    return SimpleNamespace(g=g, sizes=sizes, cams=cams, depths=split(g["depths"]), images=split(g["images"], 3), rec=rec,
                           thresh=float(g["depth_error_thresh"]))


def check_against_golden(r, keep, means, scales, quats, colors, factor=2.0):
    """Keep masks (per view [H,W]) and rows of a run against recording r: the masks equal away from the near pixels, the
    rows of the pixels both keep within factor x the yardstick, rotations as matrices."""
    got_rows, ref_rows, ok = [], [], True
    g0 = r0 = 0
    for v, (k, rk, near) in enumerate(zip(keep, r.keep, r.near)):
        k = np.asarray(k, bool)
        assert k.shape == rk.shape, (v, k.shape, rk.shape)
        differ = (k != rk) & ~near
        assert not differ.any(), (v, "keep masks differ away from the thresholds at", np.argwhere(differ)[:5].tolist())
        both = (k & rk).reshape(-1)
        got_rows.append(g0 + (np.cumsum(k.reshape(-1)) - 1)[both])
        ref_rows.append(r0 + (np.cumsum(rk.reshape(-1)) - 1)[both])
        g0, r0 = g0 + int(k.sum()), r0 + int(rk.sum())
    assert len(means) == g0 and len(r.means) == r0, (len(means), g0, len(r.means), r0)  # row order: view, then row-major
    gi, ri = np.concatenate(got_rows), np.concatenate(ref_rows)
    assert len(gi) > 0
    for name, got, ref in (("means", means, r.means), ("scales", scales, r.scales), ("colors", colors, r.colors)):
        err = np.abs(np.asarray(got)[gi].astype(f64) - ref[ri]).max()
        print(f"{name}: largest error {err:.3e}, bound {factor * r.yard[name]:.3e}")
        ok &= bool(err <= factor * r.yard[name])
    err = np.abs(quaternion_to_matrix(np.asarray(quats)[gi]) - quaternion_to_matrix(r.quaternions[ri])).max()
    print(f"rotations: largest error {err:.3e}, bound {factor * r.yard['rotations']:.3e}")
    assert ok and err <= factor * r.yard["rotations"]
