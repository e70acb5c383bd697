"""Numpy restatement of the "Chart surfels" section of include/g4s_render_maps.h: the triangulated pixel grid, the keep test,
the surfel of a kept face, pytorch3d's matrix_to_quaternion, and the voxel pick of indices.

Every function takes `dtype`: np.float32 restates the contract operation for operation (each numpy operation on float32
arrays rounds once, nothing is contracted), np.float64 evaluates the same formulas in double (the constants stay the float32
values of the contract).  Nothing here is shared with the code under test."""
import numpy as np

f32, f64 = np.float32, np.float64

BARY_BITS = (0x3EAAAAAB, 0x3EAAAAAB, 0x3EAAAAAA)
AXIS0_BITS = (0xBF3504F3, 0x3F3504F3, 0x00000000)
AXIS1_BITS = (0xBED105EC, 0xBED105EC, 0x3F5105EC)


def _from_bits(bits, dtype):
    return np.array(bits, np.uint32).view(f32).astype(dtype)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _len(a):
    return np.sqrt(_dot(a, a))


def _floor_eps(x):
    """x if x > 1e-12 else 1e-12 (also for a NaN)."""
    eps = x.dtype.type(f32(1e-12))
    return np.where(x > eps, x, eps)


# ---- faces ----------------------------------------------------------------------------------------------------------------
def face_pixels(V, H, W):
    """int64 [F,3]: the flat vertex index (v H W + r W + c) of every face's A, B, C in the contract's order."""
    if H < 2 or W < 2 or V == 0:
        return np.zeros((0, 3), np.int64)
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)[:-1, :-1].reshape(-1)
    one = np.stack([idx, idx + W, idx + 1], axis=1)
    two = np.stack([idx + W + 1, idx + 1, idx + W], axis=1)
    view = np.concatenate([one, two])
    return np.concatenate([view + v * H * W for v in range(V)])


def keep_lengths(A, B, C):
    """[F,3]: the three lengths l_i of the keep test, in the dtype of the vertices."""
    with np.errstate(all="ignore"):
        s = [C - A, A - B, B - C]
        n = [si / _floor_eps(_len(si))[..., None] for si in s]
        out = []
        for i in range(3):
            t = _dot(s[i], n[(i + 1) % 3])
            out.append(_len(s[i] - t[..., None] * n[i]))
    return np.stack(out, axis=-1)


def keep_ratio(A, B, C):
    """max(l) / min(l); NaN where a length is a NaN."""
    l = keep_lengths(A, B, C)
    with np.errstate(all="ignore"):
        return l.max(axis=-1) / l.min(axis=-1)  # numpy's max and min propagate a NaN


def keep_mask(points, masks, ratio_th, dtype):
    """(keep bool [F], ratio [F], faces [F,3]) of points [V,H,W,3]; masks [V,H,W] or None."""
    p = np.asarray(points)
    V, H, W = p.shape[:3]
    faces = face_pixels(V, H, W)
    flat = p.reshape(-1, 3).astype(dtype)
    ratio = keep_ratio(flat[faces[:, 0]], flat[faces[:, 1]], flat[faces[:, 2]])
    with np.errstate(invalid="ignore"):
        keep = ratio < dtype(f32(ratio_th))
    if masks is not None and np.asarray(masks).astype(bool).any():
        m = np.asarray(masks).astype(bool).reshape(-1)
        keep = keep & m[faces].any(axis=1)
    return keep, ratio, faces


# ---- the surfel -----------------------------------------------------------------------------------------------------------
def matrix_to_quaternion(R):
    """[n,4] (w, x, y, z) of R [n,3,3], the contract's table; in the dtype of R."""
    dt = R.dtype.type
    one = dt(1)
    m = lambda i, j: R[:, i, j]
    with np.errstate(all="ignore"):
        t = np.stack([((one + m(0, 0)) + m(1, 1)) + m(2, 2), ((one + m(0, 0)) - m(1, 1)) - m(2, 2),
                      ((one - m(0, 0)) + m(1, 1)) - m(2, 2), ((one - m(0, 0)) - m(1, 1)) + m(2, 2)], axis=1)
        q_abs = np.where(t > 0, np.sqrt(np.where(t > 0, t, one)), dt(0))
        rows = np.stack([
            np.stack([q_abs[:, 0] * q_abs[:, 0], m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], axis=1),
            np.stack([m(2, 1) - m(1, 2), q_abs[:, 1] * q_abs[:, 1], m(1, 0) + m(0, 1), m(0, 2) + m(2, 0)], axis=1),
            np.stack([m(0, 2) - m(2, 0), m(1, 0) + m(0, 1), q_abs[:, 2] * q_abs[:, 2], m(1, 2) + m(2, 1)], axis=1),
            np.stack([m(1, 0) - m(0, 1), m(2, 0) + m(0, 2), m(2, 1) + m(1, 2), q_abs[:, 3] * q_abs[:, 3]], axis=1)], axis=1)
        k = np.argmax(q_abs, axis=1)  # the first index of the largest
        n = np.arange(len(R))
        best = q_abs[n, k]
        floor = dt(f32(0.1))
        q = rows[n, k] / (dt(2) * np.where(best > floor, best, floor))[:, None]
        return np.where((q[:, 0] < 0)[:, None], -q, q)


def quaternion_to_matrix(q):
    """[n,3,3] float64 of (w, x, y, z) float: the rotation both q and -q name (pytorch3d's formula)."""
    q = np.asarray(q, f64)
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two_s = 2.0 / (q * q).sum(axis=1)
    return np.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], axis=1).reshape(-1, 3, 3)


def surfels_of_faces(A, B, C, ca, cb, cc, normalized_scales, normal_scale):
    """The surfels of the faces (A, B, C) [F,3] with vertex colours ca, cb, cc [F,3] (not yet clamped); every array already
    in the working dtype.  Returns means, scales, quaternions, colors and the rotation matrices."""
    dt = A.dtype.type
    b, e0, e1 = _from_bits(BARY_BITS, dt), _from_bits(AXIS0_BITS, dt), _from_bits(AXIS1_BITS, dt)
    ns = dt(f32(normalized_scales))

    def clamp(x):
        return np.where(x < 0, dt(0), np.where(x > 1, dt(1), x))

    with np.errstate(all="ignore"):
        means = (b[0] * A + b[1] * B) + b[2] * C
        colors = (b[0] * clamp(ca) + b[1] * clamp(cb)) + b[2] * clamp(cc)
        t0 = (e0[0] * A + e0[1] * B) + e0[2] * C
        t1 = (e1[0] * A + e1[1] * B) + e1[2] * C
        first0 = (_len(t0) >= _len(t1))[:, None]
        u, w = np.where(first0, t0, t1), np.where(first0, t1, t0)
        w2 = w - (_dot(w, u)[:, None] * u) / _dot(u, u)[:, None]
        o = [np.where(first0, u, w2), np.where(first0, w2, u)]
        scales = np.stack([_len(o[0] * ns), _len(o[1] * ns), np.full(len(A), dt(f32(normal_scale)))], axis=1)
        x = [oj / _floor_eps(_len(oj))[:, None] for oj in o]
        n = np.stack([x[0][:, 1] * x[1][:, 2] - x[0][:, 2] * x[1][:, 1], x[0][:, 2] * x[1][:, 0] - x[0][:, 0] * x[1][:, 2],
                      x[0][:, 0] * x[1][:, 1] - x[0][:, 1] * x[1][:, 0]], axis=1)
        R = np.stack([x[0], x[1], n], axis=2)  # columns
        quats = matrix_to_quaternion(R)
    return {"means": means, "scales": scales, "quaternions": quats, "colors": colors, "rotations": R}


def pointmap_surfels(points, images, masks=None, ratio_th=5.0, normalized_scales=0.5, normal_scale=1e-10, dtype=f32):
    """The whole stage on points, images [V,H,W,3], masks [V,H,W] or None: the surfels of the kept faces in order, plus
    "keep" [F], "ratio" [F] and "faces" [F,3] of all faces."""
    keep, ratio, faces = keep_mask(points, masks, ratio_th, dtype)
    flat = np.asarray(points).reshape(-1, 3).astype(dtype)
    cols = np.asarray(images).reshape(-1, 3).astype(dtype)
    k = faces[keep]
    out = surfels_of_faces(flat[k[:, 0]], flat[k[:, 1]], flat[k[:, 2]], cols[k[:, 0]], cols[k[:, 1]], cols[k[:, 2]],
                           normalized_scales, normal_scale)
    out.update(keep=keep, ratio=ratio, faces=faces)
    return out


def depth_points(depth, ray):
    """float32 [H,W,3]: the back-projection of the Visibility section (dir = D (x, y, 1), point = o + d dir), float32."""
    d = np.asarray(depth, f32)
    H, W = d.shape
    r = np.asarray(ray, f32)
    o, D = r[:3], r[3:].reshape(3, 3)
    x, y = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    return np.stack([o[c] + d * ((D[c, 0] * x + D[c, 1] * y) + D[c, 2]) for c in range(3)], axis=-1)


# ---- the voxel pick -------------------------------------------------------------------------------------------------------
def voxel_pick_indices(points, voxel_size):
    """int64 [n_voxels]: per voxel, in ascending (cz, cy, cx), the contract's rounded mean index."""
    from mesh_eval_ref import voxel_cells
    p = np.ascontiguousarray(points, f32).reshape(-1, 3)
    n = len(p)
    c = voxel_cells(p, voxel_size)
    order = np.lexsort((np.arange(n), c[:, 0], c[:, 1], c[:, 2]))
    cs = c[order]
    heads = np.concatenate([[0], np.nonzero((cs[1:] != cs[:-1]).any(axis=1))[0] + 1, [n]])
    out = np.empty(len(heads) - 1, np.int64)
    total = f64(n)
    for v in range(len(heads) - 1):
        s = f64(0)
        for i in order[heads[v]:heads[v + 1]]:
            s = s + f64(i) / total
        out[v] = np.int64(np.rint((s / f64(heads[v + 1] - heads[v])) * total))
    return out


def select_init_views(n_input, n_extra):
    """The trainer's two index lists, restated: 50 input views by linspace when there are more, and the extra views 0-9,
    15-24, 30.. when there are more than 30."""
    ids = list(range(n_input)) if n_input <= 50 else [int(x) for x in np.linspace(0, n_input - 1, 50, dtype=int)]
    extra = list(range(n_extra)) if n_extra <= 30 else list(range(10)) + list(range(15, 25)) + list(range(30, n_extra))
    return ids, extra


def check_against_golden(g, got, factor):
    """`got`: means, scales, quaternions, colors of the kept faces in order, and the keep mask of all faces."""
    near, ref_keep = g["near"], g["ref64_keep"]
    assert near.sum() <= 0.01 * len(near)
    assert np.array_equal(np.asarray(got["keep"])[~near], ref_keep[~near])
    both = np.asarray(got["keep"]) & ref_keep
    mine, theirs = (np.cumsum(got["keep"]) - 1)[both], (np.cumsum(ref_keep) - 1)[both]
    assert both.sum() >= 100
    for key in ("means", "scales", "colors"):
        err = np.abs(np.asarray(got[key], f64)[mine] - g["ref64_" + key][theirs]).max()
        print(f"{key}: largest error {err:.3e}, bound {factor * g['yard'][key]:.3e}")
        assert err <= factor * g["yard"][key], key
    R = quaternion_to_matrix(np.asarray(got["quaternions"])[mine])
    for name, want in (("rotation of the quaternion", quaternion_to_matrix(g["ref64_quaternions"][theirs])),
                       ("the reference's rotation", g["ref64_rotations"][theirs])):
        err = np.abs(R - want).max()
        print(f"{name}: largest error {err:.3e}, bound {factor * g['yard']['rotations']:.3e}")
        assert err <= factor * g["yard"]["rotations"], name
    q = np.asarray(got["quaternions"])
    assert (q[:, 0] >= 0).all()


def pair_cloud(n_pairs=40, seed=5):
    """Two points per voxel of edge 0.1, the pairs' indices i and a partner of the other parity: every index sum is odd, so
    every mean index ends in .5 -- the half-way case."""
    rng = np.random.default_rng(seed)
    centres = (np.stack(np.meshgrid(np.arange(4), np.arange(5), np.arange(2), indexing="ij"), -1).reshape(-1, 3)[:n_pairs] + 0.5) * 0.1
    order = rng.permutation(n_pairs)
    evens, odds = np.arange(0, 2 * n_pairs, 2), np.arange(1, 2 * n_pairs, 2)
    pts = np.zeros((2 * n_pairs, 3))
    pts[evens] = centres[order] + rng.uniform(-0.01, 0.01, (n_pairs, 3))
    pts[odds] = centres[rng.permutation(order)] + rng.uniform(-0.01, 0.01, (n_pairs, 3))
    return pts.astype(f32)


def random_cloud(n=1000, seed=8):
    """About three points per voxel of edge 0.1."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 0.1 * round((n / 3) ** (1 / 3)), (n, 3)).astype(f32)
