"""numpy restatement of the mesh rasteriser's contract (include/g4s_render_maps.h, "Mesh rasteriser and dilated depth").

Every float operation is float32 in the header's order and every coverage decision is made in int64, so the rasteriser,
the resolve and the dilation can be compared with the HIP library exactly.  Slow and simple: for tests only.
"""
from types import SimpleNamespace

import numpy as np

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
OK, SKIP, BEHIND, GUARD_BAND = 0, 1, 2, 3
INF = f32(np.inf)


def project(p, Wv, Pm, W, H, off, znear):
    """(sx, sy, z, usable) of positions p [...,3]; Wv None: the positions are in view space."""
    p = np.asarray(p, f32)
    Pm = np.asarray(Pm, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        if Wv is None:
            v = [p[..., 0], p[..., 1], p[..., 2]]
        else:
            Wv = np.asarray(Wv, f32).reshape(4, 4)
            v = [((p[..., 0] * Wv[0, c] + p[..., 1] * Wv[1, c]) + p[..., 2] * Wv[2, c]) + Wv[3, c] for c in range(3)]
        q = {c: ((v[0] * Pm[0, c] + v[1] * Pm[1, c]) + v[2] * Pm[2, c]) + Pm[3, c] for c in (0, 1, 3)}
        z = v[2]
        sx = ((f32(1) + q[0] / q[3]) * f32(W)) / f32(2) - f32(off)
        sy = ((f32(1) + q[1] / q[3]) * f32(H)) / f32(2) - f32(off)
        usable = (z > f32(znear)) & (z < INF) & (np.abs(sx) < INF) & (np.abs(sy) < INF)
    return sx, sy, z, usable


def setup(P3, exists, Wv, Pm, W, H, off, znear):
    """The faces P3 [F,3,3] (positions; `exists` [F] False for a face that names no valid vertices) as the sampler reads
    them: status [F] and, where it is OK, X, Y [F,3] int64, sx, sy, z [F,3], s [F], the clamped boxes x0, x1, y0, y1."""
    P3 = np.asarray(P3, f32).reshape(-1, 3, 3)
    F = len(P3)
    sx, sy, z, usable = project(P3, Wv, Pm, W, H, off, znear)
    status = np.full(F, OK, np.int64)
    with np.errstate(invalid="ignore"):
        guard = ((np.abs(sx) > f32(32768)) | (np.abs(sy) > f32(32768))).any(1)
    status[guard] = GUARD_BAND
    status[~usable.all(1)] = BEHIND
    status[~np.asarray(exists, bool)] = SKIP
    ok = status == OK
    X, Y = np.zeros((F, 3), np.int64), np.zeros((F, 3), np.int64)
    X[ok] = np.rint(sx[ok] * f32(256)).astype(np.int64)
    Y[ok] = np.rint(sy[ok] * f32(256)).astype(np.int64)
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    status[ok & (area == 0)] = SKIP
    x0 = np.maximum((X.min(1) + 255) >> 8, 0)
    x1 = np.minimum(X.max(1) >> 8, W - 1)
    y0 = np.maximum((Y.min(1) + 255) >> 8, 0)
    y1 = np.minimum(Y.max(1) >> 8, H - 1)
    return SimpleNamespace(status=status, X=X, Y=Y, sx=sx, sy=sy, z=z, s=np.sign(area), x0=x0, x1=x1, y0=y0, y1=y1, W=W, H=H)


def sample(fc, f, ii, jj):
    """Face f at the samples (ii, jj) = (rows, columns), int64 arrays: (covered, zpix, w [3])."""
    X, Y, sx, sy, z, s = fc.X[f], fc.Y[f], fc.sx[f], fc.sy[f], fc.z[f], int(fc.s[f])
    PX, PY = jj.astype(np.int64) * 256, ii.astype(np.int64) * 256
    px, py, sf = jj.astype(f32), ii.astype(f32), f32(s)
    inside = np.ones(ii.shape, bool)
    E, b = [], []
    with np.errstate(all="ignore"):
        for k in range(3):
            a, e = (k + 1) % 3, (k + 2) % 3
            dx, dy = s * int(X[e] - X[a]), s * int(Y[e] - Y[a])
            Ek = dx * (PY - int(Y[a])) - dy * (PX - int(X[a]))
            owns = dy < 0 or (dy == 0 and dx > 0)
            inside &= (Ek > 0) | ((Ek == 0) & owns)
            t = sf * ((sx[e] - sx[a]) * (py - sy[a]) - (sy[e] - sy[a]) * (px - sx[a]))
            E.append(Ek)
            b.append(np.where(t > 0, t, f32(0)).astype(f32))
        total = (b[0] + b[1]) + b[2]
        zero = total == 0
        if zero.any():
            b = [np.where(zero, Ek.astype(f32), bk).astype(f32) for Ek, bk in zip(E, b)]
            total = (b[0] + b[1]) + b[2]
        r = [(b[k] / total) / z[k] for k in range(3)]
        t = (r[0] + r[1]) + r[2]
        zpix = f32(1) / t
        w = [r[k] / t for k in range(3)]
    return inside, zpix.astype(f32), [x.astype(f32) for x in w]


def zbuffer(fc):
    """keys [H,W] uint64 = the smallest float_bits(zpix) << 32 | face per pixel, all-ones where nothing covers."""
    keys = np.full((fc.H, fc.W), EMPTY, np.uint64)
    for f in np.nonzero(fc.status == OK)[0]:
        x0, x1, y0, y1 = int(fc.x0[f]), int(fc.x1[f]), int(fc.y0[f]), int(fc.y1[f])
        if x0 > x1 or y0 > y1:
            continue
        ii, jj = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        inside, zpix, _w = sample(fc, f, ii, jj)
        key = (zpix.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        box = keys[y0:y1 + 1, x0:x1 + 1]
        keys[y0:y1 + 1, x0:x1 + 1] = np.where(inside & (key < box), key, box)
    return keys


def winners(fc, keys):
    """(pix_to_face int32, zbuf, bary [H,W,3]) of a key buffer."""
    won = keys != EMPTY
    face = np.where(won, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    zbuf = np.where(won, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)
    bary = np.zeros(keys.shape + (3,), f32)
    for f in np.unique(face[won]):
        ii, jj = np.nonzero(face == f)
        _in, _z, w = sample(fc, int(f), ii, jj)
        for k in range(3):
            bary[ii, jj, k] = w[k]
    return face.astype(np.int32), zbuf, bary


def face_positions(vertices, faces):
    """(P3 [F,3,3], exists [F]) of a mesh: a face that names an index outside [0, V) does not exist and reads nothing."""
    vertices = np.asarray(vertices, f32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    exists = ((faces >= 0) & (faces < len(vertices))).all(1)
    P3 = np.zeros((len(faces), 3, 3), f32)
    P3[exists] = vertices[faces[exists]]
    return P3, exists


def face_normals(P3, Wv, centre, flip, surfels):
    """The resolve's normal of every face, [F,3]."""
    Wv = np.asarray(Wv, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        u, v = P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0]
        g = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                      u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        positive = length > 0
        g = g / length[:, None]
        if flip:
            c = np.asarray(centre, f32)
            d = c[None, :] - ((P3[:, 0] + P3[:, 1]) + P3[:, 2]) / f32(3)
            back = ((d[:, 0] * g[:, 0] + d[:, 1] * g[:, 1]) + d[:, 2] * g[:, 2]) < 0
            g = np.where(back[:, None], -g, g)
        n = np.stack([(g[:, 0] * Wv[0, c] + g[:, 1] * Wv[1, c]) + g[:, 2] * Wv[2, c] for c in range(3)], 1)
        if surfels:
            n[:, :2] = -n[:, :2]
    return np.where(positive[:, None], n, f32(0)).astype(f32)


def render(vertices, faces, Wv, Pm, W, H, off=0.5, znear=1e-6, attributes=None, background=None, centre=None, flip=True,
           surfels=True, seen=None):
    """The whole of g4s_mesh_raster: a namespace of pix_to_face, zbuf, bary, attr, normal, seen, stats."""
    P3, exists = face_positions(vertices, faces)
    fc = setup(P3, exists, Wv, Pm, W, H, off, znear)
    stats = np.array([(fc.status == BEHIND).sum(), (fc.status == GUARD_BAND).sum()], np.int32)
    pix, zbuf, bary = winners(fc, zbuffer(fc))
    won = pix >= 0
    out = SimpleNamespace(pix_to_face=pix, zbuf=zbuf, bary=bary, stats=stats, attr=None, normal=None, fc=fc)
    idx = np.asarray(faces, np.int64).reshape(-1, 3)[np.where(won, pix, 0)] if len(P3) else np.zeros((H, W, 3), np.int64)
    if attributes is not None:
        a = np.asarray(attributes, f32)
        attr = np.empty((H, W, a.shape[1]), f32)
        attr[:] = np.asarray(background, f32)
        a0, a1, a2 = (a[idx[won][:, k]] for k in range(3))
        w = bary[won]
        attr[won] = (w[:, 0:1] * a0 + w[:, 1:2] * a1) + w[:, 2:3] * a2
        out.attr = attr
    if centre is not None or not flip:
        normal = np.zeros((H, W, 3), f32)
        if len(P3):
            normal[won] = face_normals(P3, Wv, centre, flip, surfels)[pix[won]]
        out.normal = normal
    out.seen = np.zeros(len(P3), np.uint8) if seen is None else np.array(seen, np.uint8)
    out.seen[np.unique(pix[won])] = 1
    return out


# ---- dilated depth ---------------------------------------------------------------------------------------------------
def grid_faces(W, H):
    """The vertex indices [2 (H-1)(W-1), 3] of the pointmap grid: first-kind faces, then second-kind."""
    a = np.arange(H * W).reshape(H, W)[:-1, :-1].reshape(-1)
    return np.concatenate([np.stack([a, a + W, a + 1], 1), np.stack([a + W + 1, a + 1, a + W], 1)]).astype(np.int64)


def dilated_vertices(depth, Pm, dilation_pixels, max_dilation):
    """p' [H,W,3]: the view-space vertices moved along their normals, NaN for an invalid depth."""
    d = np.asarray(depth, f32)
    Pm = np.asarray(Pm, f32).reshape(4, 4)
    H, W = d.shape
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        nx = (f32(2) * jj.astype(f32)) / f32(W) - f32(1)
        ny = (f32(2) * ii.astype(f32)) / f32(H) - f32(1)
        p = np.stack([((nx - Pm[2, 0]) * d) / Pm[0, 0], ((ny - Pm[2, 1]) * d) / Pm[1, 1], d], -1).astype(f32)
        valid = (d > 0) & (d < INF)
        n = np.zeros((H, W, 3), f32)
        if H > 1 and W > 1:
            corner = {(0, 0): p[:-1, :-1], (1, 0): p[1:, :-1], (0, 1): p[:-1, 1:], (1, 1): p[1:, 1:]}
            good = valid[:-1, :-1] & valid[1:, :-1] & valid[:-1, 1:]
            good = [good, valid[1:, 1:] & valid[:-1, 1:] & valid[1:, :-1]]
            tri = [((0, 0), (1, 0), (0, 1)), ((1, 1), (0, 1), (1, 0))]  # (a, b, c) of the two kinds, as cell corners
            cross = []
            for a, b, c in tri:
                u, v = corner[b] - corner[a], corner[c] - corner[a]
                cross.append(np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                                       u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1))
            # vertex (i, j) meets, in ascending face index, the first kind of the cells (i-1,j), (i,j-1), (i,j) and the
            # second kind of the cells (i-1,j-1), (i-1,j), (i,j-1); cell (ci, cj) = (i + di, j + dj)
            for kind, di, dj in [(0, -1, 0), (0, 0, -1), (0, 0, 0), (1, -1, -1), (1, -1, 0), (1, 0, -1)]:
                rows, cols = slice(-di, -di + H - 1), slice(-dj, -dj + W - 1)
                n[rows, cols] = np.where(good[kind][..., None], n[rows, cols] + cross[kind], n[rows, cols])
        length = np.fmax(np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]), f32(1e-6))
        focal = ((Pm[0, 0] * f32(W)) / f32(2) + (Pm[1, 1] * f32(H)) / f32(2)) / f32(2)
        delta = np.fmin((f32(dilation_pixels) / focal) * d, f32(max_dilation))
        moved = p + delta[..., None] * (n / length[..., None])
    return np.where(valid[..., None], moved, f32(np.nan)).astype(f32)


def dilated_faces(depth, Pm, dilation_pixels, max_dilation, znear=1e-6):
    """The faces of the dilated grid as the sampler reads them (setup): statuses, snapped coordinates, clamped boxes."""
    d = np.asarray(depth, f32)
    H, W = d.shape
    verts = dilated_vertices(d, Pm, dilation_pixels, max_dilation).reshape(-1, 3)
    faces = grid_faces(W, H)
    return setup(verts[faces], np.ones(len(faces), bool), None, Pm, W, H, 0.0, znear)


def box_samples(fc):
    """Samples in every face's clamped box, 0 for a face that is not drawn."""
    n = (fc.x1 - fc.x0 + 1).clip(0) * (fc.y1 - fc.y0 + 1).clip(0)
    return np.where(fc.status == OK, n, 0)


def dilate(depth, Pm, dilation_pixels=1.5, max_dilation=1e8, rgb=None, znear=1e-6):
    """One view of g4s_depth_dilate: (depth_out [H,W], rgb_out [3,H,W] or None, pix_to_face)."""
    d = np.asarray(depth, f32)
    H, W = d.shape
    faces = grid_faces(W, H)
    fc = dilated_faces(d, Pm, dilation_pixels, max_dilation, znear)
    pix, zbuf, bary = winners(fc, zbuffer(fc))
    won = pix >= 0
    out_d = np.where(won, zbuf, d).astype(f32)
    out_c = None
    if rgb is not None:
        rgb = np.asarray(rgb, f32)
        out_c = rgb.copy()
        idx = faces[pix[won]]
        w = bary[won]
        for c in range(3):
            a = np.fmin(np.fmax(rgb[c].reshape(-1), f32(0)), f32(1))
            out_c[c][won] = (w[:, 0] * a[idx[:, 0]] + w[:, 1] * a[idx[:, 1]]) + w[:, 2] * a[idx[:, 2]]
    return out_d, out_c, pix


# ---- inputs that the CPU and the GPU tests share -----------------------------------------------------------------------
def pinhole(W, H, fx, fy):
    """(Wv, Pm) of a camera at the origin looking down +z: Pm[0][0] = 2 fx / W, Pm[1][1] = 2 fy / H, q_3 = z."""
    Pm = np.zeros((4, 4), f32)
    Pm[0, 0], Pm[1, 1], Pm[2, 2], Pm[2, 3], Pm[3, 2] = 2.0 * fx / W, 2.0 * fy / H, 1.0, 1.0, -0.01
    return np.eye(4, dtype=f32), Pm


def soup(seed, n_faces, spread, W=67, H=45, f=60.0):
    """(vertices [3 n,3], faces [n,3]) of random triangles of about +-spread units at depth 2..6 in front of pinhole(W, H, f, f)."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-2, 2, n_faces), rng.uniform(-1.4, 1.4, n_faces), rng.uniform(2, 6, n_faces)], 1)
    v = (c[:, None, :] + rng.uniform(-spread, spread, (n_faces, 3, 3))).astype(f32).reshape(-1, 3)
    return v, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def step_map(W, H, at, vertical, near=1.0, far=3.0):
    """A depth step from `near` to `far` at column (vertical) or row `at`, with a ripple so that no two normals are equal."""
    d = np.full((H, W), far, f32)
    if vertical:
        d[:, :at] = near
    else:
        d[:at, :] = near
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (d + 0.05 * np.sin(jj / 3.0) + 0.04 * np.cos(ii / 4.0)).astype(f32)
