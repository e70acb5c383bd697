"""numpy restatement of the tetrahedral mesh extraction's contract (include/g4s_render_maps.h, "Adaptive TSDF at points
and marching tetrahedra").

Every float operation is float32 in the header's order, so the point TSDF, the marching tetrahedra and the bisection can
be compared with the HIP library exactly.  Slow and simple: for tests only.

A view is (world_view_transform [4,4], projection_matrix [4,4], depth [H,W], rgb [3,H,W] or None).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mtet_table  # noqa: E402
from view_tap_ref import bilinear, tap  # noqa: E402

f32 = np.float32
TET_EDGES = np.asarray(gen_mtet_table.EDGES)  # corner pairs of edge ids 0..5
_TABLE = None


def mtet_table():
    global _TABLE
    if _TABLE is None:
        _TABLE = gen_mtet_table.table()
    return _TABLE


def pixel_coordinates(points, view, znear=1e-6):
    """(ix, iy, z) of points [n,3] in one view, float32 in the contract's order."""
    Wv, Pm, depth = np.asarray(view[0], f32).reshape(4, 4), np.asarray(view[1], f32).reshape(4, 4), view[2]
    H, W = np.asarray(depth).shape
    p = np.asarray(points, f32).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = [((p[:, 0] * Wv[0, c] + p[:, 1] * Wv[1, c]) + p[:, 2] * Wv[2, c]) + Wv[3, c] for c in range(3)]
        q = {c: ((v[0] * Pm[0, c] + v[1] * Pm[1, c]) + v[2] * Pm[2, c]) + Pm[3, c] for c in (0, 1, 3)}
        qw = np.where(q[3] > f32(znear), q[3], f32(znear)).astype(f32)
        ix = ((f32(1) + q[0] / qw) * f32(W)) / f32(2)
        iy = ((f32(1) + q[1] / qw) * f32(H)) / f32(2)
    return ix, iy, v[2]


def adaptive_tsdf(points, views, trunc, znear=1e-6, zfar=1e6):
    """The per-point evaluation.  Returns (tsdf [n], colour [n,3], used [n,V])."""
    p = np.asarray(points, f32).reshape(-1, 3)
    n = len(p)
    T, zn, zf = f32(trunc), f32(znear), f32(zfar)
    tsdf, w, col = np.full(n, -1, f32), np.zeros(n, f32), np.zeros((n, 3), f32)
    used = np.zeros((n, len(views)), bool)
    for vi, view in enumerate(views):
        depth = np.asarray(view[2], f32)
        rgb = view[3]
        H, W = depth.shape
        ix, iy, z = pixel_coordinates(p, view, znear)
        with np.errstate(invalid="ignore"):
            ok = (ix >= 0) & (ix <= f32(W - 1)) & (iy >= 0) & (iy <= f32(H - 1)) & (z > zn) & (z < zf)
        idx = np.nonzero(ok)[0]
        t4 = tap(ix[idx], iy[idx], W, H)
        d = bilinear(depth, t4)
        diff = d - z[idx]
        with np.errstate(invalid="ignore"):
            keep = (d > 0) & (diff >= -T)
        k = idx[keep]
        used[k, vi] = True
        dist = np.fmin(diff[keep] / T, f32(1))
        wk = w[k]
        w1 = wk + f32(1)
        tsdf[k] = (tsdf[k] * wk + dist) / w1
        if rgb is not None:
            rgb = np.asarray(rgb, f32)
            for c in range(3):
                sc = bilinear(rgb[c], t4, keep)
                col[k, c] = np.fmin(np.fmax((col[k, c] * wk + sc) / w1, f32(0)), f32(1))
        w[k] = w1
    return tsdf, col, used


def tet_cases(n_points, tets, sdf):
    """Case [T] of every tet (0 for one that names a point outside [0, n_points))."""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    valid = ((tets >= 0) & (tets < n_points)).all(1)
    with np.errstate(invalid="ignore"):
        occ = np.asarray(sdf, f32).reshape(-1) > 0
    safe = np.where(valid[:, None], tets, 0)
    case = (occ[safe].astype(np.int64) << np.arange(4)).sum(1) if n_points > 0 else np.zeros(len(tets), np.int64)
    return np.where(valid, case, 0)


def marching_tetrahedra(n_points, tets, sdf):
    """(edges [E,2] int32, faces [F,3] int32)."""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    case = tet_cases(n_points, tets, sdf)
    tab = mtet_table()
    keys, tris = [], []  # tris: keys of the three vertices
    for t in np.nonzero((case != 0) & (case != 15))[0]:
        v = tets[t]

        def key(e):
            a, b = v[TET_EDGES[e]]
            return (int(min(a, b)) << 32) | int(max(a, b))
        keys.extend(key(e) for e in gen_mtet_table.crossing_edges(int(case[t])))
        tris.extend([key(e) for e in tri] for tri in tab[case[t]])
    uniq = np.unique(np.asarray(keys, np.uint64))
    edges = np.stack([uniq >> np.uint64(32), uniq & np.uint64(0xFFFFFFFF)], 1).astype(np.int32).reshape(-1, 2)
    faces = np.searchsorted(uniq, np.asarray(tris, np.uint64).reshape(-1, 3)).astype(np.int32).reshape(-1, 3)
    return edges, faces


def bisect(points, edges, sdf, views, trunc, steps=8, znear=1e-6, zfar=1e6):
    """vertices [E,3] float32."""
    p = np.asarray(points, f32).reshape(-1, 3)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    l, r = p[e[:, 0]].copy(), p[e[:, 1]].copy()
    ls = np.asarray(sdf, f32).reshape(-1)[e[:, 0]].copy()
    for _ in range(steps):
        m = (l + r) / f32(2)
        ms = adaptive_tsdf(m, [(a, b, d, None) for a, b, d, _c in views], trunc, znear, zfar)[0]
        low = ((ms < 0) & (ls < 0)) | ((ms > 0) & (ls > 0))
        l = np.where(low[:, None], m, l)
        r = np.where(low[:, None], r, m)
        ls = np.where(low, ms, ls)
    return ((l + r) / f32(2)).astype(f32)


# ---- shapes the tests share ------------------------------------------------------------------------------------------
def kuhn_lattice(n):
    """(points [n^3,3] float32 at integer coordinates, x fastest; tets [6 (n-1)^3, 4] int32): every cube split into the six
    tets along its main diagonal, one per order in which the axes are walked from the lower to the upper corner, all of
    positive orientation (det[v1 - v0, v2 - v0, v3 - v0] > 0)."""
    import itertools
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    points = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], 1).astype(f32)
    m = n - 1
    ck, cj, ci = np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")
    base = (ci + n * (cj + n * ck)).reshape(-1)
    stride = (1, n, n * n)
    tets = []
    for perm in itertools.permutations(range(3)):
        c = [base]
        for a in perm:
            c.append(c[-1] + stride[a])
        if perm in ((0, 2, 1), (1, 0, 2), (2, 1, 0)):  # odd: swap two corners, so every tet has positive orientation
            c[2], c[3] = c[3], c[2]
        tets.append(np.stack(c, 1))
    tets = np.stack(tets, 1).reshape(-1, 4)  # the six tets of a cube are consecutive
    return points, tets.astype(np.int32)


def edge_use(faces):
    """{(i, j): count of directed edge i->j} over the triangles."""
    from collections import Counter
    t = np.asarray(faces, np.int64).reshape(-1, 3)
    return Counter(map(tuple, np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).tolist()))


def sphere_views(W=64, H=48, background=0.0, seed=7):
    """Five analytic views of the unit sphere at the origin: (camera, world_view, projection, depth, rgb) each."""
    import math

    import tsdf_ref
    from g4splat_amd import mesh as mesh_mod
    from g4splat_amd import synthetic
    rng = np.random.default_rng(seed)
    views = []
    for e in [(3.2, 0.3, 0.2), (-0.4, 3.0, 0.5), (-3.0, -0.6, 0.9), (0.5, -0.7, -3.1), (1.9, 1.8, 1.7)]:
        cam = synthetic.look_at_camera(e, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), math.radians(55), W, H)
        intr, E = mesh_mod.camera_intrinsics(cam), mesh_mod.camera_extrinsic(cam)
        depth = tsdf_ref.sphere_depth(E, intr, W, H, (0, 0, 0), 1.0)
        depth[depth <= 0] = background
        rgb = rng.uniform(0, 1, (3, H, W)).astype(f32)
        views.append((cam, np.ascontiguousarray(cam.world_view_transform, f32),
                      np.ascontiguousarray(mesh_mod._projection_matrix(cam), f32), depth.astype(f32), rgb))
    return views
