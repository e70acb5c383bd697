"""numpy restatement of the unbounded TSDF and dense marching-cubes contract (include/g4s_render_maps.h, "Unbounded TSDF
and dense marching cubes").

Every float operation is float32 in the header's order, so the explicit-point evaluation, the lattice and the mesh can be
compared with the HIP library exactly.  `dtype=np.float64` evaluates the same expressions in double (only the golden
generator's cross-check uses it).  Slow and simple: for tests only.

A view is (M [4,4] full_proj_transform, depth [H,W], rgb [3,H,W] or None).
"""
import numpy as np

import tsdf_ref
from view_tap_ref import bilinear, tap

f32 = np.float32


def point_state(y, contracted, center, radius, voxel_size, dtype=f32):
    """(world points [n,3], truncation T [n]) of points y [n,3] in contracted or world mode."""
    ft = dtype
    y = np.asarray(y, ft).reshape(-1, 3)
    T = np.full(len(y), ft(5) * ft(voxel_size), ft)
    if not contracted:
        return y.copy(), T
    c = np.asarray(center, ft).reshape(3)
    r = ft(radius)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = np.sqrt((y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2])
        s = ft(1) / (ft(2) - m)
        u = np.where((m < 1)[:, None], y, s[:, None] * (y / m[:, None]))
        p = u * r + c[None]
        T = np.where(m > 1, T * (ft(1) / (ft(2) - np.minimum(m, ft(1.9)))), T)
    return p.astype(ft), T.astype(ft)


def sample(points, views, center, radius, voxel_size, contracted, dtype=f32):
    """The per-point evaluation.  Returns (tsdf [n], colour [n,3], margin [n,V], used [n,V]): margin is how far the
    (point, view) pair is from deciding otherwise -- a used pair: the smallest distance of px, py to +-1, of z to 0 and
    of sdf to -T; a pair outside the image: the largest distance among the conditions that failed (all of them would
    have to flip); NaN comparisons count as infinitely far."""
    ft = dtype
    p, T = point_state(points, contracted, center, radius, voxel_size, ft)
    n = len(p)
    tsdf, w, col = np.ones(n, ft), np.ones(n, ft), np.zeros((n, 3), ft)
    margins, used = np.full((n, len(views)), np.inf), np.zeros((n, len(views)), bool)
    for vi, (M, depth, rgb) in enumerate(views):
        M = np.asarray(M, ft).reshape(4, 4)
        depth = np.asarray(depth, ft)
        H, W = depth.shape
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            h = [((p[:, 0] * M[0, c] + p[:, 1] * M[1, c]) + p[:, 2] * M[2, c]) + M[3, c] for c in (0, 1, 3)]
            z = h[2]
            px, py = h[0] / z, h[1] / z
            conds = [px > -1, px < 1, py > -1, py < 1, z > 0]
            dist = [np.abs(px + 1), np.abs(1 - px), np.abs(py + 1), np.abs(1 - py), np.abs(z)]
        dist = [np.where(np.isnan(d), np.inf, d).astype(np.float64) for d in dist]
        inside = conds[0] & conds[1] & conds[2] & conds[3] & conds[4]
        failed = np.max([np.where(c, 0.0, d) for c, d in zip(conds, dist)], 0)
        margin = np.where(inside, np.min(dist, 0), failed)
        idx = np.nonzero(inside)[0]
        ix = ((px[idx] + ft(1)) / ft(2)) * ft(W - 1)
        iy = ((py[idx] + ft(1)) / ft(2)) * ft(H - 1)
        t4 = tap(ix, iy, W, H)
        x0, y0 = t4[0], t4[2]
        assert ((x0 >= 0) & (x0 <= W - 1) & (y0 >= 0) & (y0 <= H - 1)).all()
        d = bilinear(depth, t4)
        sdf = d - z[idx]
        Ti = T[idx]
        with np.errstate(invalid="ignore"):
            keep = sdf > -Ti
            near = np.abs(sdf.astype(np.float64) + Ti.astype(np.float64))
        margin[idx] = np.minimum(margin[idx], np.where(np.isnan(near), np.inf, near))
        margins[:, vi] = margin
        k = idx[keep]
        used[k, vi] = True
        t = np.minimum(ft(1), np.maximum(ft(-1), sdf[keep] / Ti[keep]))
        wk = w[k]
        w1 = wk + ft(1)
        tsdf[k] = (tsdf[k] * wk + t) / w1
        if rgb is not None:
            rgb = np.asarray(rgb, ft)
            for c in range(3):
                sc = bilinear(rgb[c], t4, keep)
                col[k, c] = (col[k, c] * wk + sc) / w1
        w[k] = w1
    return tsdf, col, margins, used


def lattice_axis(N, R):
    """(c [N], h): c(i) = -R + float(i) * h, h = (2 R) / (N - 1), in float32."""
    R = f32(R)
    h = (f32(2) * R) / f32(N - 1)
    return (-R + np.arange(N).astype(f32) * h).astype(f32), h


def lattice_points(N, R):
    """[N^3,3] contracted lattice points in storage order (x fastest)."""
    c, _h = lattice_axis(N, R)
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    return np.stack([c[i.reshape(-1)], c[j.reshape(-1)], c[k.reshape(-1)]], 1)


def lattice(N, R, views, center, radius, voxel_size):
    """tsdf [N^3] of the lattice."""
    return sample(lattice_points(N, R), views, center, radius, voxel_size, True)[0]


def dense_cubes(tsdf, N, R, center, radius, max_range=32.0):
    """Dense marching cubes: (vertices [V,3] f32 world, clamped; triangles [F,3] i32)."""
    F = np.asarray(tsdf, f32).reshape(-1)
    assert F.size == N ** 3
    c, h = lattice_axis(N, R)
    neg = (F < 0).reshape(N, N, N)  # [k, j, i]
    stride = (1, N, N * N)
    own = np.zeros((N, N, N, 3), bool)
    own[:, :, :-1, 0] = neg[:, :, :-1] != neg[:, :, 1:]
    own[:, :-1, :, 1] = neg[:, :-1, :] != neg[:, 1:, :]
    own[:-1, :, :, 2] = neg[:-1, :, :] != neg[1:, :, :]
    flat = own.reshape(-1)
    vid = np.where(flat, np.cumsum(flat) - 1, -1)
    nz = np.nonzero(flat)[0]
    idx, axis = nz // 3, nz % 3
    g = np.stack([idx % N, (idx // N) % N, idx // (N * N)], 1)
    f0, f1 = F[idx], F[idx + np.asarray(stride)[axis]]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = f0 / (f0 - f1)
    y = c[g]
    rows = np.arange(len(nz))
    y[rows, axis] = y[rows, axis] + e * h
    p, _T = point_state(y, True, center, radius, 1.0)
    mr = f32(max_range)
    verts = np.fmin(np.fmax(p, -mr), mr).astype(f32)
    cfg = np.zeros((N - 1, N - 1, N - 1), np.int64)
    for corner in range(8):
        ox, oy, oz = corner & 1, (corner >> 1) & 1, corner >> 2
        cfg |= neg[oz:N - 1 + oz, oy:N - 1 + oy, ox:N - 1 + ox].astype(np.int64) << corner
    tab = tsdf_ref.mc_table()
    owners = [tsdf_ref._edge_owner(k) for k in range(12)]
    tris = []
    for k, j, i in zip(*np.nonzero((cfg != 0) & (cfg != 255))):
        for tri in tab[cfg[k, j, i]]:
            row = []
            for edge in tri:
                (ox, oy, oz), ax = owners[edge]
                row.append(vid[3 * ((i + ox) + N * ((j + oy) + N * (k + oz))) + ax])
            tris.append(row)
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    assert (tris >= 0).all()
    return verts, tris


def closed_manifold(n_vertices, tris):
    """Asserts that the mesh is a closed, consistently oriented surface of genus 0 per component sum: every undirected
    edge lies in exactly two triangles (once each way), no unreferenced vertex; returns V - E + F."""
    use = tsdf_ref.edge_use(tris)
    assert all(n == 1 and use.get((b, a), 0) == 1 for (a, b), n in use.items())
    assert len(np.unique(tris)) == n_vertices
    return n_vertices - len(use) // 2 + len(tris)
