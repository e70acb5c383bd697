"""numpy restatement of the TSDF fusion and marching-cubes contract (include/g4s_render_maps.h, TSDF section).

Every float operation is float32 in the header's order, so the allocation, the slot order, the voxel values and the
extracted mesh can be compared with the HIP library exactly.  Subnormals are kept (numpy never flushes them): a subnormal
tsdf counts as its sign and divides exactly, which is the header's contract too.  Slow and simple: for tests only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_mc_table  # noqa: E402

f32 = np.float32
BIAS = 1 << 20
COORD_LIMIT = f32(1.0e6)


def pack_keys(b):
    """[N,3] int block coordinates -> [N] int64 packed keys."""
    b = np.asarray(b, np.int64) + BIAS
    return (b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]


def unpack_keys(k):
    k = np.asarray(k, np.int64)
    return np.stack([(k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF], 1) - BIAS


def camera_to_world(E):
    """C = rigid inverse of the 3x4 rows of E (row-major 16 floats), in double, rounded once."""
    E = np.asarray(E, f32).reshape(4, 4)
    C = np.zeros((3, 4), f32)
    for r in range(3):
        for k in range(3):
            C[r, k] = E[k, r]
        t = (float(E[0, r]) * float(E[0, 3]) + float(E[1, r]) * float(E[1, 3])) + float(E[2, r]) * float(E[2, 3])
        C[r, 3] = f32(-t)
    return C


def _affine(M, x, y, z):
    return [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]


def blocks_per_pixel(W, H, intr, voxel_size, sdf_trunc):
    fx, fy, cx, cy = (float(f32(v)) for v in intr)
    rx = max(abs(-cx), abs(W - 1 - cx)) / fx
    ry = max(abs(-cy), abs(H - 1 - cy)) / fy
    length = 2.0 * float(f32(sdf_trunc)) * np.sqrt(1.0 + rx * rx + ry * ry) / (8.0 * float(f32(voxel_size)))
    return 1 + 3 * (int(np.ceil(length * (1.0 + 1e-6))) + 1)


def valid_pixels(depth, mask, depth_trunc):
    d = np.asarray(depth, f32)
    ok = (d > 0) & (d <= f32(depth_trunc))
    if mask is not None:
        ok &= np.asarray(mask, f32) >= f32(0.5)
    return ok


def pixel_walks(depth, mask, intr, E, voxel_size, sdf_trunc, depth_trunc):
    """The DDA of every valid pixel, one row per pixel in raster order:
    pixel [n,2] (u, v); a, b [n,3] float32 segment ends in block units; inside [n] (both ends within COORD_LIMIT: the others
    allocate nothing, length 0); path [n,cap,3] the blocks in walk order, length [n] how many of them count; cut [n] (the
    walk stopped at cap before it reached floor(b)); ties [n] (steps whose smallest t was shared by two or three axes);
    cap (the key slots per pixel)."""
    H, W = depth.shape
    fx, fy, cx, cy = (f32(v) for v in intr)
    T, bs = f32(sdf_trunc), f32(8.0) * f32(voxel_size)
    cap = blocks_per_pixel(W, H, intr, voxel_size, sdf_trunc)
    C = camera_to_world(E)
    vy, vx = np.nonzero(valid_pixels(depth, mask, depth_trunc))
    d = np.asarray(depth, f32)[vy, vx]
    rx, ry = (vx.astype(f32) - cx) / fx, (vy.astype(f32) - cy) / fy
    z0, z1 = d - T, d + T
    a = np.stack(_affine(C, rx * z0, ry * z0, z0), 1) / bs
    b = np.stack(_affine(C, rx * z1, ry * z1, z1), 1) / bs
    ok = np.all((np.abs(a) < COORD_LIMIT) & (np.abs(b) < COORD_LIMIT), 1)
    n = len(d)
    sel = np.nonzero(ok)[0]
    path = np.zeros((n, cap, 3), np.int64)
    length = np.zeros(n, np.int64)
    ties = np.zeros(n, np.int64)
    cut = np.zeros(n, bool)
    a_, b_ = a[sel], b[sel]
    cell, end = np.floor(a_).astype(np.int64), np.floor(b_).astype(np.int64)
    dirv = b_ - a_
    step = np.where(end > cell, 1, -1)
    path[sel, 0] = cell
    length[sel] = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(cap - 1):
            live = np.any(cell != end, 1)
            if not live.any():
                break
            t = ((cell + (step > 0)).astype(f32) - a_) / dirv
            t = np.where(cell != end, t, np.inf)
            best = np.argmin(t, 1)  # first minimum: ties go to the lower axis
            idx = np.nonzero(live)[0]
            ties[sel[idx]] += (t[idx] == t[idx, best[idx]][:, None]).sum(1) > 1
            cell[idx, best[idx]] += step[idx, best[idx]]
            path[sel[idx], length[sel[idx]]] = cell[idx]
            length[sel[idx]] += 1
    cut[sel] = np.any(cell != end, 1)
    return dict(pixel=np.stack([vx, vy], 1), a=a, b=b, inside=ok, path=path, length=length, cut=cut, ties=ties, cap=cap)


def view_blocks(depth, mask, intr, E, voxel_size, sdf_trunc, depth_trunc):
    """Block coordinates the DDA of every valid pixel visits ([N,3], with repeats)."""
    w = pixel_walks(np.asarray(depth), mask, intr, E, voxel_size, sdf_trunc, depth_trunc)
    path, length = w["path"], w["length"]
    steps = [path[length > k, k] for k in range(int(length.max()) if len(length) else 0)]
    return np.concatenate(steps, 0) if steps else np.zeros((0, 3), np.int64)


def quantise(rgb):
    return np.floor(np.fmin(np.fmax(np.asarray(rgb, f32), f32(0)), f32(1)) * f32(255)).astype(f32)


INTEGRATED, BEHIND, OUTSIDE, INVALID, TRUNCATED = range(5)


def voxel_fates(touched, depth, mask, intr, E, voxel_size, sdf_trunc, depth_trunc):
    """What one view does to the voxels of the blocks `touched` (sorted keys), each [m,512] in lane order:
    fate -- INTEGRATED, or why the voxel is left alone: BEHIND (not z > 0), OUTSIDE (the frame), INVALID (its pixel),
    TRUNCATED (not sdf > -sdf_trunc);  z (camera depth of the centre);  u, v (its pixel, -1 if BEHIND or OUTSIDE);
    sdf (NaN unless INTEGRATED or TRUNCATED)."""
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    v_, T = f32(voxel_size), f32(sdf_trunc)
    lane = np.arange(512)
    loc = np.stack([lane & 7, (lane >> 3) & 7, lane >> 6], 1)
    g = (unpack_keys(touched)[:, None, :] * 8 + loc[None]).reshape(-1, 3)
    p = (g.astype(f32) + f32(0.5)) * v_
    E4 = np.asarray(E, f32).reshape(4, 4)
    x, y, z = _affine(E4, p[:, 0], p[:, 1], p[:, 2])
    fx, fy, cx, cy = (f32(q) for q in intr)
    with np.errstate(divide="ignore", invalid="ignore"):
        fu = np.floor((fx * x) / z + cx + f32(0.5))
        fv = np.floor((fy * y) / z + cy + f32(0.5))
    front = z > 0
    ok = front & (fu >= 0) & (fu <= W - 1) & (fv >= 0) & (fv <= H - 1)
    fate = np.where(front, OUTSIDE, BEHIND)
    U, V = np.full(len(z), -1, np.int64), np.full(len(z), -1, np.int64)
    S = np.full(len(z), np.nan, f32)
    idx = np.nonzero(ok)[0]
    u, v = fu[idx].astype(np.int64), fv[idx].astype(np.int64)
    U[idx], V[idx] = u, v
    good = valid_pixels(depth, mask, depth_trunc)[v, u]
    fate[idx[~good]] = INVALID
    idx, u, v = idx[good], u[good], v[good]
    d = depth[v, u]
    a, b = (fu[idx] - cx) / fx, (fv[idx] - cy) / fy
    sdf = (d - z[idx]) * np.sqrt((f32(1) + a * a) + b * b)
    S[idx] = sdf
    fate[idx] = np.where(sdf > -T, INTEGRATED, TRUNCATED)
    m = len(touched)
    return dict(fate=fate.reshape(m, 512), z=z.reshape(m, 512), u=U.reshape(m, 512), v=V.reshape(m, 512), sdf=S.reshape(m, 512))


class RefVolume:
    def __init__(self, voxel_size, sdf_trunc, depth_trunc):
        self.v, self.T, self.depth_trunc = f32(voxel_size), f32(sdf_trunc), f32(depth_trunc)
        self.keys = np.zeros(0, np.int64)   # sorted
        self.slots = np.zeros(0, np.int32)  # table order
        self.tsdf = np.zeros((0, 512), f32)
        self.weight = np.zeros((0, 512), f32)
        self.color = np.zeros((0, 512, 3), f32)
        self.last_touched = np.zeros(0, np.int64)  # sorted keys of the blocks the latest view touched

    def integrate(self, depth, rgb, intr, E, mask=None):
        """Fuse one view; returns (touched blocks, new blocks) like TSDFVolume.integrate.  last_touched: their keys."""
        depth = np.asarray(depth, f32)
        blocks = view_blocks(depth, mask, intr, E, self.v, self.T, self.depth_trunc)
        touched = np.unique(pack_keys(blocks)) if len(blocks) else np.zeros(0, np.int64)
        new = np.setdiff1d(touched, self.keys)
        n = len(self.keys)
        new_slots = np.arange(n, n + len(new), dtype=np.int32)
        keys = np.concatenate([self.keys, new])
        slots = np.concatenate([self.slots, new_slots])
        order = np.argsort(keys, kind="stable")
        self.keys, self.slots = keys[order], slots[order]
        self.tsdf = np.concatenate([self.tsdf, np.zeros((len(new), 512), f32)])
        self.weight = np.concatenate([self.weight, np.zeros((len(new), 512), f32)])
        self.color = np.concatenate([self.color, np.zeros((len(new), 512, 3), f32)])
        self.last_touched = touched
        if len(touched) == 0:
            return 0, 0
        tslot = self.slots[np.searchsorted(self.keys, touched)]
        f = voxel_fates(touched, depth, mask, intr, E, self.v, self.T, self.depth_trunc)
        idx = np.nonzero(f["fate"].reshape(-1) == INTEGRATED)[0]
        u, v, sdf = f["u"].reshape(-1)[idx], f["v"].reshape(-1)[idx], f["sdf"].reshape(-1)[idx]
        t = np.fmin(f32(1), sdf / self.T)
        s, l = np.repeat(tslot, 512)[idx], idx % 512
        w = self.weight[s, l]
        w1 = w + f32(1)
        self.tsdf[s, l] = (self.tsdf[s, l] * w + t) / w1
        q = quantise(np.asarray(rgb, f32)[:, v, u]).T
        self.color[s, l] = (self.color[s, l] * w[:, None] + q) / w1[:, None]
        self.weight[s, l] = w1
        return len(touched), len(new)

    def voxels(self):
        """(tsdf, weight, colour) in table order: [n,512], [n,512], [n,512,3]."""
        return self.tsdf[self.slots], self.weight[self.slots], self.color[self.slots]

    def extract(self):
        return extract_mesh(self.keys, *self.voxels(), self.v)


_TABLE = None


def mc_table():
    global _TABLE
    if _TABLE is None:
        _TABLE = gen_mc_table.table()
    return _TABLE


def _edge_owner(e):
    """(offset of the owning voxel from the cube's lower corner, axis) of cube edge e."""
    axis, n = divmod(e, 4)
    o = [0, 0, 0]
    others = [ax for ax in range(3) if ax != axis]
    o[others[0]], o[others[1]] = n & 1, n >> 1
    return tuple(o), axis


def _compress(bc):
    """Block coordinates [n,3] -> small non-negative ones with the same 27-neighbourhoods: per axis consecutive values stay
    consecutive and every larger step becomes 2 (one empty block in between), so blocks that do not touch still do not
    touch and a dense array over the result stays small wherever the keys lie."""
    out = np.empty_like(bc)
    for a in range(3):
        u, inv = np.unique(bc[:, a], return_inverse=True)
        out[:, a] = np.concatenate([[0], np.cumsum(np.where(np.diff(u) == 1, 1, 2))]).astype(np.int64)[inv.reshape(-1)]
    return out


class _Lattice:
    """The voxels of blocks `keys` (sorted) on a dense array over compressed block coordinates, one voxel of padding:
    F (tsdf, NaN where not allocated or weight 0), cv / cfg (validity and configuration of the cube at each lower
    corner), cross / owned ([..., 3]: sign change between two valid voxels on the +axis edge / one that a valid cube
    uses), g ([n,512,3] true voxel coordinates in output order) and gi ([3, n*512] their indices into the arrays)."""

    def __init__(self, keys, tsdf, weight):
        bc = unpack_keys(keys)
        lane = np.arange(512)
        loc = np.stack([lane & 7, (lane >> 3) & 7, lane >> 6], 1)
        self.g = bc[:, None, :] * 8 + loc[None]  # [n,512,3] in output order
        gc = (_compress(bc)[:, None, :] * 8 + loc[None]).reshape(-1, 3)
        self.lo = lo = gc.min(0) - 1
        self.dims = dims = gc.max(0) - lo + 2
        self.F = F = np.full(dims, np.nan, f32)
        self.gi = gi = (gc - lo).T
        F[tuple(gi)] = np.where(np.asarray(weight).reshape(-1) > 0, np.asarray(tsdf, f32).reshape(-1), np.nan)
        valid = ~np.isnan(F)
        neg = F < 0
        X, Y, Z = dims
        # cube at lower corner (x, y, z): all corners valid; configuration bits
        self.cv = cv = np.zeros(dims, bool)
        self.cfg = cfg = np.zeros(dims, np.int64)
        sl = lambda c: (slice(c[0], X - 1 + c[0]), slice(c[1], Y - 1 + c[1]), slice(c[2], Z - 1 + c[2]))
        inner = (slice(0, X - 1), slice(0, Y - 1), slice(0, Z - 1))
        cv[inner] = True
        for c in range(8):
            off = (c & 1, (c >> 1) & 1, c >> 2)
            cv[inner] &= valid[sl(off)]
            cfg[inner] |= neg[sl(off)].astype(np.int64) << c
        # edges owned by each voxel: crossing between two valid voxels used by a valid cube
        self.cross = np.zeros(tuple(dims) + (3,), bool)
        self.owned = np.zeros(tuple(dims) + (3,), bool)
        cvp = np.pad(cv, 1)  # index +1
        for a in range(3):
            e = [0, 0, 0]
            e[a] = 1
            f0 = F
            f1 = np.full(dims, np.nan, f32)
            f1[:X - e[0], :Y - e[1], :Z - e[2]] = F[e[0]:, e[1]:, e[2]:]
            cross = ~np.isnan(f0) & ~np.isnan(f1) & ((f0 < 0) != (f1 < 0))
            others = [ax for ax in range(3) if ax != a]
            used = np.zeros(dims, bool)
            for o in range(4):
                d = [0, 0, 0]
                d[others[0]], d[others[1]] = -(o & 1), -(o >> 1)
                used |= cvp[1 + d[0]:1 + d[0] + X, 1 + d[1]:1 + d[1] + Y, 1 + d[2]:1 + d[2] + Z]
            self.cross[..., a] = cross
            self.owned[..., a] = cross & used


def cube_cases(keys, tsdf, weight):
    """Per cube, by lower-corner voxel in output order ([n,512] each): valid (all eight corners valid), cfg (the
    configuration; meaningful where valid) and mixed (among the valid corners some are negative and some are not: the
    cube has a sign change whether or not it is valid)."""
    L = _Lattice(keys, tsdf, weight)
    n = len(keys)
    X, Y, Z = L.dims
    Fp = np.pad(L.F, ((0, 1), (0, 1), (0, 1)), constant_values=np.nan)
    some_neg, some_pos = np.zeros(L.dims, bool), np.zeros(L.dims, bool)
    for c in range(8):
        f = Fp[(c & 1):(c & 1) + X, ((c >> 1) & 1):((c >> 1) & 1) + Y, (c >> 2):(c >> 2) + Z]
        some_neg |= f < 0
        some_pos |= f >= 0
    pick = lambda a: a[tuple(L.gi)].reshape(n, 512)
    return pick(L.cv), pick(L.cfg), pick(some_neg & some_pos)


def unused_crossings(keys, tsdf, weight):
    """Number of edges with a sign change between two valid voxels that no valid cube uses (they carry no vertex)."""
    L = _Lattice(keys, tsdf, weight)
    return int((L.cross & ~L.owned)[tuple(L.gi)].sum())


def extract_mesh(keys, tsdf, weight, color, voxel_size):
    """Marching cubes over blocks `keys` (sorted) with voxel arrays in the same order.
    Returns (vertices [V,3] f32, colours [V,3] f32, triangles [F,3] i32)."""
    v = f32(voxel_size)
    if len(keys) == 0:
        return np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros((0, 3), np.int32)
    L = _Lattice(keys, tsdf, weight)
    g, gi, dims, F = L.g, L.gi, L.dims, L.F
    Cg = np.zeros(tuple(dims) + (3,), f32)
    Cg[tuple(gi)] = np.asarray(color, f32).reshape(-1, 3)
    # vertex ids in output order: blocks, voxels x fastest, edges +x +y +z
    own_seq = L.owned[tuple(gi)]  # [n*512, 3]
    flat = own_seq.reshape(-1)
    vid = np.full(tuple(dims) + (3,), -1, np.int64)
    ids = np.cumsum(flat) - 1
    vid_seq = np.where(flat, ids, -1).reshape(-1, 3)
    vid[tuple(gi)] = vid_seq
    nz = np.nonzero(flat)[0]
    vox, axis = nz // 3, nz % 3
    gv = g.reshape(-1, 3)[vox]
    p0 = gi.T[vox]
    p1 = p0 + np.eye(3, dtype=np.int64)[axis]
    f0, f1 = F[tuple(p0.T)], F[tuple(p1.T)]
    e = f0 / (f0 - f1)
    cen = gv.astype(f32) + f32(0.5)
    pos = cen.copy()
    pos[np.arange(len(nz)), axis] = cen[np.arange(len(nz)), axis] + e
    verts = (pos * v).astype(f32)
    c0, c1 = Cg[tuple(p0.T)], Cg[tuple(p1.T)]
    cols = ((c0 + e[:, None] * (c1 - c0)) / f32(255)).astype(f32)
    # triangles: cubes in output order (configurations 0 and 255 have none)
    tab = mc_table()
    cube_ok = L.cv[tuple(gi)]
    cube_cfg = L.cfg[tuple(gi)]
    owners = [_edge_owner(k) for k in range(12)]
    tris = []
    for i in np.nonzero(cube_ok & (cube_cfg != 0) & (cube_cfg != 255))[0]:
        for tri in tab[cube_cfg[i]]:
            row = []
            for k in tri:
                o, ax = owners[k]
                q = gi[:, i] + np.array(o)
                row.append(vid[q[0], q[1], q[2], ax])
            tris.append(row)
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    assert (tris >= 0).all()
    return verts, cols, tris


def edge_use(tris):
    """{(i, j): count of directed edge i->j} over the triangles."""
    from collections import Counter
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    return Counter(map(tuple, np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).tolist()))


def sphere_depth(cam_E, intr, W, H, center, radius):
    """Analytic z-depth of a sphere seen by a camera (0 where the ray misses)."""
    E = np.asarray(cam_E, np.float64).reshape(4, 4)
    fx, fy, cx, cy = intr
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, dtype=np.float64)], -1)
    c = E[:3, :3] @ np.asarray(center, np.float64) + E[:3, 3]
    # |z dir - c|^2 = r^2 -> z^2 |dir|^2 - 2 z dir.c + |c|^2 - r^2 = 0
    A = (dirs ** 2).sum(-1)
    B = -2 * (dirs @ c)
    Cq = c @ c - radius ** 2
    disc = B * B - 4 * A * Cq
    z = np.where(disc >= 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), 0.0)
    return z.astype(f32)
