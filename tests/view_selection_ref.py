"""numpy restatement of the view-selection contract (include/g4s_render_maps.h, "View selection").

Every float operation is float32 in the header's order, so words, counts, indices and distances can be compared with the
HIP library exactly.  `dtype=np.float64` evaluates the same expressions in double (only the golden generator's cross-check
uses it).  Slow and simple: for tests only.

A camera is anything with world_view_transform, FoVx, FoVy, image_width and image_height.
"""
import math
from types import SimpleNamespace

import numpy as np

import visibility_ref as vr

f32 = np.float32
FAR = 1e10


def camera(wvt, fovx, fovy, width, height):
    return SimpleNamespace(world_view_transform=np.asarray(wvt, np.float32).reshape(4, 4), FoVx=float(fovx), FoVy=float(fovy),
                           image_width=int(width), image_height=int(height))


def spiral_cameras(n=70, mixed=True):
    """n look-at cameras on a spiral about the origin (the "seventy" stack of test_gpu_visibility.py), 32 x 24, and with
    `mixed` every third one 64 x 48 and every seventh 40 x 40."""
    from g4splat_amd import synthetic
    cams = []
    for i in range(n):
        a, z = 2.0 * math.pi * i / 17.0, -1.5 + 3.0 * i / max(n - 1, 1)
        W, H = ((64, 48) if i % 3 == 1 else (40, 40) if i % 7 == 3 else (32, 24)) if mixed else (32, 24)
        cams.append(synthetic.look_at_camera((3.0 * math.cos(a), 3.0 * math.sin(a), z), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0),
                                             math.radians(55.0), W, H))
    return cams


# ---- A. visible bits and the covisibility table ------------------------------------------------------------------------
def visible_mask(points, cam, dtype=f32):
    """bool [P]: in image && z > 0."""
    z, _u, _v, inside = vr.project(points, cam, int(cam.image_width), int(cam.image_height), dtype)
    with np.errstate(invalid="ignore"):
        return inside & (z > 0)


def visible_masks(points, cams, dtype=f32):
    P = np.asarray(points).reshape(-1, 3).shape[0]
    return np.stack([visible_mask(points, c, dtype) for c in cams]) if P else np.zeros((len(cams), 0), bool)


def words(masks):
    """uint64 [C, ceil(P / 64)]: bit (p & 63) of words[c][p >> 6]; tail bits zero."""
    masks = np.asarray(masks, bool)
    return np.stack([vr.pack(m) for m in masks]).reshape(len(masks), (masks.shape[1] + 63) // 64)


def counts(masks):
    """int64 [C,C]: the number of points both cameras see."""
    m = np.asarray(masks, bool).astype(np.int64)
    return m @ m.T


def popcount_counts(w):
    """The same table from the words."""
    w = np.ascontiguousarray(np.asarray(w).astype("<u8"))
    C = w.shape[0]
    out = np.zeros((C, C), np.int64)
    for i in range(C):
        both = np.ascontiguousarray(w[i][None, :] & w)
        out[i] = np.unpackbits(both.view(np.uint8).reshape(C, -1), axis=1).sum(1)
    return out


def bit_counts(w, chunk_words=None):
    """The same table as the integer matrix product of the unpacked bits, in float64 (every sum is an integer far below
    2^53, so it is exact), a slice of the words at a time: seconds where popcount_counts takes C passes over C rows."""
    w = np.ascontiguousarray(np.asarray(w).astype("<u8"))
    C, W = w.shape
    step = int(chunk_words) if chunk_words else max(1, (1 << 18) // max(C, 1))  # at most 2^24 doubles of bits at a time
    out = np.zeros((C, C), np.float64)
    for w0 in range(0, W, step):
        part = np.ascontiguousarray(w[:, w0:w0 + step])
        bits = np.unpackbits(part.view(np.uint8).reshape(C, -1), axis=1).astype(np.float64)
        out += bits @ bits.T
    return out.astype(np.int64)


def random_words(C, n_words, seed):
    """uint64 [C, n_words] for the count kernel alone: the AND of two random draws (a quarter of the bits set), with row 1
    all ones, row 2 all zero and the last row non-zero in its last word only (rows that exist)."""
    rng = np.random.default_rng(seed)
    top = np.iinfo(np.uint64).max
    w = rng.integers(0, top, (C, n_words), np.uint64, endpoint=True) & rng.integers(0, top, (C, n_words), np.uint64, endpoint=True)
    if C > 1:
        w[1] = top
    if C > 2:
        w[2] = 0
    if C > 3:
        w[C - 1, :-1] = 0
        w[C - 1, -1] |= np.uint64(1) << np.uint64(63)
    return w


def ratio_of(table):
    """ratio(i, j) over a counts table, in Python numbers."""
    t = np.asarray(table).tolist()

    def ratio(i, j):
        c, a, b = t[i][j], t[i][i], t[j][j]
        return max(c / a if a > 0 else 0, c / b if b > 0 else 0)
    return ratio


# ---- B. farthest-point sampling ----------------------------------------------------------------------------------------------
def fps(cloud, k, first, dtype=f32):
    """(indices int32 [k], dist [N]) of one cloud [N,3]."""
    p = np.asarray(cloud, dtype).reshape(-1, 3)
    dist = np.full(len(p), FAR, dtype)
    idx = np.zeros(k, np.int32)
    idx[0] = first
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(1, k):
            q = p[idx[i - 1]]
            dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
            d = (dx * dx + dy * dy) + dz * dz
            dist = np.fmin(dist, d)
            idx[i] = int(np.nonzero(dist == dist.max())[0][0])  # the smallest index of the largest distance
    return idx, dist


def fps_batch(clouds, k, first, dtype=f32):
    """(indices [M,k], samples [M,k,3], dist [M,N])."""
    clouds = np.asarray(clouds, dtype)
    out = [fps(c, k, f, dtype) for c, f in zip(clouds, first)]
    idx = np.stack([o[0] for o in out])
    return idx, np.stack([c[i] for c, i in zip(clouds, idx)]), np.stack([o[1] for o in out])


def nearest_train_indices(train_centres, novel_centres, dtype=f32):
    """int64 [K]: the training centre at the smallest squared distance, d = train - novel, smallest index among equals."""
    t, c = np.asarray(train_centres, dtype), np.asarray(novel_centres, dtype)
    dx, dy, dz = (t[None, :, a] - c[:, None, a] for a in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    return np.array([int(np.nonzero(row == row.min())[0][0]) for row in d], np.int64)


def lookat_points(train_centres, clouds, novel_centres, fps_num, first, random_ids, dtype=f32):
    _idx, samples, _d = fps_batch(clouds, fps_num, first, dtype)
    return samples[nearest_train_indices(train_centres, novel_centres, dtype), np.asarray(random_ids, np.int64)]


def lattice(n=4):
    """[n^3,3] integer lattice: many equal distances."""
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
