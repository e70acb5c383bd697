"""numpy restatement of include/g4s_render_maps.h, "Plane masks", and of the host rules of g4splat_amd/plane_masks.py: the
fixed-order float64 sums, Lloyd's k-means with float32 distances, the cluster pick and merge, the 9x9 opening, the
8-connected components and the join with the masks in the reference's loop order.  Written for clarity, not speed: the tests
use small images."""
import numpy as np

SPAN = 4096  # G4S_KMEANS_SPAN
ITEMS = SPAN // 256


# ---- the fixed-order sum ------------------------------------------------------------------------------------------------
def _tree(w):
    """w [..., 64, T] -> lane 0 of the shuffle tree: lane l += lane l + off for off = 32, 16, ... 1."""
    w = w.copy()
    off = 32
    while off >= 1:
        w[..., :off, :] = w[..., :off, :] + w[..., off:2 * off, :]
        off //= 2
    return w[..., 0, :]


def span_partials(values):
    """values float64 [n, T], 0 where a pixel takes no part -> the workgroups' partials [ceil(n / SPAN), T]."""
    n, T = values.shape
    B = max((n + SPAN - 1) // SPAN, 1)
    v = np.zeros((B * SPAN, T), np.float64)
    v[:n] = values
    v = v.reshape(B, ITEMS, 256, T)
    acc = np.zeros((B, 256, T), np.float64)
    for k in range(ITEMS):  # thread t adds pixels t, t + 256, ... in ascending order
        acc = acc + v[:, k]
    w = _tree(acc.reshape(B, 4, 64, T))  # [B, 4, T]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def fold_partials(partials):
    """[B, T] -> [T]: lane l adds partials l, l + 64, ... in ascending order, then the tree."""
    B, T = partials.shape
    R = (B + 63) // 64
    p = np.zeros((R * 64, T), np.float64)
    p[:B] = partials
    p = p.reshape(R, 64, T)
    acc = np.zeros((64, T), np.float64)
    for r in range(R):
        acc = acc + p[r]
    return _tree(acc)


def fixed_sum(values):
    return fold_partials(span_partials(values))


# ---- A. k-means ---------------------------------------------------------------------------------------------------------
def valid_pixels(X):
    return ~np.isnan(X).any(axis=1)


def distances(X, C):
    """float32 [n, K]: ((dx dx + dy dy) + dz dz), every operation rounded on its own."""
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    dx = X[:, None, 0] - C[None, :, 0]
    dy = X[:, None, 1] - C[None, :, 1]
    dz = X[:, None, 2] - C[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def assign(X, C, valid):
    with np.errstate(invalid="ignore"):
        d = distances(X, C)
    labels = np.argmin(np.where(valid[:, None], d, 0), axis=1).astype(np.int8)  # the first smallest
    labels[~valid] = -1
    return labels


def cluster_sums(X, labels, K):
    """[K, 4] float64 in the fixed order: count, sum x, sum y, sum z."""
    n = X.shape[0]
    vals = np.zeros((n, 4 * K), np.float64)
    Xd = X.astype(np.float64)
    for k in range(K):
        m = labels == k
        vals[m, 4 * k] = 1.0
        vals[m, 4 * k + 1:4 * k + 4] = Xd[m]
    return fixed_sum(vals).reshape(K, 4)


def tolerance(X, valid, tol):
    Xd = np.where(valid[:, None], X.astype(np.float64), 0.0)
    s = fixed_sum(np.concatenate([valid[:, None].astype(np.float64), Xd, Xd * Xd], axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = s[0]
        var = [(s[4 + c] - s[1 + c] * s[1 + c] / n) / n for c in range(3)]
        return tol * (((var[0] + var[1]) + var[2]) / 3.0)


def kmeans_normals(normals, init, max_iter=300, tol=1e-4):
    """(labels int8 [H,W], centres float32 [K,3], counts int32 [K], n_iter)."""
    normals = np.asarray(normals, np.float32)
    H, W = normals.shape[:2]
    X = normals.reshape(-1, 3)
    C = np.array(init, np.float32).reshape(-1, 3)
    K = C.shape[0]
    valid = valid_pixels(X)
    tol_abs = tolerance(X, valid, tol)
    old, stable = None, False
    for it in range(1, max_iter + 1):
        labels = assign(X, C, valid)
        s = cluster_sums(X, labels, K)
        new = C.copy()
        for k in range(K):
            if s[k, 0] > 0:
                new[k] = (s[k, 1:] / s[k, 0]).astype(np.float32)
        e = new.astype(np.float64) - C.astype(np.float64)
        shift = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        C = new
        counts = s[:, 0]
        if old is not None and np.array_equal(labels, old):
            stable = True
            break
        total = 0.0
        for k in range(K):
            total += shift[k]
        if total <= tol_abs:
            break
        old = labels
    if not stable:
        labels = assign(X, C, valid)
        counts = np.array([(labels == k).sum() for k in range(K)])
    return labels.reshape(H, W), C, counts.astype(np.int32), it


# ---- the pick and merge of clusters ---------------------------------------------------------------------------------------
def _top(counts, n):
    """The n labels with the most members, largest first; among equal counts the smaller label first."""
    return sorted(range(len(counts)), key=lambda j: (-int(counts[j]), j))[:n]


def merge_normal_clusters(counts, top, centres):
    counts = np.asarray(counts, np.int64)
    K = len(counts)
    c = np.asarray(centres, np.float64)
    c = c / np.linalg.norm(c, axis=1, keepdims=True)
    top = [int(t) for t in top]
    target = list(range(K))
    merged = [False] * len(top)
    kept = len(top)
    for i in range(len(top)):
        if merged[i]:
            continue
        for j in range(i + 1, len(top)):
            if merged[j]:
                continue
            if np.dot(c[top[i]], c[top[j]]) > 0.95:
                target[top[j]] = top[i]
                merged[j] = True
                kept -= 1
    if kept != len(top):
        new_counts = np.zeros(K, np.int64)
        for j in range(K):
            new_counts[target[j]] += counts[j]
        top = _top(new_counts, kept)
    rank = {label: r for r, label in enumerate(top)}
    return np.array([rank.get(target[j], -1) for j in range(K)], np.int32)


def select_normal_clusters(counts, centres, n_clusters=6):
    return merge_normal_clusters(counts, _top(counts, min(n_clusters, len(counts))), centres)


# ---- B. opening and components -------------------------------------------------------------------------------------------
def open_ranks(rank):
    rank = np.asarray(rank, np.int8)
    H, W = rank.shape
    pad = np.full((H + 8, W + 8), -2, np.int8)
    pad[4:-4, 4:-4] = rank
    survive = rank >= 0
    for dy in range(9):
        for dx in range(9):
            nb = pad[dy:dy + H, dx:dx + W]
            survive &= (nb == rank) | (nb == -2)
    spad = np.zeros((H + 8, W + 8), bool)
    spad[4:-4, 4:-4] = survive
    near = np.zeros((H, W), bool)
    for dy in range(9):
        for dx in range(9):
            near |= spad[dy:dy + H, dx:dx + W]
    return np.where(near & (rank >= 0), rank, -1).astype(np.int8)


def components(opened, min_size):
    """(components int32 [H,W], sizes int32 [n], n): 8-connected, kept from min_size, ids by (rank, first pixel)."""
    opened = np.asarray(opened, np.int8)
    H, W = opened.shape
    out = np.full((H, W), -1, np.int32)
    seen = np.zeros((H, W), bool)
    sizes = []
    for r in sorted(int(x) for x in np.unique(opened) if x >= 0):
        for q in np.flatnonzero(opened.reshape(-1) == r):
            y, x = divmod(int(q), W)
            if seen[y, x]:
                continue
            seen[y, x] = True
            stack, member = [(y, x)], []
            while stack:
                cy, cx = stack.pop()
                member.append((cy, cx))
                for ny in range(max(cy - 1, 0), min(cy + 2, H)):
                    for nx in range(max(cx - 1, 0), min(cx + 2, W)):
                        if not seen[ny, nx] and opened[ny, nx] == r:
                            seen[ny, nx] = True
                            stack.append((ny, nx))
            if len(member) >= min_size:
                ys, xs = zip(*member)
                out[list(ys), list(xs)] = len(sizes)
                sizes.append(len(member))
    return out, np.array(sizes, np.int32), len(sizes)


def normal_components(labels, lut, min_size, do_open=True):
    labels = np.asarray(labels, np.int8)
    lut = np.asarray(lut, np.int32)
    inside = (labels >= 0) & (labels < len(lut))
    rank = np.where(inside, lut[np.clip(labels, 0, len(lut) - 1)], -1).astype(np.int8)
    return components(open_ranks(rank) if do_open else rank, min_size)


# ---- C. the join -----------------------------------------------------------------------------------------------------------
def fixed32(x):
    """round-half-even(clamp(x, -2, 2) 2^32) as int64, 0 for a NaN."""
    x = np.asarray(x, np.float32).astype(np.float64)
    f = np.rint(np.clip(np.nan_to_num(x, nan=0.0, posinf=2.0, neginf=-2.0), -2.0, 2.0) * 4294967296.0).astype(np.int64)
    return np.where(np.isnan(x), 0, f)


def excavate_planes(normals, masks, comps, n, min_plane_size, max_planes=100):
    """The reference's double loop, repaint and mean normals: (seg int32 [H,W], normal float64 [p,3] or None, areas int64 [p]
    or None, count = the pair ids handed out)."""
    normals = np.asarray(normals, np.float32)
    H, W = comps.shape
    masks = np.asarray(masks).reshape(-1, H, W) != 0
    order = np.argsort(masks.reshape(len(masks), H * W).sum(axis=1), kind="stable")
    seg = np.zeros((H, W), np.int32)
    count = 0
    for m in order:
        for c in range(n):
            inter = masks[m] & (comps == c)
            if inter.sum() < min_plane_size:
                continue
            count += 1
            seg[inter] = count
    new = np.zeros_like(seg)
    avg_normals, areas = [], []
    for i in range(min(max_planes, count)):
        mask = seg == i + 1
        area = int(mask.sum())
        if area < min_plane_size:
            continue
        areas.append(area)
        new[mask] = len(areas)
        avg = fixed32(normals[mask]).sum(axis=0).astype(np.float64) / 4294967296.0 / area
        avg_normals.append(avg / np.sqrt((avg ** 2).sum()))
    if not areas:
        return new, None, None, count
    return new, np.stack(avg_normals), np.array(areas, np.int64), count


def unit_normals(rng, H, W, n_dirs=5, noise=0.2):
    dirs = rng.normal(size=(n_dirs, 3))
    n = dirs[rng.integers(0, n_dirs, (H, W))] + noise * rng.normal(size=(H, W, 3))
    return (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
