"""numpy restatement of the cross-view consistency contract (include/g4s_render_maps.h, "Cross-view consistency").

Every float operation is float32 in the header's order, so confident maps, images, states, counts and anchors can be
compared with the HIP library exactly.  `dtype=np.float64` evaluates the same decisions in double (only the golden
generator's cross-check uses it).  Slow and simple: for tests only.

A camera is anything with world_view_transform, FoVx and FoVy; a view's size is its depth map's.
"""
import numpy as np

import visibility_ref as vr

f32 = np.float32
NO_STEP = np.iinfo(np.int64).max


def surface(points, cam, depth, depth_threshold=0.1, dtype=f32):
    """(vis bool [n], pix int64 [n]): SURFACE of every point in one view and the row-major index of its tap (-1 where
    the point does not pass)."""
    ft = dtype
    depth = vr._as(depth, ft)
    H, W = depth.shape
    z, u, v, inside = vr.project(points, cam, W, H, ft)
    vis = np.zeros(len(z), bool)
    pix = np.full(len(z), -1, np.int64)
    idx = np.nonzero(inside)[0]
    col = np.minimum(u[idx].astype(np.int64), W - 1)
    row = np.minimum(v[idx].astype(np.int64), H - 1)
    d = depth[row, col]
    zi = z[idx]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ok = (zi > 0) & (np.abs(zi - d) / (zi + ft(1e-6)) < ft(depth_threshold))
    vis[idx] = ok
    pix[idx[ok]] = (row * W + col)[ok]
    return vis, pix


def images_to_uint8(x):
    """uint8(trunc(x * 255.0f))"""
    return (np.asarray(x, f32) * f32(255.0)).astype(np.uint8)


def _hwc(image, H, W):
    image = np.asarray(image, f32)
    return image if image.shape == (H, W, 3) else image.transpose(1, 2, 0)


# ---- A. point solver --------------------------------------------------------------------------------------------------
def point_tables(cams, depths, points, depth_threshold=0.1, dtype=f32):
    """(vis bool [V,N], pix int64 [V,N]) -- the tables the library never stores."""
    n = len(np.asarray(points).reshape(-1, 3))
    vis, pix = np.zeros((len(cams), n), bool), np.full((len(cams), n), -1, np.int64)
    for v, (cam, depth) in enumerate(zip(cams, depths)):
        vis[v], pix[v] = surface(points, cam, depth, depth_threshold, dtype)
    return vis, pix


def point_states(cams, depths, images, points, n_input, depth_threshold=0.1, dtype=f32, tables=None):
    """(seen bool [N], visible bool [N], colours uint8 [N,3])"""
    vis, pix = tables if tables is not None else point_tables(cams, depths, points, depth_threshold, dtype)
    n = vis.shape[1]
    seen = vis[:n_input].any(0) if n_input else np.zeros(n, bool)
    visible = vis.any(0) if len(cams) else np.zeros(n, bool)
    colours = np.zeros((n, 3), np.uint8)
    idx = np.nonzero(visible & ~seen)[0]
    if len(idx):
        first = vis[:, idx].argmax(0)  # the smallest v with vis
        for v in np.unique(first):
            sel = idx[first == v]
            H, W = np.asarray(depths[v]).shape
            img = _hwc(images[v], H, W).reshape(-1, 3)
            colours[sel] = images_to_uint8(img[pix[v, sel]])
    return seen, visible, colours


def point_solver(cams, depths, images, points, n_input, depth_threshold=0.1, dtype=f32, stats=None):
    """(images_out -- float32 [H,W,3] per view --, confident maps -- uint8 [H,W] per view)."""
    tables = point_tables(cams, depths, points, depth_threshold, dtype)
    vis, pix = tables
    seen, _visible, colours = point_states(cams, depths, images, points, n_input, depth_threshold, dtype, tables)
    outs, confs = [], []
    dup = dup_diff = changed = 0
    for v, depth in enumerate(depths):
        H, W = np.asarray(depth).shape
        out = _hwc(images[v], H, W).copy().reshape(-1, 3)
        conf = np.ones(H * W, np.uint8)
        if v >= n_input:
            conf[pix[v, vis[v] & seen]] = 0
            idx = np.nonzero(vis[v] & ~seen)[0]
            winner = np.zeros(H * W, np.int64)  # i + 1 of the largest index, 0: none
            np.maximum.at(winner, pix[v, idx], idx + 1)
            hit = np.nonzero(winner)[0]
            before = out[hit].copy()
            out[hit] = colours[winner[hit] - 1].astype(f32) / f32(255.0)
            changed += int((images_to_uint8(before) != images_to_uint8(out[hit])).any(1).sum())
            hits = np.bincount(pix[v, idx], minlength=H * W)
            dup += int((hits >= 2).sum())
            for q in np.nonzero(hits >= 2)[0]:
                cand = colours[idx[pix[v, idx] == q]]
                dup_diff += int((cand != cand[0]).any())
        outs.append(out.reshape(H, W, 3))
        confs.append(conf.reshape(H, W))
    if stats is not None:
        stats.update(unseen=int((~seen).sum()), duplicate_pixels=dup, duplicate_pixels_differing=dup_diff, changed_pixels=changed,
                     conf_zeros=[int((c == 0).sum()) for c in confs[n_input:]])
    return outs, confs


# ---- B. plane solver --------------------------------------------------------------------------------------------------
def _pairs(gdict):
    return {int(k): [(int(v), int(p)) for v, p in pairs] for k, pairs in gdict.items()}


def plane_counts(cams, depths, masks, points, gdict, anchor_view_ids, depth_threshold=0.1, dtype=f32):
    """int64 [K,A]: per plane and anchor the number of the plane's points, over all its pairs, that pass SURFACE."""
    pairs = _pairs(gdict)
    counts = np.zeros((len(pairs), len(anchor_view_ids)), np.int64)
    for n, plist in enumerate(pairs.values()):
        for w, p in plist:
            sel = np.asarray(masks[w]).reshape(-1) == p
            P = np.asarray(points[w], f32).reshape(-1, 3)[sel]
            for j, a in enumerate(anchor_view_ids):
                counts[n, j] += int(surface(P, cams[a], depths[a], depth_threshold, dtype)[0].sum())
    return counts


def choose_anchor_views(counts, anchor_view_ids):
    out = []
    for row in np.asarray(counts).reshape(len(counts), len(anchor_view_ids)).tolist():
        best, view = 0, -1
        for j, c in enumerate(row):
            if c > best:
                best, view = c, int(anchor_view_ids[j])
        out.append(view)
    return out


def plane_steps(gdict, anchor_of_plane):
    steps, seen = [], set()
    for k, plist in _pairs(gdict).items():
        for pair in plist:
            if pair in seen:
                raise ValueError(f"pair {pair} listed twice")
            seen.add(pair)
        if anchor_of_plane[k] != -1:
            steps.extend((w, p, int(anchor_of_plane[k])) for w, p in plist)
    return steps


def plane_sources(cams, depths, masks, points, steps, depth_threshold=0.1, dtype=f32):
    """Per view (step int64 [H*W] -- NO_STEP: none --, source view int64 [H*W], source pixel int64 [H*W])."""
    src = [(np.full(np.asarray(m).size, NO_STEP, np.int64), np.zeros(np.asarray(m).size, np.int64),
            np.zeros(np.asarray(m).size, np.int64)) for m in masks]
    for t, (w, p, a) in enumerate(steps):
        q = np.nonzero(np.asarray(masks[w]).reshape(-1) == p)[0]
        vis, pix = surface(np.asarray(points[w], f32).reshape(-1, 3)[q], cams[a], depths[a], depth_threshold, dtype)
        assert (src[w][0][q] == NO_STEP).all()  # a mask holds one id per pixel
        src[w][0][q[vis]], src[w][1][q[vis]], src[w][2][q[vis]] = t, a, pix[vis]
    return src


def resolve_chains(images, src, lengths=None):
    """final(x) = value(x, infinity), value(x, T) = value(src(x), step(x)) if step(x) < T else original(x)."""
    outs = []
    for w, image in enumerate(images):
        image = np.asarray(image, np.uint8)
        out = np.empty_like(image).reshape(-1, 3)
        for q in range(len(out)):
            cw, cq, T, hops = w, q, NO_STEP, 0
            while src[cw][0][cq] < T:
                T, cw, cq = src[cw][0][cq], int(src[cw][1][cq]), int(src[cw][2][cq])
                hops += 1
            out[q] = np.asarray(images[cw], np.uint8).reshape(-1, 3)[cq]
            if lengths is not None:
                lengths[w][q] = hops
        outs.append(out.reshape(image.shape))
    return outs


def resolve_chains_at_once(images, src, lengths=None):
    """resolve_chains for views too large to walk pixel by pixel in Python: every pixel of every view takes its next hop in
    one indexing operation, until no chain goes on.  The same rule, the same results."""
    sizes = [len(s[0]) for s in src]
    base = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    step = np.concatenate([np.asarray(s[0], np.int64) for s in src]) if sizes else np.zeros(0, np.int64)
    source = np.concatenate([base[np.asarray(s[1], np.int64)] + np.asarray(s[2], np.int64) for s in src]) if sizes else step
    colours = np.concatenate([np.asarray(im, np.uint8).reshape(-1, 3) for im in images]) if sizes else np.zeros((0, 3), np.uint8)
    at = np.arange(len(step), dtype=np.int64)
    T = np.full(len(step), NO_STEP, np.int64)
    hops = np.zeros(len(step), np.int64)
    while True:
        go = step[at] < T
        if not go.any():
            break
        T[go] = step[at[go]]
        at[go] = source[at[go]]
        hops[go] += 1
    outs = []
    for w, image in enumerate(images):
        outs.append(colours[at[base[w]:base[w + 1]]].reshape(np.asarray(image).shape))
        if lengths is not None:
            lengths[w][:] = hops[base[w]:base[w + 1]]
    return outs


def repaint_in_place(images, src, n_steps):
    """The literal repaint: step after step, in place, the right-hand side of a step evaluated before it is assigned."""
    imgs = [np.array(im, np.uint8).reshape(-1, 3) for im in images]
    for t in range(n_steps):
        for w in range(len(imgs)):
            q = np.nonzero(src[w][0] == t)[0]
            if len(q) == 0:
                continue
            a = int(src[w][1][q[0]])
            assert (src[w][1][q] == a).all()
            colours = imgs[a][src[w][2][q]]  # advanced indexing: a copy
            imgs[w][q] = colours
    return [im.reshape(np.asarray(o).shape) for im, o in zip(imgs, images)]


def plane_solver(cams, depths, images, masks, points, gdict, anchor_view_ids, depth_threshold=0.1, dtype=f32, lengths=None,
                 resolve=None):
    """(images_out -- uint8 [H,W,3] per view --, anchor_of_plane {k: view or -1}, counts int64 [K,A]); `resolve`:
    resolve_chains (the default) or resolve_chains_at_once."""
    resolve = resolve or resolve_chains
    counts = plane_counts(cams, depths, masks, points, gdict, anchor_view_ids, depth_threshold, dtype)
    anchor_of_plane = dict(zip(_pairs(gdict), choose_anchor_views(counts, anchor_view_ids)))
    steps = plane_steps(gdict, anchor_of_plane)
    src = plane_sources(cams, depths, masks, points, steps, depth_threshold, dtype)
    return resolve(images, src, lengths), anchor_of_plane, counts
