"""The chart deformation's contract (include/g4s_losses.h, "Chart deformation") restated in numpy in a float type of the
caller's choice: float64 for pinning against the reference's float64 run, float32 as the yardstick of a generated case.
Forward and analytic gradients.  The sums over k, over the pixels and over the taps are numpy's (np.matmul, np.add.at), not
the kernels' orders: nothing here is compared bit for bit with the GPU.  Nothing here touches a GPU.

A case is a SimpleNamespace: n, H, W, cams (cameras with world_view_transform / full_proj_transform), d0 [n,H,W] float32,
levels (list of [n,C,h,w]), denc ([n,E,B] or None), coords ([n,H W] or None), weights / biases (lists, [n,out,in] / [n,out]),
scene_radius, deformation_radius (floats)."""
from types import SimpleNamespace

import numpy as np

import chart_align_ref

GOLDEN_CASES = ("one", "small", "single", "full")


def lin(K, T):
    """torch.linspace(-1, 1, K), correctly rounded: (2 i - (K - 1)) / (K - 1)"""
    if K == 1:
        return np.full(1, -1.0, T)
    return (2 * np.arange(K) - (K - 1)).astype(T) / T(K - 1)


def taps(u, size, T):
    """(i0, i1, w0, w1) of the contract's Taps(u, size)"""
    t = ((u + T(1)) * T(size) - T(1)) / T(2)
    t = np.clip(t, T(0), T(size - 1))
    f = np.floor(t)
    i0 = f.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), (f + T(1)) - t, t - f


def ray_scale(c, T):
    """sign(d0) / |D (x, y, 1)| [n,H,W]: d(depth)/d(delta); the ray records rounded to T (the kernels read them in float32)"""
    rec = chart_align_ref.ray_records(c.cams, c.W, c.H).astype(T)
    yy, xx = np.meshgrid(np.arange(c.H, dtype=T), np.arange(c.W, dtype=T), indexing="ij")
    D = rec[:, 3:12].reshape(c.n, 3, 3)
    dirs = [(D[:, k, 0, None, None] * xx + D[:, k, 1, None, None] * yy) + D[:, k, 2, None, None] for k in range(3)]
    length = np.sqrt((dirs[0] * dirs[0] + dirs[1] * dirs[1]) + dirs[2] * dirs[2])
    return np.sign(c.d0.astype(T)) / length


def _pixel_taps(c, h, w, T):
    """Per pixel of the H x W lattice the four (texel y, texel x, weight) of a level h x w: the ROW drives x."""
    x0, x1, wx0, wx1 = taps(lin(c.H, T), w, T)  # per row
    y0, y1, wy0, wy1 = taps(lin(c.W, T), h, T)  # per column
    out = []
    for ys, wy in ((y0, wy0), (y1, wy1)):
        for xs, wx in ((x0, wx0), (x1, wx1)):
            out.append((np.broadcast_to(ys[None, :], (c.H, c.W)), np.broadcast_to(xs[:, None], (c.H, c.W)), wx[:, None] * wy[None, :]))
    return out


def forward(c, T=np.float64):
    """delta, depths [n,H,W] and what the backward needs"""
    n, N = c.n, c.H * c.W
    enc = []
    for lv in c.levels:
        v = lv.astype(T)
        _n, C, h, w = v.shape
        s = 0
        for ys, xs, wt in _pixel_taps(c, h, w, T):
            s = s + v[:, :, ys, xs] * wt  # [n,C,H,W]
        enc.append(s)
    x = np.concatenate(enc, axis=1).reshape(n, -1, N).transpose(0, 2, 1)  # [n,N,E]
    dt = None
    if c.denc is not None:
        b0, b1, w0, w1 = taps(T(-1) + T(2) * c.coords.astype(T), c.denc.shape[2], T)  # [n,N]
        q = c.denc.astype(T)
        rows = np.arange(n)[:, None]
        x = x + (q[rows, :, b0] * w0[..., None] + q[rows, :, b1] * w1[..., None])
        dt = (b0, b1, w0, w1)
    acts = [x / T(c.scene_radius)]
    for j, (Wj, bj) in enumerate(zip(c.weights, c.biases)):
        z = np.matmul(acts[-1], Wj.astype(T).transpose(0, 2, 1)) + bj.astype(T)[:, None, :]
        if j < len(c.weights) - 1:
            acts.append(np.maximum(z, T(0)))
    delta = (z[..., 0] * T(c.deformation_radius)).reshape(n, c.H, c.W)
    s = ray_scale(c, T)
    d0 = c.d0.astype(T)
    depths = np.where(d0 == 0, d0, d0 + delta * s)
    return SimpleNamespace(delta=delta, depths=depths, acts=acts, scale=np.where(d0 == 0, T(0), s), denc_taps=dt)


def pre_activations(c, T=np.float64):
    """The pre-activations of every hidden layer, [n,N,S] each: the ReLU kinks"""
    a = forward(c, T).acts
    return [np.matmul(a[j], c.weights[j].astype(T).transpose(0, 2, 1)) + c.biases[j].astype(T)[:, None, :] for j in range(len(c.weights) - 1)]


def gradients(c, g, T=np.float64):
    """The gradient of sum(g * depths) to every parameter: dict(levels=[...], denc=..., weights=[...], biases=[...])"""
    f = forward(c, T)
    n, N = c.n, c.H * c.W
    gz = ((g.astype(T) * f.scale) * T(c.deformation_radius)).reshape(n, N, 1)
    dW, dB = [None] * len(c.weights), [None] * len(c.weights)
    for j in range(len(c.weights) - 1, -1, -1):
        a = f.acts[j]
        dW[j] = np.matmul(gz.transpose(0, 2, 1), a)
        dB[j] = gz.sum(axis=1)
        da = np.matmul(gz, c.weights[j].astype(T))
        gz = np.where(a > 0, da, T(0)) if j > 0 else da
    dx = gz / T(c.scene_radius)  # [n,N,E]
    dlevels, at = [], 0
    for lv in c.levels:
        _n, C, h, w = lv.shape
        d = dx[:, :, at:at + C].transpose(0, 2, 1).reshape(n, C, c.H, c.W)
        at += C
        out = np.zeros(lv.shape, T)
        for ys, xs, wt in _pixel_taps(c, h, w, T):
            np.add.at(out, (slice(None), slice(None), ys, xs), d * wt)
        dlevels.append(out)
    ddenc = None
    if c.denc is not None:
        b0, b1, w0, w1 = f.denc_taps
        ddenc = np.zeros(c.denc.shape, T)
        rows, chans = np.arange(n)[:, None, None], np.arange(c.denc.shape[1])[None, None, :]
        np.add.at(ddenc, (rows, chans, b0[..., None]), dx * w0[..., None])
        np.add.at(ddenc, (rows, chans, b1[..., None]), dx * w1[..., None])
    return dict(levels=dlevels, denc=ddenc, weights=dW, biases=dB)


def depth_coordinates(d0, n_bins):
    """ParallelAligner.__init__ lines 279-306 on float32 depths [n,H,W]: float32 [n, H W].  The quantiles are torch.quantile's
    (its float32 interpolation is not restated); the binning arithmetic is numpy's, in float32."""
    import torch
    nb = int(n_bins)
    out = []
    for d in np.asarray(d0, np.float32).reshape(len(d0), -1):
        q = np.array([torch.quantile(torch.from_numpy(d), i / nb).item() for i in range(nb)], np.float32)
        coords = np.zeros_like(d)
        for i in range(nb):
            if i < nb - 1:
                m = (d >= q[i]) & (d < q[i + 1])
                coords[m] = ((d[m] - q[i]) / (q[i + 1] - q[i]) + np.float32(i)) / np.float32(nb - 1)
            else:
                coords[d >= q[i]] = np.float32(1)
        out.append(coords)
    return np.stack(out)


# ---- names ----------------------------------------------------------------------------------------------------------------
def parameter_names(c):
    """The reference's parameter names, in the order levels, depth encoding, weights and biases per layer"""
    L = len(c.levels)
    names = [f"charts_encoding.charts_encoding.{l}.encodings" for l in range(L)] if c.multi_res else ["charts_encoding.encodings"]
    if c.denc is not None:
        names.append("depth_encoding.encodings")
    for j in range(len(c.weights)):
        names += [f"deformation.mlp.{2 * j}.weight", f"deformation.mlp.{2 * j}.bias"]
    return names


def parameters(c):
    """name -> array, in parameter_names' order"""
    vals = list(c.levels) + ([c.denc] if c.denc is not None else [])
    for Wj, bj in zip(c.weights, c.biases):
        vals += [Wj, bj]
    return dict(zip(parameter_names(c), vals))


def flat_gradients(c, grads):
    """gradients() as name -> array"""
    vals = list(grads["levels"]) + ([grads["denc"]] if c.denc is not None else [])
    for Wj, bj in zip(grads["weights"], grads["biases"]):
        vals += [Wj, bj]
    return dict(zip(parameter_names(c), vals))


# ---- cases ------------------------------------------------------------------------------------------------------------------
# name: n, H, W, resolutions (None: the single-resolution ChartsEncoding at factor 0.4), channels per level, layer size, layers,
# depth bins (0: no depth encoding)
CASES = {"one": (1, 3, 3, (0.5, 1.0), 8, 64, 3, 30), "small": (2, 4, 5, (0.25, 0.5, 0.75, 1.0), 4, 32, 2, 0),
         "single": (2, 7, 6, None, 32, 32, 4, 30), "full": (3, 33, 50, (0.05, 0.1, 0.2, 0.4), 8, 64, 3, 30),
         "wide": (3, 20, 70, (0.05, 0.1, 0.2, 0.4), 8, 64, 3, 30)}


def spatial_extent(cams):
    c = np.stack([np.linalg.inv(np.asarray(cam.world_view_transform, np.float64).reshape(4, 4).T)[:3, 3] for cam in cams])
    return 1.1 * float(np.linalg.norm(c - c.mean(axis=0, keepdims=True), axis=1).max())


def make_case(name, seed, shape=None):
    """A case with trained-like parameters: encodings uniform in +- scene_radius, Xavier-sized weights, random biases, so that
    pre-activations are O(1) and every ReLU goes both ways.  A single camera has no extent: its radii are 1.  One view of
    `full` has a few zero depths."""
    n, H, W, res, C, S, NL, B = CASES[name] if shape is None else shape
    cams, d0, _ref, _cur = chart_align_ref.scene(n, H, W, seed)
    rng = np.random.default_rng(7000 + seed)
    if name in ("full", "wide"):
        d0 = d0.copy()
        d0[n - 1].reshape(-1)[rng.choice(H * W, 5, replace=False)] = 0.0
    extent = spatial_extent(cams) if n > 1 else 0.5
    R, Rd = 2.0 * extent, 1.0 * extent
    sizes = [(int(r * H), int(r * W)) for r in res] if res is not None else [(int(0.4 * H), int(0.4 * W))]
    E = C * len(sizes)
    f32 = np.float32
    levels = [(R * rng.uniform(-1, 1, (n, C, h, w))).astype(f32) for h, w in sizes]
    denc = (R * rng.uniform(-1, 1, (n, E, B))).astype(f32) if B else None
    dims = [E] + [S] * (NL - 1) + [1]
    weights = [(rng.standard_normal((n, dims[j + 1], dims[j])) * np.sqrt(2.0 / dims[j])).astype(f32) for j in range(NL)]
    biases = [rng.uniform(-0.5, 0.5, (n, dims[j + 1])).astype(f32) for j in range(NL)]
    return SimpleNamespace(name=name, n=n, H=H, W=W, cams=cams, d0=d0, levels=levels, denc=denc, coords=None, weights=weights,
                           biases=biases, scene_radius=R, deformation_radius=Rd, multi_res=res is not None, resolutions=res,
                           channels=C, layer_size=S, layers=NL, bins=B, extent=extent)


NUDGE = 2.0 ** -10


def settle(c):
    """The case with every pre-activation away from its kink by 8 float32 errors (the PARAMETERS change, never the assertion)."""
    for attempt in range(400):
        z64, z32 = pre_activations(c, np.float64), pre_activations(c, np.float32)
        err = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(z32, z64))
        smallest = min(np.abs(b).min() for b in z64)
        if smallest > 8 * err:
            print(f"{c.name}: smallest |pre-activation| {smallest:.3e}, float32 error {err:.3e}, after {attempt} rounds")
            return c
        for j, b in enumerate(z64):
            charts, _pix, units = np.nonzero(np.abs(b) <= 8 * err)
            for i, u in set(zip(charts.tolist(), units.tolist())):
                c.biases[j][i, u] += np.float32(NUDGE)
    raise AssertionError(f"{c.name}: pre-activations within 8 float32 errors of zero remain")


def load_case(g, name):
    """A golden case (tests/golden/chart_deform.npz) with its float64 record r64 and the float32 yardsticks"""
    n, H, W, res, C, S, NL, B = CASES[name]
    key = lambda k: g[f"{name}_{k}"]  # noqa: E731
    cams = [SimpleNamespace(world_view_transform=w, projection_matrix=p, full_proj_transform=f, image_width=W, image_height=H)
            for w, p, f in zip(key("wvt"), key("proj"), key("full"))]
    L = len(res) if res is not None else 1
    c = SimpleNamespace(name=name, n=n, H=H, W=W, cams=cams, d0=key("d0"), levels=[key(f"level{l}") for l in range(L)],
                        denc=key("denc") if B else None, coords=key("depth_coords") if B else None,
                        weights=[key(f"weight{j}") for j in range(NL)], biases=[key(f"bias{j}") for j in range(NL)],
                        scene_radius=float(key("radii")[0]), deformation_radius=float(key("radii")[1]), multi_res=res is not None,
                        resolutions=res, channels=C, layer_size=S, layers=NL, bins=B, extent=float(key("radii")[2]),
                        cotangent=key("cotangent"))
    names = parameter_names(c)
    assert [str(s) for s in key("names")] == names, (name, list(key("names")), names)
    c.r64 = SimpleNamespace(delta=key("delta64"), depths=key("depths64"),
                            grads={tag: {nm: key(f"grad64_{tag}_{i}") for i, nm in enumerate(names)} for tag in ("g", "ones")})
    c.yard = SimpleNamespace(delta=float(key("yard")[0]), depths=float(key("yard")[1]),
                             grads={tag: dict(zip(names, key(f"grad_yard_{tag}"))) for tag in ("g", "ones")})
    return c
