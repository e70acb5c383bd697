"""What the tests of the two view-stack fields share: the bilinear tap into a view's maps of unbounded_ref and tetra_ref
(the contract's order of operations; the kernels' is csrc/tsdf/view_stack.h), and the probe points of the GPU tests."""
import numpy as np


def tap(ix, iy, W, H):
    """(x0, x1, y0, y1, w00, w10, w01, w11) of pixel coordinates ix, iy [n] (0 <= ix <= W-1, 0 <= iy <= H-1) in their
    own float type: the upper corner is clamped onto the map."""
    one = ix.dtype.type(1)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = ix - fx0, iy - fy0
    return x0, x1, y0, y1, (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy


def bilinear(img, t, keep=None):
    """One [H,W] plane at the tap t, or at its rows `keep`."""
    x0, x1, y0, y1, w00, w10, w01, w11 = t if keep is None else (a[keep] for a in t)
    return ((img[y0, x0] * w00 + img[y0, x1] * w10) + img[y1, x0] * w01) + img[y1, x1] * w11


def probe_points(n=257, seed=31):
    """n float32 points for fields around the unit sphere: half of them in a band about it, the rest uniform in
    [-1.8, 1.8]^3, the last four behind the cameras of tetra_ref.sphere_views or outside every frustum."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.8, 1.8, (n, 3))
    s = rng.normal(size=(n // 2, 3))
    pts[: n // 2] = s / np.linalg.norm(s, axis=1, keepdims=True) * rng.uniform(0.9, 1.2, (n // 2, 1))
    pts[-4:] = [(30.0, 0, 0), (0, -40.0, 3.0), (5.0, 5.0, 5.0), (0, 0, 9.0)]
    return pts.astype(np.float32)
