"""The chart alignment losses' contract (include/g4s_losses.h, "Chart alignment losses") restated in numpy, operation for
operation, in a float type of the caller's choice: float32 for the bit comparisons with the kernels, float64 for pinning
against the reference's float64 run.  Nothing here touches a GPU.

Shapes: depths and the other maps [n,H,W], normals [n,H,W,3], curvatures [n,H,W], gradient masks [n,H-1,W-1]."""
from types import SimpleNamespace

import numpy as np

import chart_match_ref

GRADIENT, NORMAL, CURVATURE = 1, 2, 4
EPS = 1e-12
GOLDEN_CASES = ("one", "flat_rows", "flat_cols", "small", "full", "noconf")


def ray_records(cameras, W, H):
    """float64 [n,12]: o[3], D[3][3] per view (the first twelve floats of the matcher's record)."""
    return chart_match_ref.camera_records(cameras, W, H)[:, :12]


def _signed(v):
    return (v > 0).astype(v.dtype) - (v < 0).astype(v.dtype)  # sign(0) = 0


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def geometry(cameras, depths, ftype=np.float32):
    """dir and q [n,H,W,3]; for the interior pixels ([n,H-2,W-2,...]) a, b, c = a x b and L = |c|; the normals nu [n,H,W,3]."""
    T = ftype
    D = np.ascontiguousarray(depths, T)
    n, H, W = D.shape
    rec = ray_records(cameras, W, H).astype(T)
    x = np.arange(W, dtype=T)[None, None, :]
    y = np.arange(H, dtype=T)[None, :, None]
    o, R = rec[:, 0:3], rec[:, 3:12].reshape(n, 3, 3)
    dirs = np.stack([(R[:, k, 0, None, None] * x + R[:, k, 1, None, None] * y) + R[:, k, 2, None, None] for k in range(3)], -1)
    q = D[..., None] * dirs + o[:, None, None, :]
    # the point differences in the contract's form: the depth difference along the far ray plus the near depth along the
    # (exact) difference of the two rays
    two_row, two_col = (R[:, :, 1] + R[:, :, 1])[:, None, None, :], (R[:, :, 0] + R[:, :, 0])[:, None, None, :]
    a = (D[:, 2:, 1:-1] - D[:, :-2, 1:-1])[..., None] * dirs[:, 2:, 1:-1] + D[:, :-2, 1:-1, None] * two_row
    b = (D[:, 1:-1, 2:] - D[:, 1:-1, :-2])[..., None] * dirs[:, 1:-1, 2:] + D[:, 1:-1, :-2, None] * two_col
    c = _cross(a, b)
    with np.errstate(all="ignore"):
        L = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])
        den = np.where(L < T(EPS), T(EPS), L)
        nu = np.zeros((n, H, W, 3), T)
        if H >= 3 and W >= 3:
            nu[:, 1:-1, 1:-1] = c / den[..., None]
    return SimpleNamespace(n=n, H=H, W=W, dirs=dirs, q=q, a=a, b=b, c=c, L=L, nu=nu)


def normals(cameras, depths, ftype=np.float32):
    return geometry(cameras, depths, ftype).nu


def laplacian(nu):
    """lap [n,H,W,3] in the contract's order (above, left, below, right; replicate padding)."""
    p = np.pad(nu, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    c = p[:, 1:-1, 1:-1]
    return (((p[:, :-2, 1:-1] - c) + (p[:, 1:-1, :-2] - c)) + (p[:, 2:, 1:-1] - c)) + (p[:, 1:-1, 2:] - c)


def curvatures(nu):
    """kappa [n,H,W] = (|lap_0| + |lap_1|) + |lap_2|."""
    lap = np.abs(laplacian(nu))
    return (lap[..., 0] + lap[..., 1]) + lap[..., 2]


def _grad_diffs(d, d0, gm, T):
    """gm (D_k d - D_k d0) for k = row, column: two [n,H-1,W-1] arrays."""
    row = (d[:, 1:, :-1] - d[:, :-1, :-1]) - (d0[:, 1:, :-1] - d0[:, :-1, :-1])
    col = (d[:, :-1, 1:] - d[:, :-1, :-1]) - (d0[:, :-1, 1:] - d0[:, :-1, :-1])
    if gm is not None:
        row, col = np.asarray(gm, T) * row, np.asarray(gm, T) * col
    return row, col


def evaluate(cameras, depths, reference_depths, initial_depths, initial_normals, initial_curvatures, confidence=None, masks=None,
             gradient_masks=None, lam=0.2, flags=GRADIENT | NORMAL | CURVATURE, ftype=np.float32):
    """Everything of one evaluation: the per-pixel terms, the four means, the decision quantities and the geometry."""
    T = ftype
    d, r = np.ascontiguousarray(depths, T), np.asarray(reference_depths, T)
    g = geometry(cameras, d, T)
    n, H, W = d.shape
    e = d - r
    t0 = np.abs(e)
    if confidence is not None:
        c = np.asarray(confidence, T)
        t0 = c * t0 - T(lam) * np.log(c)
    if masks is not None:
        t0 = np.asarray(masks, T) * t0
    out = SimpleNamespace(g=g, e=e, flags=flags, means=np.zeros(4, T))
    out.means[0] = t0.sum(dtype=T) / T(n * H * W)
    if flags & GRADIENT:
        out.row, out.col = _grad_diffs(d, np.asarray(initial_depths, T), gradient_masks, T)
        out.means[1] = (np.abs(out.row) + np.abs(out.col)).sum(dtype=T) / T(2 * n * (H - 1) * (W - 1))
    if flags & NORMAL:
        out.means[2] = (T(1) - _dot(np.asarray(initial_normals, T), g.nu)).sum(dtype=T) / T(n * H * W)
    if flags & CURVATURE:
        out.lap = laplacian(g.nu)
        a = np.abs(out.lap)
        out.kappa = (a[..., 0] + a[..., 1]) + a[..., 2]
        out.dk = np.asarray(initial_curvatures, T) - out.kappa
        out.means[3] = np.abs(out.dk).sum(dtype=T) / T(n * H * W)
    return out


def means(*args, **kwargs):
    return evaluate(*args, **kwargs).means


def gradients(cameras, depths, reference_depths, initial_depths, initial_normals, initial_curvatures, confidence=None, masks=None,
              gradient_masks=None, lam=0.2, flags=GRADIENT | NORMAL | CURVATURE, cotangents=(1.0, 1.0, 1.0, 1.0), ftype=np.float32):
    """(dL/ddepths [n,H,W], dL/dconfidence [n,H,W] or None) of sum_k cotangents[k] means[k], analytic, every step a gather."""
    T = ftype
    ev = evaluate(cameras, depths, reference_depths, initial_depths, initial_normals, initial_curvatures, confidence, masks,
                  gradient_masks, lam, flags, T)
    g = ev.g
    n, H, W = g.n, g.H, g.W
    nN = T(n * H * W)
    g4 = [T(np.float32(c)) for c in cotangents]  # what a float32 cotangent on the device holds
    km = g4[0] / nN
    if masks is not None:
        km = km * np.asarray(masks, T)
    dconf = None
    if confidence is not None:
        c = np.asarray(confidence, T)
        gd = (km * c) * _signed(ev.e)
        dconf = km * (np.abs(ev.e) - T(lam) / c)
    else:
        gd = km * _signed(ev.e)
    if flags & GRADIENT:
        gm = T(1) if gradient_masks is None else np.asarray(gradient_masks, T)
        srow, scol = gm * _signed(ev.row), gm * _signed(ev.col)
        s = np.zeros((n, H, W), T)
        s[:, :-1, :-1] -= srow
        s[:, :-1, :-1] -= scol
        s[:, 1:, :-1] += srow
        s[:, :-1, 1:] += scol
        gd = gd + (g4[1] / T(2 * n * (H - 1) * (W - 1))) * s
    if flags & (NORMAL | CURVATURE) and H >= 3 and W >= 3:
        G = np.zeros((n, H - 2, W - 2, 3), T)
        if flags & CURVATURE:
            w = _signed(ev.kappa - np.asarray(initial_curvatures, T))[..., None] * _signed(ev.lap)
            wc = w[:, 1:-1, 1:-1]
            G = (g4[3] / nN) * ((((w[:, :-2, 1:-1] - wc) + (w[:, 1:-1, :-2] - wc)) + (w[:, 2:, 1:-1] - wc)) + (w[:, 1:-1, 2:] - wc))
        if flags & NORMAL:
            G = G - (g4[2] / nN) * np.asarray(initial_normals, T)[:, 1:-1, 1:-1]
        L = g.L[..., None]
        with np.errstate(all="ignore"):
            f = _dot(g.c, G)[..., None] / ((L * L) * L)
            dc = np.where(L < T(EPS), G / T(EPS), G / L - g.c * f)
        A, B = np.zeros((n, H, W, 3), T), np.zeros((n, H, W, 3), T)
        A[:, 1:-1, 1:-1], B[:, 1:-1, 1:-1] = _cross(g.b, dc), _cross(dc, g.a)
        dq = np.zeros((n, H, W, 3), T)
        dq[:, 1:] += A[:, :-1]
        dq[:, :-1] -= A[:, 1:]
        dq[:, :, 1:] += B[:, :, :-1]
        dq[:, :, :-1] -= B[:, :, 1:]
        gd = gd + _dot(g.dirs, dq)
    return gd.astype(T), dconf


def kink_quantities(ev):
    """{name: array} of the quantities whose sign a kink of the loss depends on."""
    out = {"d - r": ev.e}
    if ev.flags & GRADIENT:
        out["grad row"], out["grad col"] = ev.row, ev.col
    if ev.flags & CURVATURE:
        out["lap"], out["kappa0 - kappa"] = ev.lap, ev.dk
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def make_camera(W, H, centre, yaw, pitch, p00, offset=(0.0, 0.0)):
    """float32 matrices in the row-vector convention of the reference's cameras."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    o = np.asarray(centre, np.float64)
    wvt = np.eye(4)
    wvt[:3, :3], wvt[3, :3] = R, -o @ R
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = p00, p00 * W / H
    P[2, 0], P[2, 1] = offset
    P[2, 2], P[2, 3], P[3, 2] = 100.0 / 99.99, 1.0, -100.0 * 0.01 / 99.99
    wvt32, P32 = wvt.astype(np.float32), P.astype(np.float32)
    return SimpleNamespace(world_view_transform=wvt32, projection_matrix=P32, image_width=W, image_height=H,
                           full_proj_transform=(wvt32.astype(np.float64) @ P32.astype(np.float64)).astype(np.float32))


def scene(n, H, W, seed):
    """(cameras, initial depths, reference depths, current depths): n views with different poses (view 1 has an off-centre
    principal point) of the slanted plane 0.3 x + 0.2 y + z = 4; the initial and the reference depths are the plane's times
    (1 + 3 % white noise), two draws; the current depths are the initial ones with 2 % more."""
    pool = [((0.0, 0.0, 0.0), 0.0, 0.0, 1.625, (0.0, 0.0)), ((1.3, 0.15, 0.2), -0.27, 0.04, 1.5, (0.0613, -0.0371)),
            ((-0.9, 0.55, -0.3), 0.21, -0.11, 1.75, (0.0, 0.0))]
    cams = [make_camera(W, H, *pool[v % 3]) for v in range(n)]
    rec = ray_records(cams, W, H)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rng = np.random.default_rng(seed)
    normal, d0, ref = np.array([0.3, 0.2, 1.0]), [], []
    for v in range(n):
        o, D = rec[v, 0:3], rec[v, 3:12].reshape(3, 3)
        dirs = np.stack([D[k, 0] * xx + D[k, 1] * yy + D[k, 2] for k in range(3)], -1)
        plane = (4.0 - normal @ o) / (dirs @ normal)
        assert (plane > 0.5).all()
        d0.append(plane * (1.0 + 0.03 * rng.uniform(-1.0, 1.0, (H, W))))
        ref.append(plane * (1.0 + 0.03 * rng.uniform(-1.0, 1.0, (H, W))))
    d0, ref = np.stack(d0).astype(np.float32), np.stack(ref).astype(np.float32)
    cur = (d0.astype(np.float64) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, d0.shape))).astype(np.float32)
    return cams, d0, ref, cur


# ---- the golden cases (tests/golden/chart_align.npz, make_golden_chart_align.py) -------------------------------------------
TWIN = {"noconf": "full"}  # a case on another case's scene stores only what differs from it


def load_case(g, name):
    """One case of the golden file as a namespace: cameras, inputs, the reference's float64 results (r64), the means of its
    float32 run and the yardstick, the largest error of its float32 run against its float64 run."""
    def get(key):
        return np.asarray(g[f"{name}_{key}"] if f"{name}_{key}" in g else g[f"{TWIN[name]}_{key}"])

    def opt(key):
        return np.asarray(g[f"{name}_{key}"]) if f"{name}_{key}" in g else None

    d0 = get("initial_depths")
    n, H, W = d0.shape
    cams = [SimpleNamespace(world_view_transform=w, projection_matrix=p, full_proj_transform=f, image_width=W, image_height=H)
            for w, p, f in zip(get("wvt"), get("proj"), get("full"))]
    terms = np.stack([get(f"grad64_t{t}") for t in range(4)])
    cot = float(g["cotangent"])
    c = SimpleNamespace(name=name, n=n, H=H, W=W, cams=cams, initial_depths=d0, depths=get("depths"),
                        reference_depths=get("reference_depths"), confidence=opt("confidence"), masks=opt("masks"),
                        gradient_masks=opt("gradient_masks"), lam=float(g["confidence_weighting"]), cotangent=cot,
                        means32=get("means32"), grad_yard=get("grad_yard"), conf_grad_yard=opt("conf_grad_yard"))
    grad = np.concatenate([terms, terms.sum(axis=0, keepdims=True)])  # [5,n,H,W]: each mean alone, then the sum of the four
    conf_grad = opt("conf_grad64")
    c.r64 = SimpleNamespace(means=get("means64"), normals=get("normals64"), curvatures=get("curvatures64"), grad=grad,
                            grad_c037=cot * grad, conf_grad=conf_grad, conf_grad_c037=None if conf_grad is None else cot * conf_grad)
    return c


def case_inputs(c, ftype=np.float32):
    """(positional, keyword) arguments of evaluate / gradients for a loaded case: the initial normals and curvatures are the
    restatement's own, in `ftype`."""
    nu0 = normals(c.cams, c.initial_depths, ftype)
    return ((c.cams, c.depths, c.reference_depths, c.initial_depths, nu0, curvatures(nu0)),
            dict(confidence=c.confidence, masks=c.masks, gradient_masks=c.gradient_masks, lam=c.lam, ftype=ftype))
