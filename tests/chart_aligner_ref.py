"""The contract "Chart alignment: confidence, weighted encodings, encoding regularisers" (include/g4s_losses.h) and the driver of
g4splat_amd/chart_aligner.py restated in numpy, on top of chart_deform_ref, chart_align_ref and chart_match_ref: float64 for
pinning against the reference's float64 run, float32 as a yardstick and for the exact edge values of the confidence weight.
The sums are numpy's, not the kernels' orders: apart from those edge values nothing here is compared bit for bit with the GPU.
Nothing here touches a GPU.

A case is chart_deform_ref's namespace (n, H, W, cams, d0, levels, denc, coords, weights, biases, radii)."""
from types import SimpleNamespace

import numpy as np

import chart_align_ref
import chart_deform_ref as cd
import chart_match_ref

TERM_NAMES = ("loss", "depth_loss", "grad", "hess", "normal", "curv", "matching", "ce_norm", "de_tv")


# ---- confidence ----------------------------------------------------------------------------------------------------------------
def confidence(raw, T=np.float64):
    """(conf, w): conf = 1 + exp(raw); w = 1 - exp(-(cw cw) / 2) with cw = conf - 1, taken from the ROUNDED conf"""
    raw = np.asarray(raw, T)
    conf = T(1) + np.exp(raw)
    cw = conf - T(1)
    return conf, T(1) - np.exp(-(cw * cw) / T(2))


def confidence_backward(raw, g, T=np.float64):
    return np.asarray(g, T) * np.exp(np.asarray(raw, T))


# ---- the weighted deformation and the two regularisers ----------------------------------------------------------------------------
def forward(c, w=None, T=np.float64):
    """chart_deform_ref.forward with the chart encoding of pixel p multiplied by w[i][p] before the depth encoding is added;
    also enc [n,N,E] (unweighted, without the depth encoding) and r [n,N], its norm."""
    n, N = c.n, c.H * c.W
    enc = []
    for lv in c.levels:
        v = lv.astype(T)
        s = 0
        for ys, xs, wt in cd._pixel_taps(c, v.shape[2], v.shape[3], T):
            s = s + v[:, :, ys, xs] * wt
        enc.append(s)
    enc = np.concatenate(enc, axis=1).reshape(n, -1, N).transpose(0, 2, 1)  # [n,N,E]
    x = enc if w is None else enc * np.asarray(w, T).reshape(n, N, 1)
    dt = None
    if c.denc is not None:
        b0, b1, w0, w1 = cd.taps(T(-1) + T(2) * c.coords.astype(T), c.denc.shape[2], T)
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
    s = cd.ray_scale(c, T)
    d0 = c.d0.astype(T)
    depths = np.where(d0 == 0, d0, d0 + delta * s)
    return SimpleNamespace(delta=delta, depths=depths, acts=acts, scale=np.where(d0 == 0, T(0), s), denc_taps=dt, enc=enc,
                           r=np.sqrt((enc * enc).sum(axis=-1)))


def regularizers(c, f, norm=True, tv=True, T=np.float64):
    """[2]: the mean of r over all n N pixels; the mean of |q[b+1] - q[b]| over n E (B - 1).  A term not asked for is 0."""
    out = np.zeros(2, T)
    if norm:
        out[0] = f.r.sum(dtype=T) / T(f.r.size)
    if tv:
        q = c.denc.astype(T)
        d = np.abs(q[..., 1:] - q[..., :-1])
        out[1] = d.sum(dtype=T) / T(d.size)
    return out


def gradients(c, g, greg=(0.0, 0.0), w=None, norm=False, tv=False, T=np.float64, chain=False):
    """The gradient of sum(g * depths) + greg[0] norm + greg[1] tv to every parameter, as chart_deform_ref.gradients gives it.
    chain: the bias gradients, plain sums of dz over a chart's pixels, are added one pixel after the other in T (np.cumsum) and
    not by numpy's pairwise sum: in float32 the other natural order of that sum, and the less accurate one.
    The levels take w(p) dL/dx_e(p) + greg[0] enc_e(p) / (r(p) n N) (0 where r = 0); the depth encoding takes the unweighted
    dL/dx and the total variation's sign(q[b] - q[b-1]) - sign(q[b+1] - q[b]) times greg[1] / (n E (B - 1))."""
    f = forward(c, w, T)
    n, N = c.n, c.H * c.W
    gz = ((np.asarray(g, T) * f.scale) * T(c.deformation_radius)).reshape(n, N, 1)
    dW, dB = [None] * len(c.weights), [None] * len(c.weights)
    for j in range(len(c.weights) - 1, -1, -1):
        a = f.acts[j]
        dW[j] = np.matmul(gz.transpose(0, 2, 1), a)
        dB[j] = np.cumsum(gz, axis=1, dtype=T)[:, -1] if chain else gz.sum(axis=1)
        da = np.matmul(gz, c.weights[j].astype(T))
        gz = np.where(a > 0, da, T(0)) if j > 0 else da
    dx = gz / T(c.scene_radius)  # [n,N,E]
    denc_in = dx if w is None else dx * np.asarray(w, T).reshape(n, N, 1)
    if norm:
        with np.errstate(all="ignore"):
            coef = np.where(f.r > 0, (T(greg[0]) / f.r) / T(n * N), T(0))
        denc_in = denc_in + f.enc * coef[..., None]
    dlevels, at = [], 0
    for lv in c.levels:
        _n, C, h, wd = lv.shape
        d = denc_in[:, :, at:at + C].transpose(0, 2, 1).reshape(n, C, c.H, c.W)
        at += C
        out = np.zeros(lv.shape, T)
        for ys, xs, wt in cd._pixel_taps(c, h, wd, T):
            np.add.at(out, (slice(None), slice(None), ys, xs), d * wt)
        dlevels.append(out)
    ddenc = None
    if c.denc is not None:
        b0, b1, w0, w1 = f.denc_taps
        ddenc = np.zeros(c.denc.shape, T)
        rows, chans = np.arange(n)[:, None, None], np.arange(c.denc.shape[1])[None, None, :]
        np.add.at(ddenc, (rows, chans, b0[..., None]), dx * w0[..., None])
        np.add.at(ddenc, (rows, chans, b1[..., None]), dx * w1[..., None])
        if tv:
            q = c.denc.astype(T)
            s = np.sign(q[..., 1:] - q[..., :-1])
            t = np.zeros(q.shape, T)
            t[..., 1:] += s
            t[..., :-1] -= s
            ddenc = ddenc + t * (T(greg[1]) / T(s.size))
    return dict(levels=dlevels, denc=ddenc, weights=dW, biases=dB)


def settle(c, w):
    """chart_deform_ref.settle for the unweighted AND the weighted network"""
    for attempt in range(400):
        worst, smallest, offenders = 0.0, np.inf, []
        for wt in (None, w):
            pre = {}
            for T in (np.float64, np.float32):
                a = forward(c, wt, T).acts
                pre[T] = [np.matmul(a[j], c.weights[j].astype(T).transpose(0, 2, 1)) + c.biases[j].astype(T)[:, None, :]
                          for j in range(len(c.weights) - 1)]
            err = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(pre[np.float32], pre[np.float64]))
            worst = max(worst, err)
            smallest = min(smallest, min(np.abs(b).min() for b in pre[np.float64]))
            offenders.append((err, pre[np.float64]))
        if smallest > 8 * worst:
            print(f"settled: smallest |pre-activation| {smallest:.3e}, float32 error {worst:.3e}, after {attempt} rounds")
            return c
        for _err, z64 in offenders:
            for j, b in enumerate(z64):
                charts, _pix, units = np.nonzero(np.abs(b) <= 8 * worst)
                for i, u in set(zip(charts.tolist(), units.tolist())):
                    c.biases[j][i, u] += np.float32(cd.NUDGE)
    raise AssertionError("pre-activations within 8 float32 errors of zero remain")



# ---- the driver ------------------------------------------------------------------------------------------------------------------
def total_loss(terms, reg, matching, weights, hessian=None):
    """The reference's weighted sum in its order (parallel_aligner.py:757-819); a weight of None switches a term off"""
    loss = terms[0]
    for key, value in (("gradient", terms[1]), ("hessian", hessian), ("normal", terms[2]), ("curvature", terms[3]),
                       ("matching", matching), ("norm", reg[0]), ("tv", reg[1])):
        if weights.get(key) is not None:
            loss = loss + weights[key] * value
    return loss


def hessian_term(depths, prior, T=np.float64):
    """The hessian term pixel by pixel, from the 3 x 3 window's entries and not from difference arrays: over every chart and
    every (i, j) with i < H-2, j < W-2 the four second differences of e = depths - prior,
        e(i+2,j) - 2 e(i+1,j) + e(i,j),   e(i,j+2) - 2 e(i,j+1) + e(i,j),   and twice   e(i+1,j+1) - e(i+1,j) - e(i,j+1) + e(i,j),
    in absolute value, averaged over all 4 n (H-2) (W-2) of them.  Returns (value, its gradient to depths)."""
    e = np.asarray(depths, T) - np.asarray(prior, T)
    n, H, W = e.shape
    count = 4 * n * (H - 2) * (W - 2)
    total, grad = T(0), np.zeros_like(e)
    stencils = (((2, 0, 1.0), (1, 0, -2.0), (0, 0, 1.0)), ((0, 2, 1.0), (0, 1, -2.0), (0, 0, 1.0)),
                ((1, 1, 1.0), (1, 0, -1.0), (0, 1, -1.0), (0, 0, 1.0)), ((1, 1, 1.0), (1, 0, -1.0), (0, 1, -1.0), (0, 0, 1.0)))
    for k in range(n):
        for i in range(H - 2):
            for j in range(W - 2):
                for stencil in stencils:
                    s = sum(T(c) * e[k, i + di, j + dj] for di, dj, c in stencil)
                    total += abs(s)
                    for di, dj, c in stencil:
                        grad[k, i + di, j + dj] += T(c) * np.sign(s) / T(count)
    return total / T(count), grad


def adam_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """torch.optim.Adam's rule at step t (1-based), in the arrays' type: returns (p, m, v)"""
    T = p.dtype.type
    m = T(beta1) * m + T(1 - beta1) * g
    v = T(beta2) * v + T(1 - beta2) * (g * g)
    step_size = T(lr / (1 - beta1 ** t))
    denom = np.sqrt(v) / T(np.sqrt(1 - beta2 ** t)) + T(eps)
    return p - step_size * (m / denom), m, v


def group_names(c, confidence=True):
    """The reference's trainable parameter groups in prepare_for_optimization's order"""
    names = cd.parameter_names(c)
    head = [k for k in names if k.endswith("encodings")]
    return head + (["_confidence"] if confidence else []) + [k for k in names if not k.endswith("encodings")]


def group_learning_rates(names, encodings_lr=1e-2, mlp_lr=1e-3, confidence_lr=1e-3):
    return [encodings_lr if k.endswith("encodings") else (confidence_lr if k == "_confidence" else mlp_lr) for k in names]


def updates_learning_rate(name):
    return name.endswith("encodings") or name.startswith("deformation")


def set_parameters(c, params):
    """The case with the named parameters (chart_deform_ref.parameter_names) taken from `params`"""
    names = cd.parameter_names(c)
    L, NL = len(c.levels), len(c.weights)
    c.levels = [params[k] for k in names[:L]]
    at = L
    if c.denc is not None:
        c.denc = params[names[at]]
        at += 1
    c.weights = [params[names[at + 2 * j]] for j in range(NL)]
    c.biases = [params[names[at + 2 * j + 1]] for j in range(NL)]
    return c


def optimize(c, params, raw, reference, n_iterations, weights, weighted, matching_thr=None, lr_update_iters=(), lr_update_factor=0.1,
             matching_update_iters=(), encodings_lr=1e-2, mlp_lr=1e-3, confidence_lr=1e-3, lam=0.2, T=np.float64):
    """ParallelAligner.optimize in numpy from the parameters `params` (name -> array) and the raw confidence `raw`, with a
    learnable confidence and depth maps as reference.  weights: total_loss's mapping (None: term off).  Returns
    (params, raw, losses of every iteration, the term vectors of every iteration)."""
    c = SimpleNamespace(**vars(c))
    params = {k: np.asarray(v, T).copy() for k, v in params.items()}
    raw = np.asarray(raw, T).copy()
    names = group_names(c)
    lrs = dict(zip(names, group_learning_rates(names, encodings_lr, mlp_lr, confidence_lr)))
    state = {k: (np.zeros_like(raw if k == "_confidence" else params[k]), np.zeros_like(raw if k == "_confidence" else params[k]))
             for k in names}
    reference = np.asarray(reference, T)
    d0 = c.d0.astype(T)
    nu0 = chart_align_ref.normals(c.cams, d0, T)
    curv0 = chart_align_ref.curvatures(nu0)
    flags = ((chart_align_ref.GRADIENT if weights.get("gradient") is not None else 0)
             | (chart_align_ref.NORMAL if weights.get("normal") is not None else 0)
             | (chart_align_ref.CURVATURE if weights.get("curvature") is not None else 0))
    use_norm, use_tv, use_match = (weights.get(k) is not None for k in ("norm", "tv", "matching"))
    matches = None
    if use_match:
        matches = chart_match_ref.match(c.cams, reference, matching_thr, T)[0]
    losses, vectors = [], []
    for i in range(n_iterations):
        if i in lr_update_iters:
            for k in names:
                if updates_learning_rate(k):
                    lrs[k] = lrs[k] * lr_update_factor
        set_parameters(c, params)
        conf, w = confidence(raw, T)
        w = w if weighted else None
        f = forward(c, w, T)
        reg = regularizers(c, f, use_norm, use_tv, T)
        args = (c.cams, f.depths, reference, d0, nu0, curv0)
        terms = chart_align_ref.evaluate(*args, confidence=conf, lam=lam, flags=flags, ftype=T).means
        cot = (1.0, weights.get("gradient") or 0.0, weights.get("normal") or 0.0, weights.get("curvature") or 0.0)
        gd, dconf = chart_align_ref.gradients(*args, confidence=conf, lam=lam, flags=flags, cotangents=cot, ftype=T)
        matching = None
        if use_match:
            matching = chart_match_ref.loss(c.cams, f.depths, matches, ftype=T)
            gd = gd + chart_match_ref.loss_grad(c.cams, f.depths, matches, cotangent=weights["matching"], ftype=T)
        loss = total_loss(terms, reg, matching, weights)
        losses.append(float(loss))
        vectors.append([float(loss), float(terms[0]), float(terms[1]), 0.0, float(terms[2]), float(terms[3]),
                        0.0 if matching is None else float(matching), float(reg[0]), float(reg[1])])
        grads = cd.flat_gradients(c, gradients(c, gd, (weights.get("norm") or 0.0, weights.get("tv") or 0.0), w, use_norm, use_tv, T))
        grads["_confidence"] = confidence_backward(raw, dconf, T)
        for k in names:
            m, v = state[k]
            if k == "_confidence":
                raw, m, v = adam_step(raw, grads[k], m, v, i + 1, lrs[k])
            else:
                params[k], m, v = adam_step(params[k], grads[k], m, v, i + 1, lrs[k])
            state[k] = (m, v)
        if use_match and i in matching_update_iters:
            matches = chart_match_ref.match(c.cams, f.depths, matching_thr, T)[0]
    return params, raw, losses, vectors


# ---- the golden file (tests/golden/chart_aligner.npz, make_golden_chart_aligner.py) ----------------------------------------------
ALIGNER_SHAPE = (3, 33, 50, (0.05, 0.1, 0.2, 0.4), 8, 32, 3, 16)  # chart_deform_ref.CASES' form: layer size 32 and 16 bins keep the file small
# variant: encoding weights, which cotangent, norm, total variation
VARIANTS = {"all": (True, 1, True, True), "norm": (False, 0, True, False), "tv": (False, 0, False, True),
            "weights": (True, 1, False, False), "plain": (False, 0, False, False)}
# the keywords of optimize that a configuration's `alignment:` block sets for the golden runs
OPTIMIZE_KEYS = ("use_gradient_loss", "use_hessian_loss", "use_normal_loss", "use_curvature_loss", "use_matching_loss",
                 "use_confidence_in_matching_loss", "gradient_loss_weight", "hessian_loss_weight", "normal_loss_weight",
                 "curvature_loss_weight", "matching_loss_weight", "encodings_lr", "mlp_lr", "confidence_lr", "regularize_chart_encodings_norms",
                 "chart_encodings_norm_loss_weight", "use_total_variation_on_depth_encodings", "total_variation_on_depth_encodings_weight")


def _case(g, d0, coords, params):
    n, H, W, res, C, S, NL, B = ALIGNER_SHAPE
    cams = [SimpleNamespace(world_view_transform=w, projection_matrix=p, full_proj_transform=f, image_width=W, image_height=H)
            for w, p, f in zip(g["a_wvt"], g["a_proj"], g["a_full"])]
    radii = g["a_radii"]
    c = SimpleNamespace(name="aligner", n=n, H=H, W=W, cams=cams, d0=d0, levels=[None] * len(res), denc=np.zeros((n, C * len(res), B), np.float32),
                        coords=coords, weights=[None] * NL, biases=[None] * NL, scene_radius=float(radii[0]),
                        deformation_radius=float(radii[1]), multi_res=True, resolutions=res, channels=C, layer_size=S, layers=NL, bins=B,
                        extent=float(radii[2]))
    return set_parameters(c, params)


def load_state(g):
    """Golden (a): the case with raw, cotangents, greg and, per variant, the float64 record and the float32 yardsticks"""
    names = [str(s) for s in g["a_names"]]
    L = len(ALIGNER_SHAPE[3])
    params = {k: g[f"a_level{i}"] for i, k in enumerate(names[:L])}
    params[names[L]] = g["a_denc"]
    for j in range(ALIGNER_SHAPE[6]):
        params[names[L + 1 + 2 * j]], params[names[L + 2 + 2 * j]] = g[f"a_weight{j}"], g[f"a_bias{j}"]
    c = _case(g, g["a_d0"], g["a_depth_coords"], params)
    assert cd.parameter_names(c) == names
    c.raw, c.cotangents, c.greg, c.conf64 = g["a_raw"], g["a_cotangents"], g["a_greg"], g["a_conf64"]
    pieces = {v: [g[f"a_{v}_grad64_{i}"] for i in range(len(names))] for v in ("plain", "weights")}
    c.variants = {}
    for variant, (weighted, k, norm, tv) in VARIANTS.items():
        grads = list(pieces["weights" if weighted else "plain"])
        if norm:
            for l in range(L):
                grads[l] = grads[l] + c.greg[0] * g[f"a_dnorm64_{l}"]
        if tv:
            grads[L] = grads[L] + c.greg[1] * g["a_dtv64"]
        yard, gyard = g[f"a_{variant}_yard"], g[f"a_{variant}_grad_yard"]
        c.variants[variant] = SimpleNamespace(
            weighted=weighted, cotangent=c.cotangents[k], norm=norm, tv=tv, greg=(c.greg[0] if norm else 0.0, c.greg[1] if tv else 0.0),
            depths64=g["a_weights_depths64" if weighted else "a_plain_depths64"], reg64=g["a_reg64"] * np.array([norm, tv], np.float64),
            grads64=dict(zip(names, grads)), yard=SimpleNamespace(depths=float(yard[0]), reg=(float(yard[1]), float(yard[2])), conf=float(yard[3])),
            grad_yard=dict(zip(names, gyard[:-1])))
    return c


def load_runs(g):
    """Golden (b): the scene, the recorded initial parameters, the options and per configuration the reference's curves, end
    parameters and groups"""
    import json
    names = [str(s) for s in g["b_names"]]
    init = {k: g[f"b_init_{i}"] for i, k in enumerate(names)}
    c = _case(g, g["b_d0"], g["b_depth_coords"], init)
    c.reference, c.init, c.init_confidence = g["b_reference"], init, g["b_init_confidence"]
    c.options, c.matching_thr = json.loads(str(g["b_options"])), float(g["b_matching_thr"])
    c.configs = json.loads(str(g["configs"]))
    c.runs = {}
    for flavour in ("strong", "default"):
        key = lambda k: g[f"b_{flavour}_{k}"]  # noqa: E731
        c.runs[flavour] = SimpleNamespace(
            losses32=key("losses32"), losses64=key("losses64"), end64={k: key(f"end64_{i}") for i, k in enumerate(names)},
            end_confidence64=key("end_confidence64"), group_names=[str(s) for s in key("group_names")], group_lrs=key("group_lrs"),
            group_trainable=key("group_trainable"), end_lrs=key("end_lrs"),
            group_names_trainable=[str(s) for s, t in zip(key("group_names"), key("group_trainable")) if t])
    return c


def weights_of(cfg):
    """total_loss's mapping from a configuration's `alignment:` block"""
    pick = lambda flag, weight: float(cfg[weight]) if cfg[flag] else None  # noqa: E731
    return {"gradient": pick("use_gradient_loss", "gradient_loss_weight"), "hessian": pick("use_hessian_loss", "hessian_loss_weight"),
            "normal": pick("use_normal_loss", "normal_loss_weight"), "curvature": pick("use_curvature_loss", "curvature_loss_weight"),
            "matching": pick("use_matching_loss", "matching_loss_weight"),
            "norm": pick("regularize_chart_encodings_norms", "chart_encodings_norm_loss_weight"),
            "tv": pick("use_total_variation_on_depth_encodings", "total_variation_on_depth_encodings_weight")}
