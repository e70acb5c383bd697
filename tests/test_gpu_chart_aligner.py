"""The chart aligner on the device (include/g4s_losses.h "Chart alignment: confidence, weighted encodings, encoding
regularisers": g4s_chart_confidence_*, g4s_chart_deform_reg_*; g4splat_amd/chart_aligner.py) against the reference's own float64
run (tests/golden/chart_aligner.npz, make_golden_chart_aligner.py), against the float64 restatement (tests/chart_aligner_ref.py)
for generated cases, and against itself where bits are claimed.

Measured quantities follow the rule of test_gpu_chart_deform.py: the yardstick is the largest error of the reference's float32
run against its float64 run (for a generated case the float32 restatement against the float64 one); the GPU may be off the
float64 record by at most 4 yardsticks, with a floor of one float32 ulp of the largest entry.  Every run prints the figures.

Shapes: 1 x 3 x 3 with a 1 x 1 level; 3 x 33 x 50, the golden; 2 x 65 x 70 (N = 4550: two workgroups per chart, a last tile of 6
pixels); 2 depth bins.

Measured on an MI355X, the worst error as a share of its limit: golden state, weights with both terms 0.91 and weights only 0.91
(both the second layer's bias: error 2.0e-7 of the largest entry, yardstick 5.5e-8, floor 7.0e-8), norm alone 0.35, total
variation alone 0.35, confidence 0.27; generated cases: 1 x 3 x 3 0.58 (the depths), two bins 0.42, 2 x 65 x 70 0.31 (0.31 to 0.43
over four seeds).  Convergence on the golden's scene: strong 1.4038 -> 0.9043 at iteration 25 -> 0.6025 at the end (the
reference's float32 and float64 runs: 0.8946 and 0.8894 at 25, 0.5826 and 0.5694 at the end; bound 0.8946); default 1.4030 ->
0.5122 -> 0.3520 (0.4894 and 0.4989 at 25, 0.3483 and 0.3507 at the end; bound 0.4989).  The first loss equals the reference's
float32 one to all printed digits.  The public surface (align_charts, verts, outputs, charts_data.npz): verts 1.1e-7 to 1.3e-7 of
the largest coordinate off o + d dir in float64 (limit 4 ulp of it, 4.8e-7); the hessian term 4.1517185e-05 within 6.5e-14 of
the float64 restatement (limit 16 ulp of the value, 5.8e-11)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chart_aligner_ref as ref
import chart_deform_ref as cd
from g4splat_amd import _lib, chart_align, chart_aligner, chart_deform, chart_match
from g4splat_amd.optim import FusedAdam
from support import DEV, GOLDEN, dev, host, same_bits, twice
from test_chart_deform_cpu import module_of

pytestmark = pytest.mark.gpu
MARGIN = 4.0


@pytest.fixture(scope="module")
def golden(hip_lib):
    return np.load(os.path.join(GOLDEN, "chart_aligner.npz"))


@pytest.fixture(scope="module")
def state(golden):
    return ref.load_state(golden)


@pytest.fixture(scope="module")
def runs(golden):
    return ref.load_runs(golden)


def generated(name, seed, shape):
    c = cd.make_case(name, seed, shape)
    if c.bins:
        c.coords = cd.depth_coordinates(c.d0, c.bins)
    rng = np.random.default_rng(seed)
    c.raw = rng.uniform(-2, 2, c.d0.shape).astype(np.float32)
    c.cotangent = rng.uniform(-1, 1, c.d0.shape).astype(np.float32)
    return c


@pytest.fixture(scope="module")
def edges(hip_lib):
    c = generated("edges", 23, (2, 65, 70, (0.05, 0.1, 0.2, 0.4), 8, 64, 3, 30))
    assert c.H * c.W == 4550 and -(-c.H * c.W // chart_deform.WORKGROUP_PIXELS) == 2 and (c.H * c.W) % chart_deform.TILE_PIXELS == 6
    return c


def loaded(c, **more):
    m = module_of(c, device=DEV, **more)
    m.load_reference_state_dict({k: torch.from_numpy(v) for k, v in cd.parameters(c).items()})
    if c.bins:
        same_bits(m.depth_coords, c.coords.reshape(c.n, -1), f"{c.name}: depth_coords")
    return m


def run_plain(m, cotangent):
    m.zero_grad(set_to_none=True)
    d = m.deformed_depths()
    (d * dev(cotangent)).sum().backward()
    return host(d), {k: host(p.grad) for k, p in m.named_parameters()}


def run_reg(m, cotangent, greg=(0.0, 0.0), w=None, norm=False, tv=False):
    """(depths, reg, {name: gradient}) on the host for sum(cotangent * depths) + greg . reg"""
    m.zero_grad(set_to_none=True)
    d, reg = m.deformed_depths_and_regularizers(None if w is None else (w if isinstance(w, torch.Tensor) else dev(w)), norm=norm, tv=tv)
    assert d.shape == (m.n, m.height, m.width) and d.dtype == torch.float32 and reg.shape == (2,) and reg.dtype == torch.float32
    ((d * dev(cotangent)).sum() + (reg * dev(np.asarray(greg, np.float32))).sum()).backward()
    return host(d), host(reg), {k: host(p.grad) for k, p in m.named_parameters()}


def within_yardstick(label, got, want64, yard_abs):
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert got.shape == want64.shape, (label, got.shape, want64.shape)
    top = np.abs(want64).max()
    if top == 0:
        assert not got.any(), label
        return
    err, yard, floor = np.abs(got - want64).max() / top, float(yard_abs) / top, float(np.spacing(np.float32(top))) / top
    print(f"{label}: error {err:.3e}, yardstick {yard:.3e}, floor {floor:.3e}")
    assert err <= max(MARGIN * yard, floor), (label, err, yard, floor)


def device_weights(raw):
    """(confidence, weights) of the confidence kernel for a raw map on the host"""
    conf, w = chart_aligner.confidence_and_weights(dev(raw), True)
    return conf, w


# ---- 1. the plain path is unchanged ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edges", "golden"])
def test_no_weights_and_no_terms_is_the_plain_pair_bit_for_bit(edges, state, which):
    c = edges if which == "edges" else state
    g = c.cotangent if which == "edges" else c.cotangents[0]
    m = loaded(c)
    depths, grads = run_plain(m, g)
    got_d, got_reg, got_g = run_reg(m, g)
    same_bits(got_d, depths, "depths")
    assert not got_reg.any()
    assert set(got_g) == set(grads)
    for k in grads:
        same_bits(got_g[k], grads[k], f"d/d{k}")
    # delta, which the Python surface does not return: the entry point itself
    p = [t.detach() for t in m._params()]
    out, delta = torch.empty((c.n, c.H, c.W), device=DEV), torch.empty((c.n, c.H, c.W), device=DEV)
    null = ctypes.c_void_p(0)
    _lib.call("g4s_chart_deform_reg_forward", *m._call_head(p), null, 0, _lib.ptr(out), _lib.ptr(delta), null, null, 0, _lib.stream(DEV))
    torch.cuda.synchronize(DEV)
    same_bits(out, depths, "depths through the entry point")
    same_bits(delta, m.deformations(), "delta")


# ---- 2. golden (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["all", "norm", "tv", "weights"])
def test_golden_state_within_the_references_own_error(state, variant):
    c, v = state, state.variants[variant]
    m = loaded(c)
    conf, w = device_weights(c.raw)
    within_yardstick("confidence", host(conf), c.conf64, v.yard.conf)
    depths, reg, grads = run_reg(m, v.cotangent, v.greg, w if v.weighted else None, v.norm, v.tv)
    within_yardstick(f"{variant} depths", depths, v.depths64, v.yard.depths)
    for i, on in enumerate((v.norm, v.tv)):
        if on:
            within_yardstick(f"{variant} reg[{i}]", reg[i:i + 1], v.reg64[i:i + 1], v.yard.reg[i])
        else:
            assert reg[i] == 0
    assert set(grads) == set(v.grads64)
    for k, want in v.grads64.items():
        assert grads[k].dtype == np.float32 and grads[k].any(), k
        within_yardstick(f"{variant} d/d{k}", grads[k], want, v.grad_yard[k])


def check_generated(c, weighted, norm, tv, greg=(0.7, 1.3)):
    """A generated case against the float64 restatement, the float32 restatement as the yardstick"""
    w32 = ref.confidence(c.raw, np.float32)[1] if weighted else None
    c = ref.settle(c, w32) if weighted else cd.settle(c)  # every ReLU decided alike in float32 and float64
    m = loaded(c)
    w = device_weights(c.raw)[1] if weighted else None
    if weighted:
        assert np.abs(host(w).astype(np.float64) - w32).max() <= 4 * np.spacing(np.float32(1))
    depths, reg, grads = run_reg(m, c.cotangent, greg, w, norm, tv)
    wh = host(w) if weighted else None  # the restatements read the device's weights: they are an input here
    r = {}
    for T in (np.float32, np.float64):
        f = ref.forward(c, wh, T)
        r[T] = (f.depths, ref.regularizers(c, f, norm, tv, T), cd.flat_gradients(c, ref.gradients(c, c.cotangent, greg, wh, norm, tv, T)))
    worst = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max())  # noqa: E731
    within_yardstick(f"{c.name} depths", depths, r[np.float64][0], worst(r[np.float32][0], r[np.float64][0]))
    for i in range(2):
        within_yardstick(f"{c.name} reg[{i}]", reg[i:i + 1], r[np.float64][1][i:i + 1], abs(float(r[np.float32][1][i]) - r[np.float64][1][i]))
    # a bias gradient is a plain sum of dz over a chart's pixels: numpy adds it pairwise, which in float32 is several times more
    # accurate than any chain and no measure of one; its yardstick is the larger error of the two float32 orders, pairwise and
    # one pixel after the other (the kernel's three levels -- 64 pixels, 64 tiles, the workgroups -- lie between them)
    chained = cd.flat_gradients(c, ref.gradients(c, c.cotangent, greg, wh, norm, tv, np.float32, chain=True))
    for k, want in r[np.float64][2].items():
        yard = worst(r[np.float32][2][k], want)
        if k.endswith("bias"):
            yard = max(yard, worst(chained[k], want))
        within_yardstick(f"{c.name} d/d{k}", grads[k], want, yard)
    assert np.isfinite(reg).all()
    return m


def test_two_workgroups_per_chart_and_a_partial_tile(edges):
    check_generated(edges, True, True, True)


def test_one_by_one_level(hip_lib):
    check_generated(generated("one", 31, cd.CASES["one"]), True, True, True)


def test_two_depth_bins(hip_lib):
    c = generated("two_bins", 37, (2, 9, 11, (0.25, 0.5, 0.75, 1.0), 4, 32, 2, 2))
    check_generated(c, True, True, True)


# ---- 3. regulariser cotangent only ------------------------------------------------------------------------------------------------
def test_norm_cotangent_alone_reaches_only_the_levels(edges):
    m = loaded(edges)
    _d, _reg, grads = run_reg(m, np.zeros_like(edges.cotangent), (1.0, 0.0), device_weights(edges.raw)[1], norm=True)
    for k, g in grads.items():
        if k.startswith("charts_encoding"):
            assert g.any() and np.isfinite(g).all(), k
        else:
            assert not g.any(), k
    _d, _reg, grads = run_reg(m, np.zeros_like(edges.cotangent), (0.0, 1.0), None, tv=True)
    for k, g in grads.items():
        assert bool(g.any()) == (k == "depth_encoding.encodings"), k


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------
def test_weight_zero_weight_one_and_zero_levels(edges):
    c = SimpleNamespace(**vars(edges))
    raw = c.raw.copy()
    raw[0], raw[1] = -60.0, 5.0
    conf, w = device_weights(raw)
    same_bits(host(w)[0], np.zeros_like(raw[0]), "raw = -60 gives w = 0")
    same_bits(host(w)[1], np.ones_like(raw[1]), "raw = 5 gives w = 1")
    same_bits(host(conf)[0], np.ones_like(raw[0]), "raw = -60 gives confidence 1")
    m = loaded(c)
    depths, _reg, grads = run_reg(m, c.cotangent, (0.0, 0.0), w)
    plain_d, plain_g = run_plain(m, c.cotangent)
    for k, g in grads.items():
        if k.startswith("charts_encoding"):
            assert not g[0].any(), f"w = 0: {k} of chart 0 gets nothing from the depth path"
        same_bits(g[1], plain_g[k][1], f"w = 1: d/d{k} of chart 1 as unweighted")
    assert grads["depth_encoding.encodings"][0].any()
    same_bits(depths[1], plain_d[1], "w = 1: depths of chart 1 as unweighted")
    assert not np.array_equal(depths[0], plain_d[0])
    # a chart whose levels are all zero: r = 0 everywhere, a zero norm gradient and no NaN
    z = SimpleNamespace(**vars(edges))
    z.name, z.levels = "zero-levels", [v.copy() for v in edges.levels]
    for v in z.levels:
        v[0] = 0.0
    mz = loaded(z)
    dz, regz, gz = run_reg(mz, np.zeros_like(z.cotangent), (1.0, 1.0), w, norm=True, tv=True)
    assert np.isfinite(dz).all() and np.isfinite(regz).all() and all(np.isfinite(g).all() for g in gz.values())
    for k, g in gz.items():
        if k.startswith("charts_encoding"):
            assert not g[0].any() and g[1].any(), k
    # the mean over all pixels of a chart of norm 0 and one of norm r: half the second chart's own mean
    f = ref.forward(z, None, np.float64)
    within_yardstick("norm with a zero chart", regz[:1], np.array([f.r.mean()]), abs(float(ref.forward(z, None, np.float32).r.mean(dtype=np.float64)) - f.r.mean()))


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------
def test_bit_identical_from_run_to_run(edges):
    m = loaded(edges)
    w = device_weights(edges.raw)[1]

    def once():
        d, reg, grads = run_reg(m, edges.cotangent, (0.7, 1.3), w, True, True)
        return [d, reg] + [grads[k] for k in sorted(grads)]

    twice(once)


# ---- 6. each chart reads its own weights ------------------------------------------------------------------------------------------
def test_permuting_the_weights_of_twin_charts_permutes_the_results(edges):
    t = SimpleNamespace(**vars(edges))
    both = lambda a: np.concatenate([a[:1], a[:1]])  # noqa: E731
    t.name, t.cams = "twins", [edges.cams[0], edges.cams[0]]
    t.d0, t.coords, t.denc = both(edges.d0), both(edges.coords), both(edges.denc)
    t.levels, t.weights, t.biases = [both(v) for v in edges.levels], [both(v) for v in edges.weights], [both(v) for v in edges.biases]
    m = loaded(t, spatial_extent_override=edges.extent)
    w = host(device_weights(edges.raw)[1])
    g = both(edges.cotangent)
    a = run_reg(m, g, (0.7, 1.3), w, True, True)
    b = run_reg(m, g, (0.7, 1.3), w[::-1].copy(), True, True)
    assert not np.array_equal(a[0][0], a[0][1])
    same_bits(b[0], a[0][::-1].copy(), "depths")
    for k in a[2]:
        same_bits(b[2][k], a[2][k][::-1].copy(), f"d/d{k}")


# ---- 7. the driver is the composition of the public pieces ---------------------------------------------------------------------
def aligner_of(c, flavour_cfg, **more):
    cdm = chart_deform
    E = c.channels * len(c.levels)
    return chart_aligner.ChartAligner(
        c.cams, dev(c.d0), charts_encoding_params=cdm.ChartsEncodingParams(encoding_dim=E),
        depth_encoding_params=cdm.DepthEncodingParams(encoding_dim=E, n_bins=c.bins),
        mlp_params=cdm.MLPParams(n_deformation_layers=c.layers, deformation_layer_size=c.layer_size),
        multi_res_charts_encoding_params=cdm.MultiResChartsEncodingParams(c.channels, c.resolutions),
        use_learnable_confidence=True, weight_encodings_with_confidence=flavour_cfg["weight_encodings_with_confidence"], **more)


def optimize_keywords(runs, flavour, **more):
    cfg = runs.configs[flavour]
    kw = {k: cfg[k] for k in ref.OPTIMIZE_KEYS}
    kw.update(runs.options)
    kw.update(matching_thr=runs.matching_thr, verbose=False)
    kw.update(more)
    return kw


def start_from_recorded(a, runs, kw):
    """prepare_for_optimization, then the golden's recorded initial parameters"""
    a.prepare_for_optimization(kw["encodings_lr"], kw["mlp_lr"], kw["lr_update_iters"], kw["lr_update_factor"], kw["confidence_lr"])
    a.deformation_module.load_reference_state_dict({k: torch.from_numpy(v) for k, v in runs.init.items()})
    with torch.no_grad():
        a._confidence.copy_(dev(runs.init_confidence))


def snapshot(a):
    out = [host(p) for _k, p in sorted(a.named_parameters())]
    for _k, p in sorted(a.named_parameters()):
        st = a.optimizer.state[p]
        out += [host(st["exp_avg"]), host(st["exp_avg_sq"]), host(st["step"])]
    return out


def test_one_eager_iteration_is_the_hand_composition(runs):
    cfg = runs.configs["strong"]
    kw = optimize_keywords(runs, "strong", n_iterations=1, lr_update_iters=[], matching_update_iters=None, graph=False, prepare=False)
    a = aligner_of(runs, cfg)
    start_from_recorded(a, runs, kw)
    a.optimize(dev(runs.reference), **kw)
    b = aligner_of(runs, cfg)
    start_from_recorded(b, runs, kw)
    assert isinstance(b.optimizer, FusedAdam) and [g["name"] for g in b.optimizer.param_groups] == runs.runs["strong"].group_names_trainable
    reference = dev(runs.reference)
    conf, w = chart_aligner.confidence_and_weights(b._confidence, True)
    depths, reg = b.deformation_module.deformed_depths_and_regularizers(w, norm=True, tv=True)
    losses = chart_align.AlignmentLosses(runs.cams, dev(runs.d0), 0.2)
    terms = losses.terms(depths, reference, conf, None, None, cfg["use_gradient_loss"], cfg["use_normal_loss"], cfg["use_curvature_loss"])
    matcher = chart_match.ChartMatcher(runs.cams, reference_depths=reference)
    matcher.match(runs.matching_thr)
    matching = matcher.loss(depths)
    loss = chart_aligner.total_loss(terms, reg, matching, ref.weights_of(cfg))
    loss.backward()
    b.optimizer.step()
    same_bits(snapshot(a), snapshot(b), "parameters and moments")
    logged = a.loss_terms[0]
    want = {"loss": loss, "depth_loss": terms[0], "normal": terms[2], "curv": terms[3], "matching": matching, "ce_norm": reg[0], "de_tv": reg[1]}
    assert set(logged) == set(want) and a.train_losses == [logged["loss"]]
    for k, v in want.items():
        assert logged[k] == float(v.detach()), k


# ---- 8. the graph ---------------------------------------------------------------------------------------------------------------------
def test_graph_and_eager_end_with_the_same_bits(runs):
    def run(graph):
        kw = optimize_keywords(runs, "strong", n_iterations=12, lr_update_iters=[5], matching_update_iters=[7], graph=graph, prepare=False)
        a = aligner_of(runs, runs.configs["strong"])
        start_from_recorded(a, runs, kw)
        a.optimize(dev(runs.reference), **kw)
        lrs = [g["lr"] for g in a.optimizer.param_groups]
        return a, snapshot(a) + [np.array(a.train_losses), np.array(lrs)]

    eager, e = run(False)
    first, g1 = run(True)
    _second, g2 = run(True)
    same_bits(g1, e, "graph against eager")
    same_bits(g2, g1, "two graph runs")
    assert first.graph_captures == 2 and eager.graph_captures == 0  # captured at the start and again after the matches' refresh
    assert len(first.train_losses) == 12 and all(np.isfinite(first.train_losses))
    for g in first.optimizer.param_groups:  # the confidence keeps its rate
        want = 1e-3 if g["name"] == "_confidence" else (1e-2 if g["name"].endswith("encodings") else 1e-3) * 0.5
        assert g["lr"] == pytest.approx(want, rel=1e-12), g["name"]


# ---- 9. convergence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["strong", "default"])
def test_fifty_iterations_fall_as_the_references_do(runs, flavour):
    """The golden's scene from its recorded initial parameters: the last logged loss is at most the larger of the reference's
    float32 and float64 losses at iteration 25 (the golden script asserts that the reference itself ends at most 0.8 of them)."""
    kw = optimize_keywords(runs, flavour, prepare=False)
    a = aligner_of(runs, runs.configs[flavour])
    start_from_recorded(a, runs, kw)
    losses = a.optimize(dev(runs.reference), **kw)
    r = runs.runs[flavour]
    bound = max(r.losses32[25], r.losses64[25])
    print(f"{flavour}: first {losses[0]:.6f} (reference {r.losses32[0]:.6f}), at 25 {losses[25]:.6f} ({r.losses32[25]:.6f}, "
          f"{r.losses64[25]:.6f}), last {losses[-1]:.6f} ({r.losses32[-1]:.6f}, {r.losses64[-1]:.6f}), bound {bound:.6f}")
    assert len(losses) == 50 and np.isfinite(losses).all() and all(np.isfinite(list(t.values())).all() for t in a.loss_terms)
    assert losses[-1] <= bound


# ---- 10. refusals before any launch ---------------------------------------------------------------------------------------------
def test_the_library_refuses_before_any_launch(hip_lib, state):
    m = loaded(state)
    p = [t.detach() for t in m._params()]
    head = list(m._call_head(p))
    out, reg = torch.empty((m.n, m.height, m.width), device=DEV), torch.empty(2, device=DEV)
    null, stream = ctypes.c_void_p(0), _lib.stream(DEV)
    one_bin = _lib.G4sChartDeformShape.from_buffer_copy(m._shape)
    one_bin.bins = 1
    assert hip_lib.g4s_chart_deform_reg_workspace(ctypes.byref(one_bin), chart_deform.REG_TV) == 0
    assert "at least 2 depth bins" in _lib.last_error()
    assert hip_lib.g4s_chart_deform_reg_workspace(ctypes.byref(one_bin), chart_deform.REG_NORM) > 0
    assert hip_lib.g4s_chart_deform_reg_workspace(ctypes.byref(m._shape), 4) == 0 and "bits 0" in _lib.last_error()
    with pytest.raises(RuntimeError, match="at least 2 depth bins"):
        _lib.call("g4s_chart_deform_reg_forward", ctypes.byref(one_bin), *head[1:], null, chart_deform.REG_TV, _lib.ptr(out), null,
                  _lib.ptr(reg), null, 0, stream)
    with pytest.raises(RuntimeError, match="NULL required pointer"):
        _lib.call("g4s_chart_deform_reg_forward", *head, null, 0, null, null, null, null, 0, stream)
    with pytest.raises(RuntimeError, match="NULL required pointer"):  # terms asked for and nowhere to put them
        _lib.call("g4s_chart_deform_reg_forward", *head, null, 3, _lib.ptr(out), null, null, null, 0, stream)
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call("g4s_chart_deform_reg_forward", *head, null, 1, _lib.ptr(out), null, _lib.ptr(reg), null, 0, stream)
    grads = [torch.empty_like(t) for t in p]
    lv, de, ws, bs = m._split(grads)
    tail = (_lib.ptrs(lv), _lib.ptr(de), _lib.ptrs(ws), _lib.ptrs(bs))
    short = torch.empty(m.reg_workspace_bytes(3) - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call("g4s_chart_deform_reg_backward", *head, null, 3, _lib.ptr(out), _lib.ptr(reg), *tail, _lib.ptr(short), short.numel(), stream)
    with pytest.raises(RuntimeError, match="NULL required pointer"):  # terms asked for and no cotangent for them
        _lib.call("g4s_chart_deform_reg_backward", *head, null, 3, _lib.ptr(out), null, *tail, null, 0, stream)
    assert m.reg_workspace_bytes(3) >= m.workspace_bytes + 4 * m.n * m.height * m.width
    # the forward asks for the norm's partial sums alone, not for the backward's dL/dx
    small = m.reg_workspace_bytes(1, forward=True)
    assert 0 < small < m.workspace_bytes and small == m.reg_workspace_bytes(3, forward=True)
    assert hip_lib.g4s_chart_deform_reg_forward_workspace(ctypes.byref(one_bin), chart_deform.REG_TV) == 0
    short = torch.empty(small - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call("g4s_chart_deform_reg_forward", *head, null, 1, _lib.ptr(out), null, _lib.ptr(reg), _lib.ptr(short), short.numel(), stream)
    with pytest.raises(RuntimeError, match="element count"):
        _lib.call("g4s_chart_confidence_forward", 0, _lib.ptr(out), _lib.ptr(out), null, stream)
    with pytest.raises(RuntimeError, match="NULL required pointer"):
        _lib.call("g4s_chart_confidence_backward", out.numel(), _lib.ptr(out), null, _lib.ptr(out), stream)
    with pytest.raises(ValueError, match="at least 2 depth bins"):
        loaded(generated("one_bin", 41, (1, 5, 6, (0.5, 1.0), 8, 32, 2, 1))).deformed_depths_and_regularizers(tv=True)


# ---- 11. the public surface: align_charts, verts, outputs, charts_data.npz -------------------------------------------------------
def points_of(cams, depths):
    """o + depth D (x, y, 1) in float64 from the views' ray records (chart_align_ref.ray_records) [n,H,W,3]"""
    import chart_align_ref
    n, H, W = depths.shape
    rec = chart_align_ref.ray_records(cams, W, H).astype(np.float64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([xx, yy, np.ones_like(xx)], -1)
    dirs = pix @ rec[:, 3:12].reshape(n, 1, 3, 3).transpose(0, 1, 3, 2)  # [n,H,W,3]
    return rec[:, None, None, 0:3] + depths.astype(np.float64)[..., None] * dirs


def check_points(label, cams, verts, depths):
    """A point is three float32 products and two sums for the direction, a product with the depth and a sum with the origin:
    at most 8 roundings of at most half an ulp of the largest coordinate each."""
    want = points_of(cams, host(depths))
    err, top = np.abs(host(verts).astype(np.float64) - want).max(), np.abs(want).max()
    print(f"{label}: error {err / top:.3e} of the largest coordinate")
    assert verts.shape == depths.shape + (3,) and err <= 4 * float(np.spacing(np.float32(top)))


def test_align_charts_strong_writes_what_the_initialiser_reads(runs, tmp_path):
    from g4splat_amd import chart_init
    cfg = dict(chart_aligner.ALIGNMENT_CONFIGS["strong"], n_iterations=2)
    out = chart_aligner.align_charts(runs.cams, dev(runs.d0), dev(runs.reference), scale_factor=2.0, charts_data_path=str(tmp_path),
                                     return_training_losses=True, **cfg)
    assert len(out) == 4
    verts, depths, confs, losses = out
    n, H, W = runs.d0.shape
    assert depths.shape == (n, H, W) and confs.shape == (n, H, W) and len(losses) == 2 and np.isfinite(losses).all()
    assert not (depths.requires_grad or verts.requires_grad or confs.requires_grad)
    assert not np.array_equal(host(depths), runs.d0) and bool((confs > 1).all())  # two steps moved the charts
    check_points("verts", runs.cams, verts, depths)
    data = np.load(os.path.join(str(tmp_path), "charts_data.npz"))
    assert set(data.files) == {"prior_depths", "depths", "pts", "confs", "scale_factor"} and float(data["scale_factor"]) == 2.0
    same_bits(data["prior_depths"], runs.d0, "prior_depths")
    same_bits(data["depths"], host(depths), "depths")
    same_bits(data["pts"], host(verts), "pts")
    same_bits(data["confs"], host(confs), "confs")
    charts = {"pts": dev(data["pts"]), "confs": dev(data["confs"]), "scale_factor": float(data["scale_factor"])}
    images = torch.rand((n, H, W, 3), device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    surfels = chart_init.get_gaussian_parameters_from_charts_data(charts, images)
    M = surfels["means"].shape[0]
    assert M > 0 and surfels["scales"].shape == (M, 3) and surfels["quaternions"].shape == (M, 4) and surfels["colors"].shape == (M, 3)
    means, pts = host(surfels["means"]).astype(np.float64), data["pts"].reshape(-1, 3).astype(np.float64) / 2.0
    assert all(np.isfinite(host(v)).all() for v in surfels.values())
    slack = 1e-5 * np.abs(pts).max()  # a surfel's centre lies among its face's vertices, which scale_factor divides
    assert (means >= pts.min(0) - slack).all() and (means <= pts.max(0) + slack).all()


def test_aligner_properties_at_the_recorded_parameters(runs):
    kw = optimize_keywords(runs, "strong")
    a = aligner_of(runs, runs.configs["strong"])
    start_from_recorded(a, runs, kw)
    conf, w = chart_aligner.confidence_and_weights(a._confidence, True)
    depths = a.deformation_module.deformed_depths_and_regularizers(w.detach())[0]
    same_bits(a.deformed_depths, depths, "deformed_depths")
    same_bits(a.confidence, conf, "confidence")
    check_points("verts", runs.cams, a.verts, a.deformed_depths)
    assert a.deformed_depths.requires_grad and a.verts.requires_grad and a.confidence.requires_grad
    verts, d, c = a.outputs()
    same_bits([verts, d, c], [a.verts.detach(), depths.detach(), conf.detach()], "outputs")
    assert not (verts.requires_grad or d.requires_grad or c.requires_grad)


def test_without_a_learnable_confidence(runs):
    cfg = dict(chart_aligner.ALIGNMENT_CONFIGS["default"], use_learnable_confidence=False, n_iterations=2)
    out = chart_aligner.align_charts(runs.cams, dev(runs.d0), dev(runs.reference), **cfg)
    assert len(out) == 2 and out[0].shape == runs.d0.shape + (3,) and out[1].shape == runs.d0.shape
    check_points("verts", runs.cams, *out)
    out = chart_aligner.align_charts(runs.cams, dev(runs.d0), dev(runs.reference), return_training_losses=True, graph=False, **cfg)
    assert len(out) == 3 and len(out[2]) == 2 and np.isfinite(out[2]).all()
    a = chart_aligner.ChartAligner(runs.cams, dev(runs.d0), use_learnable_confidence=False)
    assert "_confidence" not in dict(a.named_parameters())
    same_bits(a.outputs()[2], np.full(runs.d0.shape, 4.0, np.float32), "the confidences align_charts_in_parallel substitutes")
    with pytest.raises(ValueError, match="use_learnable_confidence"):
        a.optimize(dev(runs.reference), n_iterations=1, use_matching_loss=True, use_confidence_in_matching_loss=True)


def test_confidence_in_the_matching_loss(runs):
    def run(graph):
        kw = optimize_keywords(runs, "strong", n_iterations=4, lr_update_iters=[], matching_update_iters=None, graph=graph, prepare=False,
                               use_confidence_in_matching_loss=True)
        a = aligner_of(runs, runs.configs["strong"])
        start_from_recorded(a, runs, kw)
        a.optimize(dev(runs.reference), **kw)
        return a, snapshot(a) + [np.array(a.train_losses)]

    eager, e = run(False)
    _graphed, g = run(True)
    same_bits(g, e, "graph against eager")
    assert np.isfinite(eager.train_losses).all()
    # the bound handed to the matcher holds over the whole run, and is the start's largest confidence moved by every step
    top = float(eager.confidence.detach().max())
    start = 1.0 + float(np.exp(np.float64(runs.init_confidence.max())))
    assert top <= eager._options.weight_max <= start * float(np.exp(chart_aligner.ADAM_STEP_BOUND * 1e-3 * 4)) * (1 + 1e-6)
    # one iteration is the hand composition with the detached confidence as the matcher's weights
    kw = optimize_keywords(runs, "strong", n_iterations=1, lr_update_iters=[], matching_update_iters=None, graph=False, prepare=False,
                           use_confidence_in_matching_loss=True)
    a = aligner_of(runs, runs.configs["strong"])
    start_from_recorded(a, runs, kw)
    a.optimize(dev(runs.reference), **kw)
    b = aligner_of(runs, runs.configs["strong"])
    start_from_recorded(b, runs, kw)
    conf, w = chart_aligner.confidence_and_weights(b._confidence, True)
    depths = b.deformation_module.deformed_depths_and_regularizers(w, norm=True, tv=True)[0]
    matcher = chart_match.ChartMatcher(runs.cams, reference_depths=dev(runs.reference))
    matcher.match(runs.matching_thr)
    weighted = matcher.loss(depths, conf.detach(), a._options.weight_max)
    assert a.loss_terms[0]["matching"] == float(weighted) != float(matcher.loss(depths))


# ---- 12. the hessian term -------------------------------------------------------------------------------------------------------------
def test_hessian_term_in_the_iteration(runs):
    """The logged term against the pixelwise float64 restatement on the device's own depths, and bit for bit against
    hessian_term on those depths and the initial ones (the iteration hands it exactly these two maps).

    Bound.  Every depth of both maps is a multiple of u, the float32 spacing at the smallest depth.  A difference of such
    multiples is one again, and exact in float32 while it stays below 2^24 u.  With A the largest first difference, second
    differences are below 2 A and their difference between the two maps below 4 A: the test asserts 4 A < 2^24 u, so every
    entry that is averaged is exact, and what rounds are the float32 sums alone -- four of 4464 non-negative entries (a few
    serial additions per thread, then a tree of about 12 levels), three additions and a division: 32 roundings of half an
    ulp of the value at the most."""
    def run(n_iterations, graph, hessian=True):
        kw = optimize_keywords(runs, "strong", n_iterations=n_iterations, lr_update_iters=[], matching_update_iters=None, graph=graph,
                               prepare=False, use_hessian_loss=hessian, hessian_loss_weight=100.0)
        a = aligner_of(runs, runs.configs["strong"])
        start_from_recorded(a, runs, kw)
        before = host(a.deformed_depths)
        a.optimize(dev(runs.reference), **kw)
        return a, before

    a, before = run(1, False)
    want = ref.hessian_term(before, runs.d0)[0]
    got = a.loss_terms[0]["hess"]
    maps = np.stack([before, runs.d0]).astype(np.float64)
    u = float(np.spacing(np.float32(np.abs(maps).min())))
    A = max(np.abs(np.diff(maps, axis=2)).max(), np.abs(np.diff(maps, axis=3)).max())
    assert np.abs(maps).min() > 0 and 4 * A < 2.0 ** 24 * u
    limit = 16 * float(np.spacing(np.float32(want)))
    print(f"hessian term: {got:.9e} against {want:.9e}, difference {abs(got - want):.3e}, limit {limit:.3e}")
    assert want > 0 and abs(got - want) <= limit
    assert got == float(chart_aligner.hessian_term(dev(before), dev(runs.d0)))
    plain, _ = run(1, False, hessian=False)
    assert "hess" not in plain.loss_terms[0]
    # the total carries the term times its weight: the two float32 sums differ by that and by at most 7 roundings each
    extra = a.train_losses[0] - plain.train_losses[0]
    assert abs(extra - 100.0 * got) <= 7 * float(np.spacing(np.float32(a.train_losses[0])))
    assert any(not np.array_equal(x, y) for x, y in zip(snapshot(a), snapshot(plain)))  # its gradient reaches the step
    eager, _ = run(3, False)
    graphed, _ = run(3, True)
    same_bits(snapshot(graphed) + [np.array(graphed.train_losses)], snapshot(eager) + [np.array(eager.train_losses)], "graph against eager")
