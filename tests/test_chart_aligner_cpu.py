"""The numpy restatement of the chart aligner (tests/chart_aligner_ref.py) against the reference's own float64 runs
(tests/golden/chart_aligner.npz, make_golden_chart_aligner.py), and the Python surface of g4splat_amd/chart_aligner.py that needs
no GPU: the configurations, the parameter groups and their learning rates, the learning-rate rule, total_loss, the refusals and
charts_data.npz.

Bounds.  The state (a) holds to 1e-12 of the largest entry, the figure the other chart restatements hold.  The 50 float64
iterations (b) are bounded by RUN_TOL = 1e-11 of the largest entry of a parameter and of the loss curve: Adam with eps = 1e-15
divides m by sqrt(v), so the first steps are sign steps of the size of the learning rate, and a gradient's float64 rounding
(1e-16 of it, from the different sum orders of numpy and torch) is amplified where a gradient passes near zero.  On this scene
the two float64 runs stay within 4e-14 of each other (printed: the level encodings are the worst), which the bound allows to
grow 250 times; a wrong weight, group order or learning-rate rule moves parameters by 1e-4 to 1e-2 of their size within 50
steps."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chart_aligner_ref as ref
import chart_deform_ref as cd
from support import GOLDEN

TOL = 1e-12
RUN_TOL = 1e-11


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "chart_aligner.npz"))


@pytest.fixture(scope="module")
def state(golden):
    return ref.load_state(golden)


@pytest.fixture(scope="module")
def runs(golden):
    return ref.load_runs(golden)


def close(label, got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = np.abs(want).max()
    err = np.abs(got - want).max() / top
    print(f"{label}: {err:.3e} of the largest entry")
    assert got.shape == want.shape and err <= tol, (label, err)
    return err


# ---- the restatement against golden (a) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(ref.VARIANTS))
def test_restatement_equals_the_references_float64_state(state, variant):
    c, v = state, state.variants[variant]
    conf, w = ref.confidence(c.raw, np.float64)
    close("confidence", conf, c.conf64)
    w = w if v.weighted else None
    f = ref.forward(c, w, np.float64)
    close(f"{variant} depths", f.depths, v.depths64)
    reg = ref.regularizers(c, f, v.norm, v.tv, np.float64)
    for i, on in enumerate((v.norm, v.tv)):
        if on:
            close(f"{variant} reg[{i}]", reg[i:i + 1], v.reg64[i:i + 1])
        else:
            assert reg[i] == 0 and v.reg64[i] == 0
    got = cd.flat_gradients(c, ref.gradients(c, v.cotangent, v.greg, w, v.norm, v.tv, np.float64))
    for k, want in v.grads64.items():
        close(f"{variant} d/d{k}", got[k], want)


def test_confidence_edge_values_are_exact():
    conf, w = ref.confidence(np.array([-60.0, 5.0, -17.0, 3.0], np.float32), np.float32)
    assert conf.dtype == np.float32 and conf[0] == 1 and w[0] == 0 and w[1] == 1 and conf[2] == 1 and w[2] == 0 and w[3] == 1
    g = ref.confidence_backward(np.array([0.0, 1.0]), np.array([2.0, 3.0]))
    assert g[0] == 2.0 and abs(g[1] - 3.0 * np.e) < 1e-15


def test_the_norm_subgradient_is_zero_where_the_encoding_vanishes(state):
    c = SimpleNamespace(**vars(state))
    c.levels = [np.zeros_like(v) for v in state.levels]
    g = ref.gradients(c, np.zeros_like(c.cotangents[0]), (1.0, 0.0), None, True, False)
    assert all(not lv.any() and np.isfinite(lv).all() for lv in g["levels"])


# ---- the restatement's 50 iterations against golden (b) ----------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["strong", "default"])
def test_restated_optimize_equals_the_references_float64_run(runs, flavour):
    cfg, r, o = runs.configs[flavour], runs.runs[flavour], runs.options
    params, raw, losses, _vec = ref.optimize(
        runs, runs.init, runs.init_confidence, runs.reference, o["n_iterations"], ref.weights_of(cfg),
        cfg["weight_encodings_with_confidence"], matching_thr=runs.matching_thr, lr_update_iters=o["lr_update_iters"],
        lr_update_factor=o["lr_update_factor"], matching_update_iters=o["matching_update_iters"], encodings_lr=cfg["encodings_lr"],
        mlp_lr=cfg["mlp_lr"], confidence_lr=cfg["confidence_lr"])
    close(f"{flavour} loss curve", np.array(losses), r.losses64, RUN_TOL)
    for k, want in r.end64.items():
        close(f"{flavour} end {k}", params[k], want, RUN_TOL)
    close(f"{flavour} end _confidence", raw, r.end_confidence64, RUN_TOL)


def test_adam_rule_is_torchs():
    rng = np.random.default_rng(3)
    p0, grads = rng.standard_normal(7), rng.standard_normal((4, 7))
    t = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([{"params": [t], "lr": 3e-3}], lr=0.0, eps=1e-15)
    p, m, v = p0.copy(), np.zeros(7), np.zeros(7)
    for i, g in enumerate(grads):
        t.grad = torch.tensor(g)
        opt.step()
        p, m, v = ref.adam_step(p, g, m, v, i + 1, 3e-3)
    assert np.abs(p - t.detach().numpy()).max() < 1e-15


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def aligner_of(c, device="cpu", **more):
    from g4splat_amd import chart_aligner as ca
    E = c.channels * len(c.levels)
    kw = dict(charts_encoding_params=ca.ChartsEncodingParams(encoding_dim=E),
              depth_encoding_params=ca.DepthEncodingParams(encoding_dim=E, n_bins=c.bins),
              mlp_params=ca.MLPParams(n_deformation_layers=c.layers, deformation_layer_size=c.layer_size),
              multi_res_charts_encoding_params=ca.MultiResChartsEncodingParams(c.channels, c.resolutions),
              use_learnable_confidence=True, weight_encodings_with_confidence=True)
    kw.update(more)
    return ca.ChartAligner(c.cams, torch.as_tensor(c.d0, device=device), **kw)


def test_alignment_configs_are_the_yaml_blocks(golden):
    from g4splat_amd import chart_aligner as ca
    stored = json.loads(str(golden["configs"]))
    assert set(stored) == {"default", "strong"} == set(ca.ALIGNMENT_CONFIGS)
    for flavour, block in stored.items():
        assert ca.ALIGNMENT_CONFIGS[flavour] == block, flavour
    differ = {k for k in stored["default"] if stored["default"][k] != stored["strong"][k]}
    assert differ == {"weight_encodings_with_confidence", "regularize_chart_encodings_norms", "use_total_variation_on_depth_encodings"}


def test_parameter_names_groups_and_learning_rates_are_the_references(runs):
    a = aligner_of(runs)
    names = [k for k, _p in a.named_parameters()]
    assert set(names) == set(runs.init) | {"_confidence"}
    assert {k: tuple(p.shape) for k, p in a.named_parameters() if k != "_confidence"} == {k: v.shape for k, v in runs.init.items()}
    assert tuple(a._confidence.shape) == runs.d0.shape and not a._confidence.any() and a.confidence_weighting == 0.2
    r = runs.runs["strong"]
    cfg = runs.configs["strong"]
    a.prepare_for_optimization(cfg["encodings_lr"], cfg["mlp_lr"], [20], 0.5, cfg["confidence_lr"])
    groups = a.optimizer.param_groups
    want = [(k, lr) for k, lr, t in zip(r.group_names, r.group_lrs, r.group_trainable) if t]  # the reference also lists its constants
    assert [(g["name"], g["lr"]) for g in groups] == want
    assert all(len(g["params"]) == 1 and g["eps"] == 1e-15 for g in groups)
    assert [g["name"] for g in groups] == ref.group_names(runs)
    # the learning-rate rule touches exactly the reference's groups
    a.update_learning_rates()
    assert [g["lr"] for g in groups] == [lr for lr, t in zip(r.end_lrs, r.group_trainable) if t]
    touched = [g["name"] for g, (_k, lr) in zip(groups, want) if g["lr"] != lr]
    assert touched == [k for k, _lr in want if k != "_confidence"]
    from g4splat_amd import chart_aligner as ca
    assert all(ca.updates_learning_rate(k) == ref.updates_learning_rate(k) for k, _lr in want)


def test_prepare_resets_encodings_then_the_mlp_and_keeps_the_confidence(runs):
    a = aligner_of(runs)
    with torch.no_grad():
        a._confidence.fill_(0.25)
    torch.manual_seed(7)
    a.prepare_for_optimization()
    first = {k: v.clone() for k, v in a.state_dict().items()}
    torch.manual_seed(7)
    a.reset_encodings()
    a.reset_mlp()
    assert all(torch.equal(v, first[k]) for k, v in a.state_dict().items())
    assert bool((a._confidence == 0.25).all())


def test_total_loss_with_each_term_alone():
    from g4splat_amd import chart_aligner as ca
    terms, reg, matching, hessian = [2.0, 3.0, 5.0, 7.0], [11.0, 13.0], 17.0, 19.0
    none = dict.fromkeys(("gradient", "hessian", "normal", "curvature", "matching", "norm", "tv"))
    for total in (ca.total_loss, ref.total_loss):
        assert total(terms, reg, matching, none, hessian) == 2.0
        for key, value in (("gradient", 3.0), ("hessian", 19.0), ("normal", 5.0), ("curvature", 7.0), ("matching", 17.0), ("norm", 11.0),
                           ("tv", 13.0)):
            assert total(terms, reg, matching, dict(none, **{key: 0.5}), hessian) == 2.0 + 0.5 * value, key
        assert total(terms, reg, None, dict(none, normal=4.0, curvature=1.0)) == 2.0 + 20.0 + 7.0
    t = [torch.tensor(v) for v in terms]
    got = ca.total_loss(t, [torch.tensor(v) for v in reg], torch.tensor(matching), dict(none, matching=5.0, tv=5.0))
    assert got.dtype == torch.float32 and float(got) == 2.0 + 85.0 + 65.0


def test_hessian_term_against_the_pixelwise_restatement_and_known_values():
    """hessian_term is plain torch and runs on the host.  In float64 it holds to 1e-12 of the value against the restatement
    (which forms each second difference from the window's entries, another order of the same three or four additions); its
    autograd gradient likewise, away from second differences at rounding level (there are none in a random map)."""
    from g4splat_amd import chart_aligner as ca
    rng = np.random.default_rng(5)
    for shape in ((1, 3, 3), (2, 5, 4), (3, 7, 9)):
        d, p = rng.uniform(1, 2, shape), rng.uniform(1, 2, shape)
        t = torch.tensor(d, requires_grad=True)
        got = ca.hessian_term(t, torch.tensor(p))
        got.backward()
        want, grad = ref.hessian_term(d, p)
        close(f"hessian term {shape}", [float(got.detach())], [want])
        close(f"hessian gradient {shape}", t.grad.numpy(), grad)
        assert ca.hessian_term(torch.tensor(d, dtype=torch.float32), torch.tensor(p, dtype=torch.float32)).dtype == torch.float32
    i, j = np.meshgrid(np.arange(6.0), np.arange(5.0), indexing="ij")
    prior = torch.tensor(rng.integers(0, 8, (2, 6, 5)).astype(np.float64))  # small integers: every value below is exact
    for offset, value in ((3 * i + 2 * j + 1, 0.0), (i * i, 0.5), (j * j, 0.5), (i * j, 0.5), (i * i + 2 * i * j - j * j, 2.0)):
        assert float(ca.hessian_term(prior + torch.tensor(offset), prior)) == value == ref.hessian_term(prior.numpy() + offset, prior.numpy())[0]
    for bad in (torch.zeros(2, 2, 5), torch.zeros(2, 5, 2), torch.zeros(5, 5)):
        with pytest.raises(ValueError, match="hessian term"):
            ca.hessian_term(bad, bad)
    with pytest.raises(ValueError, match="hessian term"):
        ca.hessian_term(torch.zeros(2, 5, 5), torch.zeros(2, 5, 6))


def test_refusals(runs):
    from g4splat_amd import chart_aligner as ca
    a = aligner_of(runs)
    reference = torch.as_tensor(runs.reference)
    with pytest.raises(NotImplementedError, match="reprojection"):
        a.optimize(reference, use_reprojection_loss=True)
    with pytest.raises(NotImplementedError, match="points"):
        a.optimize([torch.zeros(10, 3) for _ in range(runs.n)])
    with pytest.raises(NotImplementedError, match="points"):
        a.optimize(torch.zeros(runs.n, runs.H, runs.W, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        a.optimize(reference, n_iterations=1)
    one_bin = aligner_of(runs, depth_encoding_params=ca.DepthEncodingParams(encoding_dim=32, n_bins=1))
    with pytest.raises(ValueError, match="at least 2 depth bins"):
        one_bin.optimize(reference, use_total_variation_on_depth_encodings=True)
    with pytest.raises(ValueError, match="at least 2 depth bins"):
        one_bin.deformation_module.deformed_depths_and_regularizers(tv=True)
    with pytest.raises(ValueError, match="not learnable"):
        aligner_of(runs, use_learnable_confidence=False)
    for kw in (dict(use_meta_mlp=True), dict(use_lora_mlp=True), dict(predict_in_disparity_space=True),
               dict(learnable_depth_encoding_mode="multiply")):
        with pytest.raises(NotImplementedError):
            aligner_of(runs, **kw)


def test_chart_deformation_still_refuses_the_weighting_flag(runs):
    from test_chart_deform_cpu import module_of
    with pytest.raises(NotImplementedError, match="weight_encodings_with_confidence"):
        module_of(runs, weight_encodings_with_confidence=True)


def test_charts_data_keys_and_shapes(runs, tmp_path):
    """What save_charts_data writes, formed on the host from stand-in outputs: the reference's keys, and the trainer's
    initialiser takes the file's entries up to its device check (it refuses host tensors by name, after reading them)."""
    from g4splat_amd import chart_aligner as ca, chart_init
    a = aligner_of(runs)
    n, H, W = runs.d0.shape
    depths = torch.as_tensor(runs.reference)
    outputs = (torch.zeros(n, H, W, 3), depths, 1.0 + torch.ones(n, H, W))
    a.outputs = lambda: outputs
    path = a.save_charts_data(str(tmp_path), scale_factor=2.5)
    assert os.path.basename(path) == "charts_data.npz"
    data = np.load(path)
    assert set(data.files) == {"prior_depths", "depths", "pts", "confs", "scale_factor"}
    assert data["prior_depths"].shape == (n, H, W) and np.array_equal(data["prior_depths"], runs.d0)
    assert data["depths"].shape == (n, H, W) and data["pts"].shape == (n, H, W, 3) and data["confs"].shape == (n, H, W)
    assert float(data["scale_factor"]) == 2.5 and all(data[k].dtype == np.float32 for k in ("prior_depths", "depths", "pts", "confs"))
    charts = {k: torch.as_tensor(data[k]) for k in ("pts", "confs")}
    charts["scale_factor"] = float(data["scale_factor"])
    with pytest.raises(ValueError, match=r"charts_data\['pts'\] must be a tensor on a HIP device"):
        chart_init.get_gaussian_parameters_from_charts_data(charts, None)
