"""The numpy restatement of the chart deformation's contract (tests/chart_deform_ref.py) against the reference's own float64 run
(tests/golden/chart_deform.npz, make_golden_chart_deform.py): delta, depths and the gradient to every parameter to 1e-12 of the
largest entry; the float32 depth_coords exactly.  And the Python surface that needs no GPU: ChartDeformation's parameter names
and shapes against the reference's, the state-dict round trip, depth_coordinates, the refusals."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chart_deform_ref as ref
from support import GOLDEN

TOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "chart_deform.npz"))


def close(label, got, want, tol=TOL):
    top = np.abs(want).max()
    err = np.abs(got - want).max() / top
    print(f"{label}: {err:.3e} of the largest entry")
    assert got.shape == want.shape and err <= tol, (label, err)


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_restatement_equals_the_references_float64_run(golden, name):
    c = ref.load_case(golden, name)
    f = ref.forward(c, np.float64)
    close(f"{name} delta", f.delta, c.r64.delta)
    # a zero depth: the reference's point is the camera centre, whose view-space z is a rounding error, not 0
    assert np.abs(c.r64.depths[c.d0 == 0]).max(initial=0.0) < 1e-14
    close(f"{name} depths", f.depths, c.r64.depths)
    for tag, g in (("g", c.cotangent), ("ones", np.ones_like(c.cotangent))):
        got = ref.flat_gradients(c, ref.gradients(c, g, np.float64))
        for k, want in c.r64.grads[tag].items():
            close(f"{name} {tag} d/d{k}", got[k], want)


@pytest.mark.parametrize("name", [n for n in ref.GOLDEN_CASES if ref.CASES[n][7]])
def test_depth_coords_exactly(golden, name):
    from g4splat_amd import chart_deform
    c = ref.load_case(golden, name)
    assert c.coords.dtype == np.float32 and c.coords.min() >= 0 and c.coords.max() == 1
    assert np.array_equal(ref.depth_coordinates(c.d0, c.bins), c.coords)
    got = chart_deform.depth_coordinates(torch.from_numpy(c.d0), c.bins)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), c.coords)


def module_of(c, device="cpu", **more):
    """ChartDeformation built as the case was; on the CPU it holds parameters only."""
    from g4splat_amd import chart_deform as cd
    E = c.channels * len(c.levels)
    kw = dict(charts_encoding_params=cd.ChartsEncodingParams(encoding_dim=E), depth_encoding_params=cd.DepthEncodingParams(encoding_dim=E, n_bins=c.bins or 30),
              mlp_params=cd.MLPParams(n_deformation_layers=c.layers, deformation_layer_size=c.layer_size),
              use_learnable_depth_encoding=bool(c.bins), use_multi_res_charts_encoding=c.multi_res,
              multi_res_charts_encoding_params=cd.MultiResChartsEncodingParams(c.channels, c.resolutions or (0.05, 0.1, 0.2, 0.4)),
              spatial_extent_override=c.extent if c.n == 1 else None)
    kw.update(more)
    return cd.ChartDeformation(c.cams, torch.as_tensor(c.d0, device=device), **kw)


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_parameter_names_and_shapes_are_the_references(golden, name):
    c = ref.load_case(golden, name)
    m = module_of(c)
    want = ref.parameters(c)
    own = dict(m.named_parameters())
    assert set(own) == set(want) and set(m.state_dict()) == set(want)
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: v.shape for k, v in want.items()}
    assert all(p.requires_grad and p.dtype == torch.float32 for p in own.values())
    assert m.scene_radius == c.scene_radius and m.deformation_radius == c.deformation_radius
    # a reference state dict carries over; what else it holds is ignored; the round trip is exact
    sd = {k: torch.from_numpy(v) for k, v in want.items()}
    sd.update(_verts=torch.zeros(3), depth_coords=torch.zeros(2), _confidence=torch.zeros(1))
    m.load_reference_state_dict(sd)
    back = m.state_dict()
    assert all(np.array_equal(back[k].numpy(), want[k]) for k in want)
    if c.bins:
        assert np.array_equal(m.depth_coords.numpy(), c.coords)
    with pytest.raises(KeyError):
        m.load_reference_state_dict({k: v for k, v in sd.items() if k != "deformation.mlp.0.bias"})
    with pytest.raises(RuntimeError, match="HIP device"):
        m.deformed_depths()


def test_resets_draw_as_the_reference_does(golden):
    c = ref.load_case(golden, "small")
    torch.manual_seed(5)
    m = module_of(c)
    first = {k: v.clone() for k, v in m.state_dict().items()}
    for k, v in first.items():
        if k.endswith("encodings"):
            assert 0 < float(v.abs().max()) <= 1e-4
        elif k.endswith("bias"):
            assert not v.any()
    W = first["deformation.mlp.0.weight"]  # xavier_normal_ with the ReLU gain: std = sqrt(2) sqrt(2 / (fan_in + fan_out))
    assert abs(float(W.std()) / (np.sqrt(2.0) * np.sqrt(2.0 / (W.shape[1] + W.shape[2]))) - 1) < 0.15
    # the encodings are the host generator's next uniforms, level by level
    torch.manual_seed(11)
    m.reset_encodings()
    torch.manual_seed(11)
    for l, (h, w) in enumerate([(1, 1), (2, 2), (3, 3), (4, 5)]):
        want = 1e-4 * (-1. + 2. * torch.rand(c.n, c.channels, h, w))
        assert torch.equal(m.state_dict()[f"charts_encoding.charts_encoding.{l}.encodings"], want)
    torch.manual_seed(12)
    m.reset_mlp()
    a = m.state_dict()["deformation.mlp.0.weight"].clone()
    torch.manual_seed(12)
    m.reset_mlp()
    assert torch.equal(m.state_dict()["deformation.mlp.0.weight"], a) and not torch.equal(a, W)
    m.reset_mlp(std=0.5)
    assert abs(float(m.state_dict()["deformation.mlp.0.weight"].std()) / 0.5 - 1) < 0.15


REFUSED = [dict(learnable_depth_encoding_mode=mode) for mode in ("multiply", "replace", "concatenate", "adaln")] + [
    dict(use_meta_mlp=True), dict(use_lora_mlp=True), dict(weight_encodings_with_confidence=True), dict(predict_in_disparity_space=True),
    dict(output_dim=3)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_refused_modes_raise_not_implemented(golden, kw):
    with pytest.raises(NotImplementedError):
        module_of(ref.load_case(golden, "one"), **kw)


def test_a_sigmoid_final_layer_is_refused(golden):
    from g4splat_amd import chart_deform as cd
    with pytest.raises(NotImplementedError, match="sigmoid"):
        module_of(ref.load_case(golden, "one"), mlp_params=cd.MLPParams(no_final_linearity=False))


def out_of_envelope():
    from g4splat_amd import chart_deform as cd
    return [("encoding width", dict(multi_res_charts_encoding_params=cd.MultiResChartsEncodingParams(8, (0.5, 0.7, 1.0)))),
            ("multiple of 4", dict(multi_res_charts_encoding_params=cd.MultiResChartsEncodingParams(2, (0.5,) * 8))),
            ("levels", dict(multi_res_charts_encoding_params=cd.MultiResChartsEncodingParams(4, (0.5,) * 9))),
            ("deformation_layer_size", dict(mlp_params=cd.MLPParams(deformation_layer_size=48))),
            ("deformation layers", dict(mlp_params=cd.MLPParams(n_deformation_layers=5))),
            ("deformation layers", dict(mlp_params=cd.MLPParams(n_deformation_layers=1))),
            ("depth bins", dict(depth_encoding_params=cd.DepthEncodingParams(16, n_bins=5000))),
            ("texels", dict(multi_res_charts_encoding_params=cd.MultiResChartsEncodingParams(8, (0.3, 1.0)))),
            ("charts_encoding_params.encoding_dim", dict(charts_encoding_params=cd.ChartsEncodingParams(encoding_dim=32))),
            ("depth_encoding_params.encoding_dim", dict(depth_encoding_params=cd.DepthEncodingParams(encoding_dim=32))),
            ("scene radius", dict(spatial_extent_override=0.0))]


@pytest.mark.parametrize("k", range(11))
def test_shapes_outside_the_envelope_raise_value_error_naming_the_limit(golden, k):
    what, kw = out_of_envelope()[k]
    with pytest.raises(ValueError, match=what):
        module_of(ref.load_case(golden, "one"), **kw)


def test_views_and_depths_have_to_agree(golden):
    c = ref.load_case(golden, "small")
    c2 = SimpleNamespace(**{**vars(c), "cams": c.cams[:1]})
    with pytest.raises(ValueError, match="views"):
        module_of(c2)
