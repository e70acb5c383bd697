"""render(): dict keys / shapes / post-processing semantics (2dgs/gaussian_renderer/__init__.py:108-166),
driven on the CPU through the oracle-backed rasterizer and map stand-ins (the product's are HIP-only)."""
from types import SimpleNamespace

import torch

import pytest

from cpu_rasterizer import oracle_backend
from g4splat_amd.gaussian_renderer import render, render_gslist
from oracle.render_maps_ref import depth_to_normal
from render_scenes import RENDER_KEYS, render_camera, render_model


@pytest.fixture(autouse=True)
def _oracle_backend():
    """Every render() of this module rasterizes with the CPU oracle (no GPU in the CPU suite)."""
    with oracle_backend():
        yield



def test_render_dict_and_gradients():
    cam, model = render_camera(), render_model()
    pipe = SimpleNamespace(depth_ratio=0.5, compute_cov3D_python=False, convert_SHs_python=False)
    out = render(cam, model, pipe, torch.tensor([0.1, 0.2, 0.3]))
    assert set(out) == RENDER_KEYS
    H, W = 56, 80
    assert out["render"].shape == (3, H, W) and out["rend_alpha"].shape == (1, H, W)
    assert out["rend_normal"].shape == (3, H, W) and out["surf_normal"].shape == (3, H, W)
    assert out["surf_depth"].shape == (1, H, W) and out["rend_dist"].shape == (1, H, W)
    assert out["radii"].dtype == torch.int32 and out["visibility_filter"].dtype == torch.bool
    a = out["rend_alpha"]
    assert float(a.max()) > 0.5 and float(a.min()) >= 0
    # expected depth = D / alpha with nan_to_num; median depth only where T crossed 0.5
    assert torch.isfinite(out["surf_depth"]).all() and torch.isfinite(out["rend_depth"]).all()
    # world normal = cam normal rotated by W2C^T rows: norms agree
    assert torch.allclose(out["rend_normal"].norm(dim=0), out["rend_normal_cam"].norm(dim=0), atol=1e-5)
    loss = out["render"].mean() + out["rend_dist"].mean() + (1 - (out["rend_normal"] * out["surf_normal"]).sum(0)).mean()
    loss.backward()
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert out["viewspace_points"].grad is not None and out["viewspace_points"].grad.shape == model.get_xyz.shape
    model.training_setup()
    model.add_densification_stats(out["viewspace_points"], out["visibility_filter"])
    assert float(model.denom.sum()) == float(out["visibility_filter"].sum())


def test_python_cov3d_path_matches_kernel_path():
    """pipe.compute_cov3D_python: T built in python (render(), :64-75) must reproduce the in-kernel T."""
    cam, model = render_camera(), render_model(P=120, seed=3)
    model.get_covariance = lambda mod=1: _covariance(model, mod)
    bg = torch.zeros(3)
    a = render(cam, model, SimpleNamespace(depth_ratio=0.0, compute_cov3D_python=False), bg)
    b = render(cam, model, SimpleNamespace(depth_ratio=0.0, compute_cov3D_python=True), bg)
    assert torch.allclose(a["render"], b["render"], atol=2e-4)
    assert torch.allclose(a["rend_alpha"], b["rend_alpha"], atol=2e-4)


def _covariance(model, mod):
    # build_covariance_from_scaling_rotation, gaussian_model.py:30-36 (note: uses the RAW _rotation, normalised inside)
    q = torch.nn.functional.normalize(model._rotation)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    s = torch.cat([model.get_scaling * mod, torch.ones_like(model.get_scaling[:, :1])], 1)
    RS = (R * s[:, None, :]).permute(0, 2, 1)
    trans = torch.zeros((q.shape[0], 4, 4))
    trans[:, :3, :3] = RS
    trans[:, 3, :3] = model.get_xyz
    trans[:, 3, 3] = 1
    return trans


def test_depth_to_normal_of_a_plane():
    cam = render_camera(64, 48)
    depth = torch.full((1, 48, 64), 2.0)
    n = depth_to_normal(cam, depth)
    inner = n[1:-1, 1:-1]
    # a fronto-parallel plane: normal = -+ camera forward axis in world space
    fwd = torch.linalg.inv(cam.world_view_transform.T)[:3, 2]
    assert torch.allclose(inner.reshape(-1, 3).abs() @ torch.ones(3), (fwd.abs() @ torch.ones(3)).expand(inner.numel() // 3), atol=1e-3)
    assert not n[0].any() and not n[:, 0].any()


def test_render_gslist_equals_render_of_the_union():
    """render_gslist (2dgs/gaussian_renderer/__init__.py:169-363): two models rendered together == one model holding
    both sets; dictionary keys of the reference; gradients reach both models."""
    cam = render_camera()
    a, b = render_model(P=120, seed=5), render_model(P=80, seed=6)
    pipe = SimpleNamespace(depth_ratio=0.5, compute_cov3D_python=False)
    bg = torch.tensor([0.2, 0.1, 0.3])
    out = render_gslist(cam, [a, b], pipe, bg)
    assert set(out) == (RENDER_KEYS - {"rend_normal_cam", "surf_normal_cam"}) | {"model_start_indices"}
    assert out["model_start_indices"] == [0, 120, 200]
    both = render_model(P=200, seed=0)
    with torch.no_grad():
        for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
            getattr(both, name).copy_(torch.cat([getattr(a, name), getattr(b, name)], dim=0))
    ref = render(cam, both, pipe, bg)
    for k in ("render", "rend_alpha", "rend_normal", "surf_depth", "surf_normal", "rend_dist", "rend_depth", "radii"):
        assert torch.equal(out[k], ref[k]), k
    (out["render"].mean() + out["rend_dist"].mean()).backward()
    assert a._xyz.grad is not None and b._xyz.grad is not None and b._features_rest.grad.abs().sum() > 0
    assert out["viewspace_points"].grad.shape == (200, 3)
    import pytest
    with pytest.raises(ValueError):
        render_gslist(cam, a, pipe, bg)
