"""The mip filter without a GPU: the float32 restatement of g4s_mip_filter's contract (tests/mip_filter_ref.py, the
order of operations include/g4s_optim.h spells out) and the float64 restatement of the activations with the filter on,
against what the reference's own GaussianModel produced (tests/golden/mip_filter.npz, make_golden_mip.py); the
documented all-unseen constant; and the CPU model's behaviour, which the fused path leaves alone."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mip_filter_ref import activations_mip_ref, camera_table, filter_scale, mip_filter_ref
from g4splat_amd.gaussian_model import GaussianModel

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mip_filter.npz")


def golden():
    g = np.load(GOLD)
    cams = [SimpleNamespace(R=R, T=T, focal_x=float(k[0]), focal_y=float(k[1]), image_width=int(k[2]), image_height=int(k[3]))
            for R, T, k in zip(g["in_R"], g["in_T"], g["in_intrinsics"])]
    return g, cams


def test_restatement_equals_the_reference_on_every_point():
    """rtol 1e-6 on EVERY point: the only licence is the summation order of the reference's GEMM (a few ulp of z carried
    through one multiply) and its two-step scaling.  The seen / unseen split is exact."""
    g, cams = golden()
    out, seen = mip_filter_ref(g["in_xyz"], camera_table(cams), float(g["in_znear"]),
                               filter_scale(cams, float(g["in_filter_variance"])))
    want = g["mip_filter"][:, 0]
    assert np.array_equal(seen, g["seen_by"] > 0)
    assert 5 <= (~seen).sum() < seen.sum()
    rel = np.abs(out.astype(np.float64) - want) / want
    print("largest relative difference to the reference:", rel.max())
    np.testing.assert_allclose(out, want, rtol=1e-6, atol=0)
    # unseen points carry the largest depth of the seen ones
    assert np.all(out[~seen] == out[seen].max())


def test_activation_formulas_equal_the_reference():
    g, _ = golden()
    q = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]]), (g["in_xyz"].shape[0], 1))
    (scales, _rots, opac), (d_s, _d_q, d_o) = activations_mip_ref(
        g["in_scaling"], q, g["in_opacity"], g["mip_filter"], g["in_cot_scaling"], np.zeros_like(q), g["in_cot_opacity"])
    for name, got, want in (("scales", scales, g["scales"]), ("opacities", opac, g["opacities"]),
                            ("grad_scaling", d_s, g["grad_scaling"]), ("grad_opacity", d_o, g["grad_opacity"])):
        assert got.shape == want.shape, name
        print(name, "largest relative difference:", float((np.abs(got - want) / np.abs(want)).max()))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=0, err_msg=name)


def test_all_unseen_gives_the_documented_constant():
    """No view sees any point: the reference raises on an empty max(); the contract writes 100000 * scale everywhere."""
    cam = SimpleNamespace(R=np.eye(3, dtype=np.float32), T=np.zeros(3, np.float32), focal_x=300.0, focal_y=300.0,
                          image_width=320, image_height=240)
    xyz = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 0.1], [50.0, 0.0, 1.0]], np.float32)  # behind, nearer than znear, off screen
    scale = filter_scale([cam])
    out, seen = mip_filter_ref(xyz, camera_table([cam]), 0.2, scale)
    assert not seen.any()
    assert np.all(out == np.float32(100000.0) * scale)


def test_entry_points_validate_on_the_host(hip_lib):
    """P < 0, NULL, alignment and V < 1 are refused through the shared error path before anything is launched."""
    import ctypes
    lib = hip_lib
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # never dereferenced: validation fails first

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    fwd, bwd = lib.g4s_activations_mip_forward, lib.g4s_activations_mip_backward
    expect(fwd(-1, one, one, one, one, one, one, one, nul), "must not be negative")
    expect(fwd(5, one, one, one, nul, one, one, one, nul), "NULL required pointer")
    expect(fwd(5, one, ctypes.c_void_p(264), one, one, one, one, one, nul), "16-byte aligned")
    expect(fwd(5, ctypes.c_void_p(260), one, one, one, one, one, one, nul), "8-byte")
    assert fwd(0, nul, nul, nul, nul, nul, nul, nul, nul) == 0
    expect(bwd(-1, *(one,) * 10, nul), "must not be negative")
    expect(bwd(5, one, one, one, nul, *(one,) * 6, nul), "NULL required pointer")
    expect(bwd(5, ctypes.c_void_p(260), *(one,) * 9, nul), "scale tensors must be 8-byte")
    expect(bwd(5, *(one,) * 5, ctypes.c_void_p(264), *(one,) * 4, nul), "rotation tensors 16-byte aligned")
    assert bwd(0, *(nul,) * 10, nul) == 0
    assert lib.g4s_mip_filter_workspace() >= 4
    expect(lib.g4s_mip_filter(-1, one, 1, one, 0.2, 1.0, one, one, nul), "must not be negative")
    expect(lib.g4s_mip_filter(5, one, 0, one, 0.2, 1.0, one, one, nul), "at least one view")
    expect(lib.g4s_mip_filter(5, one, 1, nul, 0.2, 1.0, one, one, nul), "NULL required pointer")
    expect(lib.g4s_mip_filter(5, one, 1, one, 0.2, 1.0, one, nul, nul), "NULL required pointer")
    expect(lib.g4s_mip_filter(5, ctypes.c_void_p(258), 1, one, 0.2, 1.0, one, one, nul), "4-byte aligned")
    assert lib.g4s_mip_filter(0, nul, 1, nul, 0.2, 1.0, nul, nul, nul) == 0


def _cpu_model(P=50, seed=3):
    g = torch.Generator().manual_seed(seed)
    m = GaussianModel(sh_degree=1)
    m.create_from_parameters(torch.randn((P, 3), generator=g), torch.rand((P, 2), generator=g) * 0.05 + 0.001,
                             torch.randn((P, 4), generator=g), torch.rand((P, 3), generator=g))
    return m


def test_cpu_model_is_unchanged():
    """get_activated on a host model is the three torch getters, filter on or off; compute_mip_filter on the host is
    the reference's loop (golden (a), to float round-off); a filter that is on but missing is a clear error."""
    m = _cpu_model()
    for on in (False, True):
        m.set_mip_filter(on)
        m.mip_filter = torch.full((50, 1), 0.01) if on else None
        for a, b in zip(m.get_activated, (m.get_scaling, m.get_rotation, m.get_opacity)):
            assert torch.equal(a, b)
    m.mip_filter = None
    with pytest.raises(RuntimeError, match="mip filter is on but has not been computed"):
        m.get_activated
    g, cams = golden()
    m = GaussianModel(sh_degree=1)
    m._xyz = torch.nn.Parameter(torch.tensor(g["in_xyz"]))
    m.set_mip_filter(True)
    m.compute_mip_filter(cams, znear=float(g["in_znear"]), filter_variance=float(g["in_filter_variance"]))
    assert m.mip_filter.shape == (g["in_xyz"].shape[0], 1)
    np.testing.assert_allclose(m.mip_filter.numpy(), g["mip_filter"], rtol=1e-6, atol=0)
