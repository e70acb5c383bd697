"""What the chart-prior losses (g4splat_amd/losses.py, include/g4s_losses.h) promise without a GPU: the reference's
schedule, the reference's consumption of the random generator, and host-side argument validation of the new entry
points.  Goldens: tests/golden/chart_losses.npz (make_golden_chart_losses.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from g4splat_amd import losses

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chart_losses.npz")
CASES = {"ragged": (70, 93), "m1": (16, 16), "m0": (5, 7), "row": (1, 40), "half": (33, 50), "flat": (40, 40)}


def test_schedule_equals_the_reference():
    g = np.load(G)
    its = [int(i) for i in g["schedule_iterations"]]
    assert its == [1, 999, 1000, 1500, 1501, 3001, 6001, 9000]
    for it, want in zip(its, g["schedule_values"]):
        assert losses.schedule_regularization_factor_2(it) == float(want), it
    assert losses.schedule_regularization_factor_2(9000) == 0.015  # the floor
    # train_with_refine_depth.py:451-459
    assert [losses.depth_order_weight(i) for i in (1, 1500, 1501, 3000, 3001, 4500, 4501, 6000, 6001)] == \
        [0.0, 0.0, 1.0, 1.0, 0.1, 0.1, 0.01, 0.01, 0.001]


@pytest.mark.parametrize("name", sorted(CASES))
def test_draw_pixel_shifts_consumes_the_generator_as_the_reference(name):
    g = np.load(G)
    H, W = CASES[name]
    torch.manual_seed(int(g[f"{name}_seed"]))
    got = losses.draw_pixel_shifts(H, W, float(g[f"{name}_ratio"]), device="cpu")
    assert got.dtype == torch.int64 and tuple(got.shape) == (H * W, 2)
    assert np.array_equal(got.numpy(), g[f"{name}_shifts"].astype(np.int64))
    # ... and leaves it where the reference's single randint call leaves it
    after = torch.get_rng_state()
    torch.manual_seed(int(g[f"{name}_seed"]))
    m = round(float(g[f"{name}_ratio"]) * max(H, W))
    torch.randint(-m, m + 1, (H * W, 2))
    assert torch.equal(after, torch.get_rng_state())


def test_half_rounds_to_even():
    assert int(losses.draw_pixel_shifts(33, 50, 0.05, device="cpu").abs().max()) == 2  # round(2.5) = 2
    assert int(losses.draw_pixel_shifts(5, 7, 0.05, device="cpu").abs().max()) == 0


def test_argument_validation_is_host_side(hip_lib):
    """The new entry points reject bad arguments before they touch the device: negative status + a message."""
    lib = hip_lib
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # never dereferenced: validation fails first
    big = 1 << 30

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    maps = (one,) * 6
    fwd = lambda w, h, m, out, ws, n: lib.g4s_chart_prior_forward(w, h, *m, 1.0, 1.0, 20.0, nul, out, ws, n, nul)
    bwd = lambda w, h, m, outs, ws, n: lib.g4s_chart_prior_backward(w, h, *m, 1.0, 1.0, 20.0, one, *outs, ws, n, nul)
    assert lib.g4s_chart_prior_workspace(1600, 1200) >= 1600 * 1200 * 8
    assert lib.g4s_chart_prior_workspace(0, 4) == 0 and lib.g4s_chart_prior_workspace(2049, 2048) == 0
    assert lib.g4s_chart_prior_workspace(2048, 2048) > 0  # exactly 2^22 pixels is allowed
    expect(fwd(0, 4, maps, one, one, big), "must be positive")
    expect(fwd(4, -1, maps, one, one, big), "must be positive")
    expect(fwd(2049, 2048, maps, one, one, big), "at most 2^22 pixels")
    expect(fwd(4, 4, maps, one, one, 8), "workspace too small")
    expect(fwd(4, 4, maps, one, nul, big), "workspace too small")
    expect(fwd(4, 4, maps, nul, one, big), "NULL required pointer")
    for k in range(6):
        expect(fwd(4, 4, maps[:k] + (nul,) + maps[k + 1:], one, one, big), "NULL required pointer")
    outs = (one,) * 4  # grad_out5 and the three gradients
    expect(bwd(4, 0, maps, outs, one, big), "must be positive")
    expect(bwd(1 << 12, (1 << 10) + 1, maps, outs, one, big), "at most 2^22 pixels")
    expect(bwd(4, 4, maps, outs, one, 8), "workspace too small")
    for k in range(4):
        expect(bwd(4, 4, maps, outs[:k] + (nul,) + outs[k + 1:], one, big), "NULL required pointer")
    expect(lib.g4s_chart_prior_forward(4, 4, *maps, 1.0, 1.0, 20.0, ctypes.c_void_p(260), one, one, big, nul), "8-byte aligned")
    # anisotropy
    assert lib.g4s_anisotropy_workspace(0) == 0 and lib.g4s_anisotropy_workspace(1_500_000) >= 1_500_000 // 256 * 4
    expect(lib.g4s_anisotropy_forward(0, one, 5.0, one, one, big, nul), "P must be positive")
    expect(lib.g4s_anisotropy_forward(5, nul, 5.0, one, one, big, nul), "NULL required pointer")
    expect(lib.g4s_anisotropy_forward(5, one, 5.0, nul, one, big, nul), "NULL required pointer")
    expect(lib.g4s_anisotropy_forward(5, one, 5.0, one, one, 8, nul), "workspace too small")
    expect(lib.g4s_anisotropy_forward(5, ctypes.c_void_p(260), 5.0, one, one, big, nul), "8-byte aligned")
    expect(lib.g4s_anisotropy_backward(0, one, 5.0, one, one, nul), "P must be positive")
    expect(lib.g4s_anisotropy_backward(5, one, 5.0, nul, one, nul), "NULL required pointer")
    expect(lib.g4s_anisotropy_backward(5, one, 5.0, one, nul, nul), "NULL required pointer")
    # a call that succeeds clears the calling thread's message again
    assert lib.g4s_densify_stats(0, nul, nul, nul, nul, nul, nul, nul) == 0 and lib.g4s_last_error() == b""


def test_no_cpu_path():
    z3, z1 = torch.zeros(3, 4, 4), torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError):
        losses.chart_prior_losses(z3, z3, z1, z1, z3, z1, 1.0)
    with pytest.raises(RuntimeError):
        losses.anisotropy_loss(torch.ones(5, 2))
