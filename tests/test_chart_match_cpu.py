"""The chart matcher's contract (tests/chart_match_ref.py, the numpy restatement of include/g4s_losses.h "Chart matcher")
against the reference's own results (tests/golden/chart_match.npz, make_golden_chart_match.py), and the packed-word
layout.  No GPU."""
import os

import numpy as np
import pytest

import chart_match_ref as ref

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chart_match.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(G)


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = np.abs(want).max()
    return 0.0 if top == 0 else float(np.abs(got - want).max() / top)


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_float64_restatement_equals_the_reference(golden, name):
    """Matches and fov exactly; errors, loss and both gradients to 1e-12 relative."""
    c = ref.load_case(golden, name)
    m, err, fov = ref.match(c.cams, c.ref_depths, c.thr, np.float64)
    assert np.array_equal(m, c.matches) and np.array_equal(fov, c.r64.match_fov)
    assert rel(err, c.r64.match_errors) <= 1e-12
    e, f = ref.reprojection_errors(c.cams, c.cur_depths, np.float64)
    assert np.array_equal(f, c.r64.fov)
    assert rel(e, c.r64.errors) <= 1e-12
    assert rel(ref.loss(c.cams, c.cur_depths, c.matches, c.weights, np.float64), c.r64.loss) <= 1e-12
    for cot, want in ((1.0, c.r64.grad), (c.cotangent, c.r64.grad_c037)):
        got = ref.loss_grad(c.cams, c.cur_depths, c.matches, c.weights, cot, np.float64)
        assert got.shape == want.shape and rel(got, want) <= 1e-12, (cot, rel(got, want))


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_float32_decisions_equal_the_references_float32_run(golden, name):
    """The generator keeps every decision at least 2^-12 from its edge, so the contract's order of float32 operations has to
    decide every pair as the reference's float32 matmuls did."""
    c = ref.load_case(golden, name)
    m, _err, fov = ref.match(c.cams, c.ref_depths, c.thr, np.float32)
    assert np.array_equal(m, c.matches) and np.array_equal(fov, c.r32.match_fov)
    _e, f = ref.reprojection_errors(c.cams, c.cur_depths, np.float32)
    assert np.array_equal(f, c.r32.fov)


def test_analytic_gradient_against_central_differences(golden):
    """n = 2 at 5x7 in float64: every element of dL/dD, with the weights of a random map."""
    c = ref.load_case(golden, "n2")
    w = np.random.default_rng(5).uniform(0.5, 2.0, c.cur_depths.shape)
    D = c.cur_depths.astype(np.float64)
    got = ref.loss_grad(c.cams, D, c.matches, w, 1.0, np.float64)
    h = 1e-6
    want = np.zeros_like(D)
    for k in range(D.size):
        up, down = D.copy().reshape(-1), D.copy().reshape(-1)
        up[k] += h
        down[k] -= h
        want.reshape(-1)[k] = (float(ref.loss(c.cams, up.reshape(D.shape), c.matches, w, np.float64))
                               - float(ref.loss(c.cams, down.reshape(D.shape), c.matches, w, np.float64))) / (2 * h)
    assert np.abs(want).max() > 0
    assert rel(got, want) <= 1e-7, rel(got, want)


def test_packed_word_layout():
    """Bit p mod 32 of word p // 32 per (i, j); the tail word's unused bits are zero; unpacking inverts packing."""
    rng = np.random.default_rng(2)
    n, H, W = 3, 5, 13  # 65 pixels: two full words and one bit
    m = rng.random((n, n, H, W)) < 0.5
    m[1, 2].reshape(-1)[[0, 31, 32, 64]] = True
    words = ref.pack_words(m)
    assert words.dtype == np.uint32 and words.shape == (n, n, 3)
    assert (words[:, :, 2] >> 1 == 0).all()
    flat = m.reshape(n, n, -1)
    for p in (0, 1, 31, 32, 33, 63, 64):
        assert np.array_equal((words[:, :, p // 32] >> np.uint32(p % 32)) & 1, flat[:, :, p].astype(np.uint32))
    assert np.array_equal(ref.unpack_words(words, H, W), m)
    ones = ref.pack_words(np.ones((1, 1, 1, 40), bool))
    assert ones.tolist() == [[[0xFFFFFFFF, 0xFF]]]


def test_spatial_extent():
    """CamerasWrapper.get_spatial_extent: 1.1 x the largest distance of a centre from the mean centre."""
    from types import SimpleNamespace
    cams = []
    for centre in ((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (2.0, 3.0, 0.0)):
        M = np.eye(4)
        M[3, :3] = -np.asarray(centre)
        cams.append(SimpleNamespace(world_view_transform=M))
    mean = np.array([2.0, 1.0, 0.0])
    want = 1.1 * max(np.linalg.norm(np.asarray(c) - mean) for c in ((0, 0, 0), (4, 0, 0), (2, 3, 0)))
    assert abs(ref.spatial_extent(cams) - want) <= 1e-12


def test_wrapper_records_workspace_and_refusals_on_the_host(hip_lib, golden):
    """What the Python surface and the entry points decide without a device: the camera records the kernels read are the
    float32 rounding of the restatement's, the words a matcher allocates are ceil(H W / 32) per pair, the workspace holds the
    block partials and the [n,H,W] 64-bit sums, and sizes beyond the range limit are refused with a message that names it."""
    import ctypes

    from g4splat_amd import _lib, chart_match
    c = ref.load_case(golden, "n3")
    got = chart_match.camera_records(c.cams, c.W, c.H)
    want = ref.camera_records(c.cams, c.W, c.H).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (3, 44) and got.tobytes() == want.tobytes()
    assert abs(chart_match.spatial_extent(c.cams) - ref.spatial_extent(c.cams)) <= 1e-12
    assert chart_match.MATCHING_THR_FACTOR == 1.0 / 20.0 and chart_match.MAX_TERMS == 2 ** 26
    N = c.H * c.W
    assert ref.pack_words(c.matches).shape == (3, 3, (N + 31) // 32)
    ws = hip_lib.g4s_chart_match_workspace(3, c.H, c.W)
    assert 3 * N * 8 + 3 * ((N + 255) // 256) * 4 <= ws <= 3 * N * 8 + 3 * ((N + 255) // 256) * 4 + 1024
    assert hip_lib.g4s_chart_match_workspace(1, 8192, 8192) > 0 and hip_lib.g4s_chart_match_workspace(1, 8192, 8193) == 0
    assert hip_lib.g4s_chart_match_workspace(0, 4, 4) == 0
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused by the host-side checks
    assert hip_lib.g4s_chart_match(0, 5, 7, p, p, 0.1, p, None, 0, None, None) != 0
    assert "n must be positive" in _lib.last_error()
    assert hip_lib.g4s_chart_match_loss_forward(1, 8192, 8193, p, p, p, None, 1.0, p, p, 1 << 40, None) != 0
    assert "at most 2^26" in _lib.last_error()
    assert hip_lib.g4s_chart_match_loss_backward(2, 5, 7, p, p, p, p, 1e7, p, p, p, 1 << 40, None) != 0
    assert "at most 2^26" in _lib.last_error() and "weight_max" in _lib.last_error()
    assert hip_lib.g4s_chart_match_loss_backward(2, 5, 7, p, p, p, p, float("nan"), p, p, p, 1 << 40, None) != 0
    assert "finite bound" in _lib.last_error()
    assert hip_lib.g4s_chart_match_loss_forward(2, 5, 7, p, p, p, None, 1.0, p, p, 16, None) != 0
    assert "workspace too small" in _lib.last_error()
    assert hip_lib.g4s_chart_match_loss_forward(2, 5, 7, p, p, p, p, 1e7, p, p, 1 << 40, None) != 0
    assert "at most 2^26" in _lib.last_error()
    nul = ctypes.c_void_p(0)
    assert hip_lib.g4s_densify_stats(0, nul, nul, nul, nul, nul, nul, nul) == 0 and _lib.last_error() == ""  # a good call clears it
