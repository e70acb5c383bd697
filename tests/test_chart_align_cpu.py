"""The chart alignment losses' contract (tests/chart_align_ref.py, the numpy restatement of include/g4s_losses.h "Chart
alignment losses") against the reference's own results (tests/golden/chart_align.npz, make_golden_chart_align.py).  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import chart_align_ref as ref

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chart_align.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(G)


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = np.abs(want).max()
    return float(np.abs(got - want).max()) if top == 0 else float(np.abs(got - want).max() / top)


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_float64_restatement_equals_the_reference(golden, name):
    """Normals, curvatures, the four means and both gradients -- of each mean alone and of the sum, at cotangents 1 and
    0.37 -- to 1e-12 of the largest entry."""
    c = ref.load_case(golden, name)
    args, kw = ref.case_inputs(c, np.float64)
    ev = ref.evaluate(*args, **kw)
    assert ev.g.nu.shape == (c.n, c.H, c.W, 3) and rel(ev.g.nu, c.r64.normals) <= 1e-12
    assert rel(ev.kappa[..., None], c.r64.curvatures) <= 1e-12
    assert rel(ev.means, c.r64.means) <= 1e-12
    for cot, want, want_conf in ((1.0, c.r64.grad, c.r64.conf_grad), (c.cotangent, c.r64.grad_c037, c.r64.conf_grad_c037)):
        for k in range(5):
            cots = [cot if k in (t, 4) else 0.0 for t in range(4)]
            gd, gc = ref.gradients(*args, cotangents=cots, **kw)
            assert gd.shape == want[k].shape and rel(gd, want[k]) <= 1e-12, (name, cot, k, rel(gd, want[k]))
            if k in (0, 4) and want_conf is not None:
                assert rel(gc, want_conf) <= 1e-12, (name, cot, k)
            elif gc is not None:
                assert not gc.any()
    if c.H < 3 or c.W < 3:  # no interior: every normal is 0
        assert not ev.g.nu.any() and ev.means[2] == 1.0 and ev.means[3] == 0.0


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_float32_kink_decisions_equal_the_float64_ones(golden, name):
    """The generator keeps every kink quantity at least 2^-12 from zero or exactly on it, so the contract's float32
    operations have to give each the sign the float64 run gave it -- the exact zeros (the corners' lap and kappa) included."""
    c = ref.load_case(golden, name)
    (a32, k32), (a64, k64) = ref.case_inputs(c, np.float32), ref.case_inputs(c, np.float64)
    q32, q64 = ref.kink_quantities(ref.evaluate(*a32, **k32)), ref.kink_quantities(ref.evaluate(*a64, **k64))
    for what in q64:
        a = np.abs(q64[what])
        assert not ((a > 0) & (a < 2.0 ** -12)).any(), what
        assert np.array_equal(np.sign(q32[what]), np.sign(q64[what])), what
    assert (q64["lap"][:, 0, 0] == 0).all() and (q64["kappa0 - kappa"][:, 0, 0] == 0).all()


@pytest.mark.parametrize("name", ("full", "noconf"))
def test_float32_restatement_within_the_references_own_error(golden, name):
    """The float32 restatement against the float64 record, by the yardstick of the GPU test: at most 4 times the error of
    the reference's float32 run, floor one float32 ulp of the largest entry."""
    c = ref.load_case(golden, name)
    args, kw = ref.case_inputs(c, np.float32)
    gd, gc = ref.gradients(*args, **kw)
    top = np.abs(c.r64.grad[4]).max()
    assert np.abs(gd - c.r64.grad[4]).max() <= max(4.0 * c.grad_yard[0, 4], float(np.spacing(np.float32(top))))
    if gc is not None:
        top = np.abs(c.r64.conf_grad).max()
        assert np.abs(gc - c.r64.conf_grad).max() <= max(4.0 * c.conf_grad_yard[0], float(np.spacing(np.float32(top))))


def test_analytic_gradient_against_central_differences(golden):
    """n = 2 at 4x5 in float64: every element of both gradients of a weighted sum of the four means."""
    c = ref.load_case(golden, "small")
    args, kw = ref.case_inputs(c, np.float64)
    cots = (1.0, 10.0, 2.0, 1.0)
    gd, gc = ref.gradients(*args, cotangents=cots, **kw)

    def value(depths, conf):
        k = dict(kw, confidence=conf)
        return float(np.dot(ref.means(args[0], depths, *args[2:], **k), cots))

    h = 1e-7
    D, C = c.depths.astype(np.float64), c.confidence.astype(np.float64)
    for which, got in (("depths", gd), ("confidence", gc)):
        want = np.zeros_like(D)
        for i in range(D.size):
            step = np.zeros(D.size)
            step[i] = h
            step = step.reshape(D.shape)
            if which == "depths":
                want.reshape(-1)[i] = (value(D + step, C) - value(D - step, C)) / (2 * h)
            else:
                want.reshape(-1)[i] = (value(D, C + step) - value(D, C - step)) / (2 * h)
        assert np.abs(want).max() > 0 and rel(got, want) <= 1e-6, (which, rel(got, want))


def test_a_term_that_is_off_is_zero_and_gives_no_gradient(golden):
    c = ref.load_case(golden, "small")
    args, kw = ref.case_inputs(c, np.float64)
    for flags in (0, ref.GRADIENT, ref.NORMAL | ref.CURVATURE):
        m = ref.means(*args, flags=flags, **kw)
        gd, _gc = ref.gradients(*args, flags=flags, cotangents=(0.0, 1.0, 1.0, 1.0), **kw)
        for k, bit in ((1, ref.GRADIENT), (2, ref.NORMAL), (3, ref.CURVATURE)):
            assert (m[k] != 0) == bool(flags & bit)
        assert gd.any() == bool(flags)


def test_workspace_and_refusals_on_the_host(hip_lib):
    """What the entry points decide without a device: the workspace holds the block partials and three [n,H,W,3] maps, and
    every refusal names its reason."""
    from g4splat_amd import _lib
    n, H, W = 3, 33, 50
    N, blocks = H * W, 3 * ((H * W + 255) // 256)
    ws = hip_lib.g4s_chart_align_workspace(n, H, W)
    assert 3 * n * N * 12 + blocks * 32 <= ws <= 3 * n * N * 12 + blocks * 32 + 2048
    assert hip_lib.g4s_chart_align_workspace(0, 4, 4) == 0 and hip_lib.g4s_chart_align_workspace(2, 0, 4) == 0
    assert hip_lib.g4s_chart_align_workspace(1, 16384, 43690) > 0 and hip_lib.g4s_chart_align_workspace(1, 16384, 43691) == 0
    p, nul = ctypes.c_void_p(256), ctypes.c_void_p(0)  # never dereferenced: every call below is refused by the host-side checks
    big = 1 << 40

    def forward(n, H, W, flags, ws_bytes=big, d0=p):
        return hip_lib.g4s_chart_align_forward(n, H, W, p, p, p, nul, nul, d0, nul, p, p, 0.2, flags, p, p, ws_bytes, None)

    def backward(n, H, W, flags, ws_bytes=big, dconf=p):
        return hip_lib.g4s_chart_align_backward(n, H, W, p, p, p, p, nul, p, nul, p, p, 0.2, flags, p, p, dconf, p, ws_bytes, None)

    for call in (forward, backward):
        assert call(0, 5, 7, 7) != 0 and "n must be positive" in _lib.last_error()
        assert call(2, 5, 0, 7) != 0 and "width, height must be positive" in _lib.last_error()
        assert call(1, 16384, 43691, 7) != 0 and "fewer than 2^31" in _lib.last_error()
        assert call(2, 5, 7, 7, 64) != 0 and "workspace too small" in _lib.last_error()
        assert call(2, 1, 7, 1) != 0 and "gradient term needs H >= 2" in _lib.last_error()
        assert call(2, 7, 1, 1) != 0 and "gradient term needs H >= 2" in _lib.last_error()
        assert call(2, 5, 7, 8) != 0 and "unknown bits" in _lib.last_error()
    assert forward(2, 5, 7, 1, d0=nul) != 0 and "initial_depths" in _lib.last_error()
    assert backward(2, 5, 7, 6, dconf=nul) != 0 and "NULL required pointer" in _lib.last_error()
    assert hip_lib.g4s_chart_align_normals(0, 5, 7, p, p, p, p, None) != 0 and "n must be positive" in _lib.last_error()
    assert hip_lib.g4s_chart_align_normals(2, 5, 7, p, p, nul, nul, None) != 0 and "no output" in _lib.last_error()
    assert hip_lib.g4s_chart_align_normals(2, 5, 7, nul, nul, nul, p, None) != 0 and "without depths" in _lib.last_error()
    assert hip_lib.g4s_densify_stats(0, nul, nul, nul, nul, nul, nul, nul) == 0 and _lib.last_error() == ""  # a good call clears it


def test_ray_records_are_the_matchers(golden):
    from g4splat_amd import chart_align, chart_match
    c = ref.load_case(golden, "full")
    got = chart_align.ray_records(c.cams, c.W, c.H)
    assert got.dtype == np.float32 and got.shape == (3, 12)
    assert got.tobytes() == chart_match.camera_records(c.cams, c.W, c.H)[:, :12].tobytes()
    assert got.tobytes() == ref.ray_records(c.cams, c.W, c.H).astype(np.float32).tobytes()
