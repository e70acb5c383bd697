"""Chart matcher (HIP, include/g4s_losses.h "Chart matcher": g4s_chart_match*; g4splat_amd/chart_match.py) against the
float32 restatement of its contract (tests/chart_match_ref.py), bit for bit where a decision or a stored float is
concerned, and against the reference's own float64 run (tests/golden/chart_match.npz, make_golden_chart_match.py) for the
loss and its gradient.

Loss and gradient are MEASURED, not pinned to a constant: the yardstick of a case is the error of the reference's float32
run against its float64 run (both in the golden; for the generated cases the float32 restatement against the float64 one),
relative for the loss, the largest absolute error over the largest float64 entry for the gradient.  The GPU may be off
the float64 record by at most 4 yardsticks -- another, equally valid summation order over the n^2 H W terms, and the
fixed-point reduction of the tap scatter -- with a floor of one float32 ulp of the largest entry.  Beside it every case is
held to the FLOAT32 restatement element by element, within a bound on what another order of the same sums can change
(same_terms_other_order): that is the tight check where a scene avoids no decision edge.

Measured on an MI355X (every run prints the figures): on the golden cases the loss is off the float64 record by at most
1.21e-6 relative (n4, whose yardstick is 4.76e-7: 2.5 yardsticks, the worst ratio), the gradient by at most 5.76e-6 of the
largest entry (n3, yardstick 4.37e-6)."""
import os

import numpy as np
import pytest
import torch

import chart_match_ref as ref
from g4splat_amd import chart_match
from support import DEV, dev, host, same_bits, twice

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chart_match.npz")
MARGIN = 4.0


@pytest.fixture(scope="module")
def golden(hip_lib):
    return np.load(G)


@pytest.fixture(scope="module")
def six(hip_lib):
    """The generated case n = 6 at 64x96 with its restatement, computed once."""
    cams, depths = ref.generated_scene(6, 64, 96, seed=3)
    thr = 0.12
    matches, errors, fov = ref.match(cams, depths, thr)
    cur = (depths * (1.0 + 0.01 * np.sin(np.arange(depths.size, dtype=np.float64).reshape(depths.shape)))).astype(np.float32)
    weights = np.random.default_rng(8).uniform(0.25, 3.0, depths.shape).astype(np.float32)
    return dict(cams=cams, depths=depths, thr=thr, matches=matches, errors=errors, fov=fov, cur=cur, weights=weights)


def matcher_of(cams, depths, thr):
    m = chart_match.ChartMatcher(cams, reference_depths=dev(depths))
    m.match(thr)
    return m


def check_decisions(m, cams, ref_depths, cur_depths, thr):
    matches, errors, fov = ref.match(cams, ref_depths, thr)
    same_bits(host(m.words).view(np.uint32), ref.pack_words(matches), "words")
    same_bits(m.reference_matches, matches, "reference_matches")
    same_bits(m.reference_errors, errors, "reference_errors")
    e, f = m.compute_reprojection_errors(depths=dev(cur_depths))
    want_e, want_f = ref.reprojection_errors(cams, cur_depths)
    same_bits(f, want_f, "fov_mask")
    same_bits(e, want_e, "errors")
    e0, f0 = m.compute_reprojection_errors(depths=dev(ref_depths))
    same_bits(f0, fov, "fov_mask at the reference depths")
    return matches


def loss_and_grad(m, depths, weights=None, cotangent=1.0, weight_max=None):
    d = dev(depths).requires_grad_(True)
    value = m.loss(d, None if weights is None else dev(weights), weight_max=weight_max)
    (grad,) = torch.autograd.grad(cotangent * value, d)
    return host(value), host(grad)


def within_yardstick(label, got, want64, yard32):
    """got against the float64 record, at most MARGIN times the float32 yardstick's error (floor: one float32 ulp of the
    largest entry); returns (error, yardstick), both relative to the largest float64 entry."""
    got, want64, yard32 = (np.asarray(a, np.float64) for a in (got, want64, yard32))
    top = np.abs(want64).max()
    err, yard = np.abs(got - want64).max() / top, np.abs(yard32 - want64).max() / top
    floor = float(np.spacing(np.float32(top))) / top
    print(f"{label}: error {err:.3e}, yardstick {yard:.3e}, floor {floor:.3e}, off the float32 yardstick itself {np.abs(got - yard32).max() / top:.3e}")
    assert err <= max(MARGIN * yard, floor), (label, err, yard, floor)
    return err, yard


def same_terms_other_order(label, value, grad, cams, depths, matches, weights=None, cotangent=1.0, weight_max=None):
    """The device against the FLOAT32 restatement, which forms the same float32 terms: the two may differ only by the order
    and the format of their sums, element by element within chart_match_ref.summation_bound (a first-order bound worked out
    from the terms themselves) and, for the loss, loss_sum_bound.  This is the tight check of the scenes that avoid no
    decision edge, where float32 and float64 may decide a pair differently and the float64 yardstick is wide."""
    v32 = ref.loss(cams, depths, matches, weights, np.float32, weight_max)
    g32, bound = ref.loss_grad(cams, depths, matches, weights, cotangent, np.float32, weight_max, with_bound=True)
    n, H, W = depths.shape
    dv, bv = abs(float(value) - float(v32)), ref.loss_sum_bound(n, H * W, v32)
    dg = np.abs(np.asarray(grad, np.float64) - g32.astype(np.float64))
    worst = int(np.argmax(np.where(bound > 0, dg / np.where(bound > 0, bound, 1.0), np.where(dg > 0, np.inf, 0.0))))
    top = float(np.abs(g32).max())
    print(f"{label}: loss off the float32 restatement by {dv:.3e} (bound {bv:.3e}); gradient by at most {dg.max():.3e} = "
          f"{dg.max() / top:.3e} of the largest entry, the element nearest to its bound {dg.reshape(-1)[worst]:.3e} of {bound.reshape(-1)[worst]:.3e}")
    assert dv <= bv, (label, dv, bv)
    assert (dg <= bound).all(), (label, int((dg > bound).sum()), dg.reshape(-1)[worst], bound.reshape(-1)[worst])


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_decisions_bit_for_bit_on_the_golden_cases(golden, name):
    """words, reference_matches, reference_errors, fov_mask and the dense errors equal the float32 restatement, which on
    these cases decides every pair as the reference did (test_chart_match_cpu.py)."""
    c = ref.load_case(golden, name)
    m = matcher_of(c.cams, c.ref_depths, c.thr)
    matches = check_decisions(m, c.cams, c.ref_depths, c.cur_depths, c.thr)
    assert np.array_equal(matches, c.matches)


def test_decisions_bit_for_bit_on_the_generated_case(six):
    m = matcher_of(six["cams"], six["depths"], six["thr"])
    check_decisions(m, six["cams"], six["depths"], six["cur"], six["thr"])
    assert six["matches"].any() and (six["fov"] & ~six["matches"]).any() and not six["fov"][5, :5].any()


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_loss_and_gradient_within_the_references_own_error(golden, name):
    """Both cotangents against the reference's float64 run, the yardstick being its float32 run.  Measured on an MI355X,
    error / yardstick: loss 7.3e-7 / 6.0e-7 (n1), 6.8e-7 / 9.0e-7 (n2), 9.7e-7 / 1.3e-6 (n3), 1.2e-6 / 4.8e-7 (n4); gradient
    1.2e-6 / 1.1e-6 (n1), 1.1e-6 / 7.0e-7 (n2), 5.8e-6 / 4.4e-6 (n3), 7.8e-7 / 1.1e-6 (n4); cotangent 0.37 within 2 % of these."""
    c = ref.load_case(golden, name)
    m = matcher_of(c.cams, c.ref_depths, c.thr)
    wmax = None if c.weights is None else float(np.abs(c.weights).max())
    v1, g1 = loss_and_grad(m, c.cur_depths, c.weights, 1.0, wmax)
    v2, g2 = loss_and_grad(m, c.cur_depths, c.weights, c.cotangent, wmax)
    assert v1.ndim == 0 and g1.shape == c.cur_depths.shape and g1.dtype == np.float32
    same_bits(v2, v1, "the loss does not depend on the cotangent")
    within_yardstick(f"{name} loss", v1, c.r64.loss, c.r32.loss)
    within_yardstick(f"{name} gradient", g1, c.r64.grad, c.r32.grad)
    within_yardstick(f"{name} gradient, cotangent 0.37", g2, c.r64.grad_c037, c.r32.grad_c037)
    assert np.abs(g1).max() > 0 and not np.array_equal(g1, g2)  # the cotangent reached the kernel
    same_terms_other_order(name, v2, g2, c.cams, c.cur_depths, c.matches, c.weights, c.cotangent, wmax)


def test_generated_case_within_the_float32_restatement(six):
    """n = 6 at 64x96, with and without weights; the yardstick is the float32 restatement against the float64 one.  Measured
    on an MI355X: loss 2.1e-8 (yardstick 1.5e-7); gradient 9.5e-3, the yardstick's own figure to four digits -- a generated scene avoids
    no edge, and where float32 and float64 decide a pair differently they do so on the device as in the restatement."""
    m = matcher_of(six["cams"], six["depths"], six["thr"])
    for label, w in (("n6", None), ("n6 weighted", six["weights"])):
        want = [f(six["cams"], six["cur"], six["matches"], w, ftype=t) for t in (np.float64, np.float32) for f in (ref.loss, ref.loss_grad)]
        v, g = loss_and_grad(m, six["cur"], w, 1.0, None if w is None else 3.0)
        within_yardstick(label + " loss", v, want[0], want[2])
        within_yardstick(label + " gradient", g, want[1], want[3])
        same_terms_other_order(label, v, g, six["cams"], six["cur"], six["matches"], w, 1.0, None if w is None else 3.0)


def test_loss_fold_beyond_one_trip(hip_lib):
    """n = 2 at 256x513: 2 x 513 = 1026 block partials with a ragged last block per view, so two threads of the one-workgroup
    fold add two rows each.  The loss against the float64 restatement with the float32 one as the yardstick and, against the
    float32 one, within loss_sum_bound -- the two checks of the loss in the tests above; two runs, the same bits."""
    n, H, W, thr = 2, 256, 513, 0.12
    cams, depths = ref.generated_scene(n, H, W, seed=5)
    matches, _errors, _fov = ref.match(cams, depths, thr)
    cur = (depths * (1.0 + 0.01 * np.sin(np.arange(depths.size, dtype=np.float64).reshape(depths.shape)))).astype(np.float32)
    m = matcher_of(cams, depths, thr)
    same_bits(host(m.words).view(np.uint32), ref.pack_words(matches), "words")
    with torch.no_grad():
        v = twice(lambda: host(m.loss(dev(cur))))
    v64, v32 = (ref.loss(cams, cur, matches, ftype=t) for t in (np.float64, np.float32))
    assert matches.any() and float(v64) > 0
    within_yardstick("2x256x513 loss", v, v64, v32)
    dv, bv = abs(float(v) - float(v32)), ref.loss_sum_bound(n, H * W, v32)
    print(f"2x256x513: loss off the float32 restatement by {dv:.3e} (bound {bv:.3e})")
    assert dv <= bv, (dv, bv)


def test_loss_fold_beyond_four_loads(hip_lib):
    """n = 2 at 700x751: 2 x 2054 = 4108 block partials (K = 1) with a ragged last block per view, so twelve threads of the
    one-workgroup fold take a second trip of four row loads of which only the first is a row.  The two checks of the loss
    of the test above; two runs, the same bits.  Measured on an MI355X: error 8.4e-7, yardstick 4.9e-7; off the float32
    restatement by 1.5e-8 (bound 1.2e-7)."""
    n, H, W, thr = 2, 700, 751, 0.12
    cams, depths = ref.generated_scene(n, H, W, seed=7)
    matches, _errors, _fov = ref.match(cams, depths, thr)
    cur = (depths * (1.0 + 0.01 * np.sin(np.arange(depths.size, dtype=np.float64).reshape(depths.shape)))).astype(np.float32)
    m = matcher_of(cams, depths, thr)
    same_bits(host(m.words).view(np.uint32), ref.pack_words(matches), "words")
    with torch.no_grad():
        v = twice(lambda: host(m.loss(dev(cur))))
    v64, v32 = (ref.loss(cams, cur, matches, ftype=t) for t in (np.float64, np.float32))
    assert matches.any() and float(v64) > 0
    within_yardstick("2x700x751 loss", v, v64, v32)
    dv, bv = abs(float(v) - float(v32)), ref.loss_sum_bound(n, H * W, v32)
    print(f"2x700x751: loss off the float32 restatement by {dv:.3e} (bound {bv:.3e})")
    assert dv <= bv, (dv, bv)


def test_forward_and_backward_are_bit_reproducible(six):
    m = matcher_of(six["cams"], six["depths"], six["thr"])
    twice(lambda: loss_and_grad(m, six["cur"], six["weights"], 0.37, 3.0))
    twice(lambda: loss_and_grad(m, six["cur"]))
    twice(lambda: host(matcher_of(six["cams"], six["depths"], six["thr"]).words))


def test_matches_stay_frozen(six):
    """After match() on the references the loss at other depths uses the old bits: it equals the restatement given those
    bits, and differs from the restatement given the matches of the new depths."""
    m = matcher_of(six["cams"], six["depths"], six["thr"])
    moved = (six["depths"] * np.float32(1.03)).astype(np.float32)
    moved[0] = six["depths"][0] * np.float32(0.9)
    v, g = loss_and_grad(m, moved)
    want = [f(six["cams"], moved, six["matches"], None, ftype=t) for t in (np.float64, np.float32) for f in (ref.loss, ref.loss_grad)]
    within_yardstick("frozen loss", v, want[0], want[2])
    within_yardstick("frozen gradient", g, want[1], want[3])
    same_terms_other_order("frozen", v, g, six["cams"], moved, six["matches"])
    rematched, _e, _f = ref.match(six["cams"], moved, six["thr"])
    assert not np.array_equal(rematched, six["matches"])
    assert abs(float(ref.loss(six["cams"], moved, rematched, None, np.float64)) - float(want[0])) > 1e-3 * float(want[0])
    same_bits(host(m.words).view(np.uint32), ref.pack_words(six["matches"]), "words after loss()")


def test_weights_of_one_and_of_zero(six):
    m = matcher_of(six["cams"], six["depths"], six["thr"])
    plain = loss_and_grad(m, six["cur"], None, 0.37)
    same_bits(loss_and_grad(m, six["cur"], np.ones_like(six["cur"]), 0.37), plain, "weights of one")
    v, g = loss_and_grad(m, six["cur"], np.zeros_like(six["cur"]), 0.37)
    assert float(v) == 0.0 and not g.any()


def test_a_weight_bound_that_is_too_small_clamps_value_and_gradient_alike(six):
    """weights up to 3 under weight_max = 1.5: forward and backward both use min(w, 1.5), so the gradient is still the
    gradient of the value returned -- both equal the restatement with the clamped weights, and differ from the unclamped."""
    m = matcher_of(six["cams"], six["depths"], six["thr"])
    v, g = loss_and_grad(m, six["cur"], six["weights"], 1.0, 1.5)
    same_terms_other_order("clamped weights", v, g, six["cams"], six["cur"], six["matches"], six["weights"], 1.0, 1.5)
    same_bits(loss_and_grad(m, six["cur"], np.minimum(six["weights"], np.float32(1.5)), 1.0, 1.5), (v, g), "weights clamped by the caller")
    full = loss_and_grad(m, six["cur"], six["weights"], 1.0, 3.0)
    assert float(full[0]) > 1.1 * float(v)


@pytest.mark.parametrize("n,H,W,thr", [(1, 7, 9, 0.3), (1, 1, 40, 3.0), (2, 1, 40, 3.0)])
def test_one_view_and_one_row(hip_lib, n, H, W, thr):
    cams, depths = ref.generated_scene(n, H, W, seed=11)
    m = matcher_of(cams, depths, thr)
    cur = (depths * np.float32(1.01)).astype(np.float32)
    matches = check_decisions(m, cams, depths, cur, thr)
    assert matches.any() and not matches.all()
    want = [f(cams, cur, matches, None, ftype=t) for t in (np.float64, np.float32) for f in (ref.loss, ref.loss_grad)]
    v, g = loss_and_grad(m, cur)
    within_yardstick(f"{n}x{H}x{W} loss", v, want[0], want[2])
    within_yardstick(f"{n}x{H}x{W} gradient", g, want[1], want[3])
    same_terms_other_order(f"{n}x{H}x{W}", v, g, cams, cur, matches)


def test_capturable_in_a_hip_graph(six):
    """Forward and backward captured in one graph (no allocation inside the library, no host synchronisation, the
    cotangent read on the device) and replayed on changed depths: the same bits as the direct calls."""
    m = matcher_of(six["cams"], six["depths"], six["thr"])
    static = dev(six["depths"]).requires_grad_(True)
    weights = dev(six["weights"])
    cot = torch.tensor(0.37, device=DEV)

    def step():
        v = m.loss(static, weights, weight_max=3.0)
        (g,) = torch.autograd.grad(v * cot, static)
        return v.detach().clone(), g

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    with torch.no_grad():
        static.copy_(dev(six["cur"]))
    graph.replay()
    torch.cuda.synchronize(DEV)
    want = step()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert float(want[0]) > 0 and bool(want[1].any())


def test_errors(hip_lib):
    cams, depths = ref.generated_scene(2, 5, 7, seed=1)
    d = dev(depths)
    with pytest.raises(ValueError, match="one size"):
        chart_match.ChartMatcher(cams, reference_depths=[d[0], d[1][:, :6]])
    with pytest.raises(ValueError, match="n = 0"):
        chart_match.ChartMatcher([], reference_depths=d[:0])
    with pytest.raises(ValueError, match="n = 0"):
        chart_match.ChartMatcher(cams, reference_depths=d[:0])
    with pytest.raises(ValueError, match="Either reference_pts or reference_depths"):
        chart_match.ChartMatcher(cams)
    with pytest.raises(ValueError, match="HIP device"):
        chart_match.ChartMatcher(cams, reference_depths=torch.tensor(depths))
    m = chart_match.ChartMatcher(cams, reference_depths=d)
    with pytest.raises(RuntimeError, match="match\\(\\) first"):
        m.loss(d)
    with pytest.raises(NotImplementedError, match="Normal threshold"):
        m.match(0.1, normal_threshold=0.5)
    m.match(0.1)
    before = host(m.words).copy()
    with pytest.raises(ValueError, match="references' shape"):
        m.loss(dev(np.zeros((2, 5, 8), np.float32)))
    with pytest.raises(ValueError, match="references' shape"):
        m.compute_reprojection_errors(depths=d[:1])
    with pytest.raises(ValueError, match="range limit 2\\^26"):
        m.loss(d, torch.ones_like(d), weight_max=1e7)
    with pytest.raises(ValueError, match="weights must have"):
        m.loss(d, torch.ones_like(d)[:, :4])
    # the library itself refuses what the wrapper would let through
    from g4splat_amd import _lib
    one = torch.zeros(1, device=DEV)
    ws = torch.empty(hip_lib.g4s_chart_match_workspace(2, 5, 7), dtype=torch.uint8, device=DEV)
    rc = hip_lib.g4s_chart_match_loss_backward(2, 5, 7, _lib.ptr(m._cams), _lib.ptr(d), _lib.ptr(m.words), _lib.ptr(d), 1e7,
                                               _lib.ptr(one), _lib.ptr(torch.empty_like(d)), _lib.ptr(ws), ws.numel(), _lib.stream(DEV))
    assert rc != 0 and "at most 2^26" in _lib.last_error()
    assert hip_lib.g4s_chart_match_workspace(1, 8193, 8192) == 0 and hip_lib.g4s_chart_match_workspace(0, 5, 7) == 0
    rc = hip_lib.g4s_chart_match(0, 5, 7, _lib.ptr(m._cams), _lib.ptr(d), 0.1, _lib.ptr(m.words), None, 0, None, _lib.stream(DEV))
    assert rc != 0 and "n must be positive" in _lib.last_error()
    torch.cuda.synchronize(DEV)
    same_bits(host(m.words), before, "words after the refused calls")  # nothing was launched


def test_reference_points_and_default_threshold(hip_lib):
    """update_references from points (their view-space z), and match(None) = spatial_extent / 20."""
    cams, depths = ref.generated_scene(3, 9, 12, seed=4)
    a = matcher_of(cams, depths, None)
    assert a.matching_thr == pytest.approx(ref.spatial_extent(cams) / 20.0, rel=1e-12)
    assert chart_match.spatial_extent(cams) == pytest.approx(ref.spatial_extent(cams), rel=1e-12)
    r = ref.evaluate(cams, depths, np.float64)
    rec = ref.camera_records(cams, 12, 9)
    yy, xx = np.meshgrid(np.arange(9.0), np.arange(12.0), indexing="ij")
    pts = np.stack([np.stack([(rec[v, 3 + 3 * k] * xx + rec[v, 4 + 3 * k] * yy + rec[v, 5 + 3 * k]) * depths[v] + rec[v, k]
                              for k in range(3)], -1) for v in range(3)])
    b = chart_match.ChartMatcher(cams, reference_pts=dev(pts.astype(np.float32)))
    assert r.n == 3 and np.abs(host(b.reference_depths) - depths).max() <= 1e-5
