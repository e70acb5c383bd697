"""Chart alignment losses (HIP, include/g4s_losses.h "Chart alignment losses": g4s_chart_align_*; g4splat_amd/chart_align.py)
against the float32 restatement of their contract (tests/chart_align_ref.py), bit for bit for the normals and the curvatures,
and against the reference's own float64 run (tests/golden/chart_align.npz, make_golden_chart_align.py) for the four means and
both gradients.

Means and gradients are MEASURED, not pinned to a constant, by the rule of test_gpu_chart_match.py: the yardstick of a
quantity is the largest error of the reference's float32 run against its float64 run (recorded in the golden; for the
generated case the float32 restatement against the float64 one), and the GPU may be off the float64 record by at most 4
yardsticks, with a floor of one float32 ulp of the largest entry.  The four means are held as one vector.  Every run prints
the figures.

Measured on an MI355X (relative to the largest float64 entry): on the golden cases the means are off the float64 record by at
most 7.5e-8 (small; yardstick 6.2e-8, floor 8.5e-8), the gradient to the depths by at most 1.4e-7 (noconf; yardstick 2.9e-6)
and the gradient to the confidence by at most 9.0e-8 (full; yardstick 6.1e-8: 1.5 yardsticks, the worst ratio)."""
import numpy as np
import pytest
import torch

import chart_align_ref as ref
from g4splat_amd import _lib, chart_align
from support import DEV, GOLDEN, dev, host, same_bits, twice

pytestmark = pytest.mark.gpu
MARGIN = 4.0
ALL = ref.GRADIENT | ref.NORMAL | ref.CURVATURE
TERM_FLAGS = (0, ref.GRADIENT, ref.NORMAL, ref.CURVATURE)


@pytest.fixture(scope="module")
def golden(hip_lib):
    import os
    return np.load(os.path.join(GOLDEN, "chart_align.npz"))


@pytest.fixture(scope="module")
def wide(hip_lib):
    """The generated case, 3 charts of 20x70 (several 256-pixel blocks per view, rows that straddle them, more than one
    tile both ways for any tile a kernel might use), with its restatement in float32 and float64, computed once."""
    from types import SimpleNamespace
    cams, d0, r, cur = ref.scene(3, 20, 70, seed=9)
    rng = np.random.default_rng(19)
    c = SimpleNamespace(name="wide", n=3, H=20, W=70, cams=cams, initial_depths=d0, reference_depths=r, depths=cur, lam=0.2,
                        confidence=rng.uniform(1.2, 4.0, d0.shape).astype(np.float32),
                        masks=(rng.random(d0.shape) < 0.8).astype(np.float32),
                        gradient_masks=(rng.random((3, 19, 69)) < 0.75).astype(np.float32))
    for t, T in ((32, np.float32), (64, np.float64)):
        args, kw = ref.case_inputs(c, T)
        gd, gc = ref.gradients(*args, **kw)
        setattr(c, f"s{t}", SimpleNamespace(means=ref.means(*args, **kw), grad=gd, conf_grad=gc))
    return c


def losses_of(c):
    return chart_align.AlignmentLosses(c.cams, dev(c.initial_depths), confidence_weighting=c.lam)


def run(a, c, flags=ALL, cotangents=(1.0, 1.0, 1.0, 1.0), confidence="case", masks="case", gradient_masks="case"):
    """(means [4], dL/ddepths, dL/dconfidence or None) on the host."""
    pick = lambda v, own: own if isinstance(v, str) else v  # noqa: E731
    conf, masks, gm = pick(confidence, c.confidence), pick(masks, c.masks), pick(gradient_masks, c.gradient_masks)
    to_dev = lambda v: v if isinstance(v, torch.Tensor) else dev(v)  # noqa: E731
    d = dev(c.depths).requires_grad_(True)
    cf = None if conf is None else dev(conf).requires_grad_(True)
    t = a.terms(d, dev(c.reference_depths), cf, to_dev(masks), to_dev(gm), use_gradient_loss=bool(flags & ref.GRADIENT),
                use_normal_loss=bool(flags & ref.NORMAL), use_curvature_loss=bool(flags & ref.CURVATURE))
    assert t.shape == (4,) and t.dtype == torch.float32
    g = torch.autograd.grad((t * dev(np.asarray(cotangents, np.float32))).sum(), [d] if cf is None else [d, cf])
    return host(t), host(g[0]), None if cf is None else host(g[1])


def within_yardstick(label, got, want64, yard_abs):
    """got against the float64 record: at most MARGIN times the yardstick's largest error, floor one float32 ulp of the
    largest entry; returns (error, yardstick) relative to the largest float64 entry."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    top = np.abs(want64).max()
    if top == 0:
        assert not got.any(), label
        return 0.0, 0.0
    err, yard, floor = np.abs(got - want64).max() / top, float(yard_abs) / top, float(np.spacing(np.float32(top))) / top
    print(f"{label}: error {err:.3e}, yardstick {yard:.3e}, floor {floor:.3e}")
    assert err <= max(MARGIN * yard, floor), (label, err, yard, floor)
    return err, yard


def check_bits(c):
    a = losses_of(c)
    for what, depths in (("initial", c.initial_depths), ("current", c.depths)):
        nu = ref.normals(c.cams, depths, np.float32)
        kappa = ref.curvatures(nu)[..., None]
        got = chart_align.depth2normal_parallel(dev(depths), c.cams)
        same_bits(got, nu, f"{c.name}: normals of the {what} depths")
        same_bits(chart_align.normal2curv_parallel(got), kappa, f"{c.name}: curvatures of the {what} depths")
        same_bits(chart_align.normal2curv_parallel(got, mask=torch.ones_like(got, dtype=torch.bool)), np.repeat(kappa, 3, axis=-1),
                  f"{c.name}: curvatures under the reference's mask of ones")
        assert not host(got)[:, 0].any() and not host(got)[:, -1].any() and not host(got)[:, :, 0].any() and not host(got)[:, :, -1].any()
    same_bits(a.initial_normals, ref.normals(c.cams, c.initial_depths, np.float32), f"{c.name}: initial_normals")
    same_bits(a.initial_curvatures, ref.curvatures(ref.normals(c.cams, c.initial_depths, np.float32))[..., None],
              f"{c.name}: initial_curvatures")
    return a


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_normals_and_curvatures_bit_for_bit_on_the_golden_cases(golden, name):
    c = ref.load_case(golden, name)
    check_bits(c)
    if c.H < 3 or c.W < 3:
        assert not host(chart_align.depth2normal_parallel(dev(c.depths), c.cams)).any()


def test_normals_and_curvatures_bit_for_bit_on_the_generated_case(wide):
    check_bits(wide)
    # a list of [H,W] maps and a wrapper with .gs_cameras are taken as the stacked tensor and the list of cameras are
    from types import SimpleNamespace
    same_bits(chart_align.depth2normal_parallel(list(dev(wide.depths)), SimpleNamespace(gs_cameras=wide.cams)),
              ref.normals(wide.cams, wide.depths, np.float32), "list of maps")


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_means_and_gradients_within_the_references_own_error(golden, name):
    """All four terms on, cotangents (1, 1, 1, 1) and 0.37 of it, against the reference's float64 run.
    Measured on an MI355X, error / yardstick (both relative to the largest entry), cases one, flat_rows, flat_cols, small,
    full, noconf: means 1.1e-8 / 1.2e-7, 2.2e-9 / 1.3e-8, 2.5e-9 / 1.2e-8, 7.5e-8 / 6.2e-8, 8.0e-9 / 1.4e-8, 8.0e-9 / 1.4e-8;
    dL/ddepths 4.8e-8 / 4.8e-8, 4.0e-8 / 4.0e-8, 3.6e-8 / 3.6e-8, 8.9e-8 / 2.8e-7, 1.4e-7 / 2.9e-6, 1.4e-7 / 2.9e-6; dL/dconfidence
    3.6e-8 / 3.6e-8, 4.5e-8 / 7.5e-8, 3.6e-8 / 8.3e-8, 5.3e-8 / 7.9e-8, 9.0e-8 / 6.1e-8 (floor 8.9e-8); at cotangent 0.37 the
    ratios are within a factor of 1.5 of these.  Where error and yardstick coincide the kernel performs the float32
    operations that torch performed."""
    c = ref.load_case(golden, name)
    a = losses_of(c)
    m1, gd1, gc1 = run(a, c)
    m2, gd2, gc2 = run(a, c, cotangents=(c.cotangent,) * 4)
    same_bits(m2, m1, "the means do not depend on the cotangent")
    assert gd1.shape == c.depths.shape and gd1.dtype == np.float32
    within_yardstick(f"{name} means", m1, c.r64.means, np.abs(c.means32.astype(np.float64) - c.r64.means).max())
    within_yardstick(f"{name} dL/ddepths", gd1, c.r64.grad[4], c.grad_yard[0, 4])
    within_yardstick(f"{name} dL/ddepths, cotangent 0.37", gd2, c.r64.grad_c037[4], c.grad_yard[1, 4])
    assert np.abs(gd1).max() > 0 and not np.array_equal(gd1, gd2)  # the cotangent reached the kernel
    if c.confidence is None:
        assert gc1 is None
    else:
        within_yardstick(f"{name} dL/dconfidence", gc1, c.r64.conf_grad, c.conf_grad_yard[0])
        within_yardstick(f"{name} dL/dconfidence, cotangent 0.37", gc2, c.r64.conf_grad_c037, c.conf_grad_yard[1])
    if c.H < 3 or c.W < 3:
        assert m1[2] == 1.0 and m1[3] == 0.0  # no interior: the normal mean is exactly 1, the curvature mean exactly 0


def test_generated_case_within_the_float32_restatement(wide):
    """3 x 20 x 70 with confidence, masks and gradient masks; the yardstick is the float32 restatement against the float64
    one.  A generated scene avoids no kink; where float32 and float64 decide one differently the yardstick carries it.
    Measured on an MI355X: means 1.9e-8 (yardstick 4.4e-8), dL/ddepths 2.1e-7 and dL/dconfidence 6.3e-8, both the
    yardstick's own figure."""
    m, gd, gc = run(losses_of(wide), wide)
    within_yardstick("wide means", m, wide.s64.means, np.abs(wide.s32.means.astype(np.float64) - wide.s64.means).max())
    within_yardstick("wide dL/ddepths", gd, wide.s64.grad, np.abs(wide.s32.grad.astype(np.float64) - wide.s64.grad).max())
    within_yardstick("wide dL/dconfidence", gc, wide.s64.conf_grad, np.abs(wide.s32.conf_grad.astype(np.float64) - wide.s64.conf_grad).max())


def test_means_fold_beyond_one_trip(hip_lib):
    """2 x 256 x 513, all four terms on, with confidence: 2 x 513 = 1026 block partials with a ragged last block per view, so
    two threads of the one-workgroup fold add two rows each.  The four means by the rule of the generated case above (the
    float64 restatement, the float32 one as the yardstick); two runs, the same bits."""
    from types import SimpleNamespace
    cams, d0, r, cur = ref.scene(2, 256, 513, seed=23)
    c = SimpleNamespace(name="fold", n=2, H=256, W=513, cams=cams, initial_depths=d0, reference_depths=r, depths=cur, lam=0.2,
                        confidence=np.random.default_rng(29).uniform(1.2, 4.0, d0.shape).astype(np.float32), masks=None,
                        gradient_masks=None)
    a = losses_of(c)
    with torch.no_grad():
        m = twice(lambda: host(a.terms(dev(c.depths), dev(c.reference_depths), dev(c.confidence), use_gradient_loss=True,
                                       use_normal_loss=True, use_curvature_loss=True)))
    m32, m64 = (ref.means(*args, **kw) for args, kw in (ref.case_inputs(c, T) for T in (np.float32, np.float64)))
    assert (m64 > 0).all()
    within_yardstick("fold means", m, m64, np.abs(m32.astype(np.float64) - m64).max())


def test_means_fold_beyond_four_loads(hip_lib):
    """2 x 1024 x 513, all four terms on, with confidence: 2 x 2052 = 4104 block partials (K = 4), so eight threads of the
    one-workgroup fold take a second trip of four row loads of which only the first is a row.  The four means by the rule of
    the test above; two runs, the same bits.  Measured on an MI355X: error 1.9e-8, yardstick 6.2e-8."""
    from types import SimpleNamespace
    cams, d0, r, cur = ref.scene(2, 1024, 513, seed=31)
    c = SimpleNamespace(name="fold4", n=2, H=1024, W=513, cams=cams, initial_depths=d0, reference_depths=r, depths=cur, lam=0.2,
                        confidence=np.random.default_rng(37).uniform(1.2, 4.0, d0.shape).astype(np.float32), masks=None,
                        gradient_masks=None)
    a = losses_of(c)
    with torch.no_grad():
        m = twice(lambda: host(a.terms(dev(c.depths), dev(c.reference_depths), dev(c.confidence), use_gradient_loss=True,
                                       use_normal_loss=True, use_curvature_loss=True)))
    m32, m64 = (ref.means(*args, **kw) for args, kw in (ref.case_inputs(c, T) for T in (np.float32, np.float64)))
    assert (m64 > 0).all()
    within_yardstick("fold4 means", m, m64, np.abs(m32.astype(np.float64) - m64).max())


@pytest.mark.parametrize("name", ("small", "full"))
def test_each_term_alone(golden, name):
    """Term k with the others switched off: its mean has the bits it has with all terms on, the other slots are exactly 0,
    and its gradient is the reference's gradient of that mean alone -- also when all terms are on and only its cotangent is
    not zero, and at cotangent 0.37, where the value is unchanged and the gradient scaled.  Measured on an MI355X on case
    full, error / yardstick of dL/ddepths for terms 0..3: 6.5e-8 / 6.5e-8, 2.0e-8 / 2.0e-8, 2.0e-7 / 4.4e-6, 1.7e-7 / 3.1e-6; on
    case small 4.6e-8 / 4.6e-8, 3.0e-8 / 3.0e-8, 1.5e-6 / 2.9e-6, 1.1e-7 / 4.6e-7."""
    c = ref.load_case(golden, name)
    a = losses_of(c)
    every, _gd, _gc = run(a, c)
    for k, flags in enumerate(TERM_FLAGS):
        e_k = tuple(1.0 if t == k else 0.0 for t in range(4))
        m, gd, gc = run(a, c, flags=flags)
        assert m[k] != 0
        same_bits(m[k], every[k], f"mean {k} alone")
        assert all(m[t] == 0 and not np.signbit(m[t]) for t in range(1, 4) if t != k)
        m_e, gd_e, gc_e = run(a, c, cotangents=e_k)
        same_bits(m_e, every, "the means do not depend on the cotangent")
        within_yardstick(f"{name} term {k}, cotangent e_k: dL/ddepths", gd_e, c.r64.grad[k], c.grad_yard[0, k])
        m_s, gd_s, gc_s = run(a, c, cotangents=tuple(c.cotangent * v for v in e_k))
        same_bits(m_s, every, "the means do not depend on the cotangent")
        within_yardstick(f"{name} term {k}, cotangent 0.37 e_k: dL/ddepths", gd_s, c.r64.grad_c037[k], c.grad_yard[1, k])
        if k == 0:
            within_yardstick(f"{name} term 0 alone: dL/ddepths", gd, c.r64.grad[0], c.grad_yard[0, 0])
            within_yardstick(f"{name} term 0: dL/dconfidence", gc_e, c.r64.conf_grad, c.conf_grad_yard[0])
            within_yardstick(f"{name} term 0, cotangent 0.37: dL/dconfidence", gc_s, c.r64.conf_grad_c037, c.conf_grad_yard[1])
        else:
            # flags = k alone still carries the depth term (it cannot be switched off): take it out by its cotangent
            _m, gd_k, gc_k = run(a, c, flags=flags, cotangents=e_k)
            within_yardstick(f"{name} term {k} alone: dL/ddepths", gd_k, c.r64.grad[k], c.grad_yard[0, k])
            assert not gc_k.any() and not gc_e.any()


def test_options(golden):
    """confidence=None, masks of ones against no mask (the same bits), masks of zeros (a zero mean and no gradient)."""
    c = ref.load_case(golden, "full")
    a = losses_of(c)
    ones, gones = np.ones_like(c.depths), np.ones((c.n, c.H - 1, c.W - 1), np.float32)
    plain = run(a, c, masks=None, gradient_masks=None)
    same_bits(run(a, c, masks=ones, gradient_masks=gones), plain, "masks of ones")
    same_bits(run(a, c, masks=dev(ones).bool(), gradient_masks=dev(gones).bool()), plain, "boolean masks of ones")
    m, gd, gc = run(a, c, flags=ref.GRADIENT, masks=np.zeros_like(c.depths), gradient_masks=np.zeros_like(gones))
    assert m[0] == 0 and m[1] == 0 and not gd.any() and not gc.any()
    m, gd, gc = run(a, c, confidence=None)
    assert gc is None
    n = ref.load_case(golden, "noconf")  # the same scene without confidence and masks
    same_bits((m[1:], ), (run(losses_of(n), n, gradient_masks=c.gradient_masks)[0][1:], ), "the other terms do not read the confidence")
    # the weighted sum with optimize's names and defaults: gradient 10, normal 2, no curvature
    d = dev(c.depths)
    t = a.terms(d, dev(c.reference_depths), dev(c.confidence), use_gradient_loss=True, use_curvature_loss=False)
    want = (t[0] + 10.0 * t[1]) + 2.0 * t[2]
    assert float(t[3]) == 0.0
    same_bits(a.loss(d, dev(c.reference_depths), dev(c.confidence)), want, "loss")


def test_forward_and_backward_are_bit_reproducible(wide):
    a = losses_of(wide)
    twice(lambda: run(a, wide, cotangents=(0.37, 10.0, 2.0, 1.0)))
    twice(lambda: run(a, wide, flags=ref.NORMAL, confidence=None, masks=None))
    twice(lambda: host(losses_of(wide).initial_curvatures))


def test_capturable_in_a_hip_graph(wide):
    """Forward and backward captured in one graph (no allocation inside the library, no host synchronisation, the
    cotangents read on the device) and replayed on changed depths: the same bits as the direct calls."""
    a = losses_of(wide)
    static = dev(wide.initial_depths).requires_grad_(True)
    conf = dev(wide.confidence).requires_grad_(True)
    r, masks, gm = dev(wide.reference_depths), dev(wide.masks), dev(wide.gradient_masks)
    cot = dev(np.array([1.0, 10.0, 2.0, 0.37], np.float32))

    def step():
        t = a.terms(static, r, conf, masks, gm, use_gradient_loss=True)
        gd, gc = torch.autograd.grad((t * cot).sum(), [static, conf])
        return t.detach().clone(), gd, gc

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
        static.copy_(dev(wide.depths))
    graph.replay()
    torch.cuda.synchronize(DEV)
    want = step()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert bool((want[0] > 0).all()) and bool(want[1].any()) and bool(want[2].any())


def test_errors(hip_lib):
    cams, d0, r, cur = ref.scene(2, 5, 7, seed=1)
    d = dev(d0)
    with pytest.raises(ValueError, match="one size"):
        chart_align.AlignmentLosses(cams, [d[0], d[1][:, :6]])
    with pytest.raises(ValueError, match="n = 0"):
        chart_align.AlignmentLosses(cams, d[:0])
    with pytest.raises(ValueError, match="2 views but 1 initial_depths"):
        chart_align.AlignmentLosses(cams, d[:1])
    with pytest.raises(ValueError, match="HIP device"):
        chart_align.AlignmentLosses(cams, torch.tensor(d0))
    with pytest.raises(ValueError, match="2 views but 1 depths"):
        chart_align.depth2normal_parallel(d[:1], cams)
    with pytest.raises(ValueError, match=r"\[n,H,W,3\]"):
        chart_align.normal2curv_parallel(d)
    a = chart_align.AlignmentLosses(cams, d)
    with pytest.raises(ValueError, match="initial depths' shape"):
        a.terms(dev(np.zeros((2, 5, 8), np.float32)), d)
    with pytest.raises(ValueError, match="reference_depths must have the shape"):
        a.terms(d, d[:1])
    with pytest.raises(ValueError, match="confidence must have"):
        a.terms(d, d, confidence=d[:, :4])
    with pytest.raises(ValueError, match="gradient_masks must have the shape"):
        a.terms(d, d, gradient_masks=d, use_gradient_loss=True)
    row = chart_align.AlignmentLosses(cams, d[:, :1])
    with pytest.raises(ValueError, match="gradient term needs H >= 2"):
        row.terms(d[:, :1], d[:, :1], use_gradient_loss=True)
    t = row.terms(d[:, :1], dev(r)[:, :1])  # one row: no interior, no gradient term
    assert host(t).tolist()[1:] == [0.0, 1.0, 0.0]
    # the library itself refuses what the wrapper would let through, and launches nothing
    out = torch.full((4,), 7.0, device=DEV)
    ws = torch.empty(hip_lib.g4s_chart_align_workspace(2, 5, 7), dtype=torch.uint8, device=DEV)
    args = (_lib.ptr(a._cams), _lib.ptr(d), _lib.ptr(d), None, None, _lib.ptr(d), None, _lib.ptr(a.initial_normals),
            _lib.ptr(a._initial_curv), 0.2)
    assert hip_lib.g4s_chart_align_forward(2, 5, 7, *args, 7, _lib.ptr(out), _lib.ptr(ws), 64, _lib.stream(DEV)) != 0
    assert "workspace too small" in _lib.last_error()
    assert hip_lib.g4s_chart_align_forward(0, 5, 7, *args, 7, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream(DEV)) != 0
    assert "n must be positive" in _lib.last_error()
    assert hip_lib.g4s_chart_align_forward(2, 1, 35, *args, 1, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream(DEV)) != 0
    assert "gradient term needs H >= 2" in _lib.last_error()
    assert hip_lib.g4s_chart_align_workspace(1, 16384, 43691) == 0 and hip_lib.g4s_chart_align_workspace(0, 5, 7) == 0
    torch.cuda.synchronize(DEV)
    assert host(out).tolist() == [7.0] * 4
