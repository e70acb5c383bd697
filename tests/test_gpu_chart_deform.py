"""Chart deformation (HIP, include/g4s_losses.h "Chart deformation": g4s_chart_deform_*; g4splat_amd/chart_deform.py) against
the reference's own float64 run (tests/golden/chart_deform.npz, make_golden_chart_deform.py) and, for generated cases, against
the float64 restatement of the contract (tests/chart_deform_ref.py).

Depths, delta and the gradient to every parameter are MEASURED by the rule of test_gpu_chart_align.py: the yardstick of a
quantity is the largest error of the reference's float32 run against its float64 run (recorded in the golden; for a generated
case the float32 restatement against the float64 one), and the GPU may be off the float64 record by at most 4 yardsticks,
with a floor of one float32 ulp of the largest entry.  Every run prints the figures.

Measured on an MI355X, the worst error as a share of its limit per case: one 0.85 (the last bias under cotangent 1: error
5.1e-8 of the largest entry, yardstick 9.2e-9, floor 6.0e-8), small 0.62, single 0.73, full 0.49 (the second bias: error 2.7e-7,
yardstick 1.4e-7), wide 0.66; depths and delta sit at one yardstick or below everywhere."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chart_deform_ref as ref
from g4splat_amd import _lib, chart_align, chart_deform, chart_match
from support import DEV, GOLDEN, dev, host, same_bits, twice
from test_chart_deform_cpu import module_of

pytestmark = pytest.mark.gpu
MARGIN = 4.0


@pytest.fixture(scope="module")
def golden(hip_lib):
    return np.load(os.path.join(GOLDEN, "chart_deform.npz"))


def generated(name, seed, shape=None):
    """A generated case with its restatement in float32 and float64, computed once, in the golden cases' form."""
    c = ref.make_case(name, seed, shape)
    if c.bins:
        c.coords = ref.depth_coordinates(c.d0, c.bins)
    c = ref.settle(c)  # every ReLU decided alike in float32 and float64: the yardsticks measure rounding, not flips
    c.cotangent = np.random.default_rng(seed).uniform(-1, 1, c.d0.shape).astype(np.float32)
    runs = {}
    for t, T in ((32, np.float32), (64, np.float64)):
        f = ref.forward(c, T)
        runs[t] = SimpleNamespace(delta=f.delta, depths=f.depths,
                                  grads={tag: ref.flat_gradients(c, ref.gradients(c, g, T))
                                         for tag, g in (("g", c.cotangent), ("ones", np.ones_like(c.cotangent)))})
    c.r64 = runs[64]
    worst = lambda a, b: float(np.abs(a.astype(np.float64) - b).max())  # noqa: E731
    c.yard = SimpleNamespace(delta=worst(runs[32].delta, runs[64].delta), depths=worst(runs[32].depths, runs[64].depths),
                             grads={tag: {k: worst(runs[32].grads[tag][k], v) for k, v in runs[64].grads[tag].items()}
                                    for tag in ("g", "ones")})
    return c


@pytest.fixture(scope="module")
def wide(hip_lib):
    """3 charts of 20 x 70, all defaults: rows that straddle the 64-pixel tiles, 22 tiles with a partial last one."""
    return generated("wide", 9)


@pytest.fixture(scope="module")
def edges(hip_lib):
    """2 charts whose pixel count is one workgroup and 52 pixels: two partials per chart for the fold, a partial last tile."""
    W = 68
    H = -(-(chart_deform.WORKGROUP_PIXELS + 1) // W)
    assert chart_deform.WORKGROUP_PIXELS < H * W < 2 * chart_deform.WORKGROUP_PIXELS and (H * W) % chart_deform.TILE_PIXELS
    return generated("edges", 17, (2, H, W, (0.05, 0.1, 0.2, 0.4), 8, 64, 3, 30))


def loaded(c, **more):
    """The case's module on the device with the case's parameters."""
    m = module_of(c, device=DEV, **more)
    m.load_reference_state_dict({k: torch.from_numpy(v) for k, v in ref.parameters(c).items()})
    if c.bins:
        same_bits(m.depth_coords, c.coords.reshape(c.n, -1), f"{c.name}: depth_coords")
    return m


def run(m, cotangent):
    """(depths, {name: gradient}) on the host for sum(cotangent * depths)"""
    m.zero_grad(set_to_none=True)
    d = m.deformed_depths()
    assert d.shape == (m.n, m.height, m.width) and d.dtype == torch.float32
    (d * (cotangent if isinstance(cotangent, torch.Tensor) else dev(cotangent))).sum().backward()
    return host(d), {k: host(p.grad) for k, p in m.named_parameters()}


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


def check_case(c):
    m = loaded(c)
    same = None
    for tag, g in (("g", c.cotangent), ("ones", np.ones_like(c.cotangent))):
        depths, grads = run(m, g)
        if same is not None:
            same_bits(depths, same, "the depths do not depend on the cotangent")
        same = depths
        within_yardstick(f"{c.name} depths", depths, c.r64.depths, c.yard.depths)
        assert set(grads) == set(c.r64.grads[tag])
        for k, want in c.r64.grads[tag].items():
            assert grads[k].dtype == np.float32 and grads[k].any(), k
            within_yardstick(f"{c.name} {tag} d/d{k}", grads[k], want, c.yard.grads[tag][k])
    within_yardstick(f"{c.name} delta", host(m.deformations()), c.r64.delta, c.yard.delta)
    zero = c.d0 == 0
    assert np.array_equal(same[zero], c.d0[zero])  # a zero depth stays exactly 0
    return m


@pytest.mark.parametrize("name", ref.GOLDEN_CASES)
def test_golden_cases_within_the_references_own_error(golden, name):
    check_case(ref.load_case(golden, name))


def test_generated_case_within_the_float32_restatement(wide):
    assert (wide.d0 == 0).sum() == 5
    check_case(wide)


def test_partial_last_tile_and_two_workgroups_per_chart(edges):
    m = check_case(edges)
    per_chart = -(-edges.H * edges.W // chart_deform.WORKGROUP_PIXELS)
    params = sum(p.numel() for p in m.parameters() if p.dim() < 4) // edges.n  # weights, biases, depth encoding of one chart
    E = edges.channels * len(edges.levels)
    lower = 4 * (edges.n * edges.H * edges.W * E + edges.n * per_chart * params)
    assert per_chart == 2 and lower <= m.workspace_bytes <= lower + 3 * 256  # dL/dx and the partials, nothing of hidden width


def twin(c, which):
    """Two charts from chart 0 of `c`: equal inputs and different weights ('weights'), or equal weights and different
    encodings ('encodings').  The radii of `c` are kept."""
    pick = lambda a, i: a[i:i + 1]  # noqa: E731
    src = {"weights": (0, 0, 0, 1), "encodings": (0, 1, 0, 0)}[which]  # chart 1's inputs, encodings, (unused), weights
    both = lambda a, j: np.concatenate([pick(a, 0), pick(a, src[j])])  # noqa: E731
    t = SimpleNamespace(**vars(c))
    t.name, t.n = f"twin-{which}", 2
    t.cams, t.d0, t.coords = [c.cams[0], c.cams[0]], both(c.d0, 0), both(c.coords, 0)
    t.levels, t.denc = [both(v, 1) for v in c.levels], both(c.denc, 1)
    t.weights, t.biases = [both(v, 3) for v in c.weights], [both(v, 3) for v in c.biases]
    return t


def solo(t, i):
    """Chart i of a twin as a case of its own."""
    s = SimpleNamespace(**vars(t))
    s.name, s.n = f"{t.name}[{i}]", 1
    s.cams, s.d0, s.coords = [t.cams[i]], t.d0[i:i + 1], t.coords[i:i + 1]
    s.levels, s.denc = [v[i:i + 1] for v in t.levels], t.denc[i:i + 1]
    s.weights, s.biases = [v[i:i + 1] for v in t.weights], [v[i:i + 1] for v in t.biases]
    return s


@pytest.mark.parametrize("which", ["weights", "encodings"])
def test_every_chart_reads_its_own_parameters(wide, which):
    """A chart of a two-chart call computes, bit for bit, what it computes alone: a chart index dropped anywhere -- weights,
    biases, encodings, coordinates, the partials' fold -- would show."""
    t = twin(wide, which)
    g = wide.cotangent[:2]
    both = run(loaded(t, spatial_extent_override=wide.extent), g)
    assert not np.array_equal(both[0][0], both[0][1])
    for i in range(2):
        alone = run(loaded(solo(t, i), spatial_extent_override=wide.extent), g[i:i + 1])
        same_bits(both[0][i:i + 1], alone[0], f"{which}: depths of chart {i}")
        for k, v in alone[1].items():
            same_bits(both[1][k][i:i + 1], v, f"{which}: d/d{k} of chart {i}")


def test_bit_identical_from_run_to_run(edges):
    m = loaded(edges)

    def once():
        depths, grads = run(m, edges.cotangent)
        return [depths] + [grads[k] for k in sorted(grads)]

    twice(once)


def test_zero_cotangent_gives_exactly_zero_gradients(wide):
    _d, grads = run(loaded(wide), np.zeros_like(wide.cotangent))
    for k, g in grads.items():
        assert not g.any(), k


def loss_step(m, losses, matcher, reference):
    d = m.deformed_depths()
    return losses.loss(d, reference) + matcher.loss(d)


def test_feeds_the_alignment_and_matching_losses_and_replays_from_a_graph(wide):
    """deformed_depths() -> AlignmentLosses.loss + ChartMatcher.loss, one backward() to every parameter; forward plus backward
    captured in a HIP graph replay bit-identically to the eager call, on changed parameters."""
    m = loaded(wide)
    d0 = dev(wide.d0)
    losses = chart_align.AlignmentLosses(wide.cams, d0)
    reference = dev((wide.d0.astype(np.float64) * 1.01).astype(np.float32))
    matcher = chart_match.ChartMatcher(wide.cams, reference_depths=reference)
    matcher.match()
    params = list(m.parameters())

    def step():
        loss = loss_step(m, losses, matcher, reference)
        return [loss.detach().clone()] + list(torch.autograd.grad(loss, params))

    eager = step()
    assert all(bool(g.any()) for g in eager[1:]) and bool(torch.isfinite(eager[0]))
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
        for p in params:
            p.mul_(0.75)
    graph.replay()
    torch.cuda.synchronize(DEV)
    want = step()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert not torch.equal(want[1], eager[1])


def test_twenty_adam_steps_end_with_the_same_parameters_in_two_runs(golden):
    """The optimiser of prepare_for_optimization (Adam, eps 1e-15, 1e-2 for the encodings and 1e-3 for the MLP) on case full
    under the alignment losses: no float atomics anywhere, so two runs agree bit for bit."""
    c = ref.load_case(golden, "full")
    reference = dev((c.d0.astype(np.float64) * 1.02).astype(np.float32))

    def train():
        m = loaded(c)
        losses = chart_align.AlignmentLosses(c.cams, dev(c.d0))
        groups = [{"params": [p], "lr": 1e-2 if k.endswith("encodings") else 1e-3, "name": k} for k, p in m.named_parameters()]
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        for _ in range(20):
            opt.zero_grad(set_to_none=True)
            losses.loss(m.deformed_depths(), reference).backward()
            opt.step()
        return [host(p) for p in m.parameters()]

    first = twice(train)
    start = list(ref.parameters(c).values())
    assert all(not np.array_equal(a, b) for a, b in zip(first, start))  # every parameter moved


def test_the_library_refuses_before_any_launch(hip_lib, wide):
    """A shape outside the envelope, a missing pointer and a short workspace return an error with the limit in its message."""
    m = loaded(wide)
    bad = _lib.G4sChartDeformShape.from_buffer_copy(m._shape)
    bad.layer_size = 48
    assert hip_lib.g4s_chart_deform_workspace(ctypes.byref(bad)) == 0 and "32 or 64" in _lib.last_error()
    for field, value, what in (("channels", 6, "multiple of 4"), ("levels", 9, "encoding levels"), ("layers", 5, "layers"),
                               ("bins", 5000, "depth bins"), ("n", 0, "no charts"), ("scene_radius", 0.0, "scene_radius")):
        bad = _lib.G4sChartDeformShape.from_buffer_copy(m._shape)
        setattr(bad, field, value)
        assert hip_lib.g4s_chart_deform_workspace(ctypes.byref(bad)) == 0 and what in _lib.last_error(), (field, _lib.last_error())
    p = [t.detach() for t in m._params()]
    head = list(m._call_head(p))
    out = torch.empty((m.n, m.height, m.width), device=DEV)
    null = ctypes.c_void_p(0)
    with pytest.raises(RuntimeError, match="NULL required pointer"):
        _lib.call("g4s_chart_deform_forward", *head, null, null, null, 0, _lib.stream(DEV))
    grads = [torch.empty_like(t) for t in p]
    lv, de, ws, bs = m._split(grads)
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call("g4s_chart_deform_backward", *head, _lib.ptr(out), _lib.ptrs(lv), _lib.ptr(de), _lib.ptrs(ws), _lib.ptrs(bs), null, 0,
                  _lib.stream(DEV))
