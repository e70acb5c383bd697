"""Depth cues on the MI355X (g4splat_amd.depth_cues, csrc/tsdf/depth_cues.hip).

Coefficients.  The device's float32 alpha, beta against the restatement's (exact sums, tests/depth_cues_ref.py), within one
float32 unit in the last place.  The bar is derived, not measured: with at most 2^20 masked pixels the float64 accumulation of
the five sums is within 2^20 * 2^-53 ~ 1.2e-10 of exact, relatively; the numerator and the denominator of beta lose at most
the inverse of the share that survives their cancellation, asserted to be at least 1 %, which leaves 1e-8 relative -- under
half a unit of float32 (6e-8).  So the device rounds to the float32 the exact value rounds to, or to its neighbour where
the exact value sits on a rounding boundary.
Per-pixel stages.  Fed the device's own coefficients, every map equals the float32 restatement bit for bit.
Golden.  The reference-named entry points and refine_depths_with_planes against the reference's float64 results, within
twice the recorded yardstick (the device's float32 steps are not the reference's and may round the other way); decisions
exactly, on the compared set.
Sizes.  The same bars where the kernels take another trip or another branch: views of more than 64 spans (the second and
third trip of the coefficient kernel's fold, partial rows behind a long view), id runs of 0 to 65 sparse ids with masks
that hold every fitted id and unfitted ones around them, an inpainted view larger than every input view, the float mask at
equality, NaN and the infinities, the plane clamp in both signs and at zero, and the ends of the two workspaces that hold
more than a view table."""
import numpy as np
import pytest
import torch

import depth_cues_ref as dr
from g4splat_amd import depth_cues, visibility
from support import DEV, dev, devs, hosts, load_depth_cues_golden, same_bits

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
SPAN = 4096  # ALIGN_SPAN of csrc/tsdf/depth_cues.hip: 256 threads of 16 pixels


def _within_one_ulp(got, want, what=""):
    got, want = f32(got), f32(want)
    if not np.isfinite(want):
        assert (np.isnan(got) and np.isnan(want)) or got == want, (what, got, want)  # the same NaN / inf pattern
        return
    err, ulp = abs(f64(got) - f64(want)), f64(np.spacing(np.abs(want)))
    print(f"{what}: device {got!r}, exact {want!r}, {err / ulp:.2f} ulp")
    assert err <= ulp, (what, got, want)


@pytest.fixture(scope="module")
def golden():
    return load_depth_cues_golden()


def _scene(sizes, seed):
    """Per view (H, W): a disparity in 0.2 .. 2, the depth of a noisy affine map of it, and a mask of about two thirds."""
    rng = np.random.default_rng(seed)
    disps, depths, masks = [], [], []
    for H, W in sizes:
        d = rng.uniform(0.2, 2.0, (H, W)).astype(f32)
        depths.append((1.0 / (0.07 + 0.55 * d + rng.normal(0, 0.01, (H, W)))).astype(f32))
        disps.append(d)
        masks.append(rng.random((H, W)) < 0.66)
    return disps, depths, masks


def _check_coeffs(disps, depths, masks, domain):
    code = {"disparity": dr.DISPARITY, "depth": dr.DEPTH}[domain]
    aligned, coeffs, counts = depth_cues.align_disparities(devs(disps), devs(depths), devs(masks), domain)
    again = depth_cues.align_disparities(devs(disps), devs(depths), devs(masks), domain)
    assert coeffs.dtype == torch.float32 and counts.dtype == torch.int32 and coeffs.device == DEV
    same_bits(coeffs, again[1], "two runs")
    got, n = coeffs.cpu().numpy(), counts.cpu().numpy()
    for v in range(len(disps)):
        alpha, beta, count = dr.align_coeffs(disps[v], depths[v], masks[v], code, f32)
        assert n[v] == count == int(np.asarray(masks[v]).sum())
        if np.isfinite(alpha) and np.isfinite(beta):  # the two conditions the one-ulp bar rests on
            assert count <= 2 ** 20 and dr.variance_share(disps[v], depths[v], masks[v], code, f32) >= 0.01
        _within_one_ulp(got[v, 0], alpha, f"view {v} alpha")
        _within_one_ulp(got[v, 1], beta, f"view {v} beta")
        # the aligned map, from the device's own coefficients
        same_bits(aligned[v], dr.aligned(got[v, 0], got[v, 1], disps[v], code, f32), f"aligned {v}", nan_payload=False)
    return got


def test_span_constant_is_the_kernels():
    src = open(depth_cues.__file__.replace("depth_cues.py", "csrc/tsdf/depth_cues.hip")).read()
    assert "constexpr int ALIGN_ITEMS = 16;" in src and "constexpr int ALIGN_SPAN = 256 * ALIGN_ITEMS;" in src
    assert SPAN == 256 * 16 == depth_cues.ALIGN_SPAN


@pytest.mark.parametrize("domain", ["disparity", "depth"])
@pytest.mark.parametrize("sizes", [[(1, SPAN - 1)], [(1, SPAN)], [(1, SPAN + 1)], [(3, 2731)],  # 3 * 2731 = 2 * SPAN + 1
                                   [(1, SPAN + 1), (45, 67), (2, SPAN)], [(48, 64), (1, 2 * SPAN + 1), (7, 5), (64, 64)]],
                         ids=["span-1", "span", "span+1", "2span+1", "three-views", "four-views"])
def test_coefficients_within_one_ulp_of_exact(sizes, domain):
    assert 3 * 2731 == 2 * SPAN + 1
    disps, depths, masks = _scene(sizes, 11 + len(sizes))
    _check_coeffs(disps, depths, masks, domain)


def test_coefficients_of_degenerate_masks_follow_ieee():
    """None set, one pixel, two equal disparities, all set, a masked zero depth -- in one call, beside a sound view."""
    (d,), (g,), _m = _scene([(6, 700)], 5)
    d[0, :2] = 0.75
    none, one, equal, full = (np.zeros(d.shape, bool) for _ in range(4))
    one[3, 77] = True
    equal[0, :2] = True
    full[:] = True
    zero_depth = g.copy()
    zero_depth[5, 699] = 0.0
    disps, depths, masks = [d] * 5, [g, g, g, g, zero_depth], [none, one, equal, full, full]
    for domain in ("disparity", "depth"):
        got = _check_coeffs(disps, depths, masks, domain)
        assert np.isnan(got[0]).all() and not np.isfinite(got[1]).any() and not np.isfinite(got[2]).any()
        assert np.isfinite(got[3]).all()
        assert np.isfinite(got[4]).all() == (domain == "depth")  # 1 / 0 poisons the disparity domain only


# ---- past 64 spans: lane l of the coefficient kernel's one wave adds the partials l, l + 64, ...; a view of more than
# 64 * SPAN = 262 144 pixels (every real one: 800 x 600 has 118 spans) takes a second trip of that loop ----
LONG_VIEWS = {"64span": [(1, 64 * SPAN)], "64span+1": [(1, 64 * SPAN + 1)], "65span-tail": [(1, 65 * SPAN)],
              "128span+1": [(1, 128 * SPAN + 1)], "800x600": [(600, 800)],
              "four-views": [(1, 64 * SPAN + 1), (45, 67), (600, 800), (1, SPAN)]}
_long_scenes = {}


def _long_scene(name):
    """_scene(LONG_VIEWS[name], 17), made once and only read; "65span-tail" has its mask cleared below 64 spans, so that only
    the partial of the second trip counts."""
    if name not in _long_scenes:
        disps, depths, masks = _scene(LONG_VIEWS[name], 17)
        if name == "65span-tail":
            masks[0][:, :64 * SPAN] = False
            assert 0 < masks[0].sum() < SPAN
        _long_scenes[name] = disps, depths, masks
    return _long_scenes[name]


@pytest.mark.parametrize("domain", ["disparity", "depth"])
@pytest.mark.parametrize("name", list(LONG_VIEWS))
def test_coefficients_past_64_spans(name, domain):
    disps, depths, masks = _long_scene(name)
    got = _check_coeffs(disps, depths, masks, domain)
    assert np.isfinite(got).all()  # so _check_coeffs has asserted the two conditions of its bar for every view


def _refill_scene(sizes, seed):
    """Targets, mono depths, plane masks over 0 and 3, confidences: _scene's affine pair read in the third domain (1 / target
    against 1 / mono), so the bar of the coefficients holds as it does there."""
    disps, depths, confs = _scene(sizes, seed)
    rng = np.random.default_rng(seed + 1)
    monos = [(f32(1) / d).astype(f32) for d in disps]
    masks = [rng.choice(np.array([0, 0, 3], np.int32), s).astype(np.int32) for s in sizes]
    return depths, monos, masks, confs


def _check_refill(sizes, n_input, seed=17):
    """refill_unseen_regions against the restatement: counts exactly, coefficients within one unit, and -- fed the device's
    coefficients -- every depth bit for bit.  Returns the unfilled regions."""
    targets, monos, masks, confs = _refill_scene(sizes, seed)
    args = devs(targets), devs(monos), devs(masks), devs(confs)
    got, coeffs, counts = depth_cues.refill_unseen_regions(*args, n_input)
    assert all(torch.equal(a, dev(b)) for a, b in zip(args[0], targets))  # the inputs are only read
    coeffs, counts = coeffs.cpu().numpy(), counts.cpu().numpy()
    assert coeffs.shape == (len(sizes), 2) and counts.shape == (len(sizes),)
    regions = []
    for v in range(len(sizes)):
        g = got[v].cpu().numpy()
        region = (masks[v] == 0) & ~confs[v]
        regions.append(region)
        if v < n_input:
            same_bits(g, targets[v], f"input view {v}", nan_payload=False)
            assert not coeffs[v].any() and counts[v] == 0
            continue
        alpha, beta, n = dr.align_coeffs(monos[v], targets[v], confs[v], dr.INVERSE_SOURCE, f32)
        assert int(counts[v]) == n == int(confs[v].sum())
        if np.isfinite(alpha) and np.isfinite(beta):  # the two conditions the one-ulp bar rests on
            assert n <= 2 ** 20 and dr.variance_share(monos[v], targets[v], confs[v], dr.INVERSE_SOURCE, f32) >= 0.01
        _within_one_ulp(coeffs[v, 0], alpha, f"refill {v} alpha")
        _within_one_ulp(coeffs[v, 1], beta, f"refill {v} beta")
        filled = dr.aligned(coeffs[v, 0], coeffs[v, 1], monos[v], dr.INVERSE_SOURCE, f32)
        same_bits(g, np.where(region, filled, targets[v]), f"refill {v}", nan_payload=False)
    return regions, coeffs


def test_refill_coefficients_past_64_spans():
    """The third domain over a real view: an inpainted 800 x 600 behind a small input view."""
    _regions, coeffs = _check_refill([(45, 67), (600, 800)], 1)
    assert np.isfinite(coeffs[1]).all()


# ---- the refill's grid is sized by the inpainted views alone ----
@pytest.mark.parametrize("sizes, n_input, large", [([(3, 3), (2, 5), (48, 64)], 2, 2), ([(3, 3), (2, 5), (7, 5), (48, 64), (5, 7)], 2, 3),
                                                   ([(3, 3), (2, 5), (48, 64)], 0, 2), ([(3, 3), (2, 5), (48, 64)], 3, 2)],
                         ids=["large-last", "large-in-the-middle", "no-input-view", "input-views-only"])
def test_refill_reaches_the_end_of_an_inpainted_view_larger_than_the_input_views(sizes, n_input, large):
    pixels = [H * W for H, W in sizes]
    assert pixels[large] == max(pixels) and all(pixels[v] <= 256 for v in range(len(sizes)) if v != large)
    regions, _coeffs = _check_refill(sizes, n_input)
    assert regions[large][-1].any() and regions[large][:-1].any()  # the unfilled region reaches the last row


def _cams(golden, sizes):
    return [golden.cams[v % golden.V] for v in range(len(sizes))]


@pytest.mark.parametrize("sizes", [[(1, 1)], [(2, 5)], [(3, 3)], [(45, 67), (48, 64)], [(3, 3), (1, 1), (45, 67), (2, 5), (48, 64)]],
                         ids=["1x1", "2x5", "3x3", "mixed", "all"])
def test_cue_maps_equal_the_restatement(golden, sizes):
    cams = _cams(golden, sizes)
    disps, warps, _m = _scene(sizes, 3)
    rng = np.random.default_rng(9)
    alphas = [np.where(rng.random(d.shape) < 0.7, 0.97, 0.4).astype(f32) for d in disps]
    args = devs(disps), devs(warps), devs(alphas)
    before = [[t.clone() for t in a] for a in args]
    cues = depth_cues.view_geometry_cues(cams, *args, visible_threshold=0.9)
    for a, b in zip(args, before):
        assert all(torch.equal(x, y) for x, y in zip(a, b))  # inputs are only read
    coeffs, counts = cues.coeffs.cpu().numpy(), cues.counts.cpu().numpy()
    for v, (H, W) in enumerate(sizes):
        vis = alphas[v] > f32(0.9)
        alpha, beta, n = dr.align_coeffs(disps[v], warps[v], vis, dr.DISPARITY, f32)
        assert counts[v] == n
        _within_one_ulp(coeffs[v, 0], alpha, f"view {v} alpha")
        _within_one_ulp(coeffs[v, 1], beta, f"view {v} beta")
        want = dr.cue_maps(cams[v], disps[v], warps[v], alphas[v], 0.9, coeffs[v, 0], coeffs[v, 1], f32)
        assert cues.visibility[v].dtype == torch.bool and np.array_equal(cues.visibility[v].cpu().numpy(), want["visibility"])
        for name in ("mono_depth", "aligned_depth", "depth", "normal_world", "normal_cam"):
            got = getattr(cues, name)[v]
            assert got.shape == ((H, W, 3) if name.startswith("normal") else (H, W))
            same_bits(got, want[name], f"{name} {v}", nan_payload=False)
        if H < 3 or W < 3:
            assert not cues.normal_world[v].any() and not cues.normal_cam[v].any()
        else:
            assert cues.normal_world[v][1:-1, 1:-1].abs().sum() > 0
    # a stacked tensor is a list of its slices
    if len(set(sizes)) == 1:
        stacked = depth_cues.view_geometry_cues(cams, *(torch.stack(a) for a in args))
        assert all(torch.equal(a, b) for a, b in zip(stacked.normal_world, cues.normal_world))


def _plane_scene(golden, sizes, seed):
    """Depths, masks over the ids 0, 3, 12, 977, and planes that face the cameras, cross a horizon or are not fitted."""
    rng = np.random.default_rng(seed)
    cams = _cams(golden, sizes)
    depths = [rng.uniform(1.0, 4.0, s).astype(f32) for s in sizes]
    masks = [rng.choice(np.array([0, 3, 12, 977], np.int32), s).astype(np.int32) for s in sizes]
    V = len(sizes)
    planes = {10: ((0.1, 0.2, 0.97), (0.0, 0.0, 0.3)), 4: ((0.9, -0.1, 0.2), (0.4, 0.0, 0.0)), 7: ((0.0, 1.0, 0.05), (0.0, 0.6, 0.0))}
    gdict = {10: [(v, 3) for v in range(V)], 5: [(v, 12) for v in range(V)], 4: [(v, 977) for v in range(0, V, 2)],
             7: [(0, 3)] + [(v, 977) for v in range(1, V, 2)]}  # 5 is not fitted; (0, 3) is listed twice: 7 wins
    return cams, depths, masks, gdict, planes


@pytest.mark.parametrize("sizes", [[(1, 1)], [(2, 5)], [(3, 3)], [(45, 67), (48, 64)], [(48, 64), (1, 1), (45, 67), (2, 5), (3, 3)]],
                         ids=["1x1", "2x5", "3x3", "mixed", "all"])
def test_plane_depths_and_refill_equal_the_restatement(golden, sizes):
    cams, depths, masks, gdict, planes = _plane_scene(golden, sizes, 21)
    V = len(sizes)
    args = devs(depths), devs(masks)
    out, replaced, zeroed = depth_cues.apply_global_planes(cams, *args, gdict, planes)
    assert all(torch.equal(a, dev(b)) for a, b in zip(args[0], depths))  # the inputs are only read
    want, want_replaced, want_zeroed, touched, _valid = dr.apply_global_planes(cams, depths, masks, gdict, planes, f32)
    assert replaced.dtype == torch.int32 and np.array_equal(replaced.cpu().numpy(), want_replaced)
    assert np.array_equal(zeroed.cpu().numpy(), want_zeroed)
    for v in range(V):
        same_bits(out[v], want[v], f"plane depth {v}", nan_payload=False)
        assert np.array_equal(out[v].cpu().numpy()[~touched[v]], depths[v][~touched[v]])  # ids 0 and 12 keep their depth
    if max(H * W for H, W in sizes) > 100:
        assert want_replaced.sum() > 0 and want_zeroed.sum() > 0
    # the refill of the last two views (or of the only one), fed the device's coefficients
    rng = np.random.default_rng(2)
    n_input = max(V - 2, 0)
    monos = [(1.0 / rng.uniform(0.2, 2.0, s)).astype(f32) for s in sizes]
    targets = [rng.uniform(1.0, 4.0, s).astype(f32) for s in sizes]
    confs = [rng.random(s) < 0.5 for s in sizes]
    got, coeffs, counts = depth_cues.refill_unseen_regions(devs(targets), devs(monos), devs(masks), devs(confs), n_input)
    coeffs = coeffs.cpu().numpy()
    for v in range(V):
        g = got[v].cpu().numpy()
        if v < n_input:
            same_bits(g, targets[v], f"input view {v}", nan_payload=False)
            continue
        alpha, beta, n = dr.align_coeffs(monos[v], targets[v], confs[v], dr.INVERSE_SOURCE, f32)
        assert int(counts[v]) == n
        _within_one_ulp(coeffs[v, 0], alpha, f"refill {v} alpha")
        _within_one_ulp(coeffs[v, 1], beta, f"refill {v} beta")
        region = (masks[v] == 0) & ~confs[v]
        filled = dr.aligned(coeffs[v, 0], coeffs[v, 1], monos[v], dr.INVERSE_SOURCE, f32)
        same_bits(g, np.where(region, filled, targets[v]), f"refill {v}", nan_payload=False)


def test_plane_aligned_depth_of_a_whole_image(golden):
    n, c = golden.planes[6]
    cam = golden.cams[1]
    depth, valid = depth_cues.plane_aligned_depth(dev(n), dev(c), cam, (45, 67))
    z, ok = dr.plane_depth_image(n, c, cam, 45, 67, f32)
    assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), ok) and ok.any() and not ok.all()
    same_bits(depth, np.where(ok, z, f32(0)), "plane_aligned_depth", nan_payload=False)


# ---- the id search of the plane depths ----
def _check_planes(cams, depths, masks, gdict, planes):
    """apply_global_planes against the restatement: depths bit for bit, both counts exactly, untouched pixels keep their bits."""
    out, replaced, zeroed = depth_cues.apply_global_planes(cams, devs(depths), devs(masks), gdict, planes)
    want, want_replaced, want_zeroed, touched, _valid = dr.apply_global_planes(cams, depths, masks, gdict, planes, f32)
    print("replaced", want_replaced.tolist(), "zeroed", want_zeroed.tolist())
    assert replaced.dtype == zeroed.dtype == torch.int32
    assert np.array_equal(replaced.cpu().numpy(), want_replaced) and np.array_equal(zeroed.cpu().numpy(), want_zeroed)
    for v in range(len(cams)):
        got = out[v].cpu().numpy()
        same_bits(got, want[v], f"plane depth {v}", nan_payload=False)
        same_bits(got[~touched[v]], depths[v][~touched[v]], f"untouched {v}", nan_payload=False)
    return out, replaced, zeroed, (want_replaced, want_zeroed, touched)


@pytest.fixture(scope="module")
def id_scene():
    return dr.id_search_scene()


def test_plane_ids_are_found_in_runs_of_0_to_65_sparse_ids(golden, id_scene):
    """Runs of 2, 0, 1, 3, 7, 64 and 65 fitted ids in one call; every entry of every run covers a pixel, and the masks hold
    ids below, between and above the fitted ones, 0 and negative values (tests/test_depth_cues_cpu.py holds the scene to that)."""
    s = id_scene
    for v, ids in enumerate(dr.fitted_ids(s.gdict, s.planes, len(s.sizes))):
        assert len(ids) == dr.ID_RUNS[v] and all((s.masks[v] == p).any() for p in ids)
    _out, _r, _z, (replaced, zeroed, touched) = _check_planes(_cams(golden, s.sizes), s.depths, s.masks, s.gdict, s.planes)
    assert replaced.sum() > 0 and zeroed.sum() > 0 and not touched[1].any()
    for v in range(len(s.sizes)):
        assert np.array_equal(touched[v], np.isin(s.masks[v], s.fitted[v]))


def test_plane_depth_clamp_in_both_signs_at_zero_and_through_the_camera():
    """|n.d| < 1e-8 in every pixel of two mirrored planes, negative, zero and positive; a third plane through the camera
    centre (num = 0) is zeroed everywhere."""
    s = dr.clamp_scene()
    for pid in (1, 2):
        nd, _num, _len = dr.plane_terms(*s.planes[pid], s.cam, s.H, s.W, f32)
        nd = nd[s.mask == pid]
        assert (nd < 0).any() and (nd == 0).any() and ((nd > 0) & (nd < f32(1e-8))).any() and (np.abs(nd) < f32(1e-8)).all()
    assert dr.plane_terms(*s.planes[3], s.cam, s.H, s.W, f32)[1] == 0
    out, _r, _z, (replaced, zeroed, touched) = _check_planes([s.cam], [s.depth], [s.mask], s.gdict, s.planes)
    assert replaced[0] > 0 and zeroed[0] > (s.mask == 3).sum() > 0
    assert not out[0].cpu().numpy()[s.mask == 3].any()
    for pid in (1, 2):  # each plane alone, over the whole image
        n, c = (np.array(x, f32) for x in s.planes[pid])
        depth, valid = depth_cues.plane_aligned_depth(dev(n), dev(c), s.cam, (s.H, s.W))
        z, ok = dr.plane_depth_image(*s.planes[pid], s.cam, s.H, s.W, f32)
        assert ok.any() and not ok.all() and np.array_equal(valid.cpu().numpy(), ok)
        same_bits(depth, np.where(ok, z, f32(0)), f"clamped plane {pid}", nan_payload=False)


# ---- the float mask at its edges ----
@pytest.mark.parametrize("threshold", [0.9, 0.1], ids=["0.9", "0.1"])
def test_float_mask_at_equality_nan_and_infinities(golden, threshold):
    """alpha > threshold in float32: equal, one float32 above and below, NaN, +inf and -inf, each in pixels of their own."""
    sizes = [(45, 67), (48, 64)]
    cams = _cams(golden, sizes)
    disps, warps, _m = _scene(sizes, 23)
    rng = np.random.default_rng(29)
    t = f32(threshold)
    edges = [t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf)), f32(np.nan), f32(np.inf), f32(-np.inf)]
    visible = [False, True, False, False, True, False]
    alphas = []
    for d in disps:
        a = np.where(rng.random(d.shape) < 0.7, 0.97, 0.04).astype(f32).reshape(-1)
        where = rng.permutation(a.size)[:60 * len(edges)].reshape(len(edges), 60)
        for e, seen, idx in zip(edges, visible, where):
            a[idx] = e
            with np.errstate(invalid="ignore"):
                assert ((a[idx] > t) == seen).all()
        alphas.append(a.reshape(d.shape))
    cues = depth_cues.view_geometry_cues(cams, devs(disps), devs(warps), devs(alphas), visible_threshold=threshold)
    coeffs, counts = cues.coeffs.cpu().numpy(), cues.counts.cpu().numpy()
    for v in range(len(sizes)):
        with np.errstate(invalid="ignore"):
            vis = alphas[v] > t
        assert cues.visibility[v].dtype == torch.bool and np.array_equal(cues.visibility[v].cpu().numpy(), vis)
        assert counts[v] == int(vis.sum())
        alpha, beta, n = dr.align_coeffs(disps[v], warps[v], vis, dr.DISPARITY, f32)
        assert n == counts[v] and n <= 2 ** 20 and dr.variance_share(disps[v], warps[v], vis, dr.DISPARITY, f32) >= 0.01
        _within_one_ulp(coeffs[v, 0], alpha, f"view {v} alpha")
        _within_one_ulp(coeffs[v, 1], beta, f"view {v} beta")
        want = dr.cue_maps(cams[v], disps[v], warps[v], alphas[v], threshold, coeffs[v, 0], coeffs[v, 1], f32)
        assert np.array_equal(want["visibility"], vis)
        for name in ("mono_depth", "aligned_depth", "depth", "normal_world", "normal_cam"):
            same_bits(getattr(cues, name)[v], want[name], f"{name} {v}", nan_payload=False)


# ---- nothing is written behind the workspaces the two larger layouts ask for ----
def _canary(nbytes, shift):
    """A buffer of 0xA5 whose workspace of `nbytes` starts `shift` bytes in (the library aligns the base itself), its 4 KiB tail."""
    buf = torch.full((shift + nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[shift:], buf[shift + nbytes:]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "base+1"])
def test_align_workspace_is_enough(hip_lib, shift):
    """g4s_depth_align keeps its view table and the partials of 65 + 1 spans inside g4s_depth_align_workspace."""
    from g4splat_amd import _lib
    sizes = [(1, 64 * SPAN + 1), (45, 67)]
    disps, depths, masks = _scene(sizes, 17)
    src, tgt, msk = devs(disps), devs(depths), [m.view(torch.uint8) for m in devs(masks)]
    c_sizes = _lib.array(_lib.c_i, [x for H, W in sizes for x in (W, H)])
    nbytes = int(hip_lib.g4s_depth_align_workspace(len(sizes), c_sizes))
    assert nbytes >= (65 + 1) * 5 * 8
    _buf, ws, tail = _canary(nbytes, shift)
    coeffs = torch.zeros((2, 2), dtype=torch.float32, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    rc = hip_lib.g4s_depth_align(dr.DISPARITY, 0, 0.0, len(sizes), c_sizes, _lib.ptrs(src), _lib.ptrs(tgt), _lib.ptrs(msk),
                                 _lib.ptr(coeffs), _lib.ptr(counts), _lib.ptr(ws), nbytes, _lib.stream(DEV))
    assert rc == 0, hip_lib.g4s_last_error()
    torch.cuda.synchronize()
    assert (tail == 0xA5).all().item(), "bytes behind the advertised workspace were written"
    _aligned, want_coeffs, want_counts = depth_cues.align_disparities(src, tgt, devs(masks), "disparity")
    same_bits(coeffs, want_coeffs, "coefficients")
    assert torch.equal(counts, want_counts)
    assert np.isfinite(coeffs.cpu().numpy()).all() and counts.cpu().numpy().tolist() == [int(m.sum()) for m in masks]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "base+1"])
def test_plane_depths_workspace_is_enough(hip_lib, golden, id_scene, shift):
    """g4s_plane_depths keeps its view table, the 142 ids with their planes and the plane rows inside g4s_plane_depths_workspace."""
    from g4splat_amd import _lib
    s = id_scene
    V = len(s.sizes)
    cams = _cams(golden, s.sizes)
    view_offset, ids, entry_plane, rows, _keys = depth_cues.plane_table(s.gdict, s.planes, V)
    assert view_offset[-1] == len(ids) == sum(dr.ID_RUNS) and len(rows) == 5
    records = np.concatenate([depth_cues.plane_camera_record(c, W, H) for c, (H, W) in zip(cams, s.sizes)])
    depth, masks = devs(s.depths), devs(s.masks)
    out = [torch.zeros_like(d) for d in depth]
    counts = torch.full((2, V), -1, dtype=torch.int32, device=DEV)
    c_sizes = _lib.array(_lib.c_i, [x for H, W in s.sizes for x in (W, H)])
    nbytes = int(hip_lib.g4s_plane_depths_workspace(V, len(ids), len(rows)))
    assert nbytes >= 8 * len(ids) + 24 * len(rows)
    _buf, ws, tail = _canary(nbytes, shift)
    rc = hip_lib.g4s_plane_depths(V, _lib.array(_lib.c_f, records.tolist()), c_sizes, _lib.ptrs(depth), _lib.ptrs(out), _lib.ptrs(masks),
                                  _lib.array(_lib.c_i, view_offset), _lib.array(_lib.c_i, ids), _lib.array(_lib.c_i, entry_plane),
                                  len(rows), _lib.array(_lib.c_f, rows.reshape(-1).tolist()), _lib.ptr(counts), _lib.ptr(ws), nbytes,
                                  _lib.stream(DEV))
    assert rc == 0, hip_lib.g4s_last_error()
    torch.cuda.synchronize()
    assert (tail == 0xA5).all().item(), "bytes behind the advertised workspace were written"
    want, replaced, zeroed = depth_cues.apply_global_planes(cams, depth, masks, s.gdict, s.planes)
    assert torch.equal(counts[0], replaced) and torch.equal(counts[1], zeroed) and int(replaced.sum()) > 0
    for v in range(V):
        same_bits(out[v], want[v], f"plane depth {v}", nan_payload=False)


def _bounded(got, want, bound, keep=None, what=""):
    err = np.abs(np.asarray(got, f64) - np.asarray(want, f64))
    worst = float(err.max() if keep is None else err[keep].max())
    print(f"{what}: largest error {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound, (what, worst, bound)


def test_golden_cues_match_the_reference(golden):
    g = golden
    cues = depth_cues.view_geometry_cues(g.cams, dev(np.stack(g.disps)), devs(g.depths), devs(g.alphas), g.threshold)
    _bounded(cues.coeffs.cpu().numpy(), g.g["ref64_coeffs"], 2 * g.yard["coeffs"], what="coeffs")
    _bounded(np.stack(hosts(cues.aligned_depth)), g.g["ref64_aligned_depth"], 2 * g.yard["aligned_depth"], what="aligned_depth")
    _bounded(np.stack(hosts(cues.depth)), g.ref_merged, 2 * g.yard["depth"], what="depth")
    _bounded(np.stack(hosts(cues.normal_world[g.n_input:])), g.g["ref64_normal_world"], 2 * g.yard["normal_world"], what="normal_world")
    _bounded(np.stack(hosts(cues.normal_cam[g.n_input:])), g.g["ref64_normal_cam"], 2 * g.yard["normal_cam"], what="normal_cam")
    assert np.array_equal(np.stack(hosts(cues.visibility)), np.stack(g.visible))
    assert np.array_equal(cues.counts.cpu().numpy(), [int(m.sum()) for m in g.visible])
    # the reference-named single-view wrappers
    for v in range(g.n_input, g.V):
        disp, warp, vis = dev(g.disps[v]), dev(g.depths[v]), dev(g.visible[v])
        aligned, alpha, beta = depth_cues.depth_linear_align(disp, warp, vis, return_alpha_beta=True)
        assert isinstance(alpha, float) and isinstance(beta, float)
        assert torch.equal(aligned, depth_cues.depth_linear_align(disp, warp, vis)) and torch.equal(aligned, cues.aligned_depth[v])
        _bounded([alpha, beta], g.g["ref64_coeffs"][v], 2 * g.yard["coeffs"], what=f"depth_linear_align {v}")
        a2, alpha2, beta2 = depth_cues.depth_linear_align_2(dev(g.monos[v]), warp, vis, return_alpha_beta=True)
        _bounded([alpha2, beta2], g.g["ref64_coeffs2"][v], 2 * g.yard["coeffs2"], what=f"depth_linear_align_2 {v}")
        _bounded(a2.cpu().numpy(), g.g["ref64_align2"][v - g.n_input], 2 * g.yard["align2"], what=f"align2 {v}")


def test_golden_refined_depths_match_the_reference(golden):
    g = golden
    for i, (key, v) in enumerate(g.g["plane_full_pairs"]):
        n, c = g.planes[int(key)]
        depth, valid = depth_cues.plane_aligned_depth(dev(n), dev(c), g.cams[int(v)], (g.H, g.W))
        keep = g.g["full_agreed"][i]
        assert np.array_equal(valid.cpu().numpy()[keep], g.g["plane_full_valid"][i][keep])
        _bounded(depth.cpu().numpy(), g.g["ref64_plane_full"][i], 2 * g.yard["plane_full"], keep, f"plane_aligned_depth {i}")
    depths, masks = devs(g.depths), devs(g.masks)
    planed, replaced, zeroed = depth_cues.apply_global_planes(g.cams, depths, masks, g.gdict, g.planes)
    planed_np = np.stack(hosts(planed))
    touched, valid = g.g["touched"], g.g["valid"]
    assert np.array_equal((planed_np > 0)[touched & g.agreed], valid[touched & g.agreed])
    assert np.array_equal(planed_np[~touched], np.stack(g.depths)[~touched])
    assert g.agreed.all()  # so the counts are the reference's
    assert np.array_equal(replaced.cpu().numpy(), valid.sum((1, 2))) and np.array_equal(zeroed.cpu().numpy(), (touched & ~valid).sum((1, 2)))
    _bounded(planed_np, g.g["ref64_planed"], 2 * g.yard["planed"], g.agreed, "planed")
    refined, points = depth_cues.refine_depths_with_planes(g.cams, depths, masks, devs(g.confs), devs(g.monos), g.gdict, g.planes,
                                                           g.n_input, return_points=True)
    _bounded(np.stack(hosts(refined)), g.g["ref64_refined"], 2 * g.yard["refined"], g.agreed, "refined")
    for v in range(g.n_input):
        assert torch.equal(refined[v], planed[v])
    for v in range(g.V):
        assert points[v].shape == (g.H * g.W, 3) and torch.equal(points[v], visibility.depths_to_points(refined[v], g.cams[v]))
    only = depth_cues.refine_depths_with_planes(g.cams, depths, masks, devs(g.confs), devs(g.monos), g.gdict, g.planes, g.n_input)
    assert all(torch.equal(a, b) for a, b in zip(only, refined))
    assert all(torch.equal(a, dev(b)) for a, b in zip(depths, g.depths))  # the inputs are only read
