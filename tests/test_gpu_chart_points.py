"""Chart points on the device (include/g4s_losses.h, "Chart points"; g4splat_amd/chart_points.py) against the numpy restatement
tests/chart_points_ref.py and the reference's record tests/golden/chart_points.npz.

What the contract states operation by operation -- view depths, pixel coordinates, sampled values, fov, fitted depths from given
coefficients, view depths of point maps, and the gradients, whose order of additions the restatement mirrors -- is compared bit
for bit with the float32 restatement.  What is a float64 sum in an order of its own (coefficients, the loss) is measured by the
rule of tests/test_gpu_chart_match.py: at most MARGIN = 4 yardsticks from the reference's float64 record, the yardstick being
the reference's own float32 error, floor one float32 ulp; against the restatement, a few float32 ulps."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chart_deform_ref as cd
import chart_points_ref as ref
from g4splat_amd import chart_aligner, chart_deform, chart_points as cp
from support import DEV, dev, host, same_bits, twice
from test_chart_points_cpu import load_golden, within_yardstick

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def golden(hip_lib):
    return load_golden()


def device_points(cams, lists, H, W):
    return cp.ChartPoints(cams, [dev(np.asarray(p, f32).reshape(-1, 3)) for p in lists], H, W)


def loss_and_grads(pts, depths, conf, cw, cotangent=1.0):
    d = dev(depths).requires_grad_()
    k = None if conf is None else dev(conf).requires_grad_()
    loss = cp.point_reference_loss(d, pts, k, cw)
    (loss * cotangent).backward()
    return host(loss), host(d.grad), None if k is None else host(k.grad)


# ---- 1. the golden scene ---------------------------------------------------------------------------------------------------------
def test_golden_scene_stored_floats_bit_for_bit(golden):
    c = golden
    z, ix, iy, clipped = ref.project(c.cams, c.points, c.chart, c.H, c.W, f32)
    pts = device_points(c.cams, c.lists, c.H, c.W)
    assert pts.counts == c.counts and pts.n_points == len(c.points)
    same_bits(pts.chart, c.chart, "chart")
    same_bits(pts.offsets, c.offsets, "offsets")
    same_bits(pts.view_depths, z, "z")
    same_bits(pts.ixy, np.stack([ix, iy], -1), "ixy")
    assert not host(pts.clipped).any()
    values, fov = twice(lambda: [host(t) for t in pts.sample(dev(c.disparities))])
    same_bits(values, ref.sample(c.disparities, c.chart, ix, iy)[0], "sampled disparities")
    assert np.array_equal(fov, c.fov)
    assert [tuple(v.shape) for v in pts.split(pts.view_depths)] == [(k,) for k in c.counts]
    for key in ("coeffs32", "coeffs_fov32"):  # fitted depths given the coefficients
        coeffs = c.g[key].astype(f32)
        got = twice(lambda: host(cp.aligned_depths(dev(c.disparities), dev(coeffs), 1.75)))
        same_bits(got, ref.apply(c.disparities, coeffs, 1.75), key, nan_payload=False)
    maps = np.random.default_rng(3).uniform(-2, 5, (c.n, c.H, c.W, 3)).astype(f32)
    got = twice(lambda: host(cp.view_depths_of_point_maps(c.cams, dev(maps), 1.375)))
    same_bits(got, ref.view_depths_of_point_maps(c.cams, maps, 1.375), "view depths of point maps")
    # the reference's one-chart names
    v0, f0 = cp.get_points_depth_in_depthmap(dev(c.lists[0]), dev(c.disparities[0]), c.cams[0])
    same_bits(v0, values[:c.counts[0]], "get_points_depth_in_depthmap")
    assert np.array_equal(host(f0), c.fov[:c.counts[0]])


def test_golden_scene_within_the_references_own_error(golden):
    c, g = golden, golden.g
    pts = device_points(c.cams, c.lists, c.H, c.W)
    for key, flag in (("coeffs", False), ("coeffs_fov", True)):
        coeffs, counts = twice(lambda: [host(t) for t in cp.fit_disparities(dev(c.disparities), pts, flag, return_counts=True)])
        within_yardstick(key, coeffs, g[key + "64"], g[key + "32"])
        assert counts.tolist() == ([int(c.fov[c.chart == v].sum()) for v in range(c.n)] if flag else c.counts)
    alpha, beta = cp.fit_depth_to_point_cloud(dev(c.disparities[2]), dev(c.lists[2]), c.cams, 2, return_alpha_beta=True)
    within_yardstick("fit_depth_to_point_cloud", [float(alpha), float(beta)], g["coeffs64"][2], g["coeffs32"][2])
    fitted = cp.fit_depth_to_point_cloud(dev(c.disparities[2]), dev(c.lists[2]), c.cams, 2, use_fov_mask=True)
    within_yardstick("fitted depth", host(fitted), g["fitted_fov64"][2], g["fitted_fov32"][2])
    loss, gd, _ = twice(lambda: loss_and_grads(pts, c.pred, None, c.cw))
    within_yardstick("loss", loss, g["loss64"], g["loss32"])
    within_yardstick("gradient", gd, g["grad64"], g["grad32"])
    loss, gd, gk = twice(lambda: loss_and_grads(pts, c.pred, c.conf, c.cw))
    assert np.isposinf(loss)  # the reference's value: a point outside its image samples a confidence of 0
    within_yardstick("gradient to the depths, with confidence", gd, g["grad_conf_d64"], g["grad_conf_d32"])
    within_yardstick("gradient to the confidence", gk, g["grad_conf_k64"], g["grad_conf_k32"])
    inside = device_points(c.cams, [p[c.fov[c.chart == v]] for v, p in enumerate(c.lists)], c.H, c.W)
    loss, gd, gk = twice(lambda: loss_and_grads(inside, c.pred, c.conf, c.cw))
    within_yardstick("loss over the points inside", loss, g["loss_conf_in64"], g["loss_conf_in32"])
    within_yardstick("its gradient to the depths", gd, g["grad_conf_in_d64"], g["grad_conf_in_d32"])
    within_yardstick("its gradient to the confidence", gk, g["grad_conf_in_k64"], g["grad_conf_in_k32"])


# ---- 2. edges, against the restatement ---------------------------------------------------------------------------------------------
def grid_camera():
    """gx = p_0 / p_2, gy = p_1 / p_2, z = p_2: with p_2 = 1 a point's pixel coordinates are exact."""
    F = np.zeros((4, 4), f32)
    F[0, 0] = F[1, 1] = F[2, 2] = F[2, 3] = 1.0
    return SimpleNamespace(world_view_transform=np.eye(4, dtype=f32), full_proj_transform=F)


def at_pixels(ix, iy, H, W, z=1.0):
    ix, iy = np.asarray(ix, f64), np.asarray(iy, f64)
    return np.stack([((2 * ix + 1) / W - 1) * z, ((2 * iy + 1) / H - 1) * z, np.full(len(ix), z)], -1).astype(f32)


def plane_points(golden, counts, seed):
    rng = np.random.default_rng(seed)
    out = []
    for c, count in enumerate(counts):
        centre = np.linalg.inv(golden.cams[c].world_view_transform.astype(f64).T)[:2, 3]
        xy = rng.uniform(-1.0, 1.0, (count, 2)) * np.array([2.9, 1.75]) + centre
        out.append(np.concatenate([xy, ((4.0 - xy @ np.array([0.3, 0.2])) / 1.0)[:, None]], 1).astype(f32))
    return out


def check_against_restatement(name, cams, lists, H, W, seed=0, expect_clipped=0):
    """Every device result of the case against the float32 restatement."""
    n = len(cams)
    rng = np.random.default_rng(100 + seed)
    points, offsets, chart = ref.pack(lists)
    z, ix, iy, clipped = ref.project(cams, points, chart, H, W, f32)
    assert int(clipped.sum()) == expect_clipped, name
    pts = device_points(cams, lists, H, W)
    same_bits(pts.view_depths, z, f"{name}: z", nan_payload=False)
    same_bits(pts.ixy, np.stack([ix, iy], -1), f"{name}: ixy")
    assert np.array_equal(host(pts.clipped), clipped)
    disp = rng.uniform(0.2, 1.5, (n, H, W)).astype(f32)
    values, fov = [host(t) for t in pts.sample(dev(disp))]
    want, want_fov = ref.sample(disp, chart, ix, iy)
    same_bits(values, want, f"{name}: values")
    assert np.array_equal(fov, want_fov)
    for flag in (False, True):
        coeffs, counts = twice(lambda: [host(t) for t in cp.fit_disparities(dev(disp), pts, flag, return_counts=True)])
        wc, wn = ref.fit(z, want, offsets, flag, f32)
        assert counts.tolist() == wn.tolist(), name
        assert np.array_equal(np.isfinite(coeffs), np.isfinite(wc)), (name, coeffs, wc)
        ok = np.isfinite(wc)
        # the float64 sums differ in their order only: a few float32 ulps after the cancellation in beta's denominator
        assert np.abs(coeffs[ok].astype(f64) - wc[ok]).max(initial=0.0) <= 2.0 ** -18 * np.abs(wc[ok]).max(initial=1.0), (name, coeffs, wc)
    if len(points) == 0:
        return pts
    depths = rng.uniform(0.5, 3.0, (n, H, W)).astype(f32)
    conf = (1.0 + np.exp(rng.uniform(-1, 1, (n, H, W)))).astype(f32)
    for k in (None, conf):
        loss, gd, gk = twice(lambda: loss_and_grads(pts, depths, k, 0.2, 0.37))
        r = ref.point_reference_loss(depths, chart, ix, iy, z, k, 0.2, cotangent=f32(0.37))
        if np.isfinite(r.loss):
            assert abs(float(loss) - float(r.loss)) <= 4 * np.spacing(f32(abs(r.loss))), (name, loss, r.loss)
        else:
            assert np.isposinf(loss) and np.isposinf(r.loss), (name, loss, r.loss)
        same_bits(gd, r.d_depths, f"{name}: gradient to the depths")
        if k is not None:
            same_bits(gk, r.d_confidence, f"{name}: gradient to the confidence", nan_payload=False)
    # sample's own backward spreads any cotangent the same way
    m = dev(depths).requires_grad_()
    g = rng.uniform(-1, 1, len(points)).astype(f32)
    (pts.sample(m)[0] * dev(g)).sum().backward()
    same_bits(m.grad, ref.spread(g, chart, ix, iy, n, H, W), f"{name}: sample backward")
    return pts


def test_pixel_centres_last_row_and_column():
    H, W = 16, 32
    ix = np.concatenate([np.arange(W), np.full(H, W - 1), [0, 5, 17]])
    iy = np.concatenate([np.full(W, H - 1), np.arange(H), [0, 3, 9]])
    pts = check_against_restatement("centres", [grid_camera()], [at_pixels(ix, iy, H, W)], H, W, 1)
    m = np.random.default_rng(0).uniform(1, 2, (1, H, W)).astype(f32)
    same_bits(pts.sample(dev(m))[0], m[0, iy, ix], "a pixel centre samples the pixel")


def test_strips_beside_the_image_and_points_outside():
    H, W = 16, 32
    ix = [-0.5, -0.25, -0.75, W - 0.5, W - 0.5, 3.0, 7.5, -1.0, -3.0, W + 4.0, 5.0, 1e6]
    iy = [4.0, -0.5, H - 0.5, H - 0.5, 2.25, -0.25, H - 0.75, 3.0, 2.0, 5.0, -7.0, 2.0]
    check_against_restatement("strips", [grid_camera()], [at_pixels(ix, iy, H, W)], H, W, 2)


def test_points_behind_the_camera_are_clipped():
    H, W = 16, 32
    p = np.concatenate([at_pixels([3.5, 9.0], [2.5, 7.0], H, W), at_pixels([4.0], [4.0], H, W, -1.0), [[0.25, 0.5, 0.0]],
                        at_pixels([20.25], [11.5], H, W, 2.0)]).astype(f32)
    pts = check_against_restatement("behind", [grid_camera()], [p], H, W, 3, expect_clipped=2)
    values, fov = pts.sample(torch.ones((1, H, W), device=DEV))
    assert host(values)[2:4].tolist() == [0.0, 0.0] and not host(fov)[2:4].any() and host(fov)[[0, 1, 4]].all()


def test_loss_fold_beyond_one_trip():
    """N = 4096 * 256 + 1 points on two charts of 16x32: 257 spans, the last of one point, so thread 0 of the loss's
    256-thread fold adds two partials.  The value against the restatement (float32 terms, float64 sum) by the bound of
    check_against_restatement, with and without a confidence; two runs, the same bits."""
    H, W, N = 16, 32, 4096 * 256 + 1
    rng = np.random.default_rng(41)
    counts = (600_000, N - 600_000)
    # the strips beside the image included, but every point with a tap inside: the sampled confidence stays positive
    lists = [at_pixels(rng.uniform(-0.75, W - 0.25, k), rng.uniform(-0.75, H - 0.25, k), H, W) for k in counts]
    cams = [grid_camera(), grid_camera()]
    points, _offsets, chart = ref.pack(lists)
    z, ix, iy, clipped = ref.project(cams, points, chart, H, W, f32)
    assert not clipped.any()
    pts = device_points(cams, lists, H, W)
    assert pts.n_points == N
    same_bits(pts.ixy, np.stack([ix, iy], -1), "ixy")
    depths = rng.uniform(0.5, 3.0, (2, H, W)).astype(f32)
    conf = (1.0 + np.exp(rng.uniform(-1, 1, (2, H, W)))).astype(f32)
    for k in (None, conf):
        with torch.no_grad():
            loss = twice(lambda: host(cp.point_reference_loss(dev(depths), pts, dev(k), 0.2)))
        want = ref.point_reference_loss(depths, chart, ix, iy, z, k, 0.2, need_grad=False).loss
        print(f"N = {N}, confidence {k is not None}: loss {float(loss):.9g}, restatement {float(want):.9g}")
        assert np.isfinite(want) and abs(float(loss) - float(want)) <= 4 * np.spacing(f32(abs(want))), (loss, want)


@pytest.mark.parametrize("counts", [(0, 5, 7), (5, 0, 7), (5, 7, 0), (1, 6, 0), (0, 0, 0)])
def test_empty_charts_and_a_chart_with_one_point(golden, counts):
    """An empty chart first, in the middle and last; one point gives NaN coefficients and no error; no point at all."""
    pts = check_against_restatement(f"counts {counts}", golden.cams, plane_points(golden, counts, 5), golden.H, golden.W, 4)
    coeffs = host(cp.fit_disparities(torch.ones((3, golden.H, golden.W), device=DEV), pts))
    assert np.isnan(coeffs[[k for k, v in enumerate(counts) if v < 2]]).all()
    if sum(counts) == 0:
        with pytest.raises(ValueError, match="no points"):
            cp.point_reference_loss(torch.ones((3, golden.H, golden.W), device=DEV), pts)


def test_counts_around_the_moments_span(golden):
    S = cp.SPAN
    assert S == ref.SPAN
    check_against_restatement("spans", golden.cams, plane_points(golden, (S - 1, S, S + 1), 6), golden.H, golden.W, 5)
    check_against_restatement("two spans and three", golden.cams[:1], plane_points(golden, (2 * S + 3,), 7), golden.H, golden.W, 6)


def test_one_pixel_with_a_chunk_and_one_with_three_chunks_and_more_than_a_round():
    """Piles on single pixels around the backward's chunk size: CHUNK + 1 taps, 3 CHUNK taps, and 65 CHUNK + 5 taps, more chunks
    than the 64 lanes of a wave sum in one round."""
    H, W = 16, 32
    K = cp.CHUNK
    assert K == ref.CHUNK
    rng = np.random.default_rng(8)
    piles = ((K + 1, 3.0, 2.0), (3 * K, 10.0, 5.0), (65 * K + 5, 20.0, 9.0))
    ix = np.concatenate([np.full(k, x) for k, x, _y in piles] + [rng.uniform(0, W - 1, 40)])
    iy = np.concatenate([np.full(k, y) for k, _x, y in piles] + [rng.uniform(0, H - 1, 40)])
    order = rng.permutation(len(ix))
    pts = check_against_restatement("piles", [grid_camera()], [at_pixels(ix[order], iy[order], H, W)], H, W, 7)
    pts.build_index()
    counts = np.diff(host(pts._starts).astype(np.int64))
    for k, x, y in piles:
        assert counts[int(y) * W + int(x)] >= k
    assert host(pts._starts)[-1] == len(host(pts._taps))  # every tap of this case lies inside the map


def test_non_contiguous_and_float64_maps(golden):
    c = golden
    pts = device_points(c.cams, c.lists, c.H, c.W)
    want = host(pts.sample(dev(c.pred))[0])
    wide = torch.zeros((c.n, c.H, 2 * c.W), device=DEV)
    wide[:, :, ::2] = dev(c.pred)
    same_bits(pts.sample(wide[:, :, ::2])[0], want, "non-contiguous")
    same_bits(pts.sample(dev(c.pred).double())[0], want, "float64")
    d = dev(c.pred).double().requires_grad_()
    cp.point_reference_loss(d, pts, None, c.cw).backward()
    assert d.grad.dtype == torch.float64
    same_bits(d.grad.float(), loss_and_grads(pts, c.pred, None, c.cw)[1], "float64 gradient")


# ---- 3. the aligner with points ----------------------------------------------------------------------------------------------------
ALIGNER_SHAPE = (3, 24, 40, (0.05, 0.1, 0.2, 0.4), 8, 32, 3, 16)
WEIGHTS = {"gradient": None, "hessian": None, "normal": 4.0, "curvature": 1.0, "matching": None, "norm": 2.0, "tv": 5.0}  # strong, no matching
OPTIMIZE = dict(use_gradient_loss=False, use_normal_loss=True, use_curvature_loss=True, use_matching_loss=False, normal_loss_weight=4.0,
                curvature_loss_weight=1.0, regularize_chart_encodings_norms=True, chart_encodings_norm_loss_weight=2.0,
                use_total_variation_on_depth_encodings=True, total_variation_on_depth_encodings_weight=5.0, lr_update_iters=[],
                prepare=False)


@pytest.fixture(scope="module")
def aligner_case(hip_lib):
    c = cd.make_case("points", 31, ALIGNER_SHAPE)
    c.coords = cd.depth_coordinates(c.d0, c.bins)
    rng = np.random.default_rng(31)
    c.init = {k: (v * f32(2.0 ** -10) if "encod" in k else v) for k, v in cd.parameters(c).items()}
    c.raw = rng.uniform(-0.5, 0.5, c.d0.shape).astype(f32)
    # reference points: each chart's own surface moved 3 % away, at random pixel centres; the middle chart has few
    import chart_align_ref
    rays = chart_align_ref.ray_records(c.cams, c.W, c.H)
    c.lists = []
    for v, count in enumerate((300, 40, 220)):
        q = rng.choice(c.H * c.W, count, replace=False)
        x, y = (q % c.W).astype(f64), (q // c.W).astype(f64)
        o, D = rays[v, :3].astype(f64), rays[v, 3:].reshape(3, 3).astype(f64)
        dirs = np.stack([D[k, 0] * x + D[k, 1] * y + D[k, 2] for k in range(3)], -1)
        c.lists.append((o + (1.03 * c.d0[v].reshape(-1)[q].astype(f64))[:, None] * dirs).astype(f32))
    return c


def run_aligner(c, graph, n_iterations=30, **more):
    E = c.channels * len(c.levels)
    a = chart_aligner.ChartAligner(
        c.cams, dev(c.d0), charts_encoding_params=chart_deform.ChartsEncodingParams(encoding_dim=E),
        depth_encoding_params=chart_deform.DepthEncodingParams(encoding_dim=E, n_bins=c.bins),
        mlp_params=chart_deform.MLPParams(n_deformation_layers=c.layers, deformation_layer_size=c.layer_size),
        multi_res_charts_encoding_params=chart_deform.MultiResChartsEncodingParams(c.channels, c.resolutions),
        use_learnable_confidence=True, weight_encodings_with_confidence=True)
    a.prepare_for_optimization(1e-2, 1e-3, [], 0.1, 1e-3)
    a.deformation_module.load_reference_state_dict({k: torch.from_numpy(v) for k, v in c.init.items()})
    with torch.no_grad():
        a._confidence.copy_(dev(c.raw))
    kw = dict(OPTIMIZE, n_iterations=n_iterations, graph=graph)
    kw.update(more)
    a.optimize(reference_points=[dev(p) for p in c.lists], **kw)
    return a, [host(p) for _k, p in sorted(a.named_parameters())] + [np.array(a.train_losses)]


def test_optimize_with_reference_points_graph_eager_and_the_restated_curve(aligner_case):
    c = aligner_case
    eager, e = run_aligner(c, False)
    first, g1 = run_aligner(c, True)
    _second, g2 = run_aligner(c, True)
    same_bits(g1, e, "graph against eager")
    same_bits(g2, g1, "two graph runs")
    assert first.graph_captures == 1 and eager.graph_captures == 0
    losses = first.train_losses
    assert len(losses) == 30 and np.isfinite(losses).all()
    assert set(first.loss_terms[0]) == {"loss", "depth_loss", "normal", "curv", "ce_norm", "de_tv"}
    # the rule of test_gpu_chart_aligner.py's curves: the float64 restatement of the same run falls, and the device's last loss
    # is at most the restatement's loss half way
    want = ref.optimize_with_points(c, c.init, c.raw, c.lists, 30, WEIGHTS, True)
    print(f"first {losses[0]:.6f} (restated {want[0]:.6f}), at 15 {losses[15]:.6f} ({want[15]:.6f}), last {losses[-1]:.6f} ({want[-1]:.6f})")
    assert abs(losses[0] - want[0]) <= 1e-5 * abs(want[0])
    assert want[-1] <= 0.9 * want[15] or want[-1] < want[15] < want[0]
    assert losses[-1] <= want[15]
    with pytest.raises(NotImplementedError, match="points"):  # pinned: points as reference_data stay refused
        eager.optimize([dev(p) for p in c.lists], n_iterations=1)


def test_build_charts_feeds_align_charts(golden, tmp_path):
    """SfM points + mono disparities -> cameras, initial depths, reference -> align_charts -> charts_data.npz with the
    reference's five keys and shapes; once with point maps (reference depths) and once with the points themselves."""
    c, g = golden, golden.g
    lists = [dev(p) for p in c.lists]
    lists[1] = dev(plane_points(golden, (0, 60, 0), 9)[1])  # the golden's middle chart is empty: no fit, NaN depths
    cams, initial, reference, factor = cp.build_charts(c.cams, dev(c.disparities), lists, target_scale=float(g["target_scale"]))
    assert abs(factor - float(g["scale_factor"])) <= 1e-6 * factor and isinstance(reference, cp.ChartPoints)
    coeffs = cp.fit_disparities(dev(c.disparities), cp.ChartPoints(c.cams, lists, c.H, c.W))
    same_bits(initial, cp.aligned_depths(dev(c.disparities), coeffs, factor), "initial depths")
    for v in (0, 2):
        within_yardstick(f"initial depths {v}", host(initial)[v] / factor, g["fitted64"][v], g["fitted32"][v])
    unscaled = host(cp.ChartPoints(c.cams, lists, c.H, c.W).view_depths).astype(f64)
    assert np.abs(host(reference.view_depths) - factor * unscaled).max() <= 1e-5 * factor * unscaled.max()  # the scene scales as a whole
    cfg = dict(chart_aligner.ALIGNMENT_CONFIGS["strong"], use_matching_loss=False, n_iterations=4, lr_update_iters=[])
    out = chart_aligner.align_charts(cams, initial, reference, scale_factor=factor, charts_data_path=str(tmp_path), **cfg)
    data = np.load(str(tmp_path / "charts_data.npz"))
    shape = (c.n, c.H, c.W)
    assert {k: data[k].shape for k in data} == {"prior_depths": shape, "depths": shape, "pts": shape + (3,), "confs": shape, "scale_factor": ()}
    assert len(out) == 3 and np.isfinite(data["depths"]).all() and float(data["scale_factor"]) == factor
    # with point maps the reference is a depth map, and the default matching loss runs
    import chart_align_ref
    rays = chart_align_ref.ray_records(c.cams, c.W, c.H).astype(f64)
    yy, xx = np.meshgrid(np.arange(c.H, dtype=f64), np.arange(c.W, dtype=f64), indexing="ij")
    dirs = np.stack([rays[:, 3 + 3 * k, None, None] * xx + rays[:, 4 + 3 * k, None, None] * yy + rays[:, 5 + 3 * k, None, None] for k in range(3)], -1)
    maps = rays[:, None, None, :3] + (host(initial).astype(f64) / factor)[..., None] * dirs  # the unscaled charts' own points
    _cams, _initial, ref_depths, _f = cp.build_charts(c.cams, dev(c.disparities), lists, point_maps=dev(maps.astype(f32)),
                                                      target_scale=float(g["target_scale"]))
    assert tuple(ref_depths.shape) == shape
    assert float((ref_depths - initial).abs().max()) <= 1e-4 * float(initial.abs().max())  # z of scale P is scale depth, to rounding
