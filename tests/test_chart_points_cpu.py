"""Chart points without a GPU (include/g4s_losses.h, "Chart points"): the numpy restatement tests/chart_points_ref.py against
the golden file that the reference's own get_points_depth_in_depthmap, fit_depth_to_point_cloud and ParallelAligner.loss (with
points) wrote, its sampler against torch's grid_sample, its gradient against finite differences, the argument checks of the
Python layer and the host part of build_charts.

The measured quantities follow the rule of tests/test_gpu_chart_match.py: the yardstick of a quantity is the error of the
reference's float32 run against its float64 run; the float32 restatement may miss the float64 record by at most MARGIN = 4
yardsticks, with a floor of one float32 ulp of the largest entry.  The float64 restatement meets the record to 1e-12."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chart_points_ref as ref
from support import GOLDEN

MARGIN = 4.0
TOL64 = 1e-12
f32, f64 = np.float32, np.float64


def load_golden():
    g = np.load(os.path.join(GOLDEN, "chart_points.npz"))
    cams = [SimpleNamespace(world_view_transform=w, projection_matrix=p, full_proj_transform=f, FoVx=float(a[0]), FoVy=float(a[1]))
            for w, p, f, a in zip(g["wvt"], g["proj"], g["full"], g["fov"])]
    offsets = g["offsets"]
    counts = np.diff(offsets)
    chart = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    n, H, W = g["disparities"].shape
    return SimpleNamespace(g=g, cams=cams, points=g["points"], offsets=offsets, counts=[int(c) for c in counts], chart=chart, n=n, H=H,
                           W=W, lists=[g["points"][a:b] for a, b in zip(offsets[:-1], offsets[1:])], disparities=g["disparities"],
                           pred=g["pred_depths"], conf=g["confidence"], cw=float(g["confidence_weighting"]), fov=g["disp_fov"])


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def within_yardstick(label, got, want64, yard32):
    """got against the float64 record: at most MARGIN yardsticks (floor: one float32 ulp of the largest entry), over the finite
    entries; a non-finite entry of the record has to be met by the same kind."""
    got, want64, yard32 = (np.asarray(a, f64) for a in (got, want64, yard32))
    assert got.shape == want64.shape, (label, got.shape, want64.shape)
    finite = np.isfinite(want64)
    assert np.array_equal(np.isnan(got), np.isnan(want64)) and np.array_equal(got[~finite & ~np.isnan(want64)], want64[~finite & ~np.isnan(want64)]), label
    if not finite.any():
        return 0.0, 0.0
    top = np.abs(want64[finite]).max()
    err, yard = np.abs(got - want64)[finite].max() / top, np.abs(yard32 - want64)[finite].max() / top
    floor = float(np.spacing(f32(top))) / top
    print(f"{label}: error {err:.3e}, yardstick {yard:.3e}, floor {floor:.3e}")
    assert err <= max(MARGIN * yard, floor), (label, err, yard, floor)
    return err, yard


def close64(label, got, want):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    finite = np.isfinite(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), label
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), label
    if not finite.any():
        return
    err = np.abs(got - want)[finite].max() / np.abs(want[finite]).max()
    print(f"{label}: {err:.3e} of the largest entry")
    assert err <= TOL64, (label, err)


def restated(c, T):
    """Every recorded quantity from the restatement in float type T."""
    z, ix, iy, clipped = ref.project(c.cams, c.points, c.chart, c.H, c.W, T)
    assert not clipped.any()
    dv, fov = ref.sample(c.disparities, c.chart, ix, iy)
    out = SimpleNamespace(z=z, ix=ix, iy=iy, disp_values=dv, fov=fov, depth_values=ref.sample(c.pred, c.chart, ix, iy)[0],
                          conf_values=ref.sample(c.conf, c.chart, ix, iy)[0])
    out.coeffs, out.counts = ref.fit(z, dv, c.offsets, False, T)
    out.coeffs_fov, out.counts_fov = ref.fit(z, dv, c.offsets, True, T)
    out.fitted, out.fitted_fov = ref.apply(c.disparities, out.coeffs), ref.apply(c.disparities, out.coeffs_fov)
    out.plain = ref.point_reference_loss(c.pred.astype(T), c.chart, ix, iy, z, None, c.cw)
    out.with_conf = ref.point_reference_loss(c.pred.astype(T), c.chart, ix, iy, z, c.conf.astype(T), c.cw)
    keep = c.fov
    out.inside = ref.point_reference_loss(c.pred.astype(T), c.chart[keep], ix[keep], iy[keep], z[keep], c.conf.astype(T), c.cw)
    return out


RECORDED = (("z", lambda r: r.z), ("disp_values", lambda r: r.disp_values), ("depth_values", lambda r: r.depth_values),
            ("conf_values", lambda r: r.conf_values), ("coeffs", lambda r: r.coeffs), ("coeffs_fov", lambda r: r.coeffs_fov),
            ("fitted", lambda r: r.fitted), ("fitted_fov", lambda r: r.fitted_fov), ("loss", lambda r: r.plain.loss),
            ("grad", lambda r: r.plain.d_depths), ("loss_conf", lambda r: r.with_conf.loss),
            ("grad_conf_d", lambda r: r.with_conf.d_depths), ("grad_conf_k", lambda r: r.with_conf.d_confidence),
            ("loss_conf_in", lambda r: r.inside.loss), ("grad_conf_in_d", lambda r: r.inside.d_depths),
            ("grad_conf_in_k", lambda r: r.inside.d_confidence))


def test_float64_restatement_equals_the_references_float64_run(golden):
    r = restated(golden, f64)
    assert np.array_equal(r.fov, golden.fov)
    assert r.counts.tolist() == golden.counts and r.counts_fov.tolist() == [int(golden.fov[golden.chart == c].sum()) for c in range(golden.n)]
    for key, get in RECORDED:
        close64(key, get(r), golden.g[key + "64"])
    assert np.isposinf(golden.g["loss_conf64"]) and np.isnan(golden.g["coeffs64"][1]).all()  # the scene's two quirks are in it


def test_float32_restatement_within_the_references_own_error(golden):
    r = restated(golden, f32)
    assert np.array_equal(r.fov, golden.fov)
    for key, get in RECORDED:
        got = get(r)
        assert np.asarray(got).dtype == f32, key
        within_yardstick(key, got, golden.g[key + "64"], golden.g[key + "32"])


@pytest.mark.parametrize("T", [f32, f64])
def test_sampler_is_grid_sample_bilinear_zeros(T):
    """The restatement's tap rule against torch.nn.functional.grid_sample (bilinear, zeros, align_corners=False) on the CPU, at
    coordinates that cover pixel centres, the last row and column, the strip (-1, 0), W - 0.5 and points well outside."""
    rng = np.random.default_rng(5)
    H, W = 16, 32
    m = rng.uniform(0.5, 2.0, (1, H, W)).astype(T)
    ix = np.concatenate([np.arange(W, dtype=T), [-0.5, -0.25, W - 0.5, W - 0.75, -1.0, -3.0, W + 2.0], rng.uniform(-2, W + 1, 200)]).astype(T)
    iy = np.concatenate([np.full(W, H - 1, T), [3.0, -0.75, 5.5, H - 0.5, 2.0, 4.0, 1.0], rng.uniform(-2, H + 1, 200)]).astype(T)
    got, fov = ref.sample(m, np.zeros(len(ix), np.int64), ix, iy)
    gx, gy = (2 * ix.astype(f64) + 1) / W - 1, (2 * iy.astype(f64) + 1) / H - 1
    grid = torch.tensor(np.stack([gx, gy], -1).reshape(1, -1, 1, 2), dtype=torch.float64)
    want = torch.nn.functional.grid_sample(torch.tensor(m.astype(f64))[None], grid, mode="bilinear", padding_mode="zeros",
                                           align_corners=False)[0, 0, :, 0].numpy()
    tol = 1e-12 if T is f64 else 2.0 ** -20  # the coordinates' and the taps' roundings of values below 2
    assert np.abs(got - want).max() <= tol
    assert np.array_equal(fov, want > 0) and (got[W + 4: W + 7] == 0).all()  # ix = -1 (weight 0 on column 0) and the two outside


def test_gradient_of_the_float64_restatement_by_finite_differences(golden):
    """Pins the restatement's gradient itself: central differences of the float64 term in the depths and the confidence, over
    the points inside their image (the term is finite there), at pixels that carry taps and at one that carries none."""
    c = golden
    z, ix, iy, _ = ref.project(c.cams, c.points, c.chart, c.H, c.W, f64)
    keep = c.fov
    args = (c.chart[keep], ix[keep], iy[keep], z[keep])
    d0, k0 = c.pred.astype(f64), c.conf.astype(f64)
    r = ref.point_reference_loss(d0, *args, k0, c.cw, cotangent=0.37)
    rng = np.random.default_rng(11)
    busy = np.flatnonzero(r.d_depths.reshape(-1) != 0)
    idle = np.flatnonzero(r.d_depths.reshape(-1) == 0)
    assert len(busy) > 100 and len(idle) > 0
    h = 2.0 ** -20  # far below the distance 2^-12 of any point to its kink
    for at in list(rng.choice(busy, 24, replace=False)) + [idle[0]]:
        for which, grad in ((0, r.d_depths), (1, r.d_confidence)):
            vals = []
            for s in (1.0, -1.0):
                d, k = d0.copy(), k0.copy()
                (d if which == 0 else k).reshape(-1)[at] += s * h
                vals.append(0.37 * float(ref.point_reference_loss(d, *args, k, c.cw, need_grad=False).loss))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - grad.reshape(-1)[at]) <= 1e-6 * max(1.0, abs(fd)), (at, which, fd, grad.reshape(-1)[at])


def test_chunked_spread_is_the_plain_sum_in_float64():
    """One pixel with CHUNK + 1 and one with 3 CHUNK taps: the chunked order changes nothing beyond rounding."""
    H, W = 4, 6
    n1, n2 = ref.CHUNK + 1, 3 * ref.CHUNK
    ix = np.concatenate([np.full(n1, 2.0), np.full(n2, 4.0)])
    iy = np.concatenate([np.full(n1, 1.0), np.full(n2, 2.0)])
    g = np.random.default_rng(3).uniform(-1, 1, n1 + n2)
    out = ref.spread(g, np.zeros(n1 + n2, np.int64), ix, iy, 1, H, W)
    assert abs(out[0, 1, 2] - g[:n1].sum()) < 1e-12 and abs(out[0, 2, 4] - g[n1:].sum()) < 1e-12
    assert np.count_nonzero(out) == 2


# ---- the Python layer's argument checks, without a device ------------------------------------------------------------------------
def test_point_list_checks(golden):
    from g4splat_amd import chart_points as cp
    cams = golden.cams
    good = [torch.zeros(4, 3), torch.zeros(0, 3), torch.zeros(2, 3)]
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        cp.ChartPoints(cams, [torch.zeros(4, 2)] + good[1:], 24, 40)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        cp.ChartPoints(cams, [torch.zeros(4, 3, 1)] + good[1:], 24, 40)
    with pytest.raises(ValueError, match=r"\[n,N,3\]"):
        cp.ChartPoints(cams, torch.zeros(3, 5, 4), 24, 40)
    with pytest.raises(ValueError, match="float"):
        cp.ChartPoints(cams, [torch.zeros(4, 3, dtype=torch.int64)] + good[1:], 24, 40)
    with pytest.raises(ValueError, match="3 views but 2 point lists"):
        cp.ChartPoints(cams, good[:2], 24, 40)
    with pytest.raises(ValueError, match="positive"):
        cp.ChartPoints(cams, good, 0, 40)
    with pytest.raises(ValueError, match="HIP device"):  # well-formed host tensors: there is no CPU path
        cp.ChartPoints(cams, good, 24, 40)


def test_reference_names_refuse_what_the_reference_refuses(golden):
    from g4splat_amd import chart_points as cp
    pts, disp = torch.zeros(4, 3), torch.ones(24, 40)
    with pytest.raises(NotImplementedError, match="padding_mode"):
        cp.get_points_depth_in_depthmap(pts, disp, golden.cams[0], padding_mode="border")
    with pytest.raises(NotImplementedError, match="Rasterizer"):
        cp.fit_depth_to_point_cloud(disp, pts, golden.cams, 0, use_rasterizer=True)
    with pytest.raises(NotImplementedError, match="Color weighting"):
        cp.fit_depth_to_point_cloud(disp, pts, golden.cams, 0, image=torch.zeros(24, 40, 3), pt_colors=torch.zeros(4, 3))
    with pytest.raises(ValueError, match="camera_idx"):
        cp.fit_depth_to_point_cloud(disp, pts, golden.cams, 3)
    with pytest.raises(ValueError, match="masks"):
        cp.point_reference_loss(torch.zeros(3, 24, 40), None, masks=torch.ones(3, 24, 40))


def test_aligner_refusals_with_points(golden):
    from g4splat_amd import chart_aligner as ca
    c = golden
    a = ca.ChartAligner(c.cams, torch.tensor(c.pred))
    pts = [torch.tensor(p) for p in c.lists]
    with pytest.raises(ValueError, match="not both"):
        a.optimize(torch.tensor(c.pred), reference_points=pts)
    with pytest.raises(NotImplementedError, match="Matching loss is not implemented when using points"):
        a.optimize(reference_points=pts, use_matching_loss=True)
    with pytest.raises(ValueError, match="masks"):
        a.optimize(reference_points=pts, masks=torch.ones(3, c.H, c.W))
    with pytest.raises(ValueError, match="reference_data .* or reference_points"):
        a.optimize()
    with pytest.raises(NotImplementedError, match="points"):  # pinned: points as reference_data stay refused
        a.optimize(pts)
    with pytest.raises(ValueError, match="3 views but 2 point lists"):
        a.optimize(reference_points=pts[:2])


def test_scale_factor_and_rescaled_cameras(golden):
    """The host part of build_charts: target_scale over the spatial extent, and rescale_cameras' rule on the matrices."""
    from g4splat_amd import chart_match, chart_points as cp
    g = golden.g
    factor = float(g["target_scale"]) / chart_match.spatial_extent(golden.cams)
    assert abs(factor - float(g["scale_factor"])) <= 1e-6 * float(g["scale_factor"])  # the reference's extent is a float32 norm
    assert abs(ref.scale_factor(golden.cams, float(g["target_scale"])) - factor) <= 1e-12 * factor
    scaled = cp.rescale_cameras(golden.cams, float(g["scale_factor"]))
    for v, cam in enumerate(scaled):
        assert cam.world_view_transform.dtype == np.float32
        assert np.abs(cam.world_view_transform - g["scaled_wvt"][v]).max() <= 2.0 ** -22 * np.abs(g["scaled_wvt"][v]).max()
        want = g["scaled_wvt"][v].astype(f64) @ g["proj"][v].astype(f64)
        assert np.abs(cam.full_proj_transform - want).max() <= 2.0 ** -21 * np.abs(want).max()
        assert np.array_equal(cam.projection_matrix, g["proj"][v]) and cam.FoVx == golden.cams[v].FoVx
        # the centre moves by the factor, the rotation stays
        centre = np.linalg.inv(cam.world_view_transform.astype(f64).T)[:3, 3]
        centre0 = np.linalg.inv(g["wvt"][v].astype(f64).T)[:3, 3]
        assert np.abs(centre - float(g["scale_factor"]) * centre0).max() <= 1e-5
