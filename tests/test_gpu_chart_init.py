"""Chart surfels on the MI355X (g4splat_amd.chart_init, csrc/tsdf/chart_init.hip, the index emit of csrc/tsdf/mesh_eval.hip).

Surfels.  Every device output equals the float32 restatement (tests/chart_init_ref.py) bit for bit: the number of rows is the
restatement's number of kept faces, and row m is its m-th kept face.  The shapes are the smallest that reach every path: one
cell; no cell; workgroups of 256 cells that straddle the half and view boundaries (37 x 29: 1008 cells per view); many
workgroups (300 x 300: 350 per view) and, with two such views, more per-workgroup counts (1400) than one chunk of the scan
holds (1024).
Golden.  The reference's float64 results within twice the recorded yardstick, the keep mask exactly away from the threshold
(tests/test_chart_init_cpu.py holds the restatement to the same bars).
Index pick.  Exactly the restatement, in voxel_down_sample's voxel order."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chart_init_ref as cr
import mesh_eval_ref as mr
from g4splat_amd import chart_init, mesh_eval, synthetic, visibility
from chart_init_ref import check_against_golden, pair_cloud, random_cloud
from support import DEV, dev, load_chart_init_golden, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
KEYS = ("means", "scales", "quaternions", "colors")


def _scene(V, H, W, seed, stretch=6.0):
    """Point maps whose faces fall on both sides of ratio 5 (columns stretched by 1 .. `stretch`), colours beyond [0,1]."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:H, 0:W].astype(np.float64)
    pts = np.empty((V, H, W, 3))
    for v in range(V):
        x = np.cumsum(rng.uniform(1.0, stretch, W))
        pts[v] = np.stack([np.broadcast_to(x, (H, W)), r, 5.0 + 0.3 * rng.standard_normal((H, W))], axis=-1)
        pts[v] += 0.05 * rng.standard_normal((H, W, 3))
    return pts.astype(f32), rng.uniform(-0.2, 1.2, (V, H, W, 3)).astype(f32)


def _check(points, images, masks=None, ratio_th=5.0, normalized_scales=0.5, normal_scale=1e-10, as_list=False):
    """pointmap_surfels on the device against the restatement; returns (device result as numpy, restatement)."""
    want = cr.pointmap_surfels(points, images, masks, ratio_th, normalized_scales, normal_scale, f32)
    p, i = dev(points), dev(images)
    m = None if masks is None else dev(masks)
    if as_list:
        p, i, m = list(p), list(i), (None if m is None else list(m))
    got = chart_init.pointmap_surfels(p, i, m, ratio_th, normalized_scales, normal_scale)
    assert set(got) == set(KEYS)
    out = {}
    for k in KEYS:
        assert got[k].dtype == torch.float32 and got[k].device == DEV and got[k].is_contiguous()
        out[k] = got[k].cpu().numpy()
        assert len(out[k]) == int(want["keep"].sum()), (k, len(out[k]), int(want["keep"].sum()))
        same_bits(out[k], want[k], k, nan_payload=False)
    return out, want


def test_one_cell(hip_lib):
    pts = np.array([[[[0, 0, 1], [1, 0.1, 1.2]], [[0.1, 1, 0.9], [1.2, 1.1, 1.0]]]], f32)
    img = np.array([[[[0.1, 0.2, 0.3], [1.5, 0.5, -0.5]], [[0.9, 0.8, 0.7], [0.4, 0.4, 0.4]]]], f32)
    got, want = _check(pts, img)
    assert len(got["means"]) == 2 and want["keep"].tolist() == [True, True]
    same_bits(got["scales"][:, 2], np.full(2, f32(1e-10)), nan_payload=False)
    assert (got["quaternions"][:, 0] >= 0).all() and (got["colors"] >= 0).all() and (got["colors"] <= 1).all()


@pytest.mark.parametrize("H, W", [(1, 5), (5, 1), (1, 1)])
def test_a_view_without_cells_is_empty(hip_lib, H, W):
    pts, img = _scene(2, H, W, 1)
    got, _want = _check(pts, img)
    assert all(got[k].shape == (0, 4 if k == "quaternions" else 3) for k in KEYS)


def test_workgroups_straddle_halves_and_views(hip_lib):
    pts, img = _scene(3, 37, 29, 2)
    got, want = _check(pts, img)
    per_half = 36 * 28
    kept = want["keep"].reshape(3, 2, per_half).sum(axis=2)
    assert per_half % 256 != 0 and per_half % 64 != 0 and (kept > 0).all() and (kept < per_half).all()
    again, _w = _check(pts, img, as_list=True)  # lists of views, and a second run: the same bits
    for k in KEYS:
        same_bits(got[k], again[k], k)


@pytest.mark.parametrize("V", [1, 2])
def test_many_workgroups_and_a_scan_of_several_chunks(hip_lib, V):
    pts, img = _scene(V, 300, 300, 3)
    _got, want = _check(pts, img)
    groups = (299 * 299 + 255) // 256
    assert groups == 350 and (2 * V * groups > 1024) == (V == 2)
    assert 0.2 < want["keep"].mean() < 0.8


def test_all_kept_and_all_dropped(hip_lib):
    pts, img = _scene(2, 19, 23, 4)
    got, want = _check(pts, img, ratio_th=1e30)
    assert want["keep"].all() and len(got["means"]) == 2 * 2 * 18 * 22
    got, want = _check(pts, img, ratio_th=0.5)  # max / min is never below 1
    assert not want["keep"].any() and len(got["means"]) == 0
    got, want = _check(pts, img, ratio_th=float("nan"))
    assert len(got["means"]) == 0


def test_repeated_vertices_and_non_finite_points(hip_lib):
    pts, img = _scene(2, 21, 17, 5, stretch=2.0)
    clean = cr.pointmap_surfels(pts, img)["keep"]
    pts[0, 4, 3] = pts[0, 4, 4]                      # two equal vertices: a zero altitude, ratio inf
    pts[0, 9, 9] = pts[0, 9, 10] = pts[0, 10, 9]     # a face collapsed to a point: 0 / 0
    pts[1, 3, 3, 1] = np.nan
    pts[1, 8, 8, 0] = np.inf
    pts[1, 12, 5, 2] = -np.inf
    pts[1, 15, 11] = np.nan
    img[1, 6, 6, 0] = np.nan  # a NaN colour of a kept face stays a NaN
    got, want = _check(pts, img)
    faces = want["faces"]
    touched = np.zeros(len(faces), bool)
    for v, r, c in ((0, 4, 3), (0, 9, 9), (0, 9, 10), (0, 10, 9), (1, 3, 3), (1, 8, 8), (1, 12, 5), (1, 15, 11)):
        touched |= (faces == v * 21 * 17 + r * 17 + c).any(axis=1)
    bad = ~np.isfinite(pts).all(axis=-1).reshape(-1)
    assert not want["keep"][bad[faces].any(axis=1)].any()       # every face with a non-finite vertex is dropped
    assert np.array_equal(want["keep"][~touched], clean[~touched]) and want["keep"].sum() < clean.sum()
    assert np.isfinite(got["means"]).all() and np.isfinite(got["quaternions"]).all() and np.isnan(got["colors"]).any()


def test_masks(hip_lib):
    pts, img = _scene(2, 37, 29, 6)
    rng = np.random.default_rng(6)
    free, _w = _check(pts, img)
    partial = rng.random(pts.shape[:3]) < 0.3
    got, want = _check(pts, img, partial)
    assert 0 < len(got["means"]) < len(free["means"])
    assert (want["keep"] & ~partial.reshape(-1)[want["faces"]].all(axis=1)).any()  # kept with a masked-out vertex: the quirk
    got, _w = _check(pts, img, partial.astype(np.uint8) * 2)  # any non-zero byte counts
    assert len(got["means"]) == int(want["keep"].sum())
    for full in (np.ones(pts.shape[:3], bool), np.zeros(pts.shape[:3], bool)):  # an all-false mask removes nothing
        got, _w = _check(pts, img, full)
        for k in KEYS:
            same_bits(got[k], free[k], k)
    single = np.zeros(pts.shape[:3], bool)
    single[1, 36, 28] = True  # the last pixel of the last view: one face_2 touches it
    got, want = _check(pts, img, single, ratio_th=1e30)
    assert len(got["means"]) == 1 and want["keep"][-1]


def test_threshold_on_a_ratio(hip_lib):
    pts, img = _scene(1, 12, 11, 7)
    flat = pts.reshape(-1, 3)
    faces = cr.face_pixels(1, 12, 11)
    ratio = cr.keep_ratio(flat[faces[:, 0]], flat[faces[:, 1]], flat[faces[:, 2]])
    assert ratio.dtype == f32
    at = int(np.argsort(ratio)[len(ratio) // 2])
    th = ratio[at]
    got, want = _check(pts, img, ratio_th=float(th))
    assert not want["keep"][at] and len(got["means"]) == int((ratio < th).sum())
    got, want = _check(pts, img, ratio_th=float(np.nextafter(th, f32(np.inf))))
    assert want["keep"][at] and len(got["means"]) == int((ratio <= th).sum())


def test_scales_follow_their_arguments(hip_lib):
    pts, img = _scene(1, 9, 8, 8)
    _check(pts, img, normalized_scales=0.37, normal_scale=1e-4)


def _cameras(n, W, H):
    return [synthetic.look_at_camera((0.4 * v - 0.3, -0.2 * v, -2.6), (0.1 * v, 0, 0), (0, 1, 0), 1.0, W, H) for v in range(n)]


def test_depth_form_equals_point_form_over_depths_to_points(hip_lib):
    V, H, W = 3, 37, 29
    rng = np.random.default_rng(9)
    cams = _cameras(V, W, H)
    depths = (2.5 + 0.6 * rng.standard_normal((V, H, W))).astype(f32)
    depths[1, 5, 5], depths[2, 7, 3] = np.nan, 0.0
    images = rng.uniform(0, 1, (V, H, W, 3)).astype(f32)
    masks = rng.random((V, H, W)) < 0.5
    d, i, m = dev(depths), dev(images), dev(masks)
    points = torch.stack([visibility.depths_to_points(d[v], cams[v]).reshape(H, W, 3) for v in range(V)])
    same_bits(points[0], cr.depth_points(depths[0], visibility.ray_record(cams[0], W, H)), nan_payload=False)
    for mask in (None, m):
        a = chart_init.depthmap_surfels(d, cams, i, mask, ratio_th=4.0)
        b = chart_init.pointmap_surfels(points, i, mask, ratio_th=4.0)
        assert 0 < a["means"].shape[0] < 2 * V * (H - 1) * (W - 1)
        for k in KEYS:
            same_bits(a[k], b[k], k, nan_payload=False)
        c = chart_init.depthmap_surfels([x[None] for x in d], cams, list(i), None if mask is None else list(mask), ratio_th=4.0)
        for k in KEYS:  # lists of views, depth maps as [1,H,W]
            same_bits(c[k], a[k], k)


def test_golden_through_the_device(hip_lib):
    g = load_chart_init_golden()
    got, want = _check(g["points"], g["images"], None, float(g["ratio_th"]), float(g["normalized_scales"]), float(g["normal_scale"]))
    check_against_golden(g, dict(got, keep=want["keep"]), 2.0)
    # the reference-named entry points: pa data ignores its masks, charts data divides by its scale factor
    p, i = dev(g["points"]), list(dev(g["images"]))
    none = [torch.zeros((1, 9, 7), device=DEV), torch.zeros((1, 9, 7), device=DEV)]
    pa = chart_init.get_gaussian_parameters_from_pa_data(p, i, normal_scale=float(g["normal_scale"]), visibility_masks=none)
    for k in KEYS:
        same_bits(pa[k], got[k], k)
    confs = torch.rand((2, 9, 7), device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    charts = chart_init.get_gaussian_parameters_from_charts_data({"pts": p * 2.0, "confs": confs, "scale_factor": 2.0}, i,
                                                                 conf_th=0.5, normal_scale=2e-10)
    masked, _w = _check(g["points"], g["images"], (confs > 0.5).cpu().numpy())
    for k in KEYS:
        same_bits(charts[k], masked[k], k)
    vis = [torch.ones((1, 9, 7), device=DEV), torch.zeros((1, 9, 7), device=DEV)]
    charts = chart_init.get_gaussian_parameters_from_charts_data({"pts": p * 2.0, "confs": confs, "scale_factor": 2.0}, i,
                                                                 conf_th=0.5, normal_scale=2e-10, visibility_masks=vis)
    masked, _w = _check(g["points"], g["images"], ((confs * torch.cat(vis)) > 0.1).cpu().numpy())
    for k in KEYS:
        same_bits(charts[k], masked[k], k)


# ---- the index pick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, cloud", [("one point", random_cloud(1, 2)), ("one voxel", mr.one_voxel_cloud()), ("pairs", pair_cloud()),
                                         ("three per voxel", random_cloud())])
def test_index_pick_equals_the_restatement(hip_lib, name, cloud):
    cloud = np.ascontiguousarray(cloud, f32).reshape(-1, 3)
    pts = dev(cloud)
    idx, factor = chart_init.voxel_downsample_gaussians({"means": pts}, voxel_size=0.1)
    want = cr.voxel_pick_indices(cloud, 0.1)
    assert idx.dtype == torch.int64 and idx.device == DEV
    got = idx.cpu().numpy()
    assert np.array_equal(got, want), name
    assert factor == len(cloud) / len(want)
    # the voxel order is voxel_down_sample's: a voxel of one point names that point, and the means are that point
    down = mesh_eval.voxel_down_sample(pts, 0.1).cpu().numpy()
    assert len(down) == len(got)
    cells = mr.voxel_cells(cloud, 0.1)
    _u, inverse, counts = np.unique(cells[:, ::-1], axis=0, return_inverse=True, return_counts=True)
    alone = np.nonzero(counts == 1)[0]
    assert np.array_equal(inverse.reshape(-1)[got[alone]], alone)
    same_bits(down[alone], cloud[got[alone]], nan_payload=False)
    if name == "one voxel":
        assert len(got) == 1
    if name == "three per voxel":
        assert len(alone) > 0 and 2.0 < factor < 4.5


# ---- the trainer's lines --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [False, True])
def test_initial_gaussians_render(hip_lib, cap):
    from g4splat_amd.gaussian_model import GaussianModel
    from g4splat_amd.gaussian_renderer import render
    W, H = 64, 48
    rng = np.random.default_rng(10)
    cams = _cameras(3, W, H)
    depths = [dev((2.5 + 0.02 * rng.standard_normal((H, W))).astype(f32)) for _ in cams]
    images = [dev(rng.uniform(0, 1, (H, W, 3)).astype(f32)) for _ in cams]
    means, scales, quats, colors = chart_init.initial_gaussians(depths[:2], cams[:2], images[:2], depths[2:], cams[2:], images[2:],
                                                                max_gaussians_num=100 if cap else 10_000_000,
                                                                use_downsample_gaussians=True)
    both = chart_init.depthmap_surfels(depths[:2], cams[:2], images[:2])
    extra = chart_init.depthmap_surfels(depths[2:], cams[2:], images[2:])
    n = both["means"].shape[0] + extra["means"].shape[0]
    assert n > 100 and scales.shape == (means.shape[0], 2) and quats.shape == (means.shape[0], 4) and colors.shape == means.shape
    if cap:
        idx, factor = chart_init.voxel_downsample_gaussians({"means": torch.cat([both["means"], extra["means"]])}, 0.01)
        assert means.shape[0] == len(idx) < n and factor == n / len(idx)
        assert torch.equal(means, torch.cat([both["means"], extra["means"]])[idx])
        assert torch.equal(scales, torch.cat([both["scales"], extra["scales"]])[idx][:, :2] * factor)
    else:
        assert means.shape[0] == n and torch.equal(means[:both["means"].shape[0]], both["means"])
        assert torch.equal(scales, torch.cat([both["scales"], extra["scales"]])[:, :2])
    model = GaussianModel(sh_degree=3)
    model.create_from_parameters(means, scales, quats, colors, 1.0)
    cam = cams[0]
    cam = SimpleNamespace(image_width=W, image_height=H, FoVx=cam.FoVx, FoVy=cam.FoVy,
                          world_view_transform=torch.tensor(cam.world_view_transform, device=DEV),
                          full_proj_transform=torch.tensor(cam.full_proj_transform, device=DEV),
                          camera_center=torch.tensor(cam.camera_center, device=DEV), znear=0.01, zfar=100.0)
    out = render(cam, model, SimpleNamespace(depth_ratio=0.5, compute_cov3D_python=False), torch.tensor([0.1, 0.2, 0.3], device=DEV))
    torch.cuda.synchronize()
    assert out["render"].shape == (3, H, W)
    for k, v in out.items():
        if isinstance(v, torch.Tensor) and v.dtype.is_floating_point:
            assert torch.isfinite(v).all(), k
