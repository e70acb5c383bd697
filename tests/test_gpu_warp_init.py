"""The warp initialiser on the MI355X (g4splat_amd.warp_init, csrc/tsdf/warp_init.hip).

Every device output -- the keep mask of every pixel and the rows -- equals the float32 restatement (tests/warp_init_ref.py)
bit for bit; a NaN meets a NaN of any payload.  The shapes are the smallest that reach every path: single views down to one
pixel (the constant normal, the 1e-3 scale map, the border copies), a view without rows inside the row order, views of
different sizes whose workgroups and waves straddle view ends, more workgroups (1 056) than one chunk of the scan holds
(1 024), more views (70) than a wave has lanes, grids that do not divide the sizes, and depths and thresholds that are NaN,
infinite, zero or negative.
Golden.  The reference's float64 results within twice the recorded yardstick, the keep masks exactly away from the thresholds
(tests/test_warp_init_cpu.py holds the restatement to the same bars)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import warp_init_ref as wr
from g4splat_amd import chart_init, warp_init
from support import DEV, dev, devs, same_bits, twice

pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS = ("means", "scale_rows", "quaternions", "colors")


def _check(depths, cams, images, want=None, **kw):
    """warp_surfels with masks on the device against the restatement (computed here unless given); returns (rows and masks
    as numpy, restatement).  kw: depth_error_thresh, min_scale, max_scale, downsample_pixel_grid_size."""
    if want is None:
        want = wr.warp_surfels(depths, cams, images, kw.get("depth_error_thresh", 0.01), kw.get("min_scale", 0.0005),
                               kw.get("max_scale", 0.05), kw.get("downsample_pixel_grid_size", -1), f32)
    got = warp_init.warp_surfels(devs(depths), cams, devs(images), return_masks=True, **kw)
    assert len(got) == 5 and len(got[4]) == len(depths)
    masks = [m.cpu().numpy() for m in got[4]]
    for v, (m, k) in enumerate(zip(masks, want.keep)):
        assert m.dtype == np.bool_
        same_bits(m, k, f"keep mask of view {v}")
    rows = []
    for t, name, width in zip(got[:4], ROWS, (3, 2, 4, 3)):
        assert t.dtype == torch.float32 and t.device == DEV and t.is_contiguous() and t.shape == (len(want.means), width), name
        rows.append(t.cpu().numpy())
        same_bits(rows[-1], getattr(want, name).reshape(-1, width), name, nan_payload=False)
    only = warp_init.warp_keep_masks(devs(depths), cams, kw.get("depth_error_thresh", 0.01), kw.get("max_scale", 0.05),
                                     kw.get("downsample_pixel_grid_size", -1))
    same_bits([m.cpu().numpy() for m in only], masks, "warp_keep_masks")
    return rows + [masks], want


@pytest.mark.parametrize("W, H", [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (7, 5)])
def test_one_view(hip_lib, W, H):
    cams, depths, images = wr.scene([(W, H)], hole=(0, 0) if W * H == 1 else (1, 1))
    got, want = _check(depths, cams, images, max_scale=10.0, min_scale=0.0)
    assert np.array_equal(want.keep[0], depths[0] > 0) and want.keep[0].sum() == W * H - (W * H > 1)  # every valid pixel is kept
    if W == 1 or H == 1:
        assert (got[1] == f32(1e-3) * f32(0.5)).all()
    if W < 3 or H < 3:
        assert np.abs(wr.quaternion_to_matrix(got[2])[:, :, 2] - np.array([0, 0, 1])).max() < 1e-6
    elif (W, H) == (7, 5):
        n = want.normals[0]
        assert np.array_equal(n[0, 0], n[1, 1]) and np.array_equal(n[4, 6], n[3, 5]) and not np.array_equal(n[1, 1], n[3, 5])
        s = np.sort(want.scales[0][want.keep[0]])
        cut = float(s[len(s) // 2])
        _got, cut_want = _check(depths, cams, images, max_scale=cut, min_scale=float(s[len(s) // 4]))
        assert 0 < cut_want.keep[0].sum() < want.keep[0].sum()  # the cut is strict: s < max_scale


def _ringed(depths):
    """Zero depths on every view's border ring: a projection onto a closed border cannot decide a pixel."""
    for d in depths:
        d[0], d[-1], d[:, 0], d[:, -1] = 0, 0, 0, 0
    return depths


def test_a_view_without_rows_inside_the_order(hip_lib):
    cams, depths, images = wr.scene([(21, 17)] * 2, poses=(wr.POSES[0], wr.POSES[1]))
    cams, depths = [cams[0], cams[0], cams[1]], _ringed([depths[0], depths[0].copy(), depths[1]])
    images = [images[0], images[1], images[1]]
    got, want = _check(depths, cams, images, max_scale=1.0)
    assert want.keep[0].sum() > 0 and want.keep[1].sum() == 0 and want.keep[2].sum() > 0
    assert np.array_equal(want.covered[1], depths[1] > 0)


MIXED = [(37, 29), (23, 41), (37, 29), (23, 41)]


@pytest.fixture(scope="module")
def mixed():
    cams, depths, images = wr.scene(MIXED, seed=21)
    return SimpleNamespace(cams=cams, depths=depths, images=images, kw=dict(max_scale=0.06, min_scale=0.03),
                           want=wr.warp_surfels(depths, cams, images, 0.01, 0.03, 0.06, -1, f32))


def test_mixed_sizes(hip_lib, mixed):
    m = mixed
    assert all((h * w) % 64 != 0 for w, h in MIXED)  # waves and workgroups straddle the ends of the views
    got, want = _check(m.depths, m.cams, m.images, m.want, **m.kw)
    assert all(0 < k.sum() < k.size for k in want.keep) and (want.scale_rows == f32(0.03)).any() and (want.scale_rows > f32(0.03)).any()
    assert all(0 < (c & (d > 0)).sum() < (d > 0).sum() for c, d in zip(want.covered[1:], m.depths[1:]))
    # the reference's entry point: views with original_image, depths [1,H,W]; twice, the same bits
    views = [SimpleNamespace(original_image=dev(im), **vars(c)) for c, im in zip(m.cams, m.images)]
    named = twice(lambda: [t.cpu().numpy() for t in warp_init.get_gaussian_parameters_by_warp_from_depths(
        [dev(d)[None] for d in m.depths], views, min_scale=0.03, max_scale=0.06)])
    same_bits(named, got[:4], "get_gaussian_parameters_by_warp_from_depths")


def test_scan_depth(hip_lib):
    sizes = [(300, 300)] * 3
    assert sum(-(-w * h // 256) for w, h in sizes) == 1056 > 1024  # more workgroup counts than one chunk of the scan
    cams, depths, images = wr.scene(sizes, seed=22)
    got, want = _check(depths, cams, images)
    share = want.keep[2].sum() / want.keep[2].size
    print(f"rows {len(want.means)}, keep share of view 2 {share:.3f}")
    assert 0.05 < share < 0.95


def test_view_count(hip_lib):
    V = 70  # more views than a wave has lanes: no 64-entry staging of the table would hold them
    cams, depths, images = wr.scene([(8, 8)] * V, poses=wr.jittered_poses(V), seed=23, hole=(1, 1))
    got, want = _check(depths, cams, images, depth_error_thresh=0.0004, max_scale=1.0)
    last = want.covered[-1]
    print(f"rows {len(want.means)}, the last view: covered {int(last.sum())}, kept {int(want.keep[-1].sum())}")
    assert last.sum() > 0 and want.keep[-1].sum() > 0
    assert sum(k.any() for k in want.keep) > 30


@pytest.mark.parametrize("g", [3, 4])
def test_grid(hip_lib, g):
    cams, depths, images = wr.scene([(37, 29), (37, 29)], seed=24)
    assert 37 % g and 29 % g
    kw = dict(max_scale=10.0, min_scale=0.0)
    got, want = _check(depths, cams, images, downsample_pixel_grid_size=g, **kw)
    full, _w = _check(depths, cams, images, **kw)
    off = np.ones((29, 37), bool)
    off[::g, ::g] = False
    row = 0
    for k, kf in zip(got[4], full[4]):
        assert not k[off].any() and k.any()
        assert np.array_equal(k, kf & ~off)  # with no scale cut the lattice decides nothing else
    scales_full = np.concatenate([np.repeat(s[k][:, None], 2, 1) for s, k in zip(_w.scales, got[4])])
    same_bits(got[1], scales_full * f32(g), "scales are g times those of the full grid")


def test_edge_values(hip_lib):
    cams, depths, images = wr.scene([(19, 13), (19, 13), (19, 13)], seed=25)
    d = depths[1]
    d[4, 5], d[4, 12], d[8, 3], d[9, 9], d[2, 15] = np.nan, np.inf, -np.inf, -1.5, 0.0
    depths[0][6, 6], depths[0][7, 10], depths[0][2, 2] = np.nan, -2.0, np.inf
    images[1][0, 5, 5], images[1][1, 5, 6] = np.nan, np.inf  # colours are copied as they are
    got, want = _check(depths, cams, images, max_scale=1.0)
    k = want.keep[1]
    assert not k[4, 5] and not k[3, 5] and not k[5, 5] and not k[4, 4] and not k[4, 6]  # beside a NaN point: a NaN scale
    assert not k[4, 12] and not k[8, 3] and not k[9, 9] and not k[2, 15]
    assert np.isnan(want.scales[1][3, 5]) and (depths[1][3, 5] > 0)
    for th in (0.0, np.inf, np.nan):
        _g, w = _check(depths, cams, images, depth_error_thresh=th, max_scale=1.0)
        if th != np.inf:
            assert not any(c.any() for c in w.covered)  # nothing is below 0, or below a NaN
        else:
            assert w.covered[2].sum() > want.covered[2].sum()
    s = np.sort(want.scales[2][want.keep[2]])
    lo, hi = float(s[len(s) // 3]), float(s[2 * len(s) // 3])
    _g, w = _check(depths, cams, images, max_scale=hi, min_scale=lo)
    assert 0 < w.keep[2].sum() < want.keep[2].sum() and (w.scale_rows == f32(lo)).any() and (w.scale_rows > f32(lo)).any()
    _g, w = _check(depths, cams, images, max_scale=0.0)
    assert len(w.means) == 0
    _g, w = _check(depths, cams, images, max_scale=np.nan)
    assert len(w.means) == 0


@pytest.mark.parametrize("name", ["A", "B"])
def test_golden(hip_lib, name):
    g = wr.load_golden()
    r = g.rec[name]
    got = warp_init.warp_surfels(devs(g.depths), g.cams, devs(g.images), g.thresh, r.min_scale, r.max_scale, r.g, return_masks=True)
    wr.check_against_golden(r, [m.cpu().numpy() for m in got[4]], *[t.cpu().numpy() for t in got[:4]], factor=2.0)


def test_trainer_path(hip_lib, mixed):
    m = mixed
    d, im = devs(m.depths), devs(m.images)
    got = chart_init.initial_gaussians(d[:2], m.cams[:2], im[:2], d[2:], m.cams[2:], im[2:], use_downsample_gaussians=True,
                                       downsample_gaussians_type="warp")
    want = warp_init.warp_surfels(d, m.cams, im)
    assert len(got) == 4 and len(got[0]) > 0
    same_bits([t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want], "initial_gaussians, warp", nan_payload=False)
    alone = chart_init.initial_gaussians(d[:2], m.cams[:2], im[:2], use_downsample_gaussians=True, downsample_gaussians_type="warp")
    same_bits([t.cpu().numpy() for t in alone], [t.cpu().numpy() for t in warp_init.warp_surfels(d[:2], m.cams[:2], im[:2])],
              "initial_gaussians, warp, no extra views")
