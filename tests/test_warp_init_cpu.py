"""The warp-surfel contract without a GPU: the numpy restatement (tests/warp_init_ref.py) against what the reference's own
function computed (tests/golden/warp_init.npz, written by tests/golden/make_golden_warp_init.py), the host-side argument
checks of the three entry points, and the Python surface's additions to chart_init.

The yardstick of every continuous output is the largest |float32 run - float64 run| of the REFERENCE over the rows both runs
keep, recorded by the generator: the float32 restatement has to be within twice it of the reference's float64 results.  Keep
masks are compared exactly on the pixels that are not near a threshold (a half-integer or border of a projection, the depth
error threshold); the generator asserts that at most 1 % of a view's pixels are near.  Rotations are compared as matrices."""
import ctypes
import inspect

import numpy as np
import pytest

import warp_init_ref as wr

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def golden():
    return wr.load_golden()


def test_golden_covers_what_it_claims(golden):
    g = golden
    assert g.sizes == [tuple(s) for s in wr.GOLDEN_SIZES] and g.thresh == f32(wr.DEPTH_ERROR_THRESH)
    cams, depths, images = wr.scene(wr.GOLDEN_SIZES)  # the stored inputs are the scene family's
    for v in range(4):
        assert np.array_equal(depths[v], g.depths[v]) and np.array_equal(images[v], g.images[v])
        assert np.array_equal(cams[v].world_view_transform, g.cams[v].world_view_transform)
        assert (g.depths[v][:3, :4] == 0).all() and (g.depths[v] > 0).sum() == g.depths[v].size - 12
    a, b = g.rec["A"], g.rec["B"]
    assert a.keep[0].sum() > 0 and all(0 < k.sum() < (d > 0).sum() for k, d in zip(a.keep[1:], g.depths[1:]))
    assert (a.scales == a.min_scale).any() and (a.scales > a.min_scale).any()  # the clamp
    assert all(n.sum() <= 0.01 * n.size for r in (a, b) for n in r.near)
    off = np.ones((18, 24), bool)
    off[::3, ::3] = False
    assert not b.keep[0][off].any() and b.keep[0].any()
    assert all(v > 0 for r in (a, b) for k, v in r.yard.items() if k != "colors")


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("dtype, factor", [(f64, 1.0), (f32, 2.0)])
def test_restatement_matches_the_reference(golden, name, dtype, factor):
    g, r = golden, golden.rec[name]
    got = wr.warp_surfels(g.depths, g.cams, g.images, g.thresh, r.min_scale, r.max_scale, r.g, dtype)
    assert got.means.dtype == dtype and got.quaternions.dtype == dtype and got.scale_rows.shape == (len(got.means), 2)
    wr.check_against_golden(r, got.keep, got.means, got.scale_rows, got.quaternions, got.colors, factor)
    # row order: views in order, the kept pixels of a view in row-major order
    want = np.concatenate([P[k] for P, k in zip(got.points, got.keep)])
    assert np.array_equal(got.means, want)
    assert np.array_equal(got.colors, np.concatenate([im.astype(dtype)[:, k].T for im, k in zip(g.images, got.keep)]))


def test_restatement_edges():
    """The pieces the golden's scene does not reach: flat maps, tiny maps, NaN propagation, the zero of the sign."""
    P = np.zeros((1, 5, 3), f32)
    assert (wr.scale_map(P) == f32(1e-3) * f32(0.5)).all() and (wr.scale_map(P, 4) == f32(1e-3) * f32(0.5) * f32(4)).all()
    assert (wr.normal_map(np.zeros((2, 7, 3), f32)) == np.array([0, 0, 1], f32)).all()
    y, x = np.mgrid[0:4, 0:5].astype(f32)
    P = np.stack([x * f32(2), y * f32(3), np.ones_like(x)], -1)
    assert (wr.scale_map(P) == 1).all() and (wr.scale_map(P, 2) == 2).all()  # min(2, 3) / 2, borders replicated
    n = wr.normal_map(P)
    assert (n == np.array([0, 0, -1], f32)).all()  # cross(d/dy, d/dx)
    P[1, 2, 0] = np.nan
    s = wr.scale_map(P)
    assert np.isnan(s[1, 1:4]).all() and np.isnan(s[0, 2]) and np.isnan(s[2, 2]) and np.isfinite(s[3]).all() and np.isfinite(s[:, 0]).all()
    q = wr.quaternions(np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0, 0]], f32))
    assert np.abs(q[0] - np.array([0.5, 0, 0, -0.5], f32) * np.sqrt(f32(2))).max() < 1e-7  # x_axis = cross((1,0,0), z) = -y
    assert np.abs(wr.quaternion_to_matrix(q[:3])[:, :, 2] - np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0]])).max() < 1e-6
    assert np.isfinite(q[3]).all()  # a zero normal: the floors of normalize keep it finite


# ---- the library's host side --------------------------------------------------------------------------------------------------
def test_workspace_queries_and_argument_refusals(hip_lib):
    lib = hip_lib
    nul, one, big = ctypes.c_void_p(0), ctypes.c_void_p(256), 1 << 30
    rows = ctypes.c_int(-7)

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    sizes = (ctypes.c_int * 4)(5, 4, 7, 3)
    # workspace: grows with the workgroups, shrinks with the grid, 0 for what is refused
    small = lib.g4s_warp_init_workspace(2, sizes, -1)
    usual = (ctypes.c_int * 160)(*([800, 600] * 50 + [512, 512] * 30))
    large, coarse = lib.g4s_warp_init_workspace(80, usual, -1), lib.g4s_warp_init_workspace(80, usual, 2)
    assert 0 < small < coarse < large and large > (50 * 1875 + 30 * 1024) * 8
    assert lib.g4s_warp_init_workspace(0, nul, -1) > 0 and lib.g4s_warp_init_workspace(2, sizes, 0) == small
    assert lib.g4s_warp_init_workspace(-1, sizes, 1) == 0 and lib.g4s_warp_init_workspace(2, nul, 1) == 0
    for bad in ((0, 4, 7, 3), (5, -1, 7, 3), (5, 4, 7, 0), (32769, 32769, 7, 3)):
        assert lib.g4s_warp_init_workspace(2, (ctypes.c_int * 4)(*bad), 1) == 0, bad
    huge = (ctypes.c_int * 4)(32768, 32768, 32768, 32768)  # 2 x 2^30 lattice cells = 2^31: refused; a grid of 2 brings it below
    assert lib.g4s_warp_init_workspace(2, huge, -1) == 0 and lib.g4s_warp_init_workspace(1, huge, -1) > 0
    assert lib.g4s_warp_init_workspace(2, huge, 2) > 0

    maps = (ctypes.c_void_p * 2)(256, 512)
    hole = (ctypes.c_void_p * 2)(256, 0)
    wv, focal, rays = (ctypes.c_float * 32)(), (ctypes.c_float * 4)(), (ctypes.c_float * 24)()
    tail = (one, big, nul)
    count = lambda **k: lib.g4s_warp_init_count(*[k.get(n, d) for n, d in (
        ("V", 2), ("wv", wv), ("focal", focal), ("sizes", sizes), ("depth", maps), ("rays", rays), ("g", -1), ("th", 0.01),
        ("max_scale", 0.05), ("keep", maps), ("rows", ctypes.byref(rows)))], *k.get("tail", tail))
    expect(count(V=-1), "must not be negative")
    expect(count(sizes=nul), "NULL required pointer")
    expect(count(sizes=(ctypes.c_int * 4)(5, 0, 7, 3)), "must be positive")
    expect(count(sizes=huge), "below 2^31")
    expect(count(rows=nul), "NULL required pointer")
    for name in ("wv", "focal", "rays"):
        expect(count(**{name: nul}), "NULL required pointer")
    expect(count(depth=nul), "depth: NULL array")
    expect(count(depth=hole), "depth[1]: NULL pointer")
    expect(count(keep=nul), "keep: NULL array")
    expect(count(keep=hole), "keep[1]: NULL pointer")  # a NULL map of one view
    expect(count(tail=(one, 64, nul)), "workspace too small")
    expect(count(tail=(nul, big, nul)), "workspace too small")
    assert rows.value == 0  # reset before the pointers are looked at
    # no view: success without a launch, whatever the pointers
    rows.value = -7
    assert lib.g4s_warp_init_count(0, nul, nul, nul, nul, nul, -1, 0.01, 0.05, nul, ctypes.byref(rows), nul, 0, nul) == 0
    assert rows.value == 0

    outs = (one, one, one, one)
    emit = lambda **k: lib.g4s_warp_init_emit(*[k.get(n, d) for n, d in (
        ("V", 2), ("wv", wv), ("focal", focal), ("sizes", sizes), ("depth", maps), ("rays", rays), ("images", maps), ("g", -1),
        ("min_scale", 0.0005), ("keep", maps), ("rows", 3))], *k.get("outs", outs), *k.get("tail", tail))
    expect(emit(rows=-1), "n_rows must lie in")
    expect(emit(rows=5 * 4 + 7 * 3 + 1), "n_rows must lie in")
    expect(emit(rows=3 * 2 + 4 * 2 + 1, g=2), "n_rows must lie in")  # the lattice of the grid: ceil(4/2) ceil(5/2) + ceil(3/2) ceil(7/2)
    expect(emit(sizes=(ctypes.c_int * 4)(5, 4, -7, 3)), "must be positive")
    expect(emit(V=-1), "must not be negative")
    for name in ("wv", "focal", "rays"):
        expect(emit(**{name: nul}), "NULL required pointer")
    expect(emit(images=nul), "images: NULL array")
    expect(emit(images=hole), "images[1]: NULL pointer")
    expect(emit(depth=hole), "depth[1]: NULL pointer")
    expect(emit(keep=hole), "keep[1]: NULL pointer")
    expect(emit(outs=(one, nul, one, one)), "NULL required pointer")
    expect(emit(tail=(one, 64, nul)), "workspace too small")
    # no row, and no view: success without a launch
    assert emit(rows=0, depth=nul, images=nul, keep=nul, outs=(nul,) * 4, tail=(nul, 0, nul)) == 0
    assert lib.g4s_warp_init_emit(0, nul, nul, nul, nul, nul, nul, -1, 0.0005, nul, 0, nul, nul, nul, nul, nul, 0, nul) == 0


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_cannot_take():
    import torch
    from g4splat_amd import chart_init, warp_init
    d, im = torch.zeros((2, 4, 5)), torch.zeros((2, 3, 4, 5))
    cams = [None, None]
    views = [type("View", (), {"original_image": im[0]})() for _ in cams]
    for call in (lambda: warp_init.warp_keep_masks(d, cams), lambda: warp_init.warp_surfels(list(d), cams, list(im)),
                 lambda: warp_init.get_gaussian_parameters_by_warp_from_depths(list(d), views),
                 lambda: chart_init.initial_gaussians(list(d), cams, list(im), use_downsample_gaussians=True,
                                                      downsample_gaussians_type="warp")):
        with pytest.raises(ValueError, match="HIP device"):
            call()
    with pytest.raises(ValueError, match="2 views but 3 depths"):
        warp_init.warp_keep_masks(torch.zeros((3, 4, 5)), cams)
    with pytest.raises(ValueError, match="'voxel' or 'warp'"):
        chart_init.initial_gaussians(list(d), cams, list(im), downsample_gaussians_type="grid")
    assert warp_init.warp_keep_masks([], []) == []
    assert [tuple(t.shape) for t in warp_init.warp_surfels([], [], [])] == [(0, 3), (0, 2), (0, 4), (0, 3)]


@pytest.mark.parametrize("n_input", [49, 50, 51, 120])
@pytest.mark.parametrize("n_extra", [0, 30, 31, 45])
def test_select_init_views_for_the_warp_path(n_input, n_extra):
    from g4splat_amd import chart_init
    input_ids, extra_ids = chart_init.select_init_views(n_input, n_extra, warp=True)
    assert input_ids == list(range(n_input)) and all(type(i) is int for i in input_ids)  # no cap on the input views
    assert extra_ids == chart_init.select_init_views(n_input, n_extra)[1]                # the extra views as before
    assert chart_init.select_init_views(n_input, n_extra, warp=False) == chart_init.select_init_views(n_input, n_extra)


def test_initial_gaussians_defaults_take_the_old_path():
    from g4splat_amd import chart_init
    p = inspect.signature(chart_init.initial_gaussians).parameters
    assert p["use_downsample_gaussians"].default is False and p["downsample_gaussians_type"].default == "voxel"
    assert p["warp_depth_error_thresh"].default == 0.01 and p["warp_downsample_pixel_grid_size"].default == -1
    assert list(p)[:8] == ["input_depths", "input_cameras", "input_images", "extra_depths", "extra_cameras", "extra_images",
                           "max_gaussians_num", "use_downsample_gaussians"]
    assert inspect.signature(chart_init.select_init_views).parameters["warp"].default is False
