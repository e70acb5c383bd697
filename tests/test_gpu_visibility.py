"""The visibility grid on the MI355X (g4splat_amd.visibility, csrc/tsdf/visibility.hip) against the numpy restatement of the
contract (tests/visibility_ref.py): words, bytes, counts and float bits are compared exactly.  The restatement itself is
pinned to the reference's code in tests/test_visibility_cpu.py.  The last tests check the meaning end to end on an
analytic sphere."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import visibility_ref as vr
from g4splat_amd import ply_io, synthetic, visibility
from support import dev, same_bits

pytestmark = pytest.mark.gpu

LO = np.array([-2.03, -1.97, -2.11], np.float32)
HI = np.array([2.07, 2.01, 1.93], np.float32)
EYES = [(3.2, 0.3, 0.2), (-0.4, 3.0, 0.5), (-3.0, -0.6, 0.9), (0.5, -0.7, -3.1), (1.9, 1.8, 1.7)]
BACKGROUND = 5.0


def _look_at(eye, W, H, fov_deg=55.0, target=(0.0, 0.0, 0.0)):
    return synthetic.look_at_camera(eye, target, (0.0, 0.0, 1.0), math.radians(fov_deg), W, H)


def _stack(name):
    """(cameras, depth maps) of a named view stack."""
    if name == "none":
        return [], []
    if name in ("one", "five"):
        cams = [_look_at(e, 64, 48) for e in EYES[: 1 if name == "one" else 5]]
    elif name == "seventy":  # half resolution, on a spiral about the sphere
        cams = []
        for i in range(70):
            a, z = 2.0 * math.pi * i / 17.0, -1.5 + 3.0 * i / 69.0
            cams.append(_look_at((3.0 * math.cos(a), 3.0 * math.sin(a), z), 32, 24))
    elif name == "mixed":
        cams = [_look_at(e, *((64, 48) if i % 2 == 0 else (32, 24))) for i, e in enumerate(EYES)]
    else:
        raise KeyError(name)
    return cams, [vr.sphere_depth(c, c.image_width, c.image_height, 1.0, BACKGROUND) for c in cams]


_cache = {}


def _case(stack, R, lo=LO, hi=HI):
    """The grid of a stack at a resolution from the library and from the restatement, each built once per session."""
    key = (stack, R, tuple(lo), tuple(hi)) if isinstance(stack, str) else None
    if key not in _cache:
        cams, depths = _stack(stack) if key else stack
        grid = visibility.VisibilityGrid(dev(lo), dev(hi), R, cams, [dev(d) for d in depths])
        bits = vr.build(lo, hi, R, list(zip(cams, depths)))
        case = SimpleNamespace(cams=cams, depths=depths, grid=grid, bits=bits, R=R)
        if key is None:
            return case
        _cache[key] = case
    return _cache[key]


def _check_grid(c):
    R = c.R
    words = c.grid.words.cpu().numpy().view(np.uint64)
    assert words.shape == ((R ** 3 + 63) // 64,) and c.grid.words.dtype == torch.int64
    assert np.array_equal(words, vr.pack(c.bits))
    if R ** 3 % 64:
        assert int(words[-1]) >> (R ** 3 % 64) == 0  # tail bits
    dense = c.grid.visibility_grid
    assert dense.shape == (R, R, R) and dense.dtype == torch.float32
    assert np.array_equal(dense.cpu().numpy().reshape(-1), vr.unpack(words, R ** 3).astype(np.float32))


@pytest.mark.parametrize("R", [1, 33, 64])
@pytest.mark.parametrize("stack", ["none", "one", "five", "seventy", "mixed"])
def test_build_equals_the_restatement(hip_lib, stack, R):
    """R = 33: 35 937 voxels = 561 words + 33 bits, words straddle rows and the last word has a tail."""
    c = _case(stack, R)
    _check_grid(c)
    if stack == "none":
        assert not c.bits.any()
    elif R > 1:
        assert 0.2 < c.bits.mean() < 0.97  # both answers occur in number (the sphere alone is 6 % of the box)


@pytest.mark.parametrize("crop", ["one_column", "one_row", "one_pixel"])
def test_build_on_cropped_maps(hip_lib, crop):
    """A view whose map is one pixel wide, high or both: its size stands in for the camera's, the tap clamps inside it."""
    rows, cols = {"one_column": (slice(None), slice(31, 32)), "one_row": (slice(23, 24), slice(None)),
                  "one_pixel": (slice(23, 24), slice(31, 32))}[crop]
    cams, depths = _stack("five")
    depths = [np.ascontiguousarray(d[rows, cols]) if i != 1 else d for i, d in enumerate(depths)]
    if crop == "one_pixel":
        cams, depths = cams[:1] + cams[2:], depths[:1] + depths[2:]  # cropped maps only
    c = _case((cams, depths), 33)
    _check_grid(c)
    assert c.bits.any() and not c.bits.all()


def test_sample_inside_outside_on_the_corner_and_nan(hip_lib):
    c = _case("five", 33)
    rng = np.random.default_rng(3)
    inside = rng.uniform(LO, HI, (3000, 3))
    outside = rng.uniform(-6.0, 6.0, (1000, 3))
    special = np.array([HI, LO, np.nextafter(HI, LO), [np.nan, 0.0, 0.0], [0.5, np.nan, -0.5], [np.nan] * 3,
                        [np.inf, -np.inf, 0.0], [1e30, 1e30, -1e30]], np.float64)
    pts = np.concatenate([inside, outside, special]).astype(np.float32)
    got = c.grid.check_valid_camera_center(dev(pts))
    assert got.dtype == torch.bool and got.shape == (len(pts),)
    want = vr.sample(c.bits, pts, LO, HI, 33)
    assert np.array_equal(got.cpu().numpy(), want) and 0.2 < want.mean() < 0.9
    # leading dimensions are kept, an empty batch works
    assert c.grid.check_valid_camera_center(dev(pts[:12]).reshape(3, 4, 3)).shape == (3, 4)
    assert c.grid.check_valid_camera_center(dev(pts[:0])).shape == (0,)


def _march(c, cam, depth, expect_S=None):
    d = dev(depth)
    before = d.clone()
    (got,) = c.grid.render_visibility_map([cam], [d])
    assert torch.equal(d, before)  # the caller's depth map is not touched
    S = vr.n_samples(depth, vr.grid_frame(LO, HI, c.R)[2].min())
    assert c.grid.n_samples(d) == S
    if expect_S is not None:
        assert expect_S(S), S
    want = vr.march(c.bits, LO, HI, c.R, depth, cam)
    assert got.dtype == torch.float32 and got.shape == depth.shape
    same_bits(got, want)
    return want, S


@pytest.mark.parametrize("S", [10, 11])
def test_march_with_no_and_with_one_sample(hip_lib, S):
    """S = 10: no sample, every valid pixel is 1.  S = 11: one sample, the camera centre."""
    c = _case("five", 33)
    cell = float(vr.grid_frame(LO, HI, 33)[2].min())
    cam = _look_at((1.6, 1.2, 1.5), 33, 17, 60.0)
    depth = vr.sphere_depth(cam, 33, 17, 1.0, BACKGROUND)
    depth = (depth * np.float32((S - 0.5) * cell / depth.max())).astype(np.float32)
    depth[3, 5] = 0.0
    want, _S = _march(c, cam, depth, lambda s: s == S)
    if S == 10:
        assert want[3, 5] == 0 and want.sum() == want.size - 1
    else:
        centre_visible = vr.sample(c.bits, np.asarray(cam.camera_center)[None], LO, HI, 33)[0]
        assert centre_visible and want.sum() == want.size - 1


def test_march_with_hundreds_of_samples_from_outside_the_box(hip_lib):
    c = _case("five", 64)
    cam = _look_at((8.0, 0.75, 0.5), 40, 30, 16.0)  # behind the first input view, looking down its frustum
    depth = vr.sphere_depth(cam, 40, 30, 1.0, 12.0)
    want, S = _march(c, cam, depth, lambda s: s >= 150)
    assert 0.02 < want.mean() < 0.98


def test_march_from_an_input_view_and_with_invalid_pixels(hip_lib):
    c = _case("five", 64)
    cam, depth = c.cams[0], c.depths[0].copy()
    want, _S = _march(c, cam, depth)
    assert 0.3 < want.mean() < 0.95
    assert not _march(c, c.cams[4], c.depths[4])[0].any()  # the last view's own centre lies in a voxel that no view sees
    depth[::5, ::3] = 0.0
    depth[1, 1], depth[2, 2], depth[3, 3], depth[4, 4] = -1.0, np.float32(1e-6), np.float32(1.0000001e-6), np.float32(1e-7)
    want, _S = _march(c, cam, depth)
    assert not want[::5, ::3].any() and want[1, 1] == 0 and want[2, 2] == 0 and want[4, 4] == 0
    # every pixel invalid: the sample count comes from the 1e-3 that stands in for them
    want, S = _march(c, cam, np.zeros_like(depth))
    assert S == 1 and not want.any()


def test_march_a_one_pixel_map(hip_lib):
    c = _case("five", 33)
    cam = _look_at((1.6, 1.2, 1.5), 1, 1, 60.0)
    for value in (2.0, 0.0):
        want, _S = _march(c, cam, np.full((1, 1), value, np.float32))
        assert want.shape == (1, 1)
    # [1,H,W] maps are accepted
    (m,) = c.grid.render_visibility_map([c.cams[0]], [dev(c.depths[0])[None]])
    assert m.shape == c.depths[0].shape


@pytest.fixture(scope="module")
def cloud():
    """Points about the scene: in and around the box, near the sphere's surface, the camera centres, a NaN."""
    rng = np.random.default_rng(11)
    pts = rng.uniform(-2.6, 2.6, (3000, 3))
    s = rng.normal(size=(1500, 3))
    pts[:1500] = s / np.linalg.norm(s, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (1500, 1))
    special = np.concatenate([np.asarray(EYES), [[np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]]])
    return np.concatenate([pts, special]).astype(np.float32)


@pytest.mark.parametrize("skip_view", [None, 2])
@pytest.mark.parametrize("mode", ["free", "surface"])
def test_view_counts_equal_the_restatement(hip_lib, cloud, mode, skip_view):
    cams, depths = _stack("mixed")
    got = visibility.view_counts(dev(cloud), cams, [dev(d) for d in depths], mode, 0.1, skip_view)
    want = vr.view_counts(cloud, list(zip(cams, depths)), vr.FREE if mode == "free" else vr.SURFACE, 0.1, skip_view)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert want.max() >= 2 and (want == 0).any()
    if skip_view is not None:
        full = vr.view_counts(cloud, list(zip(cams, depths)), vr.FREE if mode == "free" else vr.SURFACE, 0.1, None)
        assert (full != want).any()  # the skipped view mattered


def test_view_counts_without_views_or_points(hip_lib, cloud):
    assert not visibility.view_counts(dev(cloud), [], []).any()
    cams, depths = _stack("one")
    assert visibility.view_counts(dev(cloud[:0]), cams, [dev(d) for d in depths]).shape == (0,)


def test_depths_to_points_and_the_fused_pixel_counts(hip_lib):
    cams, depths = _stack("mixed")
    dd = [dev(d) for d in depths]
    for i in (0, 1):
        pts = visibility.depths_to_points(dd[i], cams[i])
        same_bits(pts, vr.depths_to_points(depths[i], cams[i]))
        for mode in ("free", "surface"):
            fused = visibility.pixel_view_counts(cams[i], dd[i], cams, dd, mode, 0.1, skip_view=i)
            explicit = visibility.view_counts(pts, cams, dd, mode, 0.1, skip_view=i)
            assert fused.shape == depths[i].shape and torch.equal(fused.reshape(-1), explicit)
            assert explicit.max() >= 1


def test_reference_named_wrappers_equal_their_restatements(hip_lib, cloud):
    cams, depths = _stack("five")
    dd = [dev(d) for d in depths]
    free = visibility.check_valid_camera_center_by_depth(cams, dd, dev(cloud))
    surf = visibility.get_visible_mask_for_input_views(cams, dd, dev(cloud), depth_threshold=0.05)
    assert free.dtype == torch.bool and surf.dtype == torch.bool
    assert np.array_equal(free.cpu().numpy(), vr.check_valid_camera_center_by_depth(cams, depths, cloud))
    assert np.array_equal(surf.cpu().numpy(), vr.get_visible_mask_for_input_views(cams, depths, cloud, 0.05))
    assert 0.1 < free.float().mean().item() < 0.9 and 0.1 < surf.float().mean().item() < 0.9


@pytest.mark.parametrize("explicit", [False, True])
def test_build_visibility_masks(hip_lib, explicit):
    cams, depths = _stack("mixed")
    dd = [dev(d)[None] for d in depths]  # [1,H,W], as the reference passes them
    host_pts = [vr.depths_to_points(d, c) for c, d in zip(cams, depths)] if explicit else None
    dev_pts = [dev(p) for p in host_pts] if explicit else None
    times = visibility.build_visibility_masks(cams, dd, dev_pts, 0.1, return_origin_masks=True)
    want_times = vr.build_visibility_masks(cams, depths, host_pts, 0.1, return_origin_masks=True)
    for k in (1, 2):
        masks = visibility.build_visibility_masks(cams, dd, dev_pts, 0.1, least_num_views=k)
        want = vr.build_visibility_masks(cams, depths, host_pts, 0.1, least_num_views=k)
        for m, w, d in zip(masks, want, depths):
            assert m.shape == (1,) + d.shape and m.dtype == torch.float32
            assert np.array_equal(m.cpu().numpy(), w)
    for t, w in zip(times, want_times):
        assert t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), w)
    assert max(w.max() for w in want_times) >= 2 and min(w.min() for w in want_times) == 0


def test_compaction_in_flat_index_order(hip_lib, tmp_path):
    c = _case("five", 33)
    centres = vr.grid_centers(LO, HI, 33)
    vis, inv = c.grid.get_all_visible_pnts(), c.grid.invisible_points()
    same_bits(vis, centres[c.bits])
    same_bits(inv, centres[~c.bits])
    bound = [float(v) for v in c.grid.get_visible_boundary()]
    assert bound == [float(v) for v in np.concatenate([centres[c.bits].min(0), centres[c.bits].max(0)])]
    path = str(tmp_path / "invisible.ply")
    c.grid.vis_invisible_pnts(path)
    v = ply_io.read_ply_vertices(path)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), centres[~c.bits])


def test_compaction_of_all_visible_and_all_invisible_grids(hip_lib, tmp_path):
    # a small box in the free space between the first camera and the sphere: every voxel is seen
    lo, hi = np.array([1.6, -0.2, -0.2], np.float32), np.array([2.1, 0.3, 0.3], np.float32)
    c = _case("one", 5, lo, hi)
    assert c.bits.all()
    _check_grid(c)
    same_bits(c.grid.get_all_visible_pnts(), vr.grid_centers(lo, hi, 5))
    assert c.grid.invisible_points().shape == (0, 3)
    path = str(tmp_path / "none.ply")
    c.grid.vis_invisible_pnts(path)  # nothing invisible: nothing is written, as in the reference
    assert not (tmp_path / "none.ply").exists()
    # no view: nothing is seen
    c = _case("none", 33)
    assert c.grid.get_all_visible_pnts() is None and c.grid.get_visible_boundary() is None
    same_bits(c.grid.invisible_points(), vr.grid_centers(LO, HI, 33))


# ---- end to end on the analytic sphere ----------------------------------------------------------------------------------
def test_ring_of_views_sees_everything_but_the_sphere(hip_lib):
    """Eight views on a ring about the unit sphere: no voxel centre inside radius 0.9 is visible (the maps are fine enough
    that a tapped pixel's ray stays inside the silhouette), and every camera centre lies in a visible voxel (each is seen,
    past the sphere, by the views at +-135 degrees)."""
    lo, hi, R = np.full(3, -3.5, np.float32), np.full(3, 3.5, np.float32), 64
    cams = [_look_at((3.0 * math.cos(a), 3.0 * math.sin(a), 0.0), 128, 96, 70.0) for a in np.arange(8) * math.pi / 4]
    depths = [dev(vr.sphere_depth(c, 128, 96, 1.0, 8.0)) for c in cams]
    grid = visibility.VisibilityGrid(dev(lo), dev(hi), R, cams, depths)
    centres = vr.grid_centers(lo, hi, R)
    dense = grid.visibility_grid.cpu().numpy().reshape(-1) > 0.5
    inner = np.linalg.norm(centres, axis=1) < 0.9
    assert inner.sum() > 1000 and not dense[inner].any()
    assert 0.3 < dense.mean() < 0.99
    eyes = dev(np.stack([c.camera_center for c in cams]))
    assert grid.check_valid_camera_center(eyes).all()
    assert visibility.check_valid_camera_center_by_depth(cams, depths, eyes).all()
    assert not grid.check_valid_camera_center(dev(np.zeros((1, 3), np.float32))).any()


def test_novel_view_is_visible_on_the_lit_side_and_not_behind_the_sphere(hip_lib):
    """One input view E of the sphere, one novel view N from the side.  A pixel of N whose samples all lie well inside E's
    frustum and well clear of the sphere and its shadow must be 1; a pixel with a sample deep inside the shadow must be 0
    (margins of three voxels; the pixels in between are not judged)."""
    lo, hi, R = np.full(3, -4.0, np.float32), np.full(3, 4.0, np.float32), 64
    cell = 8.0 / R
    E = np.array([3.5, 0.0, 0.0])
    cam_e = _look_at(tuple(E), 128, 96, 100.0)
    grid = visibility.VisibilityGrid(dev(lo), dev(hi), R, [cam_e], [dev(vr.sphere_depth(cam_e, 128, 96, 1.0, 9.0))])
    W, H = 64, 48
    cam_n = _look_at((1.0, 2.2, 0.0), W, H, 60.0)
    depth = vr.sphere_depth(cam_n, W, H, 1.0, 4.0)
    (got,) = grid.render_visibility_map([cam_n], [dev(depth)])
    got = got.cpu().numpy().reshape(-1)
    S = grid.n_samples(dev(depth))
    assert S > 30

    o, _D = vr.ray_record(cam_n, W, H, np.float64)
    dirs = vr.ray_dirs(cam_n, W, H, np.float64)
    t = np.linspace(0.0, (S - 11) / (S - 1), 400)[None, :, None] * depth.reshape(-1, 1, 1).astype(np.float64)
    p = o[None, None] + t * dirs[:, None]                       # [pixels, 400, 3]: the sampled part of every ray

    def shadowed(p, radius):  # the segment E -> p meets the sphere of `radius`
        d = p - E
        a, b, c = (d * d).sum(-1), 2.0 * (d @ E), E @ E - radius * radius
        disc = b * b - 4.0 * a * c
        s = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a)
        return (disc > 0) & (s > 0) & (s < 1)

    cam_space = p @ np.asarray(cam_e.world_view_transform, np.float64)[:3, :3] + np.asarray(cam_e.world_view_transform)[3, :3]
    # E's half angles are 50 and about 41.8 degrees; 45 and 37 leave five degrees, two voxels and more at these distances
    in_frustum = (cam_space[..., 2] > 0.5) & (np.abs(cam_space[..., 0]) < cam_space[..., 2] * math.tan(math.radians(45.0))) \
        & (np.abs(cam_space[..., 1]) < cam_space[..., 2] * math.tan(math.radians(37.0)))
    margin = 3.0 * cell
    safe_visible = (in_frustum & ~shadowed(p, 1.0 + margin) & (np.abs(p) < 4.0 - margin).all(-1)).all(1)
    safe_hidden = shadowed(p, 1.0 - margin).any(1)
    assert safe_visible.sum() > 200 and safe_hidden.sum() > 200
    assert (got[safe_visible] == 1).all()
    assert (got[safe_hidden] == 0).all()
    centre = (H // 2) * W + W // 2                              # looks at the sphere's side that E lights
    assert safe_visible[centre] and got[centre] == 1
