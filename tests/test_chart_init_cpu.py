"""The chart-surfel contract without a GPU: the numpy restatement (tests/chart_init_ref.py) against what the reference's own
function computed (tests/golden/chart_init.npz, written by tests/golden/make_golden_chart_init.py), the voxel pick against a
float64 replay of the reference's index recovery, the host-side argument checks of the new entry points, and the Python
surface's refusals.

The yardstick of every continuous output is the largest |float32 run - float64 run| of the REFERENCE over the faces both runs
keep, recorded by the generator: the float64 restatement has to be within it of the reference's float64 results, the float32
restatement within twice it.  The keep mask is compared exactly on the faces whose float64 ratio is farther from ratio_th
than the ratio's (relative) yardstick; the generator asserts that at most 1 % of the faces are nearer, and so does this
file.  Rotations are compared as matrices rebuilt from the quaternions, so q and -q are the same answer."""
import ctypes

import numpy as np
import pytest

import chart_init_ref as cr
from chart_init_ref import check_against_golden, pair_cloud, random_cloud
from support import load_chart_init_golden

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def golden():
    return load_chart_init_golden()


def test_golden_covers_what_it_claims(golden):
    g = golden
    assert g["points"].shape == (2, 9, 7, 3) and g["images"].shape == (2, 9, 7, 3)
    keep, ratio = g["ref64_keep"], g["ref64_ratio"]
    assert len(keep) == 2 * 2 * 8 * 6
    th = float(g["ratio_th"])
    assert (ratio[np.isfinite(ratio)] < th).any() and (ratio[np.isfinite(ratio)] > th).any() and (~np.isfinite(ratio)).any()
    assert np.array_equal(keep[~g["near"]], g["ref32_keep"][~g["near"]])
    assert (g["images"] < 0).any() and (g["images"] > 1).any()
    assert all(v > 0 for v in g["yard"].values())


@pytest.mark.parametrize("dtype, factor", [(f64, 1.0), (f32, 2.0)])
def test_restated_surfels_match_the_reference(golden, dtype, factor):
    g = golden
    got = cr.pointmap_surfels(g["points"], g["images"], None, g["ratio_th"], g["normalized_scales"], g["normal_scale"], dtype)
    assert got["means"].dtype == dtype and got["quaternions"].dtype == dtype
    # the ratio itself, where it matters
    ratio = g["ref64_ratio"]
    rel = np.isfinite(ratio) & (ratio < 4 * float(g["ratio_th"]))
    err = (np.abs(got["ratio"][rel].astype(f64) - ratio[rel]) / ratio[rel]).max()
    print(f"ratio: largest relative error {err:.3e}, bound {factor * g['yard']['ratio']:.3e}")
    assert err <= factor * g["yard"]["ratio"]
    check_against_golden(g, got, factor)


def test_restated_masks_follow_the_reference_quirks(golden):
    g = golden
    pts, img = g["points"], g["images"]
    free = cr.pointmap_surfels(pts, img)["keep"]
    none = np.zeros(pts.shape[:3], bool)
    assert np.array_equal(cr.pointmap_surfels(pts, img, none)["keep"], free)  # an all-false mask removes nothing
    assert np.array_equal(cr.pointmap_surfels(pts, img, ~none)["keep"], free)
    one = none.copy()
    one[1, 2, 3] = True  # one vertex: exactly the faces that touch it may survive
    keep, faces = cr.pointmap_surfels(pts, img, one)["keep"], cr.face_pixels(2, 9, 7)
    touching = (faces == 1 * 63 + 2 * 7 + 3).any(axis=1)
    assert touching.sum() == 6 and np.array_equal(keep, free & touching)


def test_face_order_and_constants():
    faces = cr.face_pixels(2, 3, 4)
    assert len(faces) == 2 * 2 * 2 * 3
    assert faces[0].tolist() == [0, 4, 1] and faces[5].tolist() == [6, 10, 7]      # face_1 of cells (0,0) and (1,2)
    assert faces[6].tolist() == [5, 1, 4] and faces[11].tolist() == [11, 7, 10]    # face_2 of the same cells
    assert faces[12].tolist() == [12, 16, 13]                                     # view 1 starts over
    assert len(cr.face_pixels(3, 1, 9)) == 0 and len(cr.face_pixels(3, 9, 1)) == 0
    b = np.array(cr.BARY_BITS, np.uint32).view(f32)
    assert np.abs(b.astype(f64) - 1 / 3).max() < 2e-8 and b[0] == b[1] != b[2]
    e0, e1 = np.array(cr.AXIS0_BITS, np.uint32).view(f32), np.array(cr.AXIS1_BITS, np.uint32).view(f32)
    assert np.array_equal(e0, np.array([-np.sqrt(2) / 2, np.sqrt(2) / 2, 0], f64).astype(f32))
    assert np.array_equal(e1, np.array([-1 / np.sqrt(6), -1 / np.sqrt(6), 2 / np.sqrt(6)], f64).astype(f32))


def test_quaternion_rows_rebuild_every_rotation():
    """Each of the four candidate rows is taken by some rotation, and the matrix comes back."""
    rng = np.random.default_rng(3)
    q = rng.standard_normal((400, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    R = cr.quaternion_to_matrix(q)
    t = np.stack([1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], 1 + R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2],
                  1 - R[:, 0, 0] + R[:, 1, 1] - R[:, 2, 2], 1 - R[:, 0, 0] - R[:, 1, 1] + R[:, 2, 2]], axis=1)
    assert set(np.argmax(t, axis=1).tolist()) == {0, 1, 2, 3}
    back = cr.matrix_to_quaternion(R)
    assert (back[:, 0] >= 0).all()
    assert np.abs(back - np.where((q[:, 0] < 0)[:, None], -q, q)).max() < 1e-12
    assert np.abs(cr.quaternion_to_matrix(cr.matrix_to_quaternion(R.astype(f32))) - R).max() < 1e-6


# ---- the voxel pick ---------------------------------------------------------------------------------------------------------
def replay_index_recovery(points, voxel_size):
    """What the reference's voxel_downsample_gaussians computes, replayed in float64 per voxel: every point's colour is its
    index over n, the voxel's colour is the sum of its points' colours in input order over their number (open3d adds the
    points of a voxel as they come), and the index is round(colour * n).  Voxels in ascending (cz, cy, cx)."""
    from mesh_eval_ref import voxel_cells
    p = np.asarray(points, f32)
    n = len(p)
    colour = np.arange(n) / n
    cells = voxel_cells(p, voxel_size)
    out = {}
    for i in range(n):
        key = (cells[i, 2], cells[i, 1], cells[i, 0])
        s, k = out.get(key, (0.0, 0))
        out[key] = (s + colour[i], k + 1)
    return np.array([np.round(out[key][0] / out[key][1] * n) for key in sorted(out)]).astype(np.int64)


@pytest.mark.parametrize("cloud", [pair_cloud(), pair_cloud(33, 6), random_cloud(), random_cloud(1, 2), random_cloud(300, 4) * f32(0.01)])
def test_restated_voxel_pick_matches_the_replay(cloud):
    from mesh_eval_ref import voxel_cells
    got, want = cr.voxel_pick_indices(cloud, 0.1), replay_index_recovery(cloud, 0.1)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert got.min() >= 0 and got.max() < len(cloud)
    assert len(got) == len(np.unique(voxel_cells(cloud, 0.1), axis=0))


def test_pair_cloud_is_the_half_way_case():
    from mesh_eval_ref import voxel_cells
    cloud = pair_cloud()
    cells = voxel_cells(cloud, 0.1)
    _u, inverse, counts = np.unique(cells[:, ::-1], axis=0, return_inverse=True, return_counts=True)  # ascending (cz, cy, cx)
    assert (counts == 2).all()
    sums = np.bincount(inverse.reshape(-1), weights=np.arange(len(cloud)))
    assert (sums % 2 == 1).all()
    picks = cr.voxel_pick_indices(cloud, 0.1)
    assert (np.abs(picks - sums / 2) == 0.5).all()  # one of the two neighbours of the half-way mean


# ---- the library's host side --------------------------------------------------------------------------------------------------
def test_workspace_queries_and_argument_refusals(hip_lib):
    lib = hip_lib
    nul, one, big = ctypes.c_void_p(0), ctypes.c_void_p(256), 1 << 30
    count = ctypes.c_int(-7)

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    # workspace: grows with the faces, 0 for sizes out of range
    small, large = lib.g4s_chart_surfels_workspace(1, 2, 2), lib.g4s_chart_surfels_workspace(80, 480, 640)
    assert 0 < small < large and large > 2 * 80 * (479 * 639 // 256) * 40
    assert lib.g4s_chart_surfels_workspace(0, 5, 5) > 0 and lib.g4s_chart_surfels_workspace(3, 1, 9) > 0
    for bad in ((-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, -2), (1, 32769, 32769), (4, 16385, 16385), (2 ** 15, 257, 257)):
        assert lib.g4s_chart_surfels_workspace(*bad) == 0, bad
    assert lib.g4s_chart_surfels_workspace(2 ** 15 - 1, 257, 129) > 0  # 2 V C = 2^31 - 2^16

    maps = (ctypes.c_void_p * 2)(256, 512)
    hole = (ctypes.c_void_p * 2)(256, 0)
    rays = (ctypes.c_float * 24)()
    tail = (one, big, nul)
    expect(lib.g4s_chart_surfels_count(-1, 4, 4, 0, maps, nul, nul, 5.0, ctypes.byref(count), *tail), "must not be negative")
    expect(lib.g4s_chart_surfels_count(2, 0, 4, 0, maps, nul, nul, 5.0, ctypes.byref(count), *tail), "must be positive")
    expect(lib.g4s_chart_surfels_count(2, 32769, 32769, 0, maps, nul, nul, 5.0, ctypes.byref(count), *tail), "below 2^31")
    expect(lib.g4s_chart_surfels_count(2, 4, 4, 0, maps, nul, nul, 5.0, nul, *tail), "NULL required pointer")
    expect(lib.g4s_chart_surfels_count(2, 4, 4, 0, nul, nul, nul, 5.0, ctypes.byref(count), *tail), "maps: NULL array")
    expect(lib.g4s_chart_surfels_count(2, 4, 4, 0, hole, nul, nul, 5.0, ctypes.byref(count), *tail), "maps[1]: NULL pointer")
    expect(lib.g4s_chart_surfels_count(2, 4, 4, 1, maps, nul, nul, 5.0, ctypes.byref(count), *tail), "NULL required pointer")
    expect(lib.g4s_chart_surfels_count(2, 4, 4, 0, maps, nul, hole, 5.0, ctypes.byref(count), *tail), "masks[1]: NULL pointer")
    expect(lib.g4s_chart_surfels_count(2, 4, 4, 0, maps, nul, nul, 5.0, ctypes.byref(count), one, 64, nul), "workspace too small")
    expect(lib.g4s_chart_surfels_count(2, 4, 4, 1, maps, rays, nul, 5.0, ctypes.byref(count), nul, big, nul), "workspace too small")
    # no faces: success without a launch, whatever the pointers
    count.value = -7
    assert lib.g4s_chart_surfels_count(2, 1, 9, 0, nul, nul, nul, 5.0, ctypes.byref(count), nul, 0, nul) == 0 and count.value == 0
    count.value = -7
    assert lib.g4s_chart_surfels_count(0, 4, 4, 0, nul, nul, nul, 5.0, ctypes.byref(count), nul, 0, nul) == 0 and count.value == 0

    outs = (one, one, one, one)
    expect(lib.g4s_chart_surfels_emit(2, 4, 4, 0, maps, nul, maps, 0.5, 1e-10, -1, *outs, *tail), "n_faces must lie in")
    expect(lib.g4s_chart_surfels_emit(2, 4, 4, 0, maps, nul, maps, 0.5, 1e-10, 37, *outs, *tail), "n_faces must lie in")
    expect(lib.g4s_chart_surfels_emit(2, 4, 0, 0, maps, nul, maps, 0.5, 1e-10, 3, *outs, *tail), "must be positive")
    expect(lib.g4s_chart_surfels_emit(2, 4, 4, 0, maps, nul, nul, 0.5, 1e-10, 3, *outs, *tail), "images: NULL array")
    expect(lib.g4s_chart_surfels_emit(2, 4, 4, 0, hole, nul, maps, 0.5, 1e-10, 3, *outs, *tail), "maps[1]: NULL pointer")
    expect(lib.g4s_chart_surfels_emit(2, 4, 4, 1, maps, nul, maps, 0.5, 1e-10, 3, *outs, *tail), "NULL required pointer")
    expect(lib.g4s_chart_surfels_emit(2, 4, 4, 0, maps, nul, maps, 0.5, 1e-10, 3, one, nul, one, one, *tail), "NULL required pointer")
    expect(lib.g4s_chart_surfels_emit(2, 4, 4, 0, maps, nul, maps, 0.5, 1e-10, 3, *outs, one, 64, nul), "workspace too small")
    assert lib.g4s_chart_surfels_emit(2, 4, 4, 0, nul, nul, nul, 0.5, 1e-10, 0, nul, nul, nul, nul, nul, 0, nul) == 0

    # the index emit shares the count phase's checks
    expect(lib.g4s_voxel_downsample_emit_index(-1, 0, one, one, big, nul), "must not be negative")
    expect(lib.g4s_voxel_downsample_emit_index(5, 6, one, one, big, nul), "n_voxels must lie in 0..n")
    expect(lib.g4s_voxel_downsample_emit_index(5, -1, one, one, big, nul), "n_voxels must lie in 0..n")
    expect(lib.g4s_voxel_downsample_emit_index(5, 2, nul, one, big, nul), "NULL required pointer")
    expect(lib.g4s_voxel_downsample_emit_index(5, 2, one, one, 64, nul), "workspace too small")
    expect(lib.g4s_voxel_downsample_emit_index(5, 2, one, nul, big, nul), "workspace too small")
    assert lib.g4s_voxel_downsample_emit_index(5, 0, nul, nul, 0, nul) == 0


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_cannot_take():
    import torch
    from g4splat_amd import chart_init
    p = torch.zeros((2, 4, 5, 3))
    d = torch.zeros((2, 4, 5))
    cams = [None, None]
    for call in (lambda: chart_init.pointmap_surfels(p, p), lambda: chart_init.pointmap_surfels(list(p), list(p)),
                 lambda: chart_init.depthmap_surfels(d, cams, p), lambda: chart_init.get_gaussian_parameters_from_pa_data(p, list(p)),
                 lambda: chart_init.get_gaussian_parameters_from_charts_data({"pts": p, "confs": d, "scale_factor": 2.0}, list(p)),
                 lambda: chart_init.voxel_downsample_gaussians({"means": p[0, 0]}),
                 lambda: chart_init.initial_gaussians(list(d), cams, list(p))):
        with pytest.raises(ValueError, match="HIP device"):
            call()
    with pytest.raises(ValueError, match="HIP device"):
        chart_init.pointmap_surfels([p[0].numpy()], [p[0]])
    # sizes
    with pytest.raises(ValueError, match="like the other views"):
        chart_init.pointmap_surfels([p[0], p[1, :3]], p)
    with pytest.raises(ValueError, match="like the other views"):
        chart_init.pointmap_surfels(p, p[:, :, :4])
    with pytest.raises(ValueError, match="like the other views"):
        chart_init.depthmap_surfels(d, cams, p, masks=torch.zeros((2, 5, 4), dtype=torch.bool))
    with pytest.raises(ValueError, match="2 views but 1 images"):
        chart_init.pointmap_surfels(p, p[:1])
    with pytest.raises(ValueError, match="2 views but 3 depths"):
        chart_init.depthmap_surfels(torch.zeros((3, 4, 5)), cams, p)
    with pytest.raises(ValueError, match="2 views but 0 masks"):
        chart_init.pointmap_surfels(p, p, [])
    with pytest.raises(ValueError, match="0 views but 2 depths"):
        chart_init.depthmap_surfels(d, [], p)
    assert {k: tuple(v.shape) for k, v in chart_init.pointmap_surfels([], []).items()} == {
        "means": (0, 3), "scales": (0, 3), "quaternions": (0, 4), "colors": (0, 3)}  # no views: no device is asked for
    with pytest.raises(ValueError, match=r"\[V,H,W,3\]"):
        chart_init.pointmap_surfels(p[0], p)
    with pytest.raises(ValueError, match=r"\[H,W,3\]"):
        chart_init.pointmap_surfels([d[0]], [p[0]])
    # dtypes
    with pytest.raises(ValueError, match="torch.float32"):
        chart_init.pointmap_surfels(p.double(), p)
    with pytest.raises(ValueError, match="torch.float32"):
        chart_init.pointmap_surfels(p, (p * 255).to(torch.uint8))
    with pytest.raises(ValueError, match="torch.float32"):
        chart_init.depthmap_surfels(d.half(), cams, p)
    with pytest.raises(ValueError, match="torch.bool or torch.uint8"):
        chart_init.pointmap_surfels(p, p, masks=d)


@pytest.mark.parametrize("n_input", [49, 50, 51, 120])
@pytest.mark.parametrize("n_extra", [0, 30, 31, 45])
def test_select_init_views(n_input, n_extra):
    from g4splat_amd import chart_init
    input_ids, extra_ids = chart_init.select_init_views(n_input, n_extra)
    assert (input_ids, extra_ids) == cr.select_init_views(n_input, n_extra)
    assert all(type(i) is int for i in input_ids + extra_ids)
    assert len(input_ids) == min(n_input, 50) and input_ids[0] == 0 and input_ids[-1] == n_input - 1
    assert input_ids == sorted(set(input_ids))
    if n_input == 51:
        assert input_ids == list(range(49)) + [50]
    if n_input == 120:
        assert input_ids[:4] == [0, 2, 4, 7] and input_ids[-3:] == [114, 116, 119]
    if n_extra <= 30:
        assert extra_ids == list(range(n_extra))
    else:
        assert extra_ids[:20] == list(range(10)) + list(range(15, 25)) and extra_ids[20:] == list(range(30, n_extra))
