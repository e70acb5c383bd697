"""The numpy restatement of the visibility-grid contract (tests/visibility_ref.py) against the reference's own code, through
tests/golden/visibility_grid.npz (made by tests/golden/make_golden_visibility.py), and the host-side pieces of
g4splat_amd.visibility.  No GPU: the kernels are compared with the restatement in tests/test_gpu_visibility.py."""
import os

import numpy as np
import pytest
import torch

import visibility_ref as vr
from support import golden_cameras, same_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visibility_grid.npz")
DECISIONS = ("grid32", "grid48", "maps32", "maps48", "centres32", "centres48", "free", "surface", "times", "masks1", "masks2")


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    cams = golden_cameras(g)
    g["cams"], g["views"] = cams, list(zip(cams, g["depths"]))
    return g


def _recorded(g, key):
    shape = tuple(g[key + "_shape"])
    n = int(np.prod(shape))
    agreed = np.unpackbits(g[key + "_agreed"])[:n].astype(bool).reshape(shape)
    val = g[key]
    if val.dtype == np.uint8:
        val = np.unpackbits(val)[:n].astype(bool).reshape(shape)
    return val, agreed


@pytest.fixture(scope="module")
def restated(golden):
    """Every decision of the golden from the restatement in float32, computed once."""
    g = golden
    lo, hi, thr, n_in = g["bbox_min"], g["bbox_max"], float(g["threshold"]), int(g["n_input"])
    cams, depths, pts = g["cams"], list(g["depths"]), g["points"]
    out = {}
    for R in (int(r) for r in g["resolutions"]):
        bits = vr.build(lo, hi, R, g["views"][:n_in])
        out[f"grid{R}"] = bits
        out[f"maps{R}"] = np.stack([vr.march(bits, lo, hi, R, d, c) > 0.5 for c, d in g["views"]])
        out[f"centres{R}"] = vr.sample(bits, pts, lo, hi, R)
    out["free"] = vr.check_valid_camera_center_by_depth(cams, depths, pts)
    out["surface"] = vr.get_visible_mask_for_input_views(cams, depths, pts, thr)
    out["times"] = np.stack(vr.build_visibility_masks(cams, depths, g["clouds"], thr, return_origin_masks=True))
    for k in (1, 2):
        out[f"masks{k}"] = np.stack(vr.build_visibility_masks(cams, depths, g["clouds"], thr, k)) > 0.5
    return out


@pytest.mark.parametrize("key", DECISIONS)
def test_restatement_equals_the_reference_on_the_agreed_set(golden, restated, key):
    want, agreed = _recorded(golden, key)
    excluded, size, _ref_differ = (int(v) for v in golden[key + "_excluded"])
    assert size == want.size and excluded == int((~agreed).sum())
    assert excluded <= 0.001 * size
    got = np.asarray(restated[key]).reshape(want.shape)
    assert np.array_equal(got[agreed], want[agreed].astype(got.dtype))
    if want.dtype == bool:  # both answers occur in number: the comparison is not vacuous
        assert 0.05 < want.mean() < 0.95


def test_back_projected_points_agree_within_tol(golden):
    tol = float(golden["tol"])
    assert 0 < tol < 1e-4
    for (cam, depth), want in zip(golden["views"], golden["clouds"]):
        got = vr.depths_to_points(depth, cam)
        assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - want).max() <= tol


def test_fused_masks_equal_the_explicit_ones(golden):
    """points=None back-projects with the restatement's own arithmetic; on this scene no decision moves."""
    g = golden
    thr = float(g["threshold"])
    fused = np.stack(vr.build_visibility_masks(g["cams"], list(g["depths"]), None, thr, return_origin_masks=True))
    own = [vr.depths_to_points(d, c) for c, d in g["views"]]
    assert np.array_equal(fused, np.stack(vr.build_visibility_masks(g["cams"], list(g["depths"]), own, thr,
                                                                     return_origin_masks=True)))


def test_linspace_is_torchs_bit_for_bit():
    for S in range(1, 701):
        want = torch.linspace(0, 1, S, dtype=torch.float32).numpy()
        same_bits(vr.linspace_t(S), want, S)


def test_point_to_voxel_clamps_at_and_beyond_both_corners():
    lo, hi = np.array([-2.03, -1.97, -2.11], np.float32), np.array([2.07, 2.01, 1.93], np.float32)
    for R in (1, 7, 32):
        eps = np.float32(1e-3)
        pts = np.stack([lo, lo - 1, lo - np.float32(1e30), hi, hi + 1, hi + np.float32(1e30), np.nextafter(hi, lo), hi - eps,
                        lo + eps, np.array([np.inf, -np.inf, np.nan], np.float32)]).astype(np.float32)
        flat, idx = vr.voxel_index(pts, lo, hi, R)
        assert idx.min() >= 0 and idx.max() <= R - 1 and flat.max() < R ** 3
        assert (idx[:3] == 0).all() and (idx[3:8] == R - 1).all() and (idx[8] == 0).all()
        assert tuple(idx[9]) == (R - 1, 0, 0)  # +inf clamps to the top, -inf to 0, NaN gives 0
        # a voxel's centre falls into that voxel
        c = vr.grid_centers(lo, hi, R)
        assert np.array_equal(vr.voxel_index(c, lo, hi, R)[0], np.arange(R ** 3))


def test_pack_and_unpack_words():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 35937):
        bits = rng.random(n) < 0.5
        words = vr.pack(bits)
        assert words.dtype == np.uint64 and len(words) == (n + 63) // 64
        assert np.array_equal(vr.unpack(words, n), bits)
        assert all(bool(words[i >> 6] >> np.uint64(i & 63) & np.uint64(1)) == bits[i] for i in range(0, n, 97))
        if n % 64:
            assert int(words[-1]) >> (n % 64) == 0  # tail bits are zero


def test_ray_record_of_the_module_is_the_restatements():
    from g4splat_amd import synthetic, visibility
    cam = synthetic.look_at_camera((1.9, 1.8, 1.7), (0.0, 0.1, 0.0), (0.0, 0.0, 1.0), 0.9, 33, 17)
    o, D = vr.ray_record(cam, 33, 17)
    rec = visibility.ray_record(cam, 33, 17)
    assert rec.dtype == np.float32 and np.array_equal(rec, np.concatenate([o, D.reshape(9)]))
    # the centre pixel's ray looks along the camera's axis, and the origin is the camera centre
    d = D @ np.array([33 / 2, 17 / 2, 1], np.float32)
    fwd = np.array([0.0, 0.1, 0.0]) - np.array([1.9, 1.8, 1.7])
    fwd /= np.linalg.norm(fwd)
    assert np.allclose(o, cam.camera_center, atol=1e-5) and np.dot(d / np.linalg.norm(d), fwd) > 0.9999


def test_point_cloud_ply_round_trip(tmp_path):
    from g4splat_amd import ply_io
    pts = np.random.default_rng(1).normal(size=(257, 3)).astype(np.float32)
    path = str(tmp_path / "sub" / "cloud.ply")
    ply_io.write_point_cloud(path, pts)
    v = ply_io.read_ply_vertices(path)
    assert list(v) == ["x", "y", "z"]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), pts)
    ply_io.write_point_cloud(path, pts[:0])
    assert len(ply_io.read_ply_vertices(path)["x"]) == 0


def test_entry_points_check_their_arguments_on_the_host(hip_lib):
    """Bad arguments are refused before anything touches the device: negative status and a message, no launch."""
    import ctypes
    lib = hip_lib
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # `one` is never dereferenced: validation fails first
    lo, hi = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    ray = (ctypes.c_float * 12)()

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    for R in (0, -3, 1291):  # 1290^3 < 2^31 <= 1291^3
        expect(lib.g4s_visgrid_build(R, lo, hi, 0, nul, nul, nul, nul, one, nul, 0, nul), "resolution must be at least 1")
        expect(lib.g4s_visgrid_expand(R, one, one, nul, 0, nul), "resolution must be at least 1")
        assert lib.g4s_visgrid_compact_workspace(R) == 0
    expect(lib.g4s_visgrid_build(4, hi, lo, 0, nul, nul, nul, nul, one, nul, 0, nul), "bbox must be finite")
    expect(lib.g4s_visgrid_build(4, lo, lo, 0, nul, nul, nul, nul, one, nul, 0, nul), "bbox must be finite")
    expect(lib.g4s_visgrid_build(4, lo, hi, 0, nul, nul, nul, nul, nul, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_visgrid_build(4, lo, hi, -1, nul, nul, nul, nul, one, nul, 0, nul), "n_views must not be negative")
    expect(lib.g4s_visgrid_build(4, lo, hi, 1, one, nul, one, one, one, one, 1 << 20, nul), "NULL required pointer")
    expect(lib.g4s_visgrid_build(4, lo, hi, 1, one, one, one, one, one, one, 8, nul), "workspace too small")
    expect(lib.g4s_visgrid_sample(4, lo, hi, one, -1, one, one, nul, 0, nul), "n_points must be in")
    expect(lib.g4s_visgrid_sample(4, lo, hi, one, 5, nul, one, nul, 0, nul), "NULL required pointer")
    assert lib.g4s_visgrid_sample(4, lo, hi, one, 0, nul, nul, nul, 0, nul) == 0
    for march in (lib.g4s_visgrid_march, lib.g4s_visgrid_march_bytes):
        expect(march(4, lo, hi, one, 0, 4, one, ray, 11, one, nul, 0, nul), "width, height must be positive")
        expect(march(4, lo, hi, one, 1 << 16, 1 << 15, one, ray, 11, one, nul, 0, nul), "width * height at most 2^30")
        expect(march(4, lo, hi, one, 4, 4, one, ray, 0, one, nul, 0, nul), "n_samples must be at least 1")
        expect(march(4, lo, hi, one, 4, 4, one, nul, 11, one, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_visgrid_compact_count(4, one, 0, nul, one, 1 << 20, nul), "NULL required pointer")
    n = ctypes.c_int(0)
    expect(lib.g4s_visgrid_compact_count(4, one, 0, ctypes.byref(n), one, 8, nul), "workspace too small")
    expect(lib.g4s_visgrid_compact_emit(4, lo, hi, one, 0, -1, one, one, 1 << 20, nul), "n_points must not be negative")
    expect(lib.g4s_visgrid_compact_emit(4, lo, hi, one, 0, 5, one, one, 8, nul), "workspace too small")
    assert lib.g4s_visgrid_compact_emit(4, lo, hi, one, 0, 0, nul, nul, 0, nul) == 0  # nothing selected: nothing to do
    expect(lib.g4s_view_counts_points(5, one, 2, 0.1, -1, 0, nul, nul, nul, nul, one, nul, 0, nul), "mode must be 0 (free) or 1")
    expect(lib.g4s_view_counts_points(5, one, 1, 0.1, -2, 0, nul, nul, nul, nul, one, nul, 0, nul), "skip_view must be")
    expect(lib.g4s_view_counts_points(5, nul, 1, 0.1, -1, 0, nul, nul, nul, nul, one, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_view_counts_pixels(4, 0, one, ray, 0, 0.1, -1, 0, nul, nul, nul, nul, one, nul, 0, nul), "width, height")
    expect(lib.g4s_view_counts_pixels(4, 4, one, nul, 0, 0.1, -1, 0, nul, nul, nul, nul, one, nul, 0, nul), "NULL required")
    expect(lib.g4s_depth_to_points(4, 4, one, ray, nul, nul, 0, nul), "NULL required pointer")
    # the size queries: records of 80 bytes behind 256 of alignment slack; two u32 per word, scan chunks, totals
    assert lib.g4s_visgrid_workspace(0) == 256 and lib.g4s_visgrid_workspace(5) == 5 * 80 + 256
    assert lib.g4s_visgrid_compact_workspace(1) == 4 * 256 + 256
    assert lib.g4s_visgrid_compact_workspace(33) >= 2 * 562 * 4 + 256
