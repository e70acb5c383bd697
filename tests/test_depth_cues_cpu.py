"""The depth-cue contract without a GPU: the numpy restatement (tests/depth_cues_ref.py) against what the reference's own
functions computed (tests/golden/depth_cues.npz, written by tests/golden/make_golden_depth_cues.py), the host-side argument
checks of the new entry points, and the host table builder of g4splat_amd.depth_cues.

The yardstick of every float output is the largest |float32 run - float64 run| of the REFERENCE over the compared pixels,
recorded by the generator: the float64 restatement has to be within it of the reference's float64 results, the float32
restatement within twice it."""
import ctypes

import numpy as np
import pytest

import depth_cues_ref as dr
from support import load_depth_cues_golden

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def golden():
    return load_depth_cues_golden()


def _within(got, want, bound, keep=None):
    err = np.abs(np.asarray(got, f64) - np.asarray(want, f64))
    worst = float(err.max() if keep is None else err[keep].max())
    print(f"largest error {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound, (worst, bound)


def test_golden_covers_what_it_claims(golden):
    g = golden
    assert g.V == 5 and g.n_input == 3 and (g.H, g.W) == (48, 64)
    assert all(np.abs(a - 0.9).min() > 1e-3 for a in g.alphas)
    touched, valid = g.g["touched"], g.g["valid"]
    assert max((touched[v] & ~valid[v]).sum() / max(touched[v].sum(), 1) for v in range(g.V)) >= 0.01
    assert all(((g.masks[v] == 0) & ~g.confs[v]).any() for v in range(g.n_input, g.V))
    v, pid = (int(x) for x in g.g["dup_pair"])
    assert sum((v, pid) in pairs for pairs in g.gdict.values()) == 2
    assert sorted(set(g.gdict) - set(g.planes)) == [7] and (g.masks[4] == 977).sum() == 9
    excluded, masked = (int(x) for x in g.g["excluded"])
    assert excluded <= 0.001 * masked and excluded == int((touched & ~g.agreed).sum())


@pytest.mark.parametrize("dtype, factor", [(f64, 1.0), (f32, 2.0)])
def test_restated_cues_match_the_reference(golden, dtype, factor):
    g = golden
    cues = dr.view_geometry_cues(g.cams, g.disps, g.depths, g.alphas, g.threshold, dtype)
    _within([c["coeffs"] for c in cues], g.g["ref64_coeffs"], factor * g.yard["coeffs"])
    _within([c["aligned_depth"] for c in cues], g.g["ref64_aligned_depth"], factor * g.yard["aligned_depth"])
    _within([c["depth"] for c in cues], g.ref_merged, factor * g.yard["depth"])
    inpainted = cues[g.n_input:]
    _within([c["normal_world"] for c in inpainted], g.g["ref64_normal_world"], factor * g.yard["normal_world"])
    _within([c["normal_cam"] for c in inpainted], g.g["ref64_normal_cam"], factor * g.yard["normal_cam"])
    for v, c in enumerate(cues):
        assert np.array_equal(c["visibility"], g.visible[v]) and c["count"] == int(g.visible[v].sum())
        assert np.array_equal(c["mono_depth"], dtype(1) / g.disps[v].astype(dtype))
    # the depth-domain variant, mono depth against the rendered depth over the visible pixels
    for v in range(g.n_input, g.V):
        alpha, beta, _n = dr.align_coeffs(g.monos[v], g.depths[v], g.visible[v], dr.DEPTH, dtype)
        _within([alpha, beta], g.g["ref64_coeffs2"][v], factor * g.yard["coeffs2"])
        _within(dr.aligned(alpha, beta, g.monos[v], dr.DEPTH, dtype), g.g["ref64_align2"][v - g.n_input], factor * g.yard["align2"])


@pytest.mark.parametrize("dtype, factor", [(f64, 1.0), (f32, 2.0)])
def test_restated_plane_depths_and_refill_match_the_reference(golden, dtype, factor):
    g = golden
    for i, (key, v) in enumerate(g.g["plane_full_pairs"]):
        z, valid = dr.plane_depth_image(*g.planes[int(key)], g.cams[int(v)], g.H, g.W, dtype)
        keep = g.g["full_agreed"][i]
        assert np.array_equal(valid[keep], g.g["plane_full_valid"][i][keep])
        _within(np.where(valid, z, 0), g.g["ref64_plane_full"][i], factor * g.yard["plane_full"], keep)
    planed, replaced, zeroed, touched, valid = dr.apply_global_planes(g.cams, g.depths, g.masks, g.gdict, g.planes, dtype)
    assert np.array_equal(np.stack(touched), g.g["touched"])
    assert np.array_equal(np.stack(valid)[g.agreed], g.g["valid"][g.agreed])
    if g.agreed.all():
        assert np.array_equal(replaced, g.g["valid"].sum((1, 2))) and np.array_equal(zeroed, (g.g["touched"] & ~g.g["valid"]).sum((1, 2)))
    _within(planed, g.g["ref64_planed"], factor * g.yard["planed"], g.agreed)
    untouched = ~g.g["touched"]
    assert np.array_equal(np.stack(planed)[untouched], np.stack(g.depths).astype(dtype)[untouched])
    refined, coeffs, _t, _v = dr.refine_depths_with_planes(g.cams, g.depths, g.masks, g.confs, g.monos, g.gdict, g.planes,
                                                           g.n_input, dtype)
    _within(coeffs, g.g["ref64_refill_coeffs"], factor * g.yard["refill_coeffs"])
    _within(refined, g.g["ref64_refined"], factor * g.yard["refined"], g.agreed)
    for v in range(g.n_input):
        assert np.array_equal(refined[v], planed[v])


def test_degenerate_alignments_follow_ieee(golden):
    """n = 0, n = 1, no variance and a masked zero depth give NaN or inf, never an exception."""
    d = np.array([[0.5, 0.75, 0.75, 1.25]], f32)
    g = np.array([[2.0, 1.5, 1.25, 0.0]], f32)
    for mask in ([0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0], [1, 1, 0, 1]):
        alpha, beta, n = dr.align_coeffs(d, g, np.array([mask], bool), dr.DISPARITY, f32)
        assert n == sum(mask) and not np.isfinite(alpha) and not np.isfinite(beta)
    alpha, beta, n = dr.align_coeffs(d, g, np.array([[1, 1, 1, 0]], bool), dr.DISPARITY, f32)
    assert n == 3 and np.isfinite(alpha) and np.isfinite(beta)


# ---- the helpers and scenes of the GPU tests, pinned to the restatement above ------------------------------------------------
@pytest.mark.parametrize("dtype", [f32, f64])
def test_plane_terms_are_those_of_plane_depth_image(golden, dtype):
    g = golden
    scene = dr.clamp_scene()
    cases = [(*g.planes[int(key)], g.cams[int(v)], g.H, g.W) for key, v in g.g["plane_full_pairs"]]
    cases += [(*scene.planes[k], scene.cam, scene.H, scene.W) for k in scene.planes]
    for normal, centre, cam, H, W in cases:
        nd, num, length = dr.plane_terms(normal, centre, cam, H, W, dtype)
        assert nd.dtype == length.dtype == dtype and nd.shape == length.shape == (H, W) and np.ndim(num) == 0
        with np.errstate(all="ignore"):
            t = num / np.copysign(np.fmax(np.abs(nd), dtype(1e-8)), nd)
            z = t / length
        want_z, want_valid = dr.plane_depth_image(normal, centre, cam, H, W, dtype)
        assert np.array_equal(z, want_z) and np.array_equal(np.signbit(z), np.signbit(want_z))
        assert np.array_equal((t > 0) & (z > 0), want_valid)


def test_clamp_scene_reaches_the_clamp_in_both_signs_and_at_zero():
    s = dr.clamp_scene()
    o, R, _fx, _fy = dr.plane_camera(s.cam, s.W, s.H, f32)
    assert not o.any() and np.array_equal(R, np.eye(3, dtype=f32))  # w = (dcx, dcy, 1)
    for pid in (1, 2):
        nd, num, _len = dr.plane_terms(*s.planes[pid], s.cam, s.H, s.W, f32)
        here = s.mask == pid
        assert (np.abs(nd) < f32(1e-8)).all() and num != 0
        assert (nd[here] < 0).any() and (nd[here] == 0).any() and ((nd[here] > 0) & (nd[here] < f32(1e-8))).any()
        assert not nd[:, s.W // 2].any() and here[:, s.W // 2].any()
        _z, valid = dr.plane_depth_image(*s.planes[pid], s.cam, s.H, s.W, f32)
        assert valid[here].any() and not valid[here].all()  # the sign of nd decides
    nd, num, _len = dr.plane_terms(*s.planes[3], s.cam, s.H, s.W, f32)
    assert num == 0 and (nd > f32(1e-8)).all() and any(s.planes[3][1])  # through the camera centre, not at it
    assert not dr.plane_depth_image(*s.planes[3], s.cam, s.H, s.W, f32)[1].any() and (s.mask == 3).any()
    _d, replaced, zeroed, touched, _v = dr.apply_global_planes([s.cam], [s.depth], [s.mask], s.gdict, s.planes, f32)
    assert replaced[0] > 0 and zeroed[0] > (s.mask == 3).sum() and (s.mask == 0).any() and not touched[0][s.mask == 0].any()


def test_id_search_scene_covers_what_it_claims(golden):
    from g4splat_amd import depth_cues
    s = dr.id_search_scene()
    V = len(s.sizes)
    assert [len(ids) for ids in s.fitted] == list(dr.ID_RUNS) == [2, 0, 1, 3, 7, 64, 65]
    assert dr.fitted_ids(s.gdict, s.planes, V) == s.fitted
    assert [sorted(pairs) for pairs in dr.fitted_pairs(s.gdict, s.planes, V)] == s.fitted
    assert 99 in s.gdict and 99 not in s.planes
    # the library's table is the restatement's
    view_offset, ids, entry_plane, _rows, keys = depth_cues.plane_table(s.gdict, s.planes, V)
    assert [ids[a:b] for a, b in zip(view_offset, view_offset[1:])] == s.fitted
    pairs = dr.fitted_pairs(s.gdict, s.planes, V)
    assert [keys[k] for k in entry_plane] == [pairs[v][p] for v in range(V) for p in s.fitted[v]]
    for v, (fit, others, mask) in enumerate(zip(s.fitted, s.unfitted, s.masks)):
        assert mask.dtype == np.int32 and mask.shape == s.sizes[v]
        assert all((mask == p).any() for p in fit), v  # every entry of the run is searched for
        assert not set(fit) & set(others) and all((mask == q).any() for q in others)
        assert (mask == 0).any() and (mask < 0).any() and (mask == -2 ** 31).any()
        a, b = view_offset[v], view_offset[v + 1]  # the table's entries beside the run belong to other views
        beside = ([ids[a - 1]] if a > 0 else []) + ([ids[b]] if b < len(ids) else [])
        assert len(beside) == (2 if 0 < v < V - 1 else 1) and all(q in fit or (mask == q).any() for q in beside)
        assert v != 1 or (beside == [6, 1000] and not fit)  # without a run of its own, both neighbours' ends are in the mask
        if fit:
            assert any(q < fit[0] for q in others) or fit[0] == 1
            assert any(q > fit[-1] for q in others) or fit[-1] == dr.ID_TOP
            assert all(any(a < q < b for q in others) for a, b in zip(fit, fit[1:]) if b - a > 1)
            planes_of = [entry_plane[view_offset[v] + i] for i in range(len(fit))]
            if len(fit) >= 7:
                assert len(set(planes_of)) < len(fit) and planes_of != sorted(planes_of)  # shared, and not ascending with the id
    assert s.fitted[5][0] > 1 and s.fitted[5][-1] < dr.ID_TOP and (s.fitted[6][0], s.fitted[6][-1]) == (1, dr.ID_TOP)
    assert (5 in s.fitted[0] and 6 in s.fitted[0])  # neighbours one apart
    cams = [golden.cams[v % golden.V] for v in range(V)]
    _d, replaced, zeroed, touched, _v = dr.apply_global_planes(cams, s.depths, s.masks, s.gdict, s.planes, f32)
    assert replaced.sum() > 0 and zeroed.sum() > 0 and replaced[1] == zeroed[1] == 0 and not touched[1].any()
    assert all(replaced[v] + zeroed[v] > 0 for v in range(V) if v != 1)
    for v in range(V):
        assert np.array_equal(touched[v], np.isin(s.masks[v], s.fitted[v]))


# ---- the host table builder ------------------------------------------------------------------------------------------------
def test_plane_table_last_wins_missing_planes_and_sparse_ids():
    from g4splat_amd import depth_cues
    n, c = (0.0, 0.0, 1.0), (0.0, 0.0, 2.0)
    gdict = {5: [(0, 977), (1, 3)], 9: [(1, 40), (0, 12)], 2: [(0, 977), (2, 7)], 11: [(1, 3)]}
    planes = {5: (n, c), 2: ((1.0, 0.0, 0.0), c), 11: (np.array(n), np.array(c))}  # 9 was never fitted
    view_offset, ids, entry_plane, rows, keys = depth_cues.plane_table(gdict, planes, 4)
    assert keys == [5, 2, 11] and rows.shape == (3, 6) and rows.dtype == np.float32
    assert view_offset == [0, 1, 2, 3, 3]  # view 3 has no entry, (0, 12) and (1, 40) have no fitted plane
    assert ids == [977, 3, 7]
    assert entry_plane == [1, 2, 1]  # (0, 977): key 2 after key 5; (1, 3): key 11 after key 5
    assert np.array_equal(rows[1], np.array([1, 0, 0, 0, 0, 2], np.float32))
    # ids come out ascending per view whatever the dict's order
    view_offset, ids, _e, _r, _k = depth_cues.plane_table({0: [(0, 977), (0, 4), (0, 31)]}, {0: (n, c)}, 1)
    assert view_offset == [0, 3] and ids == [4, 31, 977]
    assert depth_cues.plane_table({}, {}, 2)[:3] == ([0, 0, 0], [], [])
    with pytest.raises(ValueError, match="names view 4"):
        depth_cues.plane_table({0: [(4, 1)]}, {0: (n, c)}, 4)
    with pytest.raises(ValueError, match="names view 1"):
        depth_cues.plane_table({3: [(1, 1)]}, {}, 1)  # checked even where the plane was not fitted
    with pytest.raises(ValueError, match="must be positive"):
        depth_cues.plane_table({0: [(0, 0)]}, {0: (n, c)}, 1)
    with pytest.raises(ValueError, match="finite"):
        depth_cues.plane_table({0: [(0, 1)]}, {0: ((0.0, float("nan"), 1.0), c)}, 1)
    with pytest.raises(ValueError, match="finite"):
        depth_cues.plane_table({0: [(0, 1)]}, {0: (n, (0.0, 1e39, 0.0))}, 1)
    with pytest.raises(ValueError, match="finite"):
        depth_cues.plane_table({0: [(0, 1)]}, {0: ((0.0, 1.0), c)}, 1)


def test_python_argument_checks_need_no_device():
    import torch
    from g4splat_amd import depth_cues
    m = torch.zeros((4, 4))
    with pytest.raises(ValueError, match="HIP device"):
        depth_cues.align_disparities([m], [m], [m.bool()])
    with pytest.raises(ValueError, match="domain"):
        depth_cues.align_disparities([m], [m], [m.bool()], domain="log")
    with pytest.raises(ValueError, match=r"\[V,H,W\]"):
        depth_cues.view_geometry_cues([None], m, m, m)
    with pytest.raises(ValueError, match="1 views but 2"):
        depth_cues.view_geometry_cues([None], [m, m], [m], [m])
    with pytest.raises(ValueError, match="0 views but 1 targets"):
        depth_cues.align_disparities([], [m], [])
    with pytest.raises(ValueError, match="1 views but 0 depths"):
        depth_cues.apply_global_planes([None], [], [], {}, {})
    with pytest.raises(ValueError, match="names view 0 but there are 0 views"):
        depth_cues.apply_global_planes([], [], [], {0: [(0, 1)]}, {})
    with pytest.raises(ValueError, match="0 views but 1 mono_depths"):
        depth_cues.refill_unseen_regions([], [m], [], [], 0)
    with pytest.raises(ValueError, match=r"n_input_views must be in 0 \.\. 0 \(got 1\)"):
        depth_cues.refill_unseen_regions([], [], [], [], 1)
    with pytest.raises(ValueError, match="1 cameras but 0 depths"):
        depth_cues.refine_depths_with_planes([None], [], [], [], [], {}, {}, 0)
    with pytest.raises(ValueError, match="must not be NaN"):
        depth_cues.view_geometry_cues([], [], [], [], float("nan"))
    with pytest.raises(ValueError, match="img_shape must be positive"):
        depth_cues.plane_aligned_depth(m[0, :3], m[0, :3], None, (0, 4))
    # without views every entry point answers with its empty result, and asks for no device
    assert depth_cues.refine_depths_with_planes([], [], [], [], [], {}, {}, 0, return_points=True) == ([], [])
    assert depth_cues.view_geometry_cues([], [], [], []).coeffs.shape == (0, 2)
    assert depth_cues.align_disparities([], [], [])[0] == [] and depth_cues.refill_unseen_regions([], [], [], [], 0)[0] == []


# ---- host-side argument validation of the library ---------------------------------------------------------------------------
def test_library_argument_validation_is_host_side(hip_lib):
    lib = hip_lib
    nul, one, big = ctypes.c_void_p(0), ctypes.c_void_p(256), 1 << 20
    sizes = (ctypes.c_int * 4)(64, 48, 3, 3)
    maps = (ctypes.c_void_p * 2)(256, 512)
    hole = (ctypes.c_void_p * 2)(256, 0)

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    # size queries are pure host code
    assert lib.g4s_depth_align_workspace(2, sizes) >= 2 * 5 * 8 and lib.g4s_depth_align_workspace(0, nul) > 0
    assert lib.g4s_depth_align_workspace(-1, sizes) == 0 and lib.g4s_depth_align_workspace(2, nul) == 0
    assert lib.g4s_depth_align_workspace(1, (ctypes.c_int * 2)(0, 4)) == 0
    assert lib.g4s_depth_align_workspace(1, (ctypes.c_int * 2)(1 << 16, 1 << 15)) == 0
    grow = lib.g4s_depth_align_workspace(1, (ctypes.c_int * 2)(4097, 1)) - lib.g4s_depth_align_workspace(1, (ctypes.c_int * 2)(4096, 1))
    assert grow in (0, 256)  # one more span: 40 bytes, rounded
    for query in (lib.g4s_depth_align_apply_workspace, lib.g4s_depth_cue_maps_workspace, lib.g4s_depth_refill_workspace):
        assert query(3) > query(0) > 0 and query(-1) == 0 and query(65536) == 0
    assert lib.g4s_plane_depths_workspace(2, 10, 3) > lib.g4s_plane_depths_workspace(2, 0, 0) > 0
    assert lib.g4s_plane_depths_workspace(2, -1, 3) == 0 and lib.g4s_plane_depths_workspace(2, 1, -3) == 0

    # alignment sums
    align = lambda **k: lib.g4s_depth_align(*[k.get(n, d) for n, d in (  # noqa: E731
        ("domain", 0), ("is_map", 0), ("threshold", 0.0), ("n", 2), ("sizes", sizes), ("source", maps), ("target", maps),
        ("masks", maps), ("coeffs", one), ("counts", one), ("ws", one), ("bytes", big), ("stream", nul))])
    expect(align(domain=3), "domain must be")
    expect(align(is_map=1, threshold=float("nan")), "must not be NaN")
    expect(align(n=-1), "n_views must be in 0 .. 65535")
    expect(align(n=65536), "n_views must be in 0 .. 65535")
    expect(align(sizes=nul), "NULL required pointer")
    expect(align(sizes=(ctypes.c_int * 4)(64, 48, 0, 3)), "width, height must be positive")
    expect(align(sizes=(ctypes.c_int * 4)(64, 48, 1 << 15, (1 << 15) + 1)), "sizes: width, height must be positive and width * height")
    expect(align(n=65536, sizes=nul), "n_views must be in 0 .. 65535")  # the first of two bad arguments
    expect(align(sizes=(ctypes.c_int * 4)(64, 48, 0, 3), source=nul), "sizes: width, height must be positive")
    expect(align(source=nul), "source: NULL array")
    expect(align(target=hole), "target[1]: NULL pointer")
    expect(align(masks=hole), "masks[1]: NULL pointer")
    expect(align(coeffs=nul), "NULL required pointer")
    expect(align(counts=nul), "NULL required pointer")
    expect(align(bytes=64), "workspace too small")
    expect(align(bytes=lib.g4s_depth_align_workspace(2, sizes) - 1), "workspace too small")
    expect(align(ws=nul), "workspace too small")
    assert align(n=0, sizes=nul, source=nul, target=nul, masks=nul, coeffs=nul, counts=nul, ws=nul, bytes=0) == 0

    apply = lambda **k: lib.g4s_depth_align_apply(*[k.get(n, d) for n, d in (  # noqa: E731
        ("domain", 1), ("n", 2), ("sizes", sizes), ("source", maps), ("coeffs", one), ("aligned", maps), ("ws", one),
        ("bytes", big), ("stream", nul))])
    expect(apply(domain=-1), "domain must be")
    expect(apply(n=65536), "n_views must be in 0 .. 65535")
    expect(apply(sizes=(ctypes.c_int * 4)(64, 48, 3, 0)), "sizes: width, height must be positive")
    expect(apply(aligned=hole), "aligned[1]: NULL pointer")
    expect(apply(coeffs=nul), "NULL required pointer")
    expect(apply(bytes=8), "workspace too small")
    assert apply(n=0) == 0

    mats = (ctypes.c_float * 32)()
    rays = (ctypes.c_float * 24)()
    cue_defaults = [("n", 2), ("world_view", mats), ("rays", rays), ("sizes", sizes), ("disparity", maps), ("warp", maps),
                    ("alpha", maps), ("threshold", 0.9), ("coeffs", one), ("visibility", maps), ("mono", maps), ("aligned", maps),
                    ("merged", maps), ("normal_world", maps), ("normal_cam", maps), ("ws", one), ("bytes", big), ("stream", nul)]
    cue = lambda **k: lib.g4s_depth_cue_maps(*[k.get(n, d) for n, d in cue_defaults])  # noqa: E731
    expect(cue(threshold=float("nan")), "must not be NaN")
    expect(cue(n=-1), "n_views must be in 0 .. 65535")
    expect(cue(sizes=nul), "NULL required pointer")
    expect(cue(rays=nul), "NULL required pointer")
    expect(cue(world_view=nul), "NULL required pointer")
    expect(cue(coeffs=nul), "NULL required pointer")
    for name in ("disparity", "warp", "alpha", "visibility", "mono", "aligned", "merged", "normal_world", "normal_cam"):
        expect(cue(**{name: hole}), "[1]: NULL pointer")
    expect(cue(bytes=8), "workspace too small")
    assert cue(n=0) == 0

    cameras = (ctypes.c_float * 28)(*([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 60, 60] * 2))
    offsets = (ctypes.c_int * 3)(0, 2, 3)
    ids = (ctypes.c_int * 3)(4, 977, 12)
    entry = (ctypes.c_int * 3)(0, 1, 1)
    rows = (ctypes.c_float * 12)(0, 0, 1, 0, 0, 2, 1, 0, 0, 3, 0, 0)
    plane_defaults = [("n", 2), ("cameras", cameras), ("sizes", sizes), ("depth", maps), ("out", maps), ("masks", maps),
                      ("view_offset", offsets), ("ids", ids), ("entry_plane", entry), ("n_planes", 2), ("planes", rows),
                      ("counts", one), ("ws", one), ("bytes", big), ("stream", nul)]
    plane = lambda **k: lib.g4s_plane_depths(*[k.get(n, d) for n, d in plane_defaults])  # noqa: E731
    expect(plane(n_planes=-1), "n_planes must not be negative")
    expect(plane(n=65536), "n_views must be in 0 .. 65535")
    expect(plane(n_planes=-1, sizes=(ctypes.c_int * 4)(64, 48, 0, 3)), "sizes: width, height must be positive")
    expect(plane(bytes=lib.g4s_plane_depths_workspace(2, 3, 2) - 1), "workspace too small")
    expect(plane(cameras=nul), "NULL required pointer")
    expect(plane(counts=nul), "NULL required pointer")
    expect(plane(out=hole), "depth_out[1]: NULL pointer")
    expect(plane(masks=nul), "masks: NULL array")
    bad = (ctypes.c_float * 28)(*cameras)
    bad[17] = float("inf")
    expect(plane(cameras=bad), "cameras: view 1 is not finite")
    bad = (ctypes.c_float * 28)(*cameras)
    bad[12] = 0.0
    expect(plane(cameras=bad), "view 0: the focal lengths must be positive")
    expect(plane(view_offset=nul), "view_offset: NULL array")
    expect(plane(view_offset=(ctypes.c_int * 3)(1, 2, 3)), "view_offset[0] must be 0")
    expect(plane(view_offset=(ctypes.c_int * 3)(0, 2, 1)), "view_offset[2] must not decrease")
    expect(plane(ids=nul), "ids, entry_plane: NULL array")
    expect(plane(ids=(ctypes.c_int * 3)(977, 4, 12)), "strictly ascending")
    expect(plane(ids=(ctypes.c_int * 3)(4, 4, 12)), "strictly ascending")
    expect(plane(ids=(ctypes.c_int * 3)(0, 4, 12)), "must be positive")
    expect(plane(entry_plane=(ctypes.c_int * 3)(0, 2, 1)), "entry_plane[1] must be a plane below n_planes")
    expect(plane(entry_plane=(ctypes.c_int * 3)(0, 1, -1)), "entry_plane[2] must be a plane below n_planes")
    expect(plane(planes=nul), "planes: NULL array")
    bad = (ctypes.c_float * 12)(*rows)
    bad[7] = float("nan")
    expect(plane(planes=bad), "planes: plane 1 is not finite")
    expect(plane(bytes=8), "workspace too small")
    assert plane(n=0) == 0

    refill_defaults = [("n", 2), ("n_input", 1), ("sizes", sizes), ("depth", maps), ("mono", maps), ("masks", maps),
                       ("conf", maps), ("coeffs", one), ("ws", one), ("bytes", big), ("stream", nul)]
    refill = lambda **k: lib.g4s_depth_refill(*[k.get(n, d) for n, d in refill_defaults])  # noqa: E731
    expect(refill(n=65536), "n_views must be in 0 .. 65535")
    expect(refill(sizes=nul), "NULL required pointer")
    expect(refill(n_input=3), "n_input_views must be in 0 .. n_views")
    expect(refill(n_input=-1), "n_input_views must be in 0 .. n_views")
    expect(refill(mono=hole), "mono_depth[1]: NULL pointer")
    expect(refill(conf=nul), "conf: NULL array")
    expect(refill(coeffs=nul), "NULL required pointer")
    expect(refill(bytes=8), "workspace too small")
    assert refill(n_input=2) == 0  # no inpainted view: nothing is launched
    assert refill(n=0, n_input=0) == 0
