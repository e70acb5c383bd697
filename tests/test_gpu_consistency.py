"""Cross-view consistency on the MI355X (g4splat_amd.consistency, csrc/tsdf/consistency.hip) against the numpy restatement
of the contract (tests/consistency_ref.py): confident maps, images, point states, counts and anchors are compared exactly.
The restatement itself is pinned to what the reference's scripts wrote in tests/test_consistency_cpu.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import consistency_ref as cr
from g4splat_amd import consistency
from support import DEV, dev, devs, hosts, load_consistency_golden, pinhole_camera, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32


def _solve_points(cams, depths, images, points, n_input, threshold):
    """The library's (images_out, confident maps) as numpy, with the inputs checked to be untouched."""
    args = (devs(depths), devs(images), dev(np.asarray(points, f32).reshape(-1, 3)))
    before = [[t.clone() for t in args[0]], [t.clone() for t in args[1]], args[2].clone()]
    outs, confs = consistency.solve_point_inconsistency(cams, *args, n_input, threshold)
    assert all(o.dtype == torch.float32 and o.device == DEV for o in outs) and all(c.dtype == torch.uint8 for c in confs)
    same_bits(args[0] + args[1] + [args[2]], before[0] + before[1] + [before[2]], "inputs")  # NaN coordinates included
    return hosts(outs), hosts(confs)


def _check_points(cams, depths, images, points, n_input, threshold):
    """Both outputs and the point states of a scene equal the restatement's; returns the restatement's."""
    outs, confs = _solve_points(cams, depths, images, points, n_input, threshold)
    want_outs, want_confs = cr.point_solver(cams, depths, images, points, n_input, threshold)
    same_bits(outs, want_outs)
    same_bits(confs, want_confs)
    got = consistency.point_states(cams, devs(depths), devs(images), dev(np.asarray(points, f32).reshape(-1, 3)), n_input,
                                   threshold)
    want = cr.point_states(cams, depths, images, points, n_input, threshold)
    assert got[0].dtype == torch.bool and got[1].dtype == torch.bool and got[2].dtype == torch.uint8
    same_bits(hosts(got), list(want))
    return want_outs, want_confs, want


@pytest.fixture(scope="module")
def golden():
    return load_consistency_golden()


@pytest.fixture(scope="module")
def restated(golden):
    """The restatement's float32 outputs of the golden scene, computed once and left unchanged."""
    g = golden
    outs, confs = cr.point_solver(g.cams, g.depths, g.float_images, g.points, g.n_input, g.threshold)
    states = cr.point_states(g.cams, g.depths, g.float_images, g.points, g.n_input, g.threshold)
    b_outs, anchor_of_plane, counts = cr.plane_solver(g.cams, g.depths, g.images, g.masks, g.clouds, g.gdict, g.anchors,
                                                      g.threshold)
    return SimpleNamespace(outs=outs, confs=confs, states=states, b_outs=b_outs, anchor_of_plane=anchor_of_plane, counts=counts)


# ---- golden scene ---------------------------------------------------------------------------------------------------------
def test_point_solver_on_the_golden_scene(hip_lib, golden, restated):
    g, I = golden, golden.n_input
    outs, confs = _solve_points(g.cams, g.depths, g.float_images, g.points, I, g.threshold)
    same_bits(outs, restated.outs)
    same_bits(confs, restated.confs)
    # what the reference's script wrote, on the agreed set
    conf = np.stack(confs) * 255
    assert np.array_equal(conf[g.point_conf_agreed], g.point_conf[g.point_conf_agreed])
    png = np.stack(hosts([consistency.images_to_uint8(dev(o)) for o in outs[I:]]))
    assert np.array_equal(png[g.point_png_agreed], g.point_png[g.point_png_agreed])
    assert sum(int((c == 0).sum()) for c in confs) > 900 and sum(int((a != b).any(-1).sum()) for a, b in zip(outs, g.float_images)) > 1000
    # a second run is bit-identical, and so is one over [3,H,W] images (a camera's original_image)
    again = _solve_points(g.cams, g.depths, g.float_images, g.points, I, g.threshold)
    same_bits(again[0], outs)
    same_bits(again[1], confs)
    chw = _solve_points(g.cams, g.depths, [np.ascontiguousarray(im.transpose(2, 0, 1)) for im in g.float_images], g.points, I,
                        g.threshold)
    same_bits(chw[0], outs)
    same_bits(chw[1], confs)


def test_point_states_on_the_golden_scene(hip_lib, golden, restated):
    g = golden
    args = (g.cams, devs(g.depths), devs(g.float_images), dev(g.points), g.n_input, g.threshold)
    got = consistency.point_states(*args)
    same_bits(hosts(got), list(restated.states))
    seen, visible, colours = restated.states
    assert (~seen).sum() == 11454 and visible.all()  # every point lies on its own view's surface
    assert not colours[seen | ~visible].any()
    again = consistency.point_states(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def _solve_planes(cams, depths, images, masks, points, gdict, anchors, threshold):
    args = (devs(depths), devs(images), devs(masks), devs(points))
    before = [[t.clone() for t in a] for a in args]
    outs, anchor_of_plane, counts = consistency.solve_plane_inconsistency(cams, *args, gdict, anchors, threshold)
    assert all(o.dtype == torch.uint8 and o.device == DEV for o in outs) and counts.dtype == torch.int64
    for a, b in zip(args, before):  # the inputs are only read
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    return hosts(outs), anchor_of_plane, counts.numpy()


def _check_planes(cams, depths, images, masks, points, gdict, anchors, threshold, resolve=None):
    outs, anchor_of_plane, counts = _solve_planes(cams, depths, images, masks, points, gdict, anchors, threshold)
    want_outs, want_anchor, want_counts = cr.plane_solver(cams, depths, images, masks, points, gdict, anchors, threshold,
                                                          resolve=resolve)
    assert counts.shape == want_counts.shape and np.array_equal(counts, want_counts)
    assert anchor_of_plane == want_anchor and list(anchor_of_plane) == list(want_anchor)
    same_bits(outs, want_outs)
    return outs, anchor_of_plane, counts


def test_plane_solver_on_the_golden_scene(hip_lib, golden, restated):
    g = golden
    scene = (g.cams, g.depths, g.images, g.masks, g.clouds, g.gdict, g.anchors, g.threshold)
    outs, anchor_of_plane, counts = _solve_planes(*scene)
    same_bits(outs, restated.b_outs)
    assert np.array_equal(counts, restated.counts) and counts.tolist() == g.stats["counts"]
    assert anchor_of_plane == restated.anchor_of_plane and [anchor_of_plane[k] for k in g.gdict] == g.stats["anchors"]
    png = np.stack(outs[g.n_input:])
    assert np.array_equal(png[g.plane_png_agreed], g.plane_png[g.plane_png_agreed])
    assert sum(int((a != b).any(-1).sum()) for a, b in zip(outs, g.images)) > 1500
    again = _solve_planes(*scene)
    same_bits(again[0], outs)
    assert again[1] == anchor_of_plane and np.array_equal(again[2], counts)
    # int64 masks with the same ids, and points as [H,W,3]
    wide = _solve_planes(g.cams, g.depths, g.images, [m.astype(np.int64) for m in g.masks],
                         [c.reshape(m.shape + (3,)) for c, m in zip(g.clouds, g.masks)], g.gdict, g.anchors, g.threshold)
    same_bits(wide[0], outs)


# ---- edge scene -----------------------------------------------------------------------------------------------------------
EW, EH, EF, ETHRESH = 16, 8, 8.0, 0.25
FAR = 5.0  # a depth no point of the edge scene is near


def _at(u, v, z=1.0):
    """The point that an identity camera with W = 16, H = 8, fx = fy = 8 sees at (u, v) in depth z; exact for dyadic values."""
    return ((u - EW / 2) / EF * z, (v - EH / 2) / EF * z, z)


def _edge_scene():
    """(cams, depths, images, points, {name: index}): view 0 is the input view, view 1 the inpainted one, both identity
    cameras; a point at depth 1 passes where the view's depth map holds 1 and fails where it holds FAR."""
    rng = np.random.default_rng(11)
    images = [rng.random((EH, EW, 3)).astype(f32) for _ in range(2)]
    d_in, d_out = np.ones((EH, EW), f32), np.ones((EH, EW), f32)
    # |z - d| / (z + 1e-6) = 0.25 exactly: z = 1, z + 1e-6 = 1 + 2^-20 in float32, z - d = 0.25 + 2^-22
    at = f32(0.75) - f32(2.0 ** -22)
    assert (f32(1) - at) / (f32(1) + f32(1e-6)) == f32(0.25)
    specs, names = [], {}

    def add(name, p, depth_in=None, depth_out=None, pixel=None):
        names[name] = len(specs)
        specs.append(p)
        if pixel is not None:
            x, y = pixel
            d_in[y, x] = FAR if depth_in is None else depth_in
            d_out[y, x] = FAR if depth_out is None else depth_out

    # the threshold in the inpainted view (unseen points: they repaint), then in the input view (seen points: conf)
    add("at_threshold", _at(1.5, 1.5), depth_out=at, pixel=(1, 1))
    add("inside_by_an_ulp", _at(2.5, 1.5), depth_out=np.nextafter(at, f32(1)), pixel=(2, 1))
    add("outside_by_an_ulp", _at(3.5, 1.5), depth_out=np.nextafter(at, f32(0)), pixel=(3, 1))
    add("seen_at_threshold", _at(1.5, 2.5), depth_in=at, depth_out=1.0, pixel=(1, 2))
    add("seen_inside_by_an_ulp", _at(2.5, 2.5), depth_in=np.nextafter(at, f32(1)), depth_out=1.0, pixel=(2, 2))
    add("seen_outside_by_an_ulp", _at(3.5, 2.5), depth_in=np.nextafter(at, f32(0)), depth_out=1.0, pixel=(3, 2))
    add("z_zero", (0.0, 0.0, 0.0))
    add("z_negative", (0.0, 0.0, -1.0))
    add("nan_x", (np.nan, 0.0, 1.0))
    add("nan_y", (0.0, np.nan, 1.0))
    add("nan_z", (0.0, 0.0, np.nan))
    add("u_is_W", _at(16.0, 4.5))
    add("v_is_H", _at(5.5, 8.0))
    add("u_below_W", (float(f32(1) - f32(2.0 ** -23)), _at(0, 5.5)[1], 1.0), depth_out=1.0, pixel=(15, 5))  # u = 16 - 2^-20
    add("u_is_0", _at(0.0, 6.5), depth_out=1.0, pixel=(0, 6))
    add("u_on_an_integer", _at(7.0, 6.5), depth_out=1.0, pixel=(7, 6))  # int(7.0) = 7: column 7, not 6
    add("only_input", _at(10.5, 1.5), depth_in=1.0, pixel=(10, 1))
    add("only_inpainted", _at(11.5, 1.5), depth_out=1.0, pixel=(11, 1))
    add("nowhere", _at(12.5, 1.5), pixel=(12, 1))
    add("both", _at(13.5, 1.5), depth_in=1.0, depth_out=1.0, pixel=(13, 1))
    cams = [pinhole_camera(EW, EH, EF, EF), pinhole_camera(EW, EH, EF, EF)]
    return cams, [d_in, d_out], images, np.asarray(specs, np.float64).astype(f32), names


def test_point_solver_on_the_edge_scene(hip_lib):
    cams, depths, images, points, names = _edge_scene()
    outs, confs, (seen, visible, colours) = _check_points(cams, depths, images, points, 1, ETHRESH)
    changed = (outs[1] != images[1]).any(-1)

    def painted(name, x, y):
        """the point repaints pixel (x, y) of the inpainted view with its own colour there"""
        i = names[name]
        assert visible[i] and not seen[i] and changed[y, x], name
        assert np.array_equal(colours[i], cr.images_to_uint8(images[1][y, x])), name
        assert np.array_equal(outs[1][y, x], colours[i].astype(f32) / f32(255)), name

    def nowhere(name, pixels=()):
        i = names[name]
        assert not visible[i] and not seen[i] and not colours[i].any(), name
        assert all(not changed[y, x] and confs[1][y, x] == 1 for x, y in pixels), name

    nowhere("at_threshold", [(1, 1)])  # 0.25 is not below 0.25
    painted("inside_by_an_ulp", 2, 1)
    nowhere("outside_by_an_ulp", [(3, 1)])
    assert not seen[names["seen_at_threshold"]] and confs[1][2, 1] == 1 and changed[2, 1]  # unseen after all: it repaints
    assert seen[names["seen_inside_by_an_ulp"]] and confs[1][2, 2] == 0 and not changed[2, 2]
    assert not seen[names["seen_outside_by_an_ulp"]] and confs[1][2, 3] == 1 and changed[2, 3]
    for name in ("z_zero", "z_negative", "nan_x", "nan_y", "nan_z", "u_is_W", "v_is_H", "nowhere"):
        nowhere(name)
    painted("u_below_W", 15, 5)
    painted("u_is_0", 0, 6)
    painted("u_on_an_integer", 7, 6)
    i = names["only_input"]
    assert seen[i] and visible[i] and confs[1][1, 10] == 1 and not changed[1, 10]  # the inpainted view does not see it
    painted("only_inpainted", 11, 1)
    i = names["both"]
    assert seen[i] and confs[1][1, 13] == 0 and not changed[1, 13] and not colours[i].any()
    assert (confs[0] == 1).all() and np.array_equal(outs[0], images[0])
    assert int((confs[1] == 0).sum()) == 2 and int(changed.sum()) == 7


# ---- the winner of a pixel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 4099])
def test_largest_index_wins_across_waves_and_workgroups(hip_lib, n):
    """Points 0, 63, 64, 4098 (= N - 1) are unseen, each first visible in a 16 x 8 view of its own -- so each has another colour --
    and all of them hit the only pixel of the last view, a 1 x 1 image; so does a point that the input view sees."""
    hitters = [i for i in (0, 63, 64, 4098) if i < n]
    seen_point = 1 if n > 1 else None
    points = np.tile(np.array([[50.0, 50.0, -1.0]], f32), (n, 1))  # everything else is behind every camera
    rng = np.random.default_rng(n)
    cams = [pinhole_camera(EW, EH, EF, EF)]
    depths, images = [np.full((EH, EW), FAR, f32)], [rng.random((EH, EW, 3)).astype(f32)]
    if seen_point is not None:
        points[seen_point] = _at(3.5, 6.5)
        depths[0][6, 3] = 1.0
    for k, i in enumerate(hitters):
        points[i] = _at(2.5 + 3 * k, 1.5 + k)
        d = np.full((EH, EW), FAR, f32)
        d[1 + k, 2 + 3 * k] = 1.0
        cams.append(pinhole_camera(EW, EH, EF, EF))
        depths.append(d)
        images.append(rng.random((EH, EW, 3)).astype(f32))
    cams.append(pinhole_camera(1, 1, 0.5, 0.5))  # u = x / 2 + 0.5 in [0, 1) for every point above
    depths.append(np.ones((1, 1), f32))
    images.append(rng.random((1, 1, 3)).astype(f32))
    outs, confs, (seen, visible, colours) = _check_points(cams, depths, images, points, 1, ETHRESH)
    last = len(cams) - 1
    assert not seen[hitters].any() and visible[hitters].all() and int(visible.sum()) == len(hitters) + (seen_point is not None)
    assert len({tuple(colours[i]) for i in hitters}) == len(hitters)  # different colours: the order matters
    for k, i in enumerate(hitters):
        assert np.array_equal(colours[i], cr.images_to_uint8(images[1 + k][1 + k, 2 + 3 * k]))
    assert np.array_equal(outs[last][0, 0], colours[hitters[-1]].astype(f32) / f32(255))
    assert confs[last][0, 0] == (0 if seen_point is not None else 1)  # a seen point on the same pixel still zeroes conf
    assert all((c == 1).all() for c in confs[:last])


# ---- degenerate inputs ---------------------------------------------------------------------------------------------------------
def test_no_points_and_no_inpainted_views(hip_lib, golden):
    g = golden
    scene = (g.cams[:3], g.depths[:3], g.float_images[:3])
    for points, n_input in ((np.zeros((0, 3), f32), 1), (g.points, 3), (np.zeros((0, 3), f32), 3), (np.zeros((0, 3), f32), 0)):
        outs, confs, states = _check_points(*scene, points, n_input, g.threshold)
        same_bits(outs, scene[2])  # nothing but the fills
        assert all((c == 1).all() for c in confs) and len(states[0]) == len(points)
    outs, confs = consistency.solve_point_inconsistency([], [], [], dev(g.points), 0)
    assert outs == [] and confs == []
    seen, visible, colours = consistency.point_states([], [], [], dev(g.points), 0)
    assert seen.shape == (len(g.points),) and not seen.any() and not visible.any() and tuple(colours.shape) == (len(g.points), 3)


def test_no_input_views(hip_lib, golden):
    """I = 0: no point is seen, every visible point repaints and every confident map stays 1."""
    g = golden
    outs, confs, (seen, visible, _colours) = _check_points(g.cams, g.depths, g.float_images, g.points, 0, g.threshold)
    assert not seen.any() and visible.sum() > 10000 and all((c == 1).all() for c in confs)
    # a point of view 0's own surface takes view 0's colour: float32 u8 / 255 survives the round trip, so view 0 keeps its image
    assert np.array_equal(outs[0], g.float_images[0]) and all((o != im).any() for o, im in zip(outs[2:], g.float_images[2:]))


@pytest.mark.parametrize("n_input", [1, 3])
def test_chunked_view_list_equals_the_single_call(hip_lib, golden, restated, monkeypatch, n_input):
    """Two views per call: the input views in chunks of their own first, then the inpainted views, the state carried along."""
    g = golden
    whole = _solve_points(g.cams, g.depths, g.float_images, g.points, n_input, g.threshold)
    states = consistency.point_states(g.cams, devs(g.depths), devs(g.float_images), dev(g.points), n_input, g.threshold)
    monkeypatch.setattr(consistency, "MAX_VIEWS_PER_CALL", 2)
    assert consistency._view_chunks(5, n_input) == {1: [(0, 1, 1), (1, 3, 0), (3, 5, 0)], 3: [(0, 2, 2), (2, 3, 1), (3, 5, 0)]}[n_input]
    chunked = _solve_points(g.cams, g.depths, g.float_images, g.points, n_input, g.threshold)
    same_bits(chunked[0], whole[0])
    same_bits(chunked[1], whole[1])
    chunked_states = consistency.point_states(g.cams, devs(g.depths), devs(g.float_images), dev(g.points), n_input, g.threshold)
    assert all(torch.equal(a, b) for a, b in zip(states, chunked_states))
    if n_input == g.n_input:
        same_bits(whole[0], restated.outs)
    else:
        same_bits(whole[0], cr.point_solver(g.cams, g.depths, g.float_images, g.points, n_input, g.threshold)[0])


def test_views_of_different_sizes(hip_lib):
    """A 16 x 8 input view, a 5 x 3 and a 16 x 8 inpainted view over one cloud of 300 points; the small view is offset."""
    rng = np.random.default_rng(5)
    cams = [pinhole_camera(EW, EH, EF, EF), pinhole_camera(5, 3, 2.0, 2.0, (0.1, -0.2, 0.3)), pinhole_camera(EW, EH, EF, EF, (0.25, 0.0, 0.0))]
    sizes = [(EH, EW), (3, 5), (EH, EW)]
    depths = [np.where(rng.random(s) < 0.5, 1.0, 1.25).astype(f32) for s in sizes]
    images = [rng.random(s + (3,)).astype(f32) for s in sizes]
    z = rng.choice([1.0, 1.25, 0.75], 300)
    points = np.stack([rng.uniform(-1.2, 1.2, 300) * z, rng.uniform(-0.6, 0.6, 300) * z, z], 1).astype(f32)
    outs, confs, (seen, visible, _c) = _check_points(cams, depths, images, points, 1, 0.1)
    assert 20 < seen.sum() < 280 and (visible & ~seen).sum() > 20
    assert all((o != im).any() for o, im in zip(outs[1:], images[1:])) and all((c == 0).any() for c in confs[1:])


# ---- plane solver ----------------------------------------------------------------------------------------------------------
def _grid_points(z, shift=0):
    """[H*W,3]: the point of every pixel of the 16 x 8 identity view at depth z, moved `shift` pixels to the right."""
    y, x = np.meshgrid(np.arange(EH), np.arange(EW), indexing="ij")
    return np.asarray([_at(u + 0.5 + shift, v + 0.5, z) for u, v in zip(x.reshape(-1), y.reshape(-1))], np.float64).astype(f32)


def _chain_scene():
    """Three identity 16 x 8 views.  View 0 holds depth 2, view 1 depth 4, view 2 depth 1; the points of view 0's plane lie at
    depth 1, view 1's at 2, view 2's at 4, each one pixel to the right of its own pixel.  So plane 0 = [(0, 30)] is anchored in
    view 2, plane 1 = [(1, -7)] in view 0, plane 2 = [(2, 30)] in view 1: a pixel of view 2 reads view 1 (step 2), which read view
    0 (step 1), which read view 2's ORIGINAL (step 0).  Plane 3 = [(1, 900)] lies at depth 100: no anchor sees it."""
    rng = np.random.default_rng(21)
    cams = [pinhole_camera(EW, EH, EF, EF) for _ in range(3)]
    depths = [np.full((EH, EW), d, f32) for d in (2.0, 4.0, 1.0)]
    images = [rng.integers(0, 256, (EH, EW, 3)).astype(np.uint8) for _ in range(3)]
    masks = [np.full((EH, EW), 30, np.int32), np.full((EH, EW), -7, np.int32), np.full((EH, EW), 30, np.int32)]
    masks[0][:, :3] = 0  # no plane
    masks[0][7, :] = 55  # an id the dict does not name
    masks[1][0, :] = 900
    masks[2][5:, 8:] = 0
    points = [_grid_points(1.0, 1), _grid_points(2.0, 1), _grid_points(4.0, 1)]
    points[1].reshape(EH, EW, 3)[0] = _grid_points(100.0).reshape(EH, EW, 3)[0]
    gdict = {0: [(0, 30)], 1: [(1, -7)], 2: [(2, 30)], 3: [(1, 900)], 4: [(0, 77)]}  # (0, 77): an id the mask does not hold
    return cams, depths, images, masks, points, gdict


def test_hand_made_chain_of_three_views(hip_lib):
    cams, depths, images, masks, points, gdict = _chain_scene()
    outs, anchor_of_plane, counts = _check_planes(cams, depths, images, masks, points, gdict, [0, 1, 2], ETHRESH)
    assert anchor_of_plane == {0: 2, 1: 0, 2: 1, 3: -1, 4: -1}
    assert counts[3].tolist() == [0, 0, 0] and counts[4].tolist() == [0, 0, 0] and counts[0, 2] > 0 and counts[0, :2].tolist() == [0, 0]
    steps = consistency.plane_steps(gdict, anchor_of_plane)
    assert steps == [(0, 30, 2), (1, -7, 0), (2, 30, 1)]
    src = cr.plane_sources(cams, depths, masks, points, steps, ETHRESH)
    lengths = [np.zeros(EH * EW, np.int64) for _ in range(3)]
    same_bits(cr.resolve_chains(images, src, lengths), outs)
    same_bits(cr.repaint_in_place(images, src, len(steps)), outs)  # the literal sequential repaint
    assert (lengths[2] == 3).sum() > 30 and (lengths[1] == 2).sum() > 30
    # (y, x) of view 2 <- (y, x + 1) of view 1 <- (y, x + 2) of view 0 <- (y, x + 3) of view 2, untouched by the earlier steps
    assert lengths[2][2 * EW + 4] == 3 and np.array_equal(outs[2][2, 4], images[2][2, 7])
    assert np.array_equal(outs[1][0], images[1][0])  # the plane without an anchor
    assert np.array_equal(outs[0][7], images[0][7]) and np.array_equal(outs[0][:, :3], images[0][:, :3])
    assert np.array_equal(outs[2][5:, 8:], images[2][5:, 8:])
    # an anchor list that leaves plane 0 without an anchor: view 0 keeps its image, chains through it end there
    outs2, anchors2, _counts = _check_planes(cams, depths, images, masks, points, gdict, [0, 1], ETHRESH)
    assert anchors2 == {0: -1, 1: 0, 2: 1, 3: -1, 4: -1} and np.array_equal(outs2[0], images[0])
    assert np.array_equal(outs2[2][2, 4], images[0][2, 6])


def test_read_inside_a_step_sees_the_colours_before_the_step(hip_lib):
    """One view anchored in itself, its points one pixel to the right: pixel x reads pixel x + 1, which the same step repaints.
    It must get the neighbour's ORIGINAL colour."""
    rng = np.random.default_rng(3)
    cams, depths = [pinhole_camera(EW, EH, EF, EF)], [np.ones((EH, EW), f32)]
    images = [rng.integers(0, 256, (EH, EW, 3)).astype(np.uint8)]
    masks, points = [np.full((EH, EW), 4, np.int64)], [_grid_points(1.0, 1)]
    outs, anchor_of_plane, counts = _check_planes(cams, depths, images, masks, points, {0: [(0, 4)]}, [0], ETHRESH)
    assert anchor_of_plane == {0: 0} and counts.tolist() == [[EH * (EW - 1)]]
    assert np.array_equal(outs[0][:, :-1], images[0][:, 1:]) and np.array_equal(outs[0][:, -1], images[0][:, -1])


def test_empty_dict_and_no_anchors(hip_lib):
    cams, depths, images, masks, points, gdict = _chain_scene()
    outs, anchor_of_plane, counts = _check_planes(cams, depths, images, masks, points, {}, [0, 1, 2], ETHRESH)
    assert anchor_of_plane == {} and tuple(counts.shape) == (0, 3)
    same_bits(outs, images)
    outs, anchor_of_plane, counts = _check_planes(cams, depths, images, masks, points, gdict, [], ETHRESH)
    assert set(anchor_of_plane.values()) == {-1} and tuple(counts.shape) == (5, 0)
    same_bits(outs, images)
    outs, anchor_of_plane, counts = consistency.solve_plane_inconsistency([], [], [], [], [], {0: []}, [])
    assert outs == [] and anchor_of_plane == {0: -1} and tuple(counts.shape) == (1, 0)


def test_plane_views_of_different_sizes(hip_lib):
    """A 16 x 8 view of depth 1 and a 5 x 3 view of depth 2; the small view's points lie at depth 1, so its plane is anchored in
    the large view (step 0), and the large view's at depth 2, so its plane is anchored in the small one (step 1)."""
    rng = np.random.default_rng(9)
    cams = [pinhole_camera(EW, EH, EF, EF), pinhole_camera(5, 3, 2.0, 2.0)]
    depths = [np.ones((EH, EW), f32), np.full((3, 5), 2.0, f32)]
    images = [rng.integers(0, 256, (EH, EW, 3)).astype(np.uint8), rng.integers(0, 256, (3, 5, 3)).astype(np.uint8)]
    masks = [rng.choice([0, 3, 8], (EH, EW)).astype(np.int32), rng.choice([0, 3], (3, 5)).astype(np.int32)]
    y, x = np.meshgrid(np.arange(3), np.arange(5), indexing="ij")
    small = np.stack([(x.reshape(-1) + 0.5 - 2.5) / 2.0, (y.reshape(-1) + 0.5 - 1.5) / 2.0, np.ones(15)], 1).astype(f32)
    gdict = {5: [(1, 3)], 2: [(0, 3), (0, 8)]}
    outs, anchor_of_plane, _counts = _check_planes(cams, depths, images, masks, [_grid_points(2.0), small], gdict, [0, 1], ETHRESH)
    assert anchor_of_plane == {5: 0, 2: 1} and (outs[1] != images[1]).any() and (outs[0] != images[0]).any()


def _pixel_points(W, H, f, z):
    """[H*W,3]: the point that an identity camera with focal length f sees in the centre of every pixel of a W x H image at
    depth z; exact for the dyadic values used."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([(x.reshape(-1) + 0.5 - W / 2) / f * z, (y.reshape(-1) + 0.5 - H / 2) / f * z, np.full(W * H, z)], 1).astype(f32)


def test_plane_counts_past_the_grid_cap(hip_lib):
    """The count kernel launches at most CONS_COUNT_BLOCKS = 256 workgroups of 256 pixels per view: 65 536 pixels a pass.
    Two 300 x 220 views (66 000 pixels: workgroup 0 takes a second block of 256 pixels, workgroup 1 one of 208) about a
    5 x 3 view, whose 15 pixels end the loop of every workgroup but the first at once.  View 0 has depth 1 and points at
    depth 2, view 2 depth 2 and points at depth 1: each is the other's anchor.  Plane id 77 covers the last row of view 0
    only, pixels 65 700 and up: a kernel that stops after one pass counts nothing for it and leaves it without an
    anchor."""
    one_pass = 256 * 256  # CONS_COUNT_BLOCKS * 256 pixels
    BW, BH, BF = 300, 220, 256.0
    assert BW * BH > one_pass and (BH - 1) * BW >= one_pass
    rng = np.random.default_rng(66)
    cams = [pinhole_camera(BW, BH, BF, BF), pinhole_camera(5, 3, 2.0, 2.0), pinhole_camera(BW, BH, BF, BF)]
    depths = [np.ones((BH, BW), f32), np.full((3, 5), 4.0, f32), np.full((BH, BW), 2.0, f32)]
    images = [rng.integers(0, 256, d.shape + (3,)).astype(np.uint8) for d in depths]
    masks = [rng.choice([0, 3, 8], (BH, BW)).astype(np.int32), rng.choice([0, 3], (3, 5)).astype(np.int32),
             rng.choice([0, 3, 8], (BH, BW)).astype(np.int32)]
    masks[0][BH - 1] = 77
    points = [_pixel_points(BW, BH, BF, 2.0), _pixel_points(5, 3, 2.0, 1.0), _pixel_points(BW, BH, BF, 1.0)]
    gdict = {5: [(1, 3)], 2: [(0, 3), (0, 8)], 9: [(0, 77)], 4: [(2, 8), (2, 3)]}
    outs, anchor_of_plane, counts = _check_planes(cams, depths, images, masks, points, gdict, [0, 1, 2], ETHRESH,
                                                  resolve=cr.resolve_chains_at_once)
    assert anchor_of_plane == {5: 0, 2: 2, 9: 2, 4: 0}
    assert counts[2].tolist() == [0, 0, BW] and np.nonzero(masks[0].reshape(-1) == 77)[0].min() == (BH - 1) * BW
    # every plane of the large views has pixels in both passes, and the reference counts them all
    assert counts[1].tolist() == [0, 0, int(np.isin(masks[0], (3, 8)).sum())] and counts[3].tolist() == [int((masks[2] != 0).sum()), 0, 0]
    assert np.isin(masks[0].reshape(-1)[one_pass:], (3, 8)).sum() > 50 and (masks[2].reshape(-1)[one_pass:] != 0).sum() > 100
    assert 0 < counts[0, 0] <= 15 and counts[0, 1:].tolist() == [0, 0]
    # the last row of view 0 now shows view 2's last row
    assert np.array_equal(outs[0][BH - 1], images[2][BH - 1]) and (outs[0][BH - 1] != images[0][BH - 1]).any()
    # a pixel of view 2 reads the same pixel of view 0, which an earlier step repainted from view 2's original where it has a plane
    there, chained = (masks[2] != 0) & (masks[0] == 0), (masks[2] != 0) & (masks[0] != 0)
    assert np.array_equal(outs[2][there], images[0][there]) and np.array_equal(outs[2][chained], images[2][chained])
    assert np.array_equal(outs[2][masks[2] == 0], images[2][masks[2] == 0]) and (outs[1] != images[1]).any()


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_python_arguments_are_checked_before_any_launch(hip_lib, golden):
    g = golden
    depths, images, points = devs(g.depths), devs(g.float_images), dev(g.points)

    def point_call(**changes):
        a = dict(cameras=g.cams, depths=depths, images=images, points=points, n_input_views=1)
        a.update(changes)
        return consistency.solve_point_inconsistency(**a)

    with pytest.raises(ValueError, match="5 cameras but 4 images"):
        point_call(images=images[:4])
    with pytest.raises(ValueError, match=r"images\[2\] must have shape"):
        point_call(images=images[:2] + [images[2][:, :10]] + images[3:])
    with pytest.raises(RuntimeError, match=r"images\[1\] must be torch.float32"):
        point_call(images=images[:1] + [dev(g.images[1])] + images[2:])
    with pytest.raises(RuntimeError, match=r"images\[0\] must be a tensor on cuda"):
        point_call(images=[images[0].cpu()] + images[1:])
    with pytest.raises(RuntimeError, match="depth must be a tensor on cuda"):
        point_call(depths=[depths[0].cpu()] + depths[1:])
    with pytest.raises(RuntimeError, match="points must be a floating-point tensor"):
        point_call(points=points.to(torch.int32))
    with pytest.raises(ValueError, match="n_input_views must be in 0 .. 5"):
        point_call(n_input_views=6)

    u8, masks, clouds = devs(g.images), devs(g.masks), devs(g.clouds)

    def plane_call(**changes):
        a = dict(cameras=g.cams, depths=depths, images=u8, plane_masks=masks, points=clouds, global_3Dplane_ID_dict=g.gdict,
                 anchor_view_ids=g.anchors)
        a.update(changes)
        return consistency.solve_plane_inconsistency(**a)

    with pytest.raises(RuntimeError, match=r"images\[0\] must be torch.uint8"):
        plane_call(images=images)
    with pytest.raises(ValueError, match=r"plane_masks\[1\] must have shape"):
        plane_call(plane_masks=masks[:1] + [masks[1][:, :7]] + masks[2:])
    with pytest.raises(RuntimeError, match="a plane mask must be an integer tensor"):
        plane_call(plane_masks=[masks[0].float()] + masks[1:])
    with pytest.raises(ValueError, match=r"points\[4\] must have shape"):
        plane_call(points=clouds[:4] + [clouds[4][:100]])
    with pytest.raises(RuntimeError, match=r"points\[0\] must be torch.float32"):
        plane_call(points=[clouds[0].double()] + clouds[1:])
    with pytest.raises(RuntimeError, match=r"points\[3\] must be a tensor on cuda"):
        plane_call(points=clouds[:3] + [clouds[3].cpu()] + clouds[4:])
    with pytest.raises(ValueError, match="twice"):
        plane_call(global_3Dplane_ID_dict={0: [(0, 5)], 1: [(0, 5)]})
    with pytest.raises(ValueError, match="names view 5"):
        plane_call(global_3Dplane_ID_dict={0: [(5, 5)]})
    for bad in ([3, 5, 1], [3, -1]):  # the library's own check names the entry
        with pytest.raises(RuntimeError, match=r"anchor_views\[1\] must be a view index below n_views"):
            plane_call(anchor_view_ids=bad)
        assert b"anchor_views[1]" in hip_lib.g4s_last_error()


def test_library_arguments_are_checked_on_the_host(hip_lib):
    """Bad sizes and NULL pointers return the library's error code with a message that names the argument, before anything is
    launched: the pointers below are never dereferenced."""
    lib = hip_lib
    nul, one, big = ctypes.c_void_p(0), ctypes.c_void_p(256), 1 << 20
    INVALID = -1

    def expect(rc, text):
        assert rc == INVALID, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    wv, focal = (ctypes.c_float * 32)(), (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    sizes, bad_sizes = (ctypes.c_int * 4)(4, 4, 2, 2), (ctypes.c_int * 4)(4, 4, 0, 2)
    maps, no_map = (ctypes.c_void_p * 2)(256, 256), (ctypes.c_void_p * 2)(256, 0)
    chw = (ctypes.c_int * 2)(0, 1)
    assert lib.g4s_consistency_points_workspace(2, 1, sizes) >= 2 * 120 + 16
    assert lib.g4s_consistency_points_workspace(2, 0, sizes) > lib.g4s_consistency_points_workspace(2, 1, sizes)
    assert lib.g4s_consistency_points_workspace(2, 3, sizes) == 0 and lib.g4s_consistency_points_workspace(2, 1, bad_sizes) == 0

    def points(n=5, pts=one, thr=0.1, V=2, n_in=1, sz=sizes, depth=maps, images=maps, layout=chw, outs=maps, conf=maps, state=one,
               ws=one, ws_bytes=big):
        return lib.g4s_consistency_points(n, pts, thr, V, n_in, wv, focal, sz, depth, images, layout, outs, conf, 0, state, ws,
                                          ws_bytes, nul)

    expect(points(n=-1), "n_points must be in")
    expect(points(thr=float("nan")), "depth_threshold must not be NaN")
    expect(points(V=-1), "n_views must be in 0 .. 65535")
    expect(points(V=70000), "n_views must be in 0 .. 65535")
    expect(points(n_in=3), "n_input_views must be in 0 .. n_views")
    expect(points(sz=bad_sizes), "sizes: width, height must be positive")
    expect(points(sz=(ctypes.c_int * 4)(4, 4, 1 << 15, (1 << 15) + 1)), "width * height at most 2^30")
    expect(points(sz=nul), "NULL required pointer")
    expect(points(sz=bad_sizes, n_in=3), "sizes: width, height must be positive")  # the first of two bad arguments
    expect(points(ws_bytes=lib.g4s_consistency_points_workspace(2, 1, sizes) - 1), "workspace too small")
    expect(points(outs=nul), "images_out and conf must both be there or both be NULL")
    expect(points(state=nul), "state: NULL")
    expect(points(pts=nul), "points: NULL")
    expect(points(depth=no_map), "depth[1]: NULL pointer")
    expect(points(images=no_map), "images[1]: NULL pointer")
    expect(points(images=nul), "images: NULL array")
    expect(points(layout=nul), "image_chw: NULL array")
    expect(points(outs=no_map), "images_out[1]: NULL pointer")
    expect(points(conf=no_map), "conf[1]: NULL pointer")
    expect(points(ws_bytes=8), "workspace too small")
    expect(points(ws=nul), "workspace too small")
    assert points(V=0, n_in=0) == 0  # no view: nothing to do

    offs, bad_offs = (ctypes.c_int * 3)(0, 2, 3), (ctypes.c_int * 3)(0, 2, 2)
    slot_plane, bad_plane = (ctypes.c_int * 3)(-1, 0, -1), (ctypes.c_int * 3)(-1, 2, -1)
    anchors, bad_anchors = (ctypes.c_int * 2)(1, 0), (ctypes.c_int * 2)(1, 2)
    assert lib.g4s_consistency_plane_counts_workspace(2, 3, 2) >= 2 * 128 + 20
    assert lib.g4s_consistency_plane_counts_workspace(-1, 3, 2) == 0

    def counts(thr=0.1, V=2, sz=sizes, depth=maps, masks=maps, pts=maps, off=offs, plane=slot_plane, K=2, A=2, anchor=anchors,
               out=one, ws_bytes=big):
        return lib.g4s_consistency_plane_counts(thr, V, wv, focal, sz, depth, masks, pts, off, plane, K, A, anchor, out, one,
                                                ws_bytes, nul)

    expect(counts(thr=float("nan")), "depth_threshold must not be NaN")
    expect(counts(V=65536), "n_views must be in 0 .. 65535")
    expect(counts(sz=bad_sizes), "sizes: width, height must be positive")
    expect(counts(ws_bytes=lib.g4s_consistency_plane_counts_workspace(2, 3, 2) - 1), "workspace too small")
    expect(counts(K=-1), "n_planes, n_anchors must not be negative")
    expect(counts(anchor=nul), "anchor_views: NULL array")
    expect(counts(anchor=bad_anchors), "anchor_views[1] must be a view index below n_views")
    expect(counts(masks=no_map), "masks[1]: NULL pointer")
    expect(counts(pts=nul), "points: NULL array")
    expect(counts(off=nul), "slot_offset: NULL array")
    expect(counts(off=bad_offs), "slot_offset[2]: every view has at least slot 0")
    expect(counts(plane=nul), "slot_plane: NULL array")
    expect(counts(plane=bad_plane), "slot_plane[1] must be -1 or a plane below n_planes")
    expect(counts(out=nul), "counts: NULL pointer")
    expect(counts(ws_bytes=8), "workspace too small")
    assert counts(K=0, plane=(ctypes.c_int * 3)(-1, -1, -1)) == 0  # no plane: nothing to count

    step, bad_step = (ctypes.c_int * 3)(-1, 0, -1), (ctypes.c_int * 3)(-1, -2, -1)
    anchor_of, bad_anchor_of = (ctypes.c_int * 3)(0, 1, 0), (ctypes.c_int * 3)(0, 2, 0)
    assert lib.g4s_consistency_plane_repaint_workspace(2, sizes, 3) >= 2 * 128 + 3 * 20 * 4
    assert lib.g4s_consistency_plane_repaint_workspace(2, bad_sizes, 3) == 0

    def repaint(V=2, sz=sizes, masks=maps, images=maps, outs=maps, off=offs, st=step, an=anchor_of, ws_bytes=big):
        return lib.g4s_consistency_plane_repaint(0.1, V, wv, focal, sz, maps, masks, maps, images, outs, off, st, an, one, ws_bytes,
                                                 nul)

    expect(repaint(V=-1), "n_views must be in 0 .. 65535")
    expect(repaint(V=65536), "n_views must be in 0 .. 65535")
    expect(repaint(sz=nul), "NULL required pointer")
    expect(repaint(sz=bad_sizes), "sizes: width, height must be positive")
    expect(repaint(sz=(ctypes.c_int * 4)(1 << 15, 1 << 15, 1 << 15, 1 << 15)), "fewer than 2^31 pixels in all")
    expect(repaint(ws_bytes=lib.g4s_consistency_plane_repaint_workspace(2, sizes, 3) - 1), "workspace too small")
    expect(repaint(masks=nul), "masks: NULL array")
    expect(repaint(images=no_map), "images[1]: NULL pointer")
    expect(repaint(outs=nul), "images_out: NULL array")
    expect(repaint(off=bad_offs), "slot_offset[2]")
    expect(repaint(st=nul), "slot_step: NULL array")
    expect(repaint(st=bad_step), "slot_step[1] must be -1 or a step")
    expect(repaint(an=nul), "slot_anchor: NULL array")
    expect(repaint(an=bad_anchor_of), "slot_anchor[1] must be a view index below n_views")
    expect(repaint(ws_bytes=8), "workspace too small")
    assert repaint(V=0) == 0
