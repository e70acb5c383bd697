"""The numpy restatement of the cross-view consistency contract (tests/consistency_ref.py) and the host decisions of
g4splat_amd/consistency.py against what the reference's two solver scripts wrote (tests/golden/make_golden_consistency.py):
confident maps and repainted images on the agreed set, the anchors, the step order, the chain walk against a literal
in-place repaint.  No GPU: the GPU tests (tests/test_gpu_consistency.py) hold the library to the restatement bit for bit."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import consistency_ref as cr
from g4splat_amd import consistency
from support import load_consistency_golden

f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return load_consistency_golden()


@pytest.fixture(scope="module")
def restated(golden):
    """The restatement's float32 outputs of the golden scene, computed once and left unchanged."""
    g = golden
    stats = {}
    outs, confs = cr.point_solver(g.cams, g.depths, g.float_images, g.points, g.n_input, g.threshold, f32, stats)
    lengths = [np.zeros(m.size, np.int64) for m in g.masks]
    b_outs, anchor_of_plane, counts = cr.plane_solver(g.cams, g.depths, g.images, g.masks, g.clouds, g.gdict, g.anchors,
                                                      g.threshold, f32, lengths)
    return SimpleNamespace(outs=outs, confs=confs, stats=stats, b_outs=b_outs, anchor_of_plane=anchor_of_plane, counts=counts,
                           lengths=lengths)


def test_restatement_equals_what_the_point_solver_script_wrote(golden, restated):
    g, I = golden, golden.n_input
    conf = np.stack(restated.confs) * 255
    assert g.point_conf_agreed.mean() >= 0.999 and g.point_png_agreed.mean() >= 0.999
    assert np.array_equal(conf[g.point_conf_agreed], g.point_conf[g.point_conf_agreed])
    assert (conf[:I] == 255).all()
    png = np.stack([cr.images_to_uint8(o) for o in restated.outs[I:]])
    assert np.array_equal(png[g.point_png_agreed], g.point_png[g.point_png_agreed])
    for v in range(I):  # an input view keeps its image
        assert np.array_equal(restated.outs[v], g.float_images[v])


def test_restatement_equals_what_the_plane_solver_script_wrote(golden, restated):
    g = golden
    png = np.stack(restated.b_outs[g.n_input:])
    assert g.plane_png_agreed.mean() >= 0.999
    assert np.array_equal(png[g.plane_png_agreed], g.plane_png[g.plane_png_agreed])


def test_golden_scene_has_the_cases_the_solvers_need(golden, restated):
    g, s = golden, restated.stats
    assert s == {k: golden.stats[k] for k in s}  # as recorded when the scripts ran
    assert s["duplicate_pixels_differing"] > 1000 and s["changed_pixels"] > 1000 and max(s["conf_zeros"]) > 100
    chain = np.bincount(np.concatenate(restated.lengths[g.n_input:]), minlength=3)
    assert chain[2:].sum() > 100 and chain.tolist() == golden.stats["chain_lengths"]
    assert golden.stats["own_view_anchor_pixels"] > 100
    anchors = [restated.anchor_of_plane[k] for k in g.gdict]
    assert anchors == golden.stats["anchors"] and len(set(anchors) - {-1}) >= 2
    assert restated.counts.tolist() == golden.stats["counts"]
    assert len(cr.plane_steps(g.gdict, restated.anchor_of_plane)) == golden.stats["steps"]
    # the float64 evaluation decides the same way but for a handful of (point, view) pairs
    vis32, _ = cr.point_tables(g.cams, g.depths, g.points, g.threshold, f32)
    vis64, _ = cr.point_tables(g.cams, g.depths, g.points, g.threshold, np.float64)
    assert (vis32 != vis64).sum() <= 0.001 * vis32.size


def test_choose_anchor_views():
    choose = consistency.choose_anchor_views
    assert choose([[3, 7, 7], [0, 0, 0], [5, 5, 5], [0, 1, 0]], [9, 4, 2]) == [4, -1, 9, 4]  # a tie: the first wins
    assert choose([[2], [0]], [6]) == [6, -1]  # a single anchor
    assert choose([], [1, 2]) == [] and choose([[], []], []) == [-1, -1]
    assert choose(torch.tensor([[1, 2], [4, 3]]), [0, 1]) == [1, 0] and choose(np.array([[1, 2]]), (5, 8)) == [8]
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 4, (50, 6))
    assert choose(counts, list(range(10, 16))) == cr.choose_anchor_views(counts, list(range(10, 16)))


def test_plane_steps():
    gdict = {0: [(0, 5), (2, 7)], 1: [(1, 5)], 2: [(2, 9), (0, 8), (1, 1)]}
    assert consistency.plane_steps(gdict, {0: 2, 1: -1, 2: 0}) == [(0, 5, 2), (2, 7, 2), (2, 9, 0), (0, 8, 0), (1, 1, 0)]
    assert consistency.plane_steps(gdict, {0: -1, 1: -1, 2: -1}) == []
    assert consistency.plane_steps({"3": [[1, 2]]}, {3: 0}) == [(1, 2, 0)]  # as loaded from JSON
    assert consistency.plane_steps({7: [(1, 2)], 3: [(0, 2)]}, {3: 1, 7: 0}) == [(1, 2, 0), (0, 2, 1)]  # dict order, not key order
    for bad in ({0: [(0, 5), (0, 5)]}, {0: [(0, 5)], 1: [(1, 1), (0, 5)]}):
        with pytest.raises(ValueError, match="twice"):
            consistency.plane_steps(bad, {0: 0, 1: 0})
    with pytest.raises(ValueError, match="twice"):  # even in a plane without an anchor
        consistency.plane_steps({0: [(0, 5)], 1: [(0, 5)]}, {0: 0, 1: -1})


def test_images_to_uint8():
    x = np.array([0.0, 0.5, 1.0, 0.999, 1.0 / 255.0, 254.9 / 255.0], f32)
    want = np.array([0, 127, 255, 254, int(f32(1.0) / f32(255.0) * f32(255.0)), int(f32(254.9) / f32(255.0) * f32(255.0))], np.uint8)
    assert np.array_equal(consistency.images_to_uint8(x), want)
    got = consistency.images_to_uint8(torch.tensor(x))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    # float32 u8 / 255 * 255 comes back for every byte although the save step truncates: an untouched pixel keeps its colour
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(consistency.images_to_uint8(u8.astype(f32) / f32(255)), u8)
    assert np.array_equal(cr.images_to_uint8(u8.astype(f32) / f32(255)), u8)


@pytest.mark.parametrize("seed", range(8))
def test_chain_walk_equals_the_literal_in_place_repaint(seed):
    """Random sources over three small views: every step has one target view and one anchor, a pixel is in at most one step,
    anchors may be the view itself and may have been repainted by an earlier step."""
    rng = np.random.default_rng(seed)
    sizes = [(3, 4), (2, 5), (4, 4)]
    images = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    src = [(np.full(h * w, cr.NO_STEP, np.int64), np.zeros(h * w, np.int64), np.zeros(h * w, np.int64)) for h, w in sizes]
    n_steps = 9
    for t in range(n_steps):
        w, a = int(rng.integers(3)), int(rng.integers(3))
        free = np.nonzero(src[w][0] == cr.NO_STEP)[0]
        q = rng.permutation(free)[: int(rng.integers(0, 5))]
        src[w][0][q], src[w][1][q] = t, a
        src[w][2][q] = rng.integers(0, sizes[a][0] * sizes[a][1], len(q))
    lengths = [np.zeros(h * w, np.int64) for h, w in sizes]
    walked = cr.resolve_chains(images, src, lengths)
    literal = cr.repaint_in_place(images, src, n_steps)
    for a, b in zip(walked, literal):
        assert np.array_equal(a, b)
    assert max(l.max() for l in lengths) >= 1


def _random_sources(seed, sizes=((3, 4), (2, 5), (4, 4)), n_steps=9):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    src = [(np.full(h * w, cr.NO_STEP, np.int64), np.zeros(h * w, np.int64), np.zeros(h * w, np.int64)) for h, w in sizes]
    for t in range(n_steps):
        w, a = int(rng.integers(len(sizes))), int(rng.integers(len(sizes)))
        free = np.nonzero(src[w][0] == cr.NO_STEP)[0]
        q = rng.permutation(free)[: int(rng.integers(0, 5))]
        src[w][0][q], src[w][1][q] = t, a
        src[w][2][q] = rng.integers(0, sizes[a][0] * sizes[a][1], len(q))
    return images, src


@pytest.mark.parametrize("seed", range(8))
def test_walking_all_chains_at_once_equals_the_walk_pixel_by_pixel(seed):
    """cr.resolve_chains_at_once serves the GPU test whose views are too large for cr.resolve_chains; here both run, on
    the random sources of the test above, with the chain lengths."""
    images, src = _random_sources(seed)
    lengths = [np.zeros(len(s[0]), np.int64) for s in src]
    lengths_at_once = [np.full(len(s[0]), -1, np.int64) for s in src]
    walked = cr.resolve_chains(images, src, lengths)
    at_once = cr.resolve_chains_at_once(images, src, lengths_at_once)
    for a, b, la, lb in zip(walked, at_once, lengths, lengths_at_once):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) and np.array_equal(la, lb)
    assert max(l.max() for l in lengths) >= 1
    literal = cr.repaint_in_place(images, src, 9)
    assert all(np.array_equal(a, b) for a, b in zip(at_once, literal))


def test_walking_all_chains_at_once_on_the_golden_scene(golden, restated):
    g = golden
    lengths = [np.zeros(m.size, np.int64) for m in g.masks]
    outs, anchor_of_plane, counts = cr.plane_solver(g.cams, g.depths, g.images, g.masks, g.clouds, g.gdict, g.anchors, g.threshold,
                                                    f32, lengths, cr.resolve_chains_at_once)
    assert anchor_of_plane == restated.anchor_of_plane and np.array_equal(counts, restated.counts)
    for a, b, la, lb in zip(outs, restated.b_outs, lengths, restated.lengths):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) and np.array_equal(la, lb)
    assert max(l.max() for l in lengths) >= 2  # chains of more than one hop
    assert cr.resolve_chains_at_once([], []) == []


def test_same_step_read_sees_the_state_before_the_step():
    """View 0 repaints itself from itself, shifted by one pixel: pixel q reads q + 1, which the same step repaints."""
    image = np.arange(5 * 3, dtype=np.uint8).reshape(1, 5, 3)
    src = [(np.array([0, 0, 0, 0, cr.NO_STEP]), np.zeros(5, np.int64), np.array([1, 2, 3, 4, 0]))]
    for out in (cr.resolve_chains([image], src)[0], cr.repaint_in_place([image], src, 1)[0]):
        assert np.array_equal(out[0, :4], image[0, 1:]) and np.array_equal(out[0, 4], image[0, 4])


def test_solver_arguments_are_checked_before_the_device():
    d, img, pts = torch.ones((3, 4)), torch.zeros((3, 4, 3)), torch.zeros((5, 3))
    point, plane = consistency.solve_point_inconsistency, consistency.solve_plane_inconsistency
    with pytest.raises(ValueError, match="1 cameras but 0 depths"):
        point([None], [], [img], pts, 0)
    with pytest.raises(ValueError, match="1 cameras but 0 images"):
        point([None], [d], [], pts, 0)
    for n_input in (-1, 2):
        with pytest.raises(ValueError, match=r"n_input_views must be in 0 \.\. 1"):
            point([None], [d], [img], pts, n_input)
    for bad in ([[0.0, 0.0, 0.0]], pts.long()):
        with pytest.raises(RuntimeError, match="floating-point tensor on a HIP device"):
            consistency.point_states([None], [d], [img], bad, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        point([None], [d], [img], pts, 1)
    masks, clouds = [torch.zeros((3, 4), dtype=torch.int32)], [torch.zeros((12, 3))]
    with pytest.raises(ValueError, match="1 cameras but 0 plane_masks"):
        plane([None], [d], [img], [], clouds, {}, [0])
    with pytest.raises(ValueError, match="twice"):
        plane([None], [d], [img], masks, clouds, {0: [(0, 1)], 1: [(0, 1)]}, [0])
    with pytest.raises(RuntimeError, match="depth must be a tensor on a HIP device"):
        plane([None], [[1.0]], [img], masks, clouds, {}, [0])
    with pytest.raises(RuntimeError, match="HIP device"):
        plane([None], [d], [img], masks, clouds, {0: [(0, 1)]}, [0])
    outs, anchors, counts = plane([], [], [], [], [], {0: [(0, 1)], "3": []}, [0, 1])  # no views: nothing is asked of a device
    assert outs == [] and anchors == {0: -1, 3: -1} and counts.shape == (2, 2) and counts.dtype == torch.int64
