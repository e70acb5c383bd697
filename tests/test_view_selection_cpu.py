"""View selection without a GPU: the numpy restatement of the contract (tests/view_selection_ref.py) against what the
reference's own code produced (tests/golden/view_selection.npz, make_golden_view_selection.py), the host-side decisions of
g4splat_amd.view_selection against the reference's ids and random state, and the argument checks."""
import json
import os
import random

import numpy as np
import pytest
import torch

import view_selection_ref as sr
from g4splat_amd import _lib, view_selection as vs
from support import same_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "view_selection.npz")))
    g["cams"] = [sr.camera(w, f[0], f[1], s[0], s[1]) for w, f, s in zip(g["wvt"], g["fov"], g["sizes"])]
    shape = tuple(g["masks_shape"])
    for key in ("masks", "masks_ref64", "masks_agreed"):
        g[key] = np.unpackbits(g[key])[: shape[0] * shape[1]].reshape(shape).astype(bool)
    g["selection"] = json.loads(str(g["selection"]))
    g["sampling"] = json.loads(str(g["sampling"]))
    g["restated"] = sr.visible_masks(g["points"], g["cams"])
    g["table"] = sr.counts(g["restated"])
    return g


def test_restated_masks_equal_the_reference_on_the_agreed_set(gold):
    agreed = gold["masks_agreed"]
    excluded, size, _ref_differ, _restatement_differs = gold["masks_excluded"]
    assert size == agreed.size == 70 * 4000 and excluded == (~agreed).sum() and excluded <= 0.001 * size
    assert np.array_equal(gold["restated"][agreed], gold["masks"][agreed])
    assert 0.1 < gold["masks"].mean() < 0.6  # both answers occur in number


def test_restated_counts_are_symmetric_and_equal_the_popcounts_of_the_bits(gold):
    masks, table = gold["restated"], gold["table"]
    assert np.array_equal(table, table.T)
    assert np.array_equal(np.diag(table), masks.sum(1))
    words = sr.words(masks)
    assert words.shape == (70, 63) and words.dtype == np.uint64
    assert (words[:, -1] >> np.uint64(4000 % 64) == 0).all()  # tail bits
    assert np.array_equal(sr.popcount_counts(words), table)
    assert np.array_equal(np.stack([sr.vr.unpack(w, 4000) for w in words]), masks)


@pytest.mark.parametrize("C,n_words,chunk_words", [(1, 1, None), (4, 1, None), (17, 129, None), (33, 130, 64), (70, 63, 1)])
def test_the_matrix_product_of_the_bits_equals_the_popcounts(gold, C, n_words, chunk_words):
    """sr.bit_counts serves the GPU tests of the count kernel where sr.popcount_counts is too slow; here both run, on the
    generator those tests use, whole and in slices that do not divide the row."""
    w = sr.random_words(C, n_words, 1000 * C + n_words)
    assert w.dtype == np.uint64 and w.shape == (C, n_words)
    want = sr.popcount_counts(w)
    got = sr.bit_counts(w, chunk_words)
    assert got.dtype == np.int64 and np.array_equal(got, want) and np.array_equal(got, got.T)
    if C > 3:
        assert want[1, 1] == 64 * n_words and not want[2].any() and 1 <= want[C - 1, C - 1] <= 64
        assert np.array_equal(want[1], np.diag(want)) and not w[C - 1, :-1].any()  # the row of ones counts every row's bits
        assert 0.2 < want[0, 0] / (64.0 * n_words) < 0.3 or n_words == 1
    if C == 70:  # and on the golden scene's own words
        words = sr.words(gold["restated"])
        assert np.array_equal(sr.bit_counts(words, 7), gold["table"])


def ratio_from(common, visible1, visible2):
    return sr.ratio_of([[visible1, common], [common, visible2]])(0, 1)


def test_restated_ratios_equal_the_reference_up_to_the_bits_in_doubt(gold):
    """d bits in doubt between the two cameras move a ratio by at most 2 d / min|V| (the generator's margin); every camera
    has its own centre (z = 0) among the points, so d is rarely 0."""
    ratio = sr.ratio_of(gold["table"])
    doubt = (~gold["masks_agreed"] | (gold["restated"] != gold["masks"])).sum(1)
    visible = gold["masks"].sum(1)
    assert doubt.max() <= 4
    for (i, j), want in zip(gold["pairs"], gold["pair_ratios"]):
        d = int(doubt[i] + doubt[j])
        assert abs(ratio(int(i), int(j)) - want) <= 2.0 * d / min(visible[i], visible[j]), (i, j)
    assert gold["pair_ratios"][-1] == 1.0 and 0.3 < gold["pair_ratios"][1] < 0.95
    # the device table's ratio is planes.covisibility_rate over its integers: the reference's expression, value for value
    for c, a, b in [(0, 0, 0), (0, 0, 7), (3, 4, 5), (5, 5, 9), (2, 6, 3)]:
        assert vs.covisibility_rate(c, a, b) == ratio_from(c, a, b)


@pytest.mark.parametrize("name", ["random257", "random11", "three", "lattice", "identical", "far"])
def test_restated_sampling_equals_the_reference(gold, name):
    case, cloud = gold["sampling"][name], gold["cloud_" + name]
    idx, dist = sr.fps(cloud, case["k"], case["first"])
    assert idx.tolist() == case["indices"]
    if name == "identical":
        assert idx.tolist() == [case["first"]] + [0] * (case["k"] - 1) and not dist.any()
    if name == "lattice":
        assert len(set(idx.tolist())) == case["k"]
    if name == "far":
        assert (dist == np.float32(1e10)).any()  # the cap binds


def test_restated_lookat_points_equal_the_reference_given_its_draws(gold):
    clouds = np.load(os.path.join(GOLDEN, "visibility_grid.npz"))["clouds"]
    assert np.array_equal(sr.nearest_train_indices(gold["lookat_train"], gold["lookat_novel"]), gold["lookat_closest"])
    got = sr.lookat_points(gold["lookat_train"], clouds, gold["lookat_novel"], int(gold["lookat_fps_num"]), gold["lookat_first"],
                           gold["lookat_ids"])
    assert got.dtype == np.float32
    same_bits(got, gold["lookat"])
    t, c = torch.tensor(gold["lookat_train"]), torch.tensor(gold["lookat_novel"])
    assert np.array_equal(vs.nearest_train_indices(t, c).numpy(), gold["lookat_closest"])
    # a tie goes to the smallest index
    assert vs.nearest_train_indices(torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [1.0, 0, 0]]), torch.zeros(2, 3)).tolist() == [0, 0]


def test_the_draw_helper_reproduces_the_recorded_draws(gold):
    M, N = 5, 64 * 48
    torch.manual_seed(int(gold["lookat_seed"]))
    first, ids = vs.draw_lookat_indices(M, N, len(gold["lookat_novel"]), int(gold["lookat_fps_num"]), torch.device("cpu"))
    assert first.tolist() == gold["lookat_first"].tolist() and ids.tolist() == gold["lookat_ids"].tolist()
    # a cloud that is returned whole draws no first index, as in the reference
    torch.manual_seed(5)
    want = torch.randint(0, 10, (4,))
    torch.manual_seed(5)
    first, ids = vs.draw_lookat_indices(3, 10, 4, 10, torch.device("cpu"))
    assert first is None and torch.equal(ids, want)


@pytest.mark.parametrize("name", ["typical", "early", "tight", "step4", "step5", "empty", "none_left", "one"])
def test_select_views_returns_the_reference_ids_and_leaves_its_random_state(gold, name):
    case = gold["selection"][name]
    asked = []
    ratio = sr.ratio_of(gold["table"])

    def counting(i, j):
        asked.append((i, j))
        return ratio(i, j)
    random.seed(case["seed"])
    ids = vs.select_views(case["rates"], counting, case["select_num"], case["low"], case["high"], case["bound"], rng=random)
    assert ids == case["ids"]
    assert random.random() == case["next_random"]
    if name == "none_left":
        assert ids == [] and not asked
    if name == "one":
        assert len(ids) == 2  # the reference's quirk: the first view skips the stop test


class _Rng:
    """Counts the shuffles and leaves every list as it is."""

    def __init__(self):
        self.shuffles = []

    def shuffle(self, x):
        self.shuffles.append(list(x))


def test_each_step_of_select_views_on_its_own():
    never = lambda i, j: 0.0  # noqa: E731
    always = lambda i, j: 1.0  # noqa: E731
    # steps 1-3: the first view in range is taken unasked, the others while their ratios allow; one shuffle
    rng = _Rng()
    assert vs.select_views([0.2, 0.9, 0.3, 0.01, 0.4], never, 3, rng=rng) == [0, 2, 4]
    assert len(rng.shuffles) == 1 and rng.shuffles[0] == [(0, 0.2), (1, 0.9), (2, 0.3), (3, 0.01), (4, 0.4)]
    # a candidate above the bound against ONE selected view is rejected; the bound itself is not above
    pairs = {(0, 2): 0.81, (0, 4): 0.8, (4, 5): 0.8000001}
    ratio = lambda i, j: pairs.get((i, j), 0.0)  # noqa: E731
    rng = _Rng()
    assert vs.select_views([0.2, 0.9, 0.3, 0.6, 0.4, 0.5], ratio, 3, rng=rng) == [0, 4, 2]
    assert len(rng.shuffles) == 2 and rng.shuffles[1] == [2, 5]  # step 5 fills from the views at or below the upper bound
    # step 4: the views below the lower bound, in shuffled order, under the same ratio test
    rng = _Rng()
    assert vs.select_views([0.2, 0.01, 0.02, 0.03], lambda i, j: 1.0 if (i, j) == (0, 2) else 0.0, 3, rng=rng) == [0, 1, 3]
    assert len(rng.shuffles) == 1
    # an empty filtered list: step 4 starts from nothing
    assert vs.select_views([0.01, 0.02, 0.9], always, 2, rng=_Rng()) == [0, 1]
    # step 5 alone: everything is covisible, the rest fills up in (here unshuffled) index order, rates above the bound stay out
    rng = _Rng()
    assert vs.select_views([0.2, 0.3, 0.9, 0.01, 0.4], always, 4, rng=rng) == [0, 1, 3, 4]
    assert rng.shuffles[1] == [1, 3, 4]
    # select_num reached early: no further ratio is asked for
    asked = []
    assert vs.select_views([0.2, 0.3, 0.4, 0.45], lambda i, j: asked.append((i, j)) or 0.0, 2, rng=_Rng()) == [0, 1]
    assert asked == [(0, 1)]


def test_arguments_are_checked_before_the_library_is_touched(gold, monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", touched)
    monkeypatch.setattr(_lib, "load", touched)
    cams, pts = gold["cams"][:2], torch.zeros(5, 3)
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        vs.Covisibility(torch.zeros(5, 2), cams)
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        vs.Covisibility(torch.zeros(2, 5, 3), cams)
    with pytest.raises(ValueError, match="at least one camera"):
        vs.Covisibility(pts, [])
    with pytest.raises(ValueError, match="at least one camera"):
        vs.select_need_inpaint_views([], [], pts)
    with pytest.raises(ValueError, match="2 cameras but 3 rates"):
        vs.select_need_inpaint_views(cams, [0.1, 0.2, 0.3], pts)
    clouds = torch.zeros(2, 12, 3)
    with pytest.raises(ValueError, match="num_samples"):
        vs.farthest_point_indices(clouds, 1, [0, 0])
    with pytest.raises(ValueError, match="num_samples"):
        vs.farthest_point_indices(clouds, 12, [0, 0])
    with pytest.raises(ValueError, match=r"\[M,N,3\]"):
        vs.farthest_point_indices(torch.zeros(12, 3), 4, [0])
    with pytest.raises(ValueError, match="first index 12 of cloud 1"):
        vs.farthest_point_indices(clouds, 4, [0, 12])
    with pytest.raises(ValueError, match="first index -1 of cloud 0"):
        vs.farthest_point_indices(clouds, 4, torch.tensor([-1, 3]))
    with pytest.raises(ValueError, match="2 clouds but 1 first"):
        vs.farthest_point_indices(clouds, 4, [0])
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        vs.farthest_point_sample(torch.zeros(12, 2), 4)
    with pytest.raises(ValueError, match="num_samples"):
        vs.farthest_point_sample(torch.zeros(12, 3), 1, 0)
    # the reference's quirk needs no device: a cloud of at most num_samples points comes back as it is
    small = torch.rand(4, 3)
    assert vs.farthest_point_sample(small, 4) is small and vs.farthest_point_sample(small, 9) is small
    # with valid arguments the next thing asked for is a HIP device
    with pytest.raises(RuntimeError, match="HIP device"):
        vs.Covisibility(pts, cams)
    with pytest.raises(RuntimeError, match="HIP device"):
        vs.farthest_point_indices(clouds, 4, [0, 11])


def test_the_library_checks_its_arguments_on_the_host(hip_lib):
    import ctypes
    lib = hip_lib
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # never dereferenced: validation fails first
    wv, focal = (ctypes.c_float * 16)(), (ctypes.c_float * 2)(1.0, 1.0)
    sizes, bad_sizes = (ctypes.c_int * 2)(4, 4), (ctypes.c_int * 2)(4, 0)
    big = 1 << 20

    def expect(rc, text):
        assert rc == -1, rc
        assert text.encode() in lib.g4s_last_error(), lib.g4s_last_error()

    expect(lib.g4s_view_bits(-1, one, 1, wv, focal, sizes, one, one, big, nul), "n_points must be in")
    expect(lib.g4s_view_bits(2 ** 31 - 63, one, 1, wv, focal, sizes, one, one, big, nul), "n_points must be in")
    expect(lib.g4s_view_bits(5, one, 0, wv, focal, sizes, one, one, big, nul), "n_views must be in")
    expect(lib.g4s_view_bits(5, nul, 1, wv, focal, sizes, one, one, big, nul), "NULL required pointer")
    expect(lib.g4s_view_bits(5, one, 1, wv, focal, bad_sizes, one, one, big, nul), "width, height must be positive")
    expect(lib.g4s_view_bits(5, one, 1, wv, focal, sizes, one, one, 8, nul), "workspace too small")
    assert lib.g4s_view_bits(0, nul, 1, wv, focal, sizes, nul, one, big, nul) == 0  # no point: nothing to do
    expect(lib.g4s_view_overlap(0, 1, one, one, nul, 0, nul), "n_views must be in")
    expect(lib.g4s_view_overlap(2, -1, one, one, nul, 0, nul), "n_words must be in")
    expect(lib.g4s_view_overlap(2, 1, nul, one, nul, 0, nul), "NULL required pointer")
    expect(lib.g4s_view_overlap(2, 0, nul, nul, nul, 0, nul), "NULL required pointer")
    first, bad_first = (ctypes.c_int * 2)(0, 9), (ctypes.c_int * 2)(0, 10)
    expect(lib.g4s_fps(0, 10, one, first, 4, one, one, one, one, big, nul), "n_clouds must be in")
    expect(lib.g4s_fps(2, 2, one, first, 2, one, one, one, one, big, nul), "n_points must be in")
    expect(lib.g4s_fps(2, 10, one, first, 1, one, one, one, one, big, nul), "n_samples must be in")
    expect(lib.g4s_fps(2, 10, one, first, 10, one, one, one, one, big, nul), "n_samples must be in")
    expect(lib.g4s_fps(2, 10, one, first, 4, one, one, nul, one, big, nul), "NULL required pointer")
    expect(lib.g4s_fps(2, 10, one, bad_first, 4, one, one, one, one, big, nul), "first[1] must be a point index")
    expect(lib.g4s_fps(2, 10, one, first, 4, one, one, one, one, 8, nul), "workspace too small")
    assert lib.g4s_view_bits_workspace(70) >= 70 * 80 and lib.g4s_fps_workspace(24, 10) >= 24 * 10 * 8 + 24 * 4
    assert lib.g4s_fps_workspace(0, 10) == 0 and lib.g4s_fps_workspace(3, 1) == 0
    # a call that succeeds clears the message of the last one that did not
    assert lib.g4s_view_bits(0, nul, 1, wv, focal, sizes, nul, one, big, nul) == 0 and lib.g4s_last_error() == b""


def test_cameras_and_centres_are_checked_before_the_device(gold):
    from types import SimpleNamespace
    cam, pts = gold["cams"][0], torch.zeros(5, 3)
    small = SimpleNamespace(world_view_transform=torch.eye(3), FoVx=1.0, FoVy=1.0, image_width=4, image_height=3)
    with pytest.raises(ValueError, match="camera 1: world_view_transform must be 4 x 4"):
        vs.Covisibility(pts, [cam, small])
    for W, H in ((0, 3), (4, -1)):
        flat = SimpleNamespace(world_view_transform=torch.eye(4), FoVx=1.0, FoVy=1.0, image_width=W, image_height=H)
        with pytest.raises(ValueError, match="camera 0: image_width and image_height must be positive"):
            vs.Covisibility(pts, [flat])
    with pytest.raises(ValueError, match="points must be a tensor"):
        vs.Covisibility([[0.0, 0.0, 0.0]], [cam])
    with pytest.raises(ValueError, match="at least one cloud"):
        vs.farthest_point_indices(torch.zeros(0, 6, 3), 2, [])
    with pytest.raises(ValueError, match="gs_train_view_points must be a tensor"):
        vs.get_novel_cams_lookat_points(torch.zeros(2, 3), torch.zeros(6, 3), torch.zeros(1, 3))
    with pytest.raises(ValueError, match="train_cam_centers must be"):
        vs.get_novel_cams_lookat_points(torch.zeros(3, 3), torch.zeros(2, 6, 3), torch.zeros(1, 3))
